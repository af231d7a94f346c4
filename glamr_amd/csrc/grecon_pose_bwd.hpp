// Vector-Jacobian product from the world poses a stage launch reports (orient_world, trans_world) back to the trajectory variables of the
// scene parameters, for ONE person slot -- the link a caller-defined loss term on the world poses needs.  Written against the
// block runtime like traj_global_bwd.hpp, which does the work between the assembled local rows and the poses: DeviceRT on the device
// (grecon_pose_bwd.hip), the host runtime of tests/hostsim on the CPU.
//
// The function differentiated is get_pred_trajectory_base plus the world_dheading step (global_recon_model.py:394-426, 459-465), phases A-C of
// grecon_algo.hpp.  For existing frames [fr_start, fr_end), row e = frame fr_start + e:
//   A[e][0:2]  = prior[e][0:2] + (e == 0 ? local_xy : local_dxy[e]),   A[e][2] = prior[e][2] + local_z[e],   A[e][3:9] = prior[e][3:9] + local_rot[e]
//   h_e        = atan2s(prior[e][10], prior[e][9]) + (e == 0 ? local_heading : local_dheading[e] * dheading_mask[e])      (no mask = 0)
//   A[e][9:11] = (cos h_e, sin h_e)
//   (trans_world, base)[fr_start + e] = traj_local2global_heading(A) + quaternion_to_angle_axis                         (traj_global_bwd)
//   orient_world[t] = has_world_dheading ? aa(q_z(world_dheading[t]) (x) aa_to_quat(base[t])) : base[t]      for every t < seq_len,
// where base[t] = base_orient[t], a constant, outside the existing range.  The poses outside the range are constants otherwise.
//
// Three passes: (0) row e is assembled by thread e mod nthreads, the world_dheading gradient of a frame OUTSIDE the range by thread t mod nthreads;
// (1) traj_global_bwd on the assembled rows (its world_dheading arguments take the step inside the range); (2) the row gradients are
// dealt to the variables of stage->var_mask: d h_e = gA[10] cos h_e - gA[9] sin h_e is the heading's.  Every sum is one of traj_global_bwd's
// scans.  accumulate: the values are ADDED to the gradient array and an entry that receives nothing is not touched; otherwise they are
// stored and everything else of the person's block is stored as zero.  Empty and frozen slots read nothing (store mode: their block is zeroed).
#pragma once
#include "traj_global_bwd.hpp"
#include "../../include/glamr_hip.h"

namespace glamr {

constexpr int GPB_WS_FLOATS_PER_FRAME = 11 + 11 + TGB_WS_FLOATS_PER_FRAME + 1;      // A, gA, traj_global_bwd's four, g_world_dheading

struct PoseBwdBatch {      // what the VJP reads of glamr_scene_batch + glamr_stage_desc + the call; the pointers are the batch's own
  int P, T;
  unsigned var_mask, flags;
  int accumulate;
  const int32_t *n_persons, *seq_len, *fr_start, *fr_end, *frozen;
  const float *prior, *dmask, *base_orient, *params;
  const float *g_orient, *g_trans;
  float* grads;
  float* ws;
};

inline PoseBwdBatch pose_bwd_batch(const glamr_scene_batch& b, const glamr_stage_desc& st, const float* g_orient, const float* g_trans, float* grads, int accumulate, float* ws) {
  return PoseBwdBatch{b.max_persons, b.max_len, st.var_mask, st.flags, accumulate, b.n_persons, b.seq_len, b.fr_start, b.fr_end, b.frozen,
                      b.traj_local_pred, b.dheading_mask, b.base_orient, b.params, g_orient, g_trans, grads, ws};
}

GLAMR_HD int gpb_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// store mode: the scene's camera block (the floats before the first person's) is zero; thread i mod nthreads stores element i
template <class RT>
GLAMR_HD void grecon_pose_bwd_clear(RT& rt, float* g, int count) {
  for (int i = rt.tid(); i < count; i += rt.nthreads()) g[i] = 0.0f;
}

template <class RT>
GLAMR_HD void grecon_pose_bwd(RT& rt, const PoseBwdBatch& b, const glamr_param_layout& l, int slot) {
  const int tid = rt.tid(), nt = rt.nthreads(), T = b.T;
  const int si = slot / b.P, pi = slot - si * b.P;
  const size_t block = (size_t)si * l.scene_stride + l.person0 + (size_t)pi * l.person_stride;
  float* g = b.grads + block;
  const bool acc = b.accumulate != 0;
  if (pi >= b.n_persons[si] || (b.frozen && b.frozen[slot] != 0)) {      // uniform over the workgroup
    if (!acc) grecon_pose_bwd_clear(rt, g, l.person_stride);
    return;
  }
  const int seq = gpb_clamp(b.seq_len[si], 0, T);
  const int fe = gpb_clamp(b.fr_end[slot], 0, seq), fs = gpb_clamp(b.fr_start[slot], 0, fe), n = fe - fs;
  const size_t frames = (size_t)slot * T;
  const float* p = b.params + block;
  const float* prior = b.prior + frames * 11;
  const float* dmask = b.dmask ? b.dmask + frames : nullptr;
  const float* g_orient = b.g_orient ? b.g_orient + frames * 3 : nullptr;
  const float* g_trans = b.g_trans ? b.g_trans + frames * 3 : nullptr;
  float* A = b.ws + frames * GPB_WS_FLOATS_PER_FRAME;
  float* gA = A + (size_t)T * 11;
  float* tgb = gA + (size_t)T * 11;
  float* gw = tgb + (size_t)T * TGB_WS_FLOATS_PER_FRAME;
  const bool wd = (b.flags & GLAMR_FLAG_HAS_WORLD_DHEADING) != 0 && g_orient != nullptr;

  // (0) the assembled rows; the world_dheading gradient of the frames whose base orientation is a constant
  for (int e = tid; e < n; e += nt) {
    const float* pr = prior + (size_t)e * 11;
    const bool first = e == 0;
    const int ixy = first ? l.local_xy : l.local_dxy + e * 2;
    const int ih = first ? l.local_heading : l.local_dheading + e;
    float* a = A + (size_t)e * 11;
    a[0] = pr[0] + p[ixy];
    a[1] = pr[1] + p[ixy + 1];
    a[2] = pr[2] + p[l.local_z + e];
    for (int k = 0; k < 6; ++k) a[3 + k] = pr[3 + k] + p[l.local_rot + e * 6 + k];
    const float hp = rm::atan2s(pr[10], pr[9]);
    const float h = hp + (first ? p[ih] : (dmask ? p[ih] * dmask[e] : 0.0f));
    float sn, cs;
    rm::sincos_(h, sn, cs);
    a[9] = cs; a[10] = sn;
  }
  for (int t = tid; t < T; t += nt) {
    float v = 0.0f;
    if (wd && t < seq && (t < fs || t >= fe)) {
      const float base[3] = {b.base_orient[(frames + t) * 3], b.base_orient[(frames + t) * 3 + 1], b.base_orient[(frames + t) * 3 + 2]};
      const float ga[3] = {g_orient[(size_t)t * 3], g_orient[(size_t)t * 3 + 1], g_orient[(size_t)t * 3 + 2]};
      v = world_dheading_bwd(base, p[l.world_dheading + t], ga, nullptr);
    }
    gw[t] = v;
  }
  rt.sync();

  // (1) assembled rows <- poses
  if (n > 0)
    traj_global_bwd(rt, n, T, A, g_trans ? g_trans + (size_t)fs * 3 : nullptr, g_orient ? g_orient + (size_t)fs * 3 : nullptr, nullptr, gA, tgb,
                    wd ? p + l.world_dheading + fs : nullptr, wd ? gw + fs : nullptr);
  rt.sync();

  // (2) variables <- assembled rows.  Index e is the row of the per-row variables and the video frame of world_dheading
  const unsigned vm = b.var_mask;
  auto put = [&](int i, float v, bool on) {
    if (acc) { if (on) g[i] += v; }
    else g[i] = on ? v : 0.0f;
  };
  for (int e = tid; e < T; e += nt) {
    const bool in = e < n;
    float r[11] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float gh = 0.0f;
    if (in) {
      for (int c = 0; c < 11; ++c) r[c] = gA[(size_t)e * 11 + c];
      gh = r[10] * A[(size_t)e * 11 + 9] - r[9] * A[(size_t)e * 11 + 10];
    }
    if (e == 0) {
      put(l.local_xy, r[0], in && (vm & GLAMR_VAR_LOCAL_XY));
      put(l.local_xy + 1, r[1], in && (vm & GLAMR_VAR_LOCAL_XY));
      put(l.local_heading, gh, in && (vm & GLAMR_VAR_LOCAL_HEADING));
      for (int i = l.local_heading + 1; i < l.local_dxy; ++i) put(i, 0.0f, false);      // (padding between the blocks)
      put(l.local_dxy, 0.0f, false);
      put(l.local_dxy + 1, 0.0f, false);
      put(l.local_dheading, 0.0f, false);
    } else {
      put(l.local_dxy + e * 2, r[0], in && (vm & GLAMR_VAR_LOCAL_DXY));
      put(l.local_dxy + e * 2 + 1, r[1], in && (vm & GLAMR_VAR_LOCAL_DXY));
      const bool on = in && dmask && (vm & GLAMR_VAR_LOCAL_DHEADING);
      put(l.local_dheading + e, on ? gh * dmask[e] : 0.0f, on);
    }
    put(l.local_z + e, r[2], in && (vm & GLAMR_VAR_LOCAL_Z));
    for (int k = 0; k < 6; ++k) put(l.local_rot + e * 6 + k, r[3 + k], in && (vm & GLAMR_VAR_LOCAL_ROT));
    put(l.world_dheading + e, gw[e], wd && e < seq && (vm & GLAMR_VAR_WORLD_DHEADING));
  }
}

}  // namespace glamr
