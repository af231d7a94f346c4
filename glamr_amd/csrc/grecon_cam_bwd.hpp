// Vector-Jacobian product from the world-to-camera transforms a stage launch reports (cam_pose) back to what the stage optimises, for ONE
// scene -- the link a caller-defined loss term that sees the camera needs.  Written against the block runtime like
// grecon_pose_bwd.hpp: DeviceRT on the device (grecon_cam_bwd.hip), the host runtime of tests/hostsim on the CPU.
//
// The function differentiated is the camera block of forward (global_recon_model.py:473-508), one case per camera mode of the stage
// (camera_mode of grecon_algo.hpp), evaluated at the parameters and poses the last launch left in the batch:
//   GCB_PER_FRAME   cam_pose[t] = [rot6d_to_rotmat(cam_rot6d[t]) | cam_trans[t]]                                          t < seq_len
//   GCB_FIXED       the same with row 0 for every frame: the nine gradients are sums over t < seq_len (thread-strided partial sums in frame
//                   order, then ONE block reduction of all nine)
//   GCB_DERIVED     n[t] = persons with vis != 0, src[t] = nearest frame <= t with n > 0 (the first such frame before it),
//                   avg = sum_visible [aa_to_rotmat_k(orient_world[src]) | trans_world[src]] . person2cam[src] / n[src],
//                   r6 = avg's first two columns (+ cam_inv_rot_res[t] where n[t] == 0),
//                   cam_pose[t] = invert([rot6d_to_rotmat(r6) | avg_t + cam_inv_trans_res[t]])
// Derived mode, three passes: (A) n[t]; (B) frame t: the averaged transform of its source again, the gradient of the residuals, and the
// gradient of the average into the workspace; (C) a source frame t sums the average's gradient over the contiguous run of frames it feeds, in
// frame order (the leading person-less frames first when t is the first source), and sends it through mul34_bwd and aa_to_rotmat_k_bwd to the
// pose gradients of its visible persons.  Only thread t mod nthreads touches frame t's pose gradients: no atomics.
//
// accumulate: the values are ADDED to the gradient array and an entry that receives nothing is not touched; otherwise they are stored and
// every other entry of the scene's gradient is stored as zero.  The pose gradients are added into in both settings.  Empty and frozen slots
// count as absent: nothing of theirs is read.
//
// invert34_bwd, mul34, mul34_bwd and get_R are grecon_algo.hpp's own, INCLUDED: nothing of that header moved or changed.
#pragma once
#include "grecon_algo.hpp"

namespace glamr {

constexpr int GCB_WS_FLOATS_PER_FRAME = 1 + 12;      // n[t] (as int), the gradient of the averaged transform
enum { GCB_DERIVED = 0, GCB_PER_FRAME = 1, GCB_FIXED = 2, GCB_CONSTANT = 3 };      // camera_mode's values

struct CamBwdBatch {       // what the VJP reads of glamr_scene_batch + the call; the pointers are the batch's own
  int P, T;
  int accumulate;
  const int32_t *n_persons, *seq_len, *frozen;
  const float *vis, *person2cam, *orient_world, *trans_world, *params;
  const float* g_cam;
  float* grads;
  float *g_orient, *g_trans;
  float* ws;
};

inline CamBwdBatch cam_bwd_batch(const glamr_scene_batch& b, const float* g_cam, float* grads, int accumulate, float* g_orient, float* g_trans, float* ws) {
  return CamBwdBatch{b.max_persons, b.max_len, accumulate, b.n_persons, b.seq_len, b.frozen, b.vis, b.person2cam, b.orient_world, b.trans_world, b.params,
                     g_cam, grads, g_orient, g_trans, ws};
}

GLAMR_HD int gcb_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// gradient of [rot6d_to_rotmat(r6) | t] with respect to r6, and the fourth column
GLAMR_HD void gcb_rot6d_trans_bwd(const float* r6, const float* G, float g6[6], float gt[3]) {
  float gR[9];
  GLAMR_GRECON_NS::get_R(G, gR);
  const float d6[6] = {r6[0], r6[1], r6[2], r6[3], r6[4], r6[5]};
  for (int k = 0; k < 6; ++k) g6[k] = 0.0f;
  rm::rot6d_to_rotmat_bwd(d6, gR, g6);
  for (int k = 0; k < 3; ++k) gt[k] = G[k * 4 + 3];
}

// [aa_to_rotmat_k(orient) | trans]: make_transform(..., 'axis_angle')
GLAMR_HD void gcb_pose_transform(const float* orient, const float* trans, float Tw[12]) {
  const float aa[3] = {orient[0], orient[1], orient[2]};
  float R[9];
  rm::aa_to_rotmat_k(aa, R);
  for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Tw[i * 4 + j] = R[i * 3 + j]; Tw[i * 4 + 3] = trans[i]; }
}

template <int MODE, class RT>
GLAMR_HD void grecon_cam_bwd(RT& rt, const CamBwdBatch& b, const glamr_param_layout& l, int si) {
  using namespace GLAMR_GRECON_NS;
  const int tid = rt.tid(), nt = rt.nthreads(), T = b.T, P = b.P;
  float* g = b.grads + (size_t)si * l.scene_stride;
  const float* p = b.params + (size_t)si * l.scene_stride;
  const float* G = b.g_cam + (size_t)si * T * 12;
  const bool acc = b.accumulate != 0;
  const int seq = gcb_clamp(b.seq_len[si], 0, T);
  // the two blocks of the mode are neighbours: [lo, lo + 9 T)
  const int lo = MODE == GCB_DERIVED ? l.cam_inv_rot_res : l.cam_rot6d;
  const int i6 = lo, i3 = lo + 6 * T;
  if (!acc)       // store mode: everything else of the scene; thread i mod nthreads stores element i
    for (int i = tid; i < l.scene_stride; i += nt)
      if (i < lo || i >= lo + 9 * T) g[i] = 0.0f;
  auto put = [&](int i, float v, bool on) {
    if (acc) { if (on) g[i] += v; }
    else g[i] = on ? v : 0.0f;
  };

  if (MODE == GCB_PER_FRAME) {
    for (int t = tid; t < T; t += nt) {
      const bool on = t < seq;
      float g6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gt[3] = {0.f, 0.f, 0.f};
      if (on) gcb_rot6d_trans_bwd(p + l.cam_rot6d + t * 6, G + (size_t)t * 12, g6, gt);
      for (int k = 0; k < 6; ++k) put(i6 + t * 6 + k, g6[k], on);
      for (int k = 0; k < 3; ++k) put(i3 + t * 3 + k, gt[k], on);
    }
  } else if (MODE == GCB_FIXED) {
    float s[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t = tid; t < seq; t += nt) {
      float g6[6], gt[3];
      gcb_rot6d_trans_bwd(p + l.cam_rot6d, G + (size_t)t * 12, g6, gt);
      for (int k = 0; k < 6; ++k) s[k] += g6[k];
      for (int k = 0; k < 3; ++k) s[6 + k] += gt[k];
    }
    rt.reduce_sum_n(s);
    // one lane per parameter; selects, not an indexed read of the register array
    for (int k = tid; k < 9; k += nt) {
      float gk = s[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int q = 1; q < 9; ++q) gk = (k == q) ? s[q] : gk;
      put(k < 6 ? i6 + k : i3 + (k - 6), gk, true);
    }
    if (!acc)
      for (int i = tid; i < 9 * T; i += nt)
        if (!(i < 6 || (i >= 6 * T && i < 6 * T + 3))) g[lo + i] = 0.0f;
  } else {
    int* nv = reinterpret_cast<int*>(b.ws + (size_t)si * T * GCB_WS_FLOATS_PER_FRAME);
    float* gavg = b.ws + (size_t)si * T * GCB_WS_FLOATS_PER_FRAME + T;
    const int np = gcb_clamp(b.n_persons[si], 0, P);
    auto live = [&](int q) { return !(b.frozen && b.frozen[si * P + q] != 0); };
    auto frame = [&](int q, int t) { return ((size_t)si * P + q) * T + t; };
    // (A) persons visible at every frame
    for (int t = tid; t < seq; t += nt) {
      int n = 0;
      for (int q = 0; q < np; ++q) if (live(q) && b.vis[frame(q, t)] != 0.f) ++n;
      nv[t] = n;
    }
    rt.sync();
    // (B) residuals <- camera; gradient of the averaged transform
    for (int t = tid; t < T; t += nt) {
      int src = t < seq ? t : -1;
      while (src >= 0 && nv[src] == 0) --src;
      if (src < 0 && t < seq) { src = 0; while (src < seq - 1 && nv[src] == 0) ++src; }
      const int ns = src >= 0 ? nv[src] : 0;
      const bool on = ns > 0;      // (a scene without a visible person has no camera: nothing)
      float g6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gt[3] = {0.f, 0.f, 0.f};
      bool empty = false;
      if (on) {
        float avg[12];
        for (int k = 0; k < 12; ++k) avg[k] = 0.f;
        for (int q = 0; q < np; ++q) {
          if (!live(q) || b.vis[frame(q, src)] == 0.f) continue;
          float Tw[12], C[12];
          gcb_pose_transform(b.orient_world + frame(q, src) * 3, b.trans_world + frame(q, src) * 3, Tw);
          mul34(Tw, b.person2cam + frame(q, src) * 12, C);
          for (int k = 0; k < 12; ++k) avg[k] += C[k];
        }
        const float inv_n = 1.0f / (float)ns;
        for (int k = 0; k < 12; ++k) avg[k] *= inv_n;
        empty = nv[t] == 0;
        float r6[6];
        for (int r = 0; r < 3; ++r) { r6[r] = avg[r * 4 + 0]; r6[3 + r] = avg[r * 4 + 1]; }
        if (empty) for (int k = 0; k < 6; ++k) r6[k] += p[l.cam_inv_rot_res + t * 6 + k];
        float R[9], Mi[12], gMi[12];
        rm::rot6d_to_rotmat(r6, R);
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Mi[i * 4 + j] = R[i * 3 + j]; Mi[i * 4 + 3] = avg[i * 4 + 3] + p[l.cam_inv_trans_res + t * 3 + i]; }
        for (int k = 0; k < 12; ++k) gMi[k] = 0.f;
        invert34_bwd(Mi, G + (size_t)t * 12, gMi);      // cam_pose = invert(cam_inv)
        gcb_rot6d_trans_bwd(r6, gMi, g6, gt);
        float* ga = gavg + (size_t)t * 12;
        for (int r = 0; r < 3; ++r) { ga[r * 4 + 0] = g6[r]; ga[r * 4 + 1] = g6[3 + r]; ga[r * 4 + 2] = 0.f; ga[r * 4 + 3] = gt[r]; }
      }
      for (int k = 0; k < 6; ++k) put(i6 + t * 6 + k, g6[k], on && empty);
      for (int k = 0; k < 3; ++k) put(i3 + t * 3 + k, gt[k], on);
    }
    rt.sync();
    // (C) poses <- averaged transform: a source frame takes the run of frames it feeds, in frame order
    for (int t = tid; t < seq; t += nt) {
      const int ns = nv[t];
      if (ns == 0) continue;
      float ga[12];
      for (int k = 0; k < 12; ++k) ga[k] = 0.f;
      int u = t - 1;
      while (u >= 0 && nv[u] == 0) --u;
      if (u < 0)                                    // the first source: the leading person-less frames are its own
        for (u = 0; u < t; ++u) for (int k = 0; k < 12; ++k) ga[k] += gavg[(size_t)u * 12 + k];
      u = t;
      do { for (int k = 0; k < 12; ++k) ga[k] += gavg[(size_t)u * 12 + k]; ++u; } while (u < seq && nv[u] == 0);
      const float inv_n = 1.0f / (float)ns;
      for (int k = 0; k < 12; ++k) ga[k] *= inv_n;
      for (int q = 0; q < np; ++q) {
        if (!live(q) || b.vis[frame(q, t)] == 0.f) continue;
        const float* ow = b.orient_world + frame(q, t) * 3;
        float Tw[12], gTw[12], gR[9];
        gcb_pose_transform(ow, b.trans_world + frame(q, t) * 3, Tw);
        for (int k = 0; k < 12; ++k) gTw[k] = 0.f;
        mul34_bwd(Tw, b.person2cam + frame(q, t) * 12, ga, gTw, nullptr);
        get_R(gTw, gR);
        const float aa[3] = {ow[0], ow[1], ow[2]};
        float gaa[3] = {0.f, 0.f, 0.f};
        rm::aa_to_rotmat_k_bwd(aa, gR, gaa);
        for (int k = 0; k < 3; ++k) { b.g_orient[frame(q, t) * 3 + k] += gaa[k]; b.g_trans[frame(q, t) * 3 + k] += gTw[k * 4 + 3]; }
      }
    }
  }
}

}  // namespace glamr
