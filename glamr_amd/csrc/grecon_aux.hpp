// The six loss_cfg terms of the reference the fused stage kernel does not hold, values and adjoints together, for ONE scene.
// Written against the block runtime like grecon_cam_bwd.hpp: DeviceRT on the device (grecon_aux.hip), the host runtime of tests/hostsim on
// the CPU.  Everything is evaluated at what the stage's gradient launch left in the batch: params, trans_world and cam_pose = [R_t | c_t].
//
// With T = the scene's seq_len, persons q < n_persons, a slot's existing frames [fr_start, fr_end), n = fr_end - fr_start (loss_func.py):
//   0 cam_rot_smoothness      :60-65    mean_{t < T-1} sum_6 (30 (r[t] - r[t+1]))^2 on the raw cam_rot6d rows of params   -> grads, cam_rot6d rows
//   1 cam_trans_smoothness    :68-73    the same on the cam_trans rows (3 per frame)                                     -> grads, cam_trans rows
//   2 cam_depth_smoothness    :94-103   o_t = -R_t^T c_t, z_t = third row of R_t, d_t = 30 (o_t - o_{t+1}) . z_{t+1};
//                                       SUM_{t < T-1} d_t^2 (the reference's mean is taken of a scalar)                  -> g_cam_pose
//   3 traj_trans_smoothness   :135-144  sum_q sum_{t < T-1} |30 (x_q[t+1] - x_q[t])|^2 / (n_persons (T - 1)), every frame -> g_trans_world
//   4 cam_traj_trans          :175-186  frames with vis != 0: diff = R_t x_q[t] + c_t - root_trans_cam_q[t], the person's first visible
//                                       frame times first_frame_weight; sum diff^2 / sum_q n_vis_q                       -> g_trans_world, g_cam_pose
//   5 local_traj_dheading_reg :216-217  sum_q sum_{e=1..n-1} (30 dh_q[e])^2 / sum_q (n_q - 1) on local_dheading itself    -> grads, when in var_mask
// With a fixed camera every row of 0 and 1 is row 0: the value is exactly 0 and nothing is written.  A zero denominator (T == 1, nobody
// visible, every n == 1) is NaN in the reference; here the value is 0 and there is no gradient -- the one deliberate deviation.
//
// Passes: (zero fill in store mode) | (A, term 4 only) thread q finds person q's first visible frame into the workspace, the visible frames
// are counted (one block sum) | (B) thread t mod nthreads owns frame t: its row of every term, the adjoints of ITS rows of g_cam_pose,
// g_trans_world and the camera blocks of grads (a difference term is evaluated for both neighbours of the frame, so no thread writes another's
// row); terms 0 and 1 in a frame loop of their own (with both loops' pointers live the kernel spilled scalar registers) | (C) row e of
// local_dheading likewise | one block sum of the six partial values.  No atomics, fixed order: two calls give the same bits.
//
// accumulate: adjoints are ADDED and nothing else is touched; otherwise every given output array is zero-filled for the scene first (all of
// grads' scene, all slots and frames of g_trans_world, all frames of g_cam_pose).  Monitor-only terms give their value alone.  Never read: rows
// at or beyond seq_len, empty slots, parameter blocks of inactive terms, root_trans_cam and (without terms 2 / 3) cam_pose / trans_world at
// frames where no person / the person is not visible.
#pragma once
#include "grecon_algo.hpp"

namespace glamr {

enum { GAUX_DERIVED = 0, GAUX_PER_FRAME = 1, GAUX_FIXED = 2, GAUX_CONSTANT = 3 };      // camera_mode's values
constexpr int GAUX_N = GLAMR_AUX_NUM_TERMS;
constexpr uint32_t GAUX_ALL = (1u << GAUX_N) - 1u;
constexpr uint32_t GAUX_ON_PARAMS = (1u << GLAMR_AUX_CAM_ROT_SMOOTHNESS) | (1u << GLAMR_AUX_CAM_TRANS_SMOOTHNESS) | (1u << GLAMR_AUX_LOCAL_TRAJ_DHEADING_REG);
constexpr uint32_t GAUX_ON_TRANS = (1u << GLAMR_AUX_TRAJ_TRANS_SMOOTHNESS) | (1u << GLAMR_AUX_CAM_TRAJ_TRANS);
constexpr uint32_t GAUX_ON_CAM = (1u << GLAMR_AUX_CAM_DEPTH_SMOOTHNESS) | (1u << GLAMR_AUX_CAM_TRAJ_TRANS);

struct AuxBatch {       // what the call reads of glamr_scene_batch, the stage and the term descriptor; the pointers are the caller's own
  int P, T;
  int accumulate, cam_mode;
  uint32_t var_mask, mask, grad_mask;      // terms evaluated / terms that give a gradient
  float weight[GAUX_N], first_frame_weight;
  const int32_t *n_persons, *seq_len, *fr_start, *fr_end;
  const float *vis, *trans_world, *cam_pose, *params, *root_trans_cam;
  float *values, *g_trans, *g_cam, *grads;
  int32_t* ws;      // first visible frame per slot
};

// The argument checks of glamr_grecon_aux_terms (the entry point and the host build share them): 0 or a GLAMR_E_* code and its message.
inline int aux_check(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const glamr_aux_desc* aux, const float* root_trans_cam, const float* values,
                     const float* g_trans_world, const float* g_cam_pose, const float* grads, const void* workspace, const char** msg) {
#define GAUX_FAIL(code, text) do { *msg = text; return code; } while (0)
  if (!batch || !stage || !aux || !values || !workspace) GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: NULL argument (batch, stage, aux, values, workspace)");
  if (!(batch->n_scenes >= 0 && batch->max_persons >= 1 && batch->max_persons <= 32 && batch->max_len >= 1))
    GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: bad batch geometry (n_scenes >= 0, 1 <= max_persons <= 32, max_len >= 1)");
  if (!((int64_t)batch->max_len * 12 * batch->max_persons < 0x7fffffff)) GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: sequence too long");
  if (aux->loss_mask & ~GAUX_ALL) GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: loss_mask has bits beyond GLAMR_AUX_NUM_TERMS");
  if (batch->frozen) GAUX_FAIL(GLAMR_E_UNSUPPORTED, "glamr_grecon_aux_terms: person-sharded batches (batch->frozen) are not supported: a rank would see its own persons only");
  const uint32_t mask = aux->loss_mask, gm = mask & ~aux->monitor_mask;
  const int mode = GLAMR_GRECON_NS::camera_mode(*stage);
  if ((mask & ((1u << GLAMR_AUX_CAM_ROT_SMOOTHNESS) | (1u << GLAMR_AUX_CAM_TRANS_SMOOTHNESS))) && !(stage->var_mask & GLAMR_VAR_CAM))
    GAUX_FAIL(GLAMR_E_UNSUPPORTED, "glamr_grecon_aux_terms: cam_rot_smoothness / cam_trans_smoothness in a stage that does not optimise the camera (GLAMR_VAR_CAM): "
                                   "the cam_rot6d / cam_trans rows of params are not the stage's variables");
  if (batch->n_scenes == 0) return GLAMR_OK;
  if (!(batch->seq_len && batch->n_persons)) GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: NULL batch array (seq_len, n_persons)");
  if ((mask & GAUX_ON_PARAMS) && !batch->params) GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: NULL batch array (params)");
  if ((mask & (1u << GLAMR_AUX_LOCAL_TRAJ_DHEADING_REG)) && !(batch->fr_start && batch->fr_end)) GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: NULL batch array (fr_start, fr_end)");
  if ((mask & GAUX_ON_TRANS) && !batch->trans_world) GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: NULL batch array (trans_world)");
  if ((mask & GAUX_ON_CAM) && !batch->cam_pose) GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: NULL batch array (cam_pose)");
  if ((mask & (1u << GLAMR_AUX_CAM_TRAJ_TRANS)) && !(batch->vis && root_trans_cam)) GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: cam_traj_trans needs batch->vis and root_trans_cam");
  if ((gm & GAUX_ON_PARAMS) && !grads) GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: grads is required by a term on the variables that is not monitor-only");
  if ((gm & GAUX_ON_TRANS) && !g_trans_world) GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: g_trans_world is required by traj_trans_smoothness / cam_traj_trans");
  if ((gm & GAUX_ON_CAM) && mode != GAUX_CONSTANT && !g_cam_pose)
    GAUX_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_terms: g_cam_pose is required by cam_depth_smoothness / cam_traj_trans unless the camera is a constant of the stage");
#undef GAUX_FAIL
  return GLAMR_OK;
}

inline AuxBatch aux_batch(const glamr_scene_batch& b, const glamr_stage_desc& st, const glamr_aux_desc& d, const float* root_trans_cam, float* values,
                          float* g_trans_world, float* g_cam_pose, float* grads, int accumulate, void* workspace) {
  AuxBatch a{};
  a.P = b.max_persons; a.T = b.max_len; a.accumulate = accumulate; a.cam_mode = GLAMR_GRECON_NS::camera_mode(st);
  a.var_mask = st.var_mask; a.mask = d.loss_mask & GAUX_ALL; a.grad_mask = a.mask & ~d.monitor_mask;
  for (int k = 0; k < GAUX_N; ++k) a.weight[k] = d.weight[k];
  a.first_frame_weight = d.first_frame_weight;
  a.n_persons = b.n_persons; a.seq_len = b.seq_len; a.fr_start = b.fr_start; a.fr_end = b.fr_end;
  a.vis = b.vis; a.trans_world = b.trans_world; a.cam_pose = b.cam_pose; a.params = b.params; a.root_trans_cam = root_trans_cam;
  a.values = values; a.g_trans = g_trans_world; a.g_cam = g_cam_pose; a.grads = grads; a.ws = static_cast<int32_t*>(workspace);
  return a;
}

GLAMR_HD int gaux_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// camera origin in the world o = -R^T c of a world-to-camera row C = [R | c]
GLAMR_HD void gaux_origin(const float* C, float o[3]) {
  for (int i = 0; i < 3; ++i) o[i] = -(C[0 * 4 + i] * C[3] + C[1 * 4 + i] * C[7] + C[2 * 4 + i] * C[11]);
}

template <class RT>
GLAMR_HD void grecon_aux_terms(RT& rt, const AuxBatch& b, const glamr_param_layout& l, int si) {
  const int tid = rt.tid(), nt = rt.nthreads(), T = b.T, P = b.P;
  const bool acc = b.accumulate != 0;
  const int seq = gaux_clamp(b.seq_len[si], 0, T), np = gaux_clamp(b.n_persons[si], 0, P);
  auto on = [&](int k) { return (b.mask >> k & 1u) != 0; };
  auto live = [&](int k) { return (b.grad_mask >> k & 1u) != 0; };
  auto frame = [&](int q, int t) { return ((size_t)si * P + q) * T + t; };
  const bool cam_live = b.cam_mode != GAUX_CONSTANT && b.g_cam != nullptr;
  const bool per_frame = b.cam_mode == GAUX_PER_FRAME;
  float* g = b.grads ? b.grads + (size_t)si * l.scene_stride : nullptr;
  const float* p = b.params ? b.params + (size_t)si * l.scene_stride : nullptr;
  const float* C = b.cam_pose ? b.cam_pose + (size_t)si * T * 12 : nullptr;
  float* gC = b.g_cam ? b.g_cam + (size_t)si * T * 12 : nullptr;
  float* gX = b.g_trans ? b.g_trans + (size_t)si * P * T * 3 : nullptr;
  int32_t* first = b.ws + (size_t)si * P;

  if (!acc) {       // store mode: the scene's part of every given output; thread i mod nthreads stores element i
    if (g) for (int i = tid; i < l.scene_stride; i += nt) g[i] = 0.0f;
    if (gC) for (int i = tid; i < T * 12; i += nt) gC[i] = 0.0f;
    if (gX) for (int i = tid; i < P * T * 3; i += nt) gX[i] = 0.0f;
    rt.sync();
  }

  // (A) cam_traj_trans: the first visible frame of every person, the number of visible frames
  float n_vis = 0.0f;
  if (on(GLAMR_AUX_CAM_TRAJ_TRANS)) {
    for (int q = tid; q < np; q += nt) {
      int f = -1;
      for (int t0 = 0; t0 < seq && f < 0; t0 += 8)
        for (int k = 0; k < 8; ++k) { const int t = t0 + k; if (t < seq && f < 0 && b.vis[frame(q, t)] != 0.f) f = t; }
      first[q] = f;
    }
    for (int t = tid; t < seq; t += nt)
      for (int q = 0; q < np; ++q) if (b.vis[frame(q, t)] != 0.f) n_vis += 1.0f;
    n_vis = rt.reduce_sum(n_vis);
    rt.sync();
  }
  // denominators and the adjoints' common factors (0: no gradient)
  int n_dh = 0;
  if (on(GLAMR_AUX_LOCAL_TRAJ_DHEADING_REG))
    for (int q = 0; q < np; ++q) {
      const int n = gaux_clamp(b.fr_end[si * P + q], 0, T) - gaux_clamp(b.fr_start[si * P + q], 0, T);
      if (n > 1) n_dh += n - 1;
    }
  auto den = [&](int k) {
    return k == GLAMR_AUX_CAM_DEPTH_SMOOTHNESS ? 1.0f : k == GLAMR_AUX_TRAJ_TRANS_SMOOTHNESS ? (float)np * (float)(seq - 1) :
           k == GLAMR_AUX_CAM_TRAJ_TRANS ? n_vis : k == GLAMR_AUX_LOCAL_TRAJ_DHEADING_REG ? (float)n_dh : (float)(seq - 1);
  };
  const float sq = GLAMR_GRECON_NS::FPS * GLAMR_GRECON_NS::FPS;
  auto factor = [&](int k, float scale) { return live(k) && den(k) > 0.0f ? b.weight[k] * 2.0f * scale / den(k) : 0.0f; };
  const float c_rot = per_frame ? factor(GLAMR_AUX_CAM_ROT_SMOOTHNESS, sq) : 0.0f, c_tr = per_frame ? factor(GLAMR_AUX_CAM_TRANS_SMOOTHNESS, sq) : 0.0f;
  const float c_depth = factor(GLAMR_AUX_CAM_DEPTH_SMOOTHNESS, GLAMR_GRECON_NS::FPS), c_tt = factor(GLAMR_AUX_TRAJ_TRANS_SMOOTHNESS, sq);
  const float c_ct = factor(GLAMR_AUX_CAM_TRAJ_TRANS, 1.0f), c_dh = (b.var_mask & GLAMR_VAR_LOCAL_DHEADING) ? factor(GLAMR_AUX_LOCAL_TRAJ_DHEADING_REG, sq) : 0.0f;

  float s[GAUX_N];
  for (int k = 0; k < GAUX_N; ++k) s[k] = 0.0f;

  // (B) frame t: its row of every term, the adjoints of its own rows.  0, 1: differences of the raw variable rows (a fixed camera has one
  // row: exactly 0, nothing is read); a loop of their own -- the pointers of the two halves are never live together
  if (per_frame && (on(GLAMR_AUX_CAM_ROT_SMOOTHNESS) || on(GLAMR_AUX_CAM_TRANS_SMOOTHNESS)))
    for (int t = tid; t < seq; t += nt) {
      const bool has_next = t < seq - 1, has_prev = t > 0;
      for (int blk = 0; blk < 2; ++blk) {
        if (!on(blk)) continue;
        const int w = blk == 0 ? 6 : 3, base = (blk == 0 ? l.cam_rot6d : l.cam_trans) + t * w;
        const float c = blk == 0 ? c_rot : c_tr;
        for (int k = 0; k < w; ++k) {
          const float r = p[base + k];
          const float dn = has_next ? r - p[base + w + k] : 0.0f, dp = has_prev ? p[base - w + k] - r : 0.0f;
          s[blk] += sq * dn * dn;
          if (c != 0.0f) g[base + k] += c * (dn - dp);
        }
      }
    }
  for (int t = tid; t < seq; t += nt) {
    const bool has_next = t < seq - 1, has_prev = t > 0;
    float G[12];
    for (int k = 0; k < 12; ++k) G[k] = 0.0f;
    bool cam_written = false;
    // 2: the camera origin's step along the LATER frame's viewing axis
    if (on(GLAMR_AUX_CAM_DEPTH_SMOOTHNESS)) {
      const float* Ct = C + (size_t)t * 12;
      float o[3], go[3] = {0.f, 0.f, 0.f}, gz[3] = {0.f, 0.f, 0.f};
      gaux_origin(Ct, o);
      if (has_next) {
        const float* Cn = Ct + 12;
        float on_[3];
        gaux_origin(Cn, on_);
        const float d = GLAMR_GRECON_NS::FPS * ((o[0] - on_[0]) * Cn[8] + (o[1] - on_[1]) * Cn[9] + (o[2] - on_[2]) * Cn[10]);
        s[GLAMR_AUX_CAM_DEPTH_SMOOTHNESS] += d * d;
        for (int i = 0; i < 3; ++i) go[i] += c_depth * d * Cn[8 + i];
      }
      if (has_prev && c_depth != 0.0f) {
        float op[3];
        gaux_origin(Ct - 12, op);
        const float d = GLAMR_GRECON_NS::FPS * ((op[0] - o[0]) * Ct[8] + (op[1] - o[1]) * Ct[9] + (op[2] - o[2]) * Ct[10]);
        for (int i = 0; i < 3; ++i) { go[i] -= c_depth * d * Ct[8 + i]; gz[i] = c_depth * d * (op[i] - o[i]); }
      }
      if (c_depth != 0.0f && cam_live) {       // o = -R^T c: dR[j][i] = -c_j go_i, dc_j = -sum_i R[j][i] go_i; z is R's third row
        for (int j = 0; j < 3; ++j) {
          for (int i = 0; i < 3; ++i) G[j * 4 + i] -= Ct[j * 4 + 3] * go[i];
          G[j * 4 + 3] -= Ct[j * 4 + 0] * go[0] + Ct[j * 4 + 1] * go[1] + Ct[j * 4 + 2] * go[2];
        }
        for (int i = 0; i < 3; ++i) G[8 + i] += gz[i];
        cam_written = true;
      }
    }
    for (int q = 0; q < np; ++q) {
      const size_t f = frame(q, t);
      float gx[3] = {0.f, 0.f, 0.f};
      bool x_written = false;
      // 3: every frame of a present slot
      if (on(GLAMR_AUX_TRAJ_TRANS_SMOOTHNESS)) {
        const float* x = b.trans_world + f * 3;
        for (int k = 0; k < 3; ++k) {
          const float dn = has_next ? x[3 + k] - x[k] : 0.0f, dp = has_prev ? x[k] - x[k - 3] : 0.0f;
          s[GLAMR_AUX_TRAJ_TRANS_SMOOTHNESS] += sq * dn * dn;
          gx[k] += c_tt * (dp - dn);
        }
        x_written = c_tt != 0.0f;
      }
      // 4: the root in the camera against root_trans_cam, on visible frames
      if (on(GLAMR_AUX_CAM_TRAJ_TRANS) && b.vis[f] != 0.f) {
        const float* x = b.trans_world + f * 3;
        const float* Ct = C + (size_t)t * 12;
        const float fw = t == first[q] ? b.first_frame_weight : 1.0f;
        float gd[3];
        for (int i = 0; i < 3; ++i) {
          const float diff = fw * (Ct[i * 4 + 0] * x[0] + Ct[i * 4 + 1] * x[1] + Ct[i * 4 + 2] * x[2] + Ct[i * 4 + 3] - b.root_trans_cam[f * 3 + i]);
          s[GLAMR_AUX_CAM_TRAJ_TRANS] += diff * diff;
          gd[i] = c_ct * diff * fw;
        }
        if (c_ct != 0.0f) {
          for (int j = 0; j < 3; ++j) gx[j] += Ct[0 * 4 + j] * gd[0] + Ct[1 * 4 + j] * gd[1] + Ct[2 * 4 + j] * gd[2];
          x_written = true;
          if (cam_live) {
            for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) G[i * 4 + j] += gd[i] * x[j]; G[i * 4 + 3] += gd[i]; }
            cam_written = true;
          }
        }
      }
      if (x_written) for (int k = 0; k < 3; ++k) b.g_trans[f * 3 + k] += gx[k];      // (f counts from the batch's first slot)
    }
    if (cam_written) for (int k = 0; k < 12; ++k) gC[(size_t)t * 12 + k] += G[k];
  }

  // (C) 5: row e >= 1 of the heading increments themselves
  if (on(GLAMR_AUX_LOCAL_TRAJ_DHEADING_REG))
    for (int q = 0; q < np; ++q) {
      const int n = gaux_clamp(b.fr_end[si * P + q], 0, T) - gaux_clamp(b.fr_start[si * P + q], 0, T);
      const int base = l.person0 + q * l.person_stride + l.local_dheading;
      for (int e = 1 + tid; e < n; e += nt) {
        const float dh = p[base + e];
        s[GLAMR_AUX_LOCAL_TRAJ_DHEADING_REG] += sq * dh * dh;
        if (c_dh != 0.0f) g[base + e] += c_dh * dh;
      }
    }

  rt.reduce_sum_n(s);
  // one lane per term; selects, not an indexed read of the register arrays
  for (int k = tid; k < GAUX_N; k += nt) {
    float v = s[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 1; q < GAUX_N; ++q) v = (k == q) ? s[q] : v;
    const float d = den(k);
    b.values[(size_t)si * GAUX_N + k] = (on(k) && d > 0.0f) ? v / d : 0.0f;
  }
}

}  // namespace glamr
