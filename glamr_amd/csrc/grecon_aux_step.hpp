// One Adam iteration's tail for ONE scene when the stage lists terms of glamr_grecon_aux_terms and nothing else the stage kernel lacks
// (DESIGN.md 20): the three stand-alone algorithms of grecon_aux.hpp, grecon_cam_bwd.hpp and grecon_pose_bwd.hpp, INCLUDED and called in
// turn on scratch adjoints in the workspace, then torch.optim.Adam's step on the scene's row.  Written against the block runtime like the
// three: DeviceRT on the device (grecon_aux_step.hip), the host runtime of tests/hostsim on the CPU.
//
// Phases of a scene, a workgroup barrier between two that read what other threads wrote:
//   (1) the scene's scratch adjoints are zeroed: g_trans_world (P T 3), g_orient_world (P T 3, camera derived from the persons only),
//       g_cam_pose (T 12, unless the camera is a constant of the stage)
//   (2) grecon_aux_terms in add mode: adjoints into the scratch arrays and into `grads`, the six unweighted values into the workspace, from
//       where the lane that wrote value k copies it to values[scene, iteration, k]
//   (3) grecon_cam_bwd<MODE> on the scratch g_cam_pose, accumulating, when a term outside the monitor mask writes to it (derived: it adds
//       into the scratch pose adjoints)
//   (4) grecon_pose_bwd on slot scene P + p for p < n_persons[scene], accumulating, when a pose adjoint is live
//   (5) GLAMR_GRECON_NS::adam on element i mod nthreads of the scene's row of params / exp_avg / exp_avg_sq, coefficients by value
// `grads` comes in holding the stage kernel's gradient and goes out holding the iteration's complete gradient; it is not cleared.
// (3) and (4) run on exactly the condition extra_loss_schedule.ExtraLossSchedule launches them on, so a schedule whose terms are all
// monitor-only leaves `grads` untouched.  No atomics, the three algorithms' fixed orders of additions: two calls give the same bits.
#pragma once
#include "grecon_aux.hpp"
#include "grecon_cam_bwd.hpp"
#include "grecon_pose_bwd.hpp"

namespace glamr {

static_assert((int)GAUX_DERIVED == (int)GCB_DERIVED && (int)GAUX_PER_FRAME == (int)GCB_PER_FRAME && (int)GAUX_FIXED == (int)GCB_FIXED &&
              (int)GAUX_CONSTANT == (int)GCB_CONSTANT, "one camera_mode for both headers");

struct AuxStepBatch {
  AuxBatch aux;            // accumulate = 1; values -> the workspace's (n_scenes, 6); g_trans / g_cam -> the scratch adjoints
  CamBwdBatch cam;         // accumulate = 1; g_cam = the scratch; g_orient / g_trans = the scratch pose adjoints
  PoseBwdBatch pose;       // accumulate = 1; g_orient / g_trans = the scratch pose adjoints that are live, else NULL
  int run_cam, run_pose;   // phases (3) / (4) run at all
  float *g_orient, *g_trans, *g_cam;      // the scratch adjoints, whole batch
  float *params, *exp_avg, *exp_avg_sq, *grads;
  float* values;           // (n_scenes, values_stride): the six values of this call at [scene][6 * iteration ...]
  int values_stride, iteration;
  GLAMR_GRECON_NS::AdamCoef coef;
};

// The workspace, in floats: the scratch adjoints, the call's six values per scene, then the three algorithms' own workspaces
struct AuxStepWorkspace {
  size_t g_trans, g_orient, g_cam, vals, aux, cam, pose, total;
};
inline AuxStepWorkspace aux_step_workspace(int S, int P, int T) {
  AuxStepWorkspace w{};
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 3) & ~(size_t)3; return at; };      // every array 16-byte aligned
  w.g_trans = take((size_t)S * P * T * 3);
  w.g_orient = take((size_t)S * P * T * 3);
  w.g_cam = take((size_t)S * T * 12);
  w.vals = take((size_t)S * GAUX_N);
  w.aux = take((size_t)S * P);
  w.cam = take((size_t)S * T * GCB_WS_FLOATS_PER_FRAME);
  w.pose = take((size_t)S * P * T * GPB_WS_FLOATS_PER_FRAME);
  w.total = o;
  return w;
}

// torch/optim/adam.py's scalars of the 1-based `step`, as glamr_adam_step forms them (host: libm pow in double, IEEE division)
inline GLAMR_GRECON_NS::AdamCoef aux_step_coef(double lr, int step) {
  float tab[2];
  GLAMR_GRECON_NS::adam_coef_host(lr, step, tab);
  GLAMR_GRECON_NS::AdamCoef c{tab[0], tab[1], 0.0f};
  c.inv_bc2_sqrt = 1.0f / tab[1];
  return c;
}

// The argument checks of glamr_grecon_aux_step (the entry point and the host build share them): aux_check's on the scratch adjoints, the two
// VJPs' geometry limits and refusals, the step's own.  0 or a GLAMR_E_* code and its message.
inline int aux_step_check(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const glamr_aux_desc* aux, const float* root_trans_cam, const float* values,
                          int values_stride, int iteration, const float* grads, const float* exp_avg, const float* exp_avg_sq, double lr, int step,
                          const void* workspace, const char** msg) {
#define GAS_FAIL(code, text) do { *msg = text; return code; } while (0)
  if (!batch || !stage || !aux || !values || !grads || !exp_avg || !exp_avg_sq || !workspace)
    GAS_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_step: NULL argument (batch, stage, aux, values, grads, exp_avg, exp_avg_sq, workspace)");
  if (!(batch->n_scenes >= 0 && batch->max_persons >= 1 && batch->max_persons <= 32 && batch->max_len >= 2))
    GAS_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_step: bad batch geometry (n_scenes >= 0, 1 <= max_persons <= 32, max_len >= 2)");
  if (!((int64_t)batch->n_scenes * batch->max_persons < 0x7fffffff)) GAS_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_step: too many person slots");
  if (!(step >= 1 && lr > 0.0)) GAS_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_step: step must be >= 1 (1-based, as torch counts) and lr > 0");
  if (!(iteration >= 0 && (int64_t)values_stride >= ((int64_t)iteration + 1) * GAUX_N))
    GAS_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_step: iteration >= 0 and values_stride >= 6 (iteration + 1) are required");
  const float* scratch = static_cast<const float*>(workspace);
  if (const int rc = aux_check(batch, stage, aux, root_trans_cam, values, scratch, scratch, grads, workspace, msg)) return rc;      // (sequence too long, frozen, ...)
  if (stage->flags & GLAMR_FLAG_ABSOLUTE_HEADING)
    GAS_FAIL(GLAMR_E_UNSUPPORTED, "glamr_grecon_aux_step: GLAMR_FLAG_ABSOLUTE_HEADING is not supported (glamr_grecon_pose_backward differentiates heading increments)");
  if (batch->n_scenes == 0) return GLAMR_OK;
  if (!batch->params) GAS_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_step: NULL batch array (params)");
  const uint32_t gm = aux->loss_mask & ~aux->monitor_mask & GAUX_ALL;
  const int mode = GLAMR_GRECON_NS::camera_mode(*stage);
  const bool run_cam = (gm & GAUX_ON_CAM) && mode != GAUX_CONSTANT, derived = run_cam && mode == GAUX_DERIVED;
  if (derived && !(batch->vis && batch->person2cam && batch->orient_world && batch->trans_world))
    GAS_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_step: NULL batch array (vis, person2cam, orient_world, trans_world)");
  if (((gm & GAUX_ON_TRANS) || derived) && !(batch->fr_start && batch->fr_end && batch->traj_local_pred))
    GAS_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_step: NULL batch array (fr_start, fr_end, traj_local_pred)");
  if (derived && (stage->flags & GLAMR_FLAG_HAS_WORLD_DHEADING) && !batch->base_orient)
    GAS_FAIL(GLAMR_E_INVALID, "glamr_grecon_aux_step: NULL base_orient with GLAMR_FLAG_HAS_WORLD_DHEADING");
#undef GAS_FAIL
  return GLAMR_OK;
}

inline AuxStepBatch aux_step_batch(const glamr_scene_batch& b, const glamr_stage_desc& st, const glamr_aux_desc& d, const float* root_trans_cam, float* values,
                                   int values_stride, int iteration, float* grads, float* exp_avg, float* exp_avg_sq, double lr, int step, void* workspace) {
  const AuxStepWorkspace w = aux_step_workspace(b.n_scenes, b.max_persons, b.max_len);
  float* ws = static_cast<float*>(workspace);
  AuxStepBatch s{};
  s.g_trans = ws + w.g_trans; s.g_orient = ws + w.g_orient; s.g_cam = ws + w.g_cam;
  s.aux = aux_batch(b, st, d, root_trans_cam, ws + w.vals, s.g_trans, s.g_cam, grads, 1, ws + w.aux);
  const bool trans_live = (s.aux.grad_mask & GAUX_ON_TRANS) != 0;
  s.run_cam = (s.aux.grad_mask & GAUX_ON_CAM) != 0 && s.aux.cam_mode != GAUX_CONSTANT;
  const bool derived = s.run_cam && s.aux.cam_mode == GAUX_DERIVED;
  s.run_pose = trans_live || derived;
  s.cam = cam_bwd_batch(b, s.g_cam, grads, 1, derived ? s.g_orient : nullptr, derived ? s.g_trans : nullptr, ws + w.cam);
  s.pose = pose_bwd_batch(b, st, derived ? s.g_orient : nullptr, s.run_pose ? s.g_trans : nullptr, grads, 1, ws + w.pose);
  s.params = b.params; s.exp_avg = exp_avg; s.exp_avg_sq = exp_avg_sq; s.grads = grads;
  s.values = values; s.values_stride = values_stride; s.iteration = iteration;
  s.coef = aux_step_coef(lr, step);
  return s;
}

template <int MODE, class RT>
GLAMR_HD void grecon_aux_step(RT& rt, const AuxStepBatch& s, const glamr_param_layout& l, int si) {
  const int tid = rt.tid(), nt = rt.nthreads(), P = s.aux.P, T = s.aux.T;
  // (1) the scene's scratch adjoints; thread i mod nthreads stores element i
  {
    float* gX = s.g_trans + (size_t)si * P * T * 3;
    for (int i = tid; i < P * T * 3; i += nt) gX[i] = 0.0f;
    if (MODE == GAUX_DERIVED) {
      float* gO = s.g_orient + (size_t)si * P * T * 3;
      for (int i = tid; i < P * T * 3; i += nt) gO[i] = 0.0f;
    }
    if (MODE != GAUX_CONSTANT) {
      float* gC = s.g_cam + (size_t)si * T * 12;
      for (int i = tid; i < T * 12; i += nt) gC[i] = 0.0f;
    }
  }
  rt.sync();
  // (2) values and adjoints; value k is copied by the lane that stored it
  grecon_aux_terms(rt, s.aux, l, si);
  for (int k = tid; k < GAUX_N; k += nt)
    s.values[(size_t)si * s.values_stride + (size_t)s.iteration * GAUX_N + k] = s.aux.values[(size_t)si * GAUX_N + k];
  rt.sync();
  // (3) camera adjoints -> the camera's variables (derived: the residuals, and the pose adjoints)
  if (MODE != GAUX_CONSTANT && s.run_cam) {
    grecon_cam_bwd<MODE>(rt, s.cam, l, si);
    rt.sync();
  }
  // (4) pose adjoints -> the trajectory variables, slot by slot (n_persons is uniform over the workgroup)
  if (s.run_pose) {
    const int np = gaux_clamp(s.aux.n_persons[si], 0, P);
    for (int p = 0; p < np; ++p) {
      grecon_pose_bwd(rt, s.pose, l, si * P + p);
      rt.sync();
    }
  }
  // (5) torch.optim.Adam on the scene's row
  const size_t row = (size_t)si * l.scene_stride;
  for (int i = tid; i < l.scene_stride; i += nt) GLAMR_GRECON_NS::adam(s.params[row + i], s.exp_avg[row + i], s.exp_avg_sq[row + i], s.grads[row + i], s.coef);
}

}  // namespace glamr
