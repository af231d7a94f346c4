// glamr_grecon_aux_step: what follows the gradient launch in an Adam iteration of a stage that lists terms of glamr_grecon_aux_terms -- the
// terms' values and adjoints, the camera and pose VJPs and torch.optim.Adam's step -- the algorithm of grecon_aux_step.hpp on the device in
// ONE launch, one workgroup of 256 threads per scene, one kernel instance per camera mode.  DESIGN.md 20.
//
// Latency-bound like the three kernels it composes: a scene's phases are separated by workgroup barriers instead of launch boundaries, and
// the adjoints between them stay in the caller's workspace (L2-resident: P T 6 + T 12 floats per scene).  The only LDS is the block runtime's
// exchange area.  Plain fp32, no atomics, a fixed order of additions: two calls give the same bits.  `iteration` and `step` are plain
// arguments: every iteration is a launch -- and a graph node -- of its own.  The host side checks its arguments and launches, so the call can
// be recorded into a stream capture.
// (grecon_algo.hpp in a namespace of this file's own, as grecon_aux.hip has it: no symbol of the stage kernels' translation units is shared)
#define GLAMR_GRECON_NS grecon_step
#include "common.hpp"
#include "block_rt.hpp"
#include "grecon_aux_step.hpp"

namespace glamr {
namespace {

constexpr int GAS_THREADS = 256;

template <int MODE>
__global__ __launch_bounds__(GAS_THREADS) void grecon_aux_step_kernel(AuxStepBatch s, glamr_param_layout l) {
  __shared__ __attribute__((aligned(16))) float red[RT_RED_FLOATS];
  DeviceRT rt{red};
  grecon_aux_step<MODE>(rt, s, l, blockIdx.x);
}

}  // namespace
}  // namespace glamr

extern "C" size_t glamr_grecon_aux_step_workspace_bytes(int n_scenes, int max_persons, int max_len) {
  if (n_scenes <= 0 || max_persons <= 0 || max_len <= 0) return 0;
  return glamr::aux_step_workspace(n_scenes, max_persons, max_len).total * sizeof(float);
}

extern "C" int glamr_grecon_aux_step(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const glamr_aux_desc* aux, const float* root_trans_cam,
                                     float* values, int values_stride, int iteration, float* grads, float* exp_avg, float* exp_avg_sq, double lr, int step,
                                     void* workspace, void* stream) {
  using namespace glamr;
  const char* msg = nullptr;
  const int rc = aux_step_check(batch, stage, aux, root_trans_cam, values, values_stride, iteration, grads, exp_avg, exp_avg_sq, lr, step, workspace, &msg);
  if (rc != GLAMR_OK) return fail(rc, "%s", msg);
  if (batch->n_scenes == 0) return GLAMR_OK;
  glamr_param_layout l;
  GLAMR_GRECON_NS::param_layout(batch->max_persons, batch->max_len, l);
  const AuxStepBatch s = aux_step_batch(*batch, *stage, *aux, root_trans_cam, values, values_stride, iteration, grads, exp_avg, exp_avg_sq, lr, step, workspace);
  const dim3 grid(batch->n_scenes), block(GAS_THREADS);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int mode = s.aux.cam_mode;
  if (mode == GAUX_PER_FRAME) hipLaunchKernelGGL(grecon_aux_step_kernel<GAUX_PER_FRAME>, grid, block, 0, st, s, l);
  else if (mode == GAUX_FIXED) hipLaunchKernelGGL(grecon_aux_step_kernel<GAUX_FIXED>, grid, block, 0, st, s, l);
  else if (mode == GAUX_DERIVED) hipLaunchKernelGGL(grecon_aux_step_kernel<GAUX_DERIVED>, grid, block, 0, st, s, l);
  else hipLaunchKernelGGL(grecon_aux_step_kernel<GAUX_CONSTANT>, grid, block, 0, st, s, l);
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}
