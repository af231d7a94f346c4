// glamr_grecon_aux_terms: the reference's loss_cfg terms the stage kernel does not hold (cam_rot_smoothness, cam_trans_smoothness,
// cam_depth_smoothness, traj_trans_smoothness, cam_traj_trans, local_traj_dheading_reg) -- the algorithm of grecon_aux.hpp on the device, one
// workgroup of 256 threads per scene, frames strided over the threads, values and adjoints from ONE launch.  DESIGN.md 19.
//
// Latency-bound like glamr_grecon_cam_backward: a few dozen flops per frame and person.  The only LDS is the block reduction's exchange area
// (the visible-frame count, the six partial values); the workspace holds one int per slot (a person's first visible frame).  Plain fp32, no
// atomics, a fixed order of additions: two calls give the same bits.  Persons per scene, lengths and visibility are read on the device; the
// host side checks its arguments and launches, so the call can be recorded into a stream capture.
// (grecon_algo.hpp in a namespace of this file's own, as grecon_cam_bwd.hip has it: no symbol of the stage kernels' translation units is shared)
#define GLAMR_GRECON_NS grecon_aux
#include "common.hpp"
#include "block_rt.hpp"
#include "grecon_aux.hpp"

namespace glamr {
namespace {

constexpr int GAUX_THREADS = 256;

__global__ __launch_bounds__(GAUX_THREADS) void grecon_aux_terms_kernel(AuxBatch b, glamr_param_layout l) {
  __shared__ __attribute__((aligned(16))) float red[RT_RED_FLOATS];
  DeviceRT rt{red};
  grecon_aux_terms(rt, b, l, blockIdx.x);
}

}  // namespace
}  // namespace glamr

extern "C" size_t glamr_grecon_aux_terms_workspace_bytes(int n_scenes, int max_persons, int max_len) {
  if (n_scenes <= 0 || max_persons <= 0 || max_len <= 0) return 0;
  return (size_t)n_scenes * max_persons * sizeof(int32_t);
}

extern "C" int glamr_grecon_aux_terms(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const glamr_aux_desc* aux, const float* root_trans_cam,
                                      float* values, float* g_trans_world, float* g_cam_pose, float* grads, int accumulate, void* workspace, void* stream) {
  using namespace glamr;
  const char* msg = nullptr;
  const int rc = aux_check(batch, stage, aux, root_trans_cam, values, g_trans_world, g_cam_pose, grads, workspace, &msg);
  if (rc != GLAMR_OK) return fail(rc, "%s", msg);
  if (batch->n_scenes == 0) return GLAMR_OK;
  glamr_param_layout l;
  GLAMR_GRECON_NS::param_layout(batch->max_persons, batch->max_len, l);
  const AuxBatch b = aux_batch(*batch, *stage, *aux, root_trans_cam, values, g_trans_world, g_cam_pose, grads, accumulate, workspace);
  hipLaunchKernelGGL(grecon_aux_terms_kernel, dim3(batch->n_scenes), dim3(GAUX_THREADS), 0, static_cast<hipStream_t>(stream), b, l);
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}
