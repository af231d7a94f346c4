// glamr_grecon_cam_backward: the vector-Jacobian product from the world-to-camera transforms of a stage launch (cam_pose) to what the stage
// optimises -- the algorithm of grecon_cam_bwd.hpp on the device, one workgroup of 256 threads per scene, frames strided over the threads, one
// kernel instance per camera mode.  DESIGN.md 17.
//
// Latency-bound like glamr_grecon_pose_backward.  The derived mode keeps the per-frame person counts and the gradient of the averaged transform
// in the caller's workspace (13 floats per scene and frame); the only LDS is the block reduction's exchange area (the fixed camera's nine
// sums).  Plain fp32, no atomics, a fixed order of additions: linear in g_cam_pose, two calls give the same bits.  Persons per scene, lengths,
// visibility and the frozen table are read on the device; the host side checks its arguments and launches, so the call can be recorded into a
// stream capture.
// (grecon_algo.hpp in a namespace of this file's own, as grecon_wide.hip has it: no symbol of the stage kernels' translation units is shared)
#define GLAMR_GRECON_NS grecon_cam
#include "common.hpp"
#include "block_rt.hpp"
#include "grecon_cam_bwd.hpp"

namespace glamr {
namespace {

constexpr int GCB_THREADS = 256;

template <int MODE>
__global__ __launch_bounds__(GCB_THREADS) void grecon_cam_bwd_kernel(CamBwdBatch b, glamr_param_layout l) {
  __shared__ __attribute__((aligned(16))) float red[RT_RED_FLOATS];
  DeviceRT rt{red};
  grecon_cam_bwd<MODE>(rt, b, l, blockIdx.x);
}

}  // namespace
}  // namespace glamr

extern "C" size_t glamr_grecon_cam_backward_workspace_bytes(int n_scenes, int max_persons, int max_len) {
  if (n_scenes <= 0 || max_persons <= 0 || max_len <= 0) return 0;
  return (size_t)n_scenes * max_len * glamr::GCB_WS_FLOATS_PER_FRAME * sizeof(float);
}

extern "C" int glamr_grecon_cam_backward(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const float* g_cam_pose, float* grads, int accumulate,
                                         float* g_orient_world, float* g_trans_world, void* workspace, void* stream) {
  using namespace glamr;
  GLAMR_REQUIRE(batch && stage && g_cam_pose && grads && workspace, "glamr_grecon_cam_backward: NULL argument (batch, stage, g_cam_pose, grads, workspace)");
  GLAMR_REQUIRE(batch->n_scenes >= 0 && batch->max_persons >= 1 && batch->max_persons <= 32 && batch->max_len >= 1,
                "glamr_grecon_cam_backward: bad batch geometry (n_scenes >= 0, 1 <= max_persons <= 32, max_len >= 1)");
  GLAMR_REQUIRE((int64_t)batch->max_len * 12 * batch->max_persons < 0x7fffffff, "glamr_grecon_cam_backward: sequence too long");
  const int mode = GLAMR_GRECON_NS::camera_mode(*stage);
  if (mode == GCB_CONSTANT)
    return fail(GLAMR_E_UNSUPPORTED, "glamr_grecon_cam_backward: the stage neither optimises the camera (GLAMR_VAR_CAM) nor derives it from the persons "
                                     "(GLAMR_FLAG_CAM_FROM_PERSON): cam_pose is a constant");
  GLAMR_REQUIRE(mode != GCB_DERIVED || (g_orient_world && g_trans_world),
                "glamr_grecon_cam_backward: g_orient_world and g_trans_world are required when the camera is derived from the persons");
  if (batch->n_scenes == 0) return GLAMR_OK;
  GLAMR_REQUIRE(batch->seq_len && batch->params, "glamr_grecon_cam_backward: NULL batch array (seq_len, params)");
  GLAMR_REQUIRE(mode != GCB_DERIVED || (batch->n_persons && batch->vis && batch->person2cam && batch->orient_world && batch->trans_world),
                "glamr_grecon_cam_backward: NULL batch array (n_persons, vis, person2cam, orient_world, trans_world)");
  glamr_param_layout l;
  GLAMR_GRECON_NS::param_layout(batch->max_persons, batch->max_len, l);
  const CamBwdBatch b = cam_bwd_batch(*batch, g_cam_pose, grads, accumulate, g_orient_world, g_trans_world, static_cast<float*>(workspace));
  const dim3 grid(batch->n_scenes), block(GCB_THREADS);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode == GCB_PER_FRAME) hipLaunchKernelGGL(grecon_cam_bwd_kernel<GCB_PER_FRAME>, grid, block, 0, s, b, l);
  else if (mode == GCB_FIXED) hipLaunchKernelGGL(grecon_cam_bwd_kernel<GCB_FIXED>, grid, block, 0, s, b, l);
  else hipLaunchKernelGGL(grecon_cam_bwd_kernel<GCB_DERIVED>, grid, block, 0, s, b, l);
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}
