// glamr_grecon_pose_backward: the vector-Jacobian product from the world poses of a stage launch (orient_world, trans_world) to the trajectory
// variables of the scene parameters -- the algorithm of grecon_pose_bwd.hpp on the device, one workgroup of 256 threads per person slot,
// frames strided over the threads.  DESIGN.md 15.
//
// Latency-bound like glamr_traj_local_to_global_backward, whose per-sequence algorithm does the work between the assembled local rows and
// the poses: the assembled rows, their gradients and the scan arrays live in the caller's workspace (27 floats per frame), the only LDS is
// the scans' exchange area.  Plain fp32, no atomics, every sum one of the scans: linear in the upstream gradients, two calls give the same
// bits.  Persons per scene, lengths, existing ranges, the frozen table and the heading mask are read on the device; the host side checks its
// arguments and launches, so the call can be recorded into a stream capture.
#include "common.hpp"
#include "block_rt.hpp"
#include "grecon_pose_bwd.hpp"

namespace glamr {
namespace {

constexpr int GPB_THREADS = 256;

__global__ __launch_bounds__(GPB_THREADS) void grecon_pose_bwd_kernel(PoseBwdBatch b, glamr_param_layout l) {
  __shared__ __attribute__((aligned(16))) float red[RT_RED_FLOATS];
  DeviceRT rt{red};
  const int slot = blockIdx.x;
  if (!b.accumulate && slot % b.P == 0) grecon_pose_bwd_clear(rt, b.grads + (size_t)(slot / b.P) * l.scene_stride, l.person0);
  grecon_pose_bwd(rt, b, l, slot);
}

}  // namespace
}  // namespace glamr

extern "C" size_t glamr_grecon_pose_backward_workspace_bytes(int n_scenes, int max_persons, int max_len) {
  if (n_scenes <= 0 || max_persons <= 0 || max_len <= 0) return 0;
  return (size_t)n_scenes * max_persons * max_len * glamr::GPB_WS_FLOATS_PER_FRAME * sizeof(float);
}

extern "C" int glamr_grecon_pose_backward(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const float* g_orient_world, const float* g_trans_world,
                                          float* grads, int accumulate, void* workspace, void* stream) {
  using namespace glamr;
  GLAMR_REQUIRE(batch && stage && grads && workspace, "glamr_grecon_pose_backward: NULL argument (batch, stage, grads, workspace)");
  GLAMR_REQUIRE(batch->n_scenes >= 0 && batch->max_persons >= 1 && batch->max_persons <= 32 && batch->max_len >= 2,
                "glamr_grecon_pose_backward: bad batch geometry (n_scenes >= 0, 1 <= max_persons <= 32, max_len >= 2)");
  GLAMR_REQUIRE((int64_t)batch->max_len * 11 < 0x7fffffff, "glamr_grecon_pose_backward: sequence too long");
  GLAMR_REQUIRE((int64_t)batch->n_scenes * batch->max_persons < 0x7fffffff, "glamr_grecon_pose_backward: too many person slots");
  GLAMR_REQUIRE(g_orient_world || g_trans_world, "glamr_grecon_pose_backward: at least one of g_orient_world and g_trans_world must be given");
  if (stage->flags & GLAMR_FLAG_ABSOLUTE_HEADING)
    return fail(GLAMR_E_UNSUPPORTED, "glamr_grecon_pose_backward: GLAMR_FLAG_ABSOLUTE_HEADING is not supported (the headings of the assembled rows are increments)");
  if (batch->n_scenes == 0) return GLAMR_OK;
  GLAMR_REQUIRE(batch->n_persons && batch->seq_len && batch->fr_start && batch->fr_end && batch->traj_local_pred && batch->params,
                "glamr_grecon_pose_backward: NULL batch array (n_persons, seq_len, fr_start, fr_end, traj_local_pred, params)");
  GLAMR_REQUIRE(!(stage->flags & GLAMR_FLAG_HAS_WORLD_DHEADING) || !g_orient_world || batch->base_orient,
                "glamr_grecon_pose_backward: NULL base_orient with GLAMR_FLAG_HAS_WORLD_DHEADING");
  glamr_param_layout l;
  if (int rc = glamr_grecon_param_layout(batch->max_persons, batch->max_len, &l)) return rc;
  const PoseBwdBatch b = pose_bwd_batch(*batch, *stage, g_orient_world, g_trans_world, grads, accumulate, static_cast<float*>(workspace));
  hipLaunchKernelGGL(grecon_pose_bwd_kernel, dim3(batch->n_scenes * batch->max_persons), dim3(GPB_THREADS), 0, static_cast<hipStream_t>(stream), b, l);
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}
