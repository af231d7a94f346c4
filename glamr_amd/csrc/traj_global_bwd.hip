// glamr_traj_local_to_global_backward: the vector-Jacobian product of glamr_traj_local_to_global (traj_local2global_heading,
// traj_pred/utils/traj_utils.py:65-88, + quaternion_to_angle_axis) -- the algorithm of traj_global_bwd.hpp on the device, one workgroup of
// 256 threads per sequence, frames strided over the threads.  DESIGN.md 14.
//
// The kernel is latency-bound (one prefix and three suffix scans per workgroup, ~130 bytes per frame): the scan arrays live in the caller's
// workspace (4 floats per frame), the only LDS is the scans' exchange area, and a sequence of at most 256 frames keeps its local row in
// registers between the phases.  Plain fp32 throughout: the result is linear in the upstream gradient to rounding.  No atomics, every sum
// is one of the scans: two calls give the same bits.  The lengths are read on the device and clamped to [0, T]; the host side only checks
// its arguments and launches, so the call can be recorded into a stream capture.
#include "common.hpp"
#include "block_rt.hpp"
#include "traj_global_bwd.hpp"

namespace glamr {
namespace {

constexpr int TGB_THREADS = 256;

__global__ __launch_bounds__(TGB_THREADS) void traj_global_bwd_kernel(int T, const int32_t* lens, const float* local_traj, const float* g_trans, const float* g_orient,
                                                                      const float* g_orient_q, float* g_local_traj, float* workspace) {
  __shared__ __attribute__((aligned(16))) float red[RT_RED_FLOATS];
  DeviceRT rt{red};
  const size_t b = blockIdx.x, frames = b * (size_t)T;
  const int n = lens ? min(max(lens[b], 0), T) : T;
  traj_global_bwd(rt, n, T, local_traj + frames * 11, g_trans ? g_trans + frames * 3 : nullptr, g_orient ? g_orient + frames * 3 : nullptr,
                  g_orient_q ? g_orient_q + frames * 4 : nullptr, g_local_traj + frames * 11, workspace + frames * TGB_WS_FLOATS_PER_FRAME);
}

}  // namespace
}  // namespace glamr

extern "C" size_t glamr_traj_local_to_global_backward_workspace_bytes(int n_seq, int T) {
  if (n_seq <= 0 || T <= 0) return 0;
  return (size_t)n_seq * T * glamr::TGB_WS_FLOATS_PER_FRAME * sizeof(float);
}

extern "C" int glamr_traj_local_to_global_backward(int n_seq, int T, const int32_t* lens_dev, const float* local_traj, const float* g_trans, const float* g_orient,
                                                   const float* g_orient_q, float* g_local_traj, void* workspace, void* stream) {
  using namespace glamr;
  GLAMR_REQUIRE(n_seq >= 0 && T >= 1, "glamr_traj_local_to_global_backward: bad geometry (n_seq >= 0, T >= 1)");
  if (n_seq == 0) return GLAMR_OK;
  GLAMR_REQUIRE(local_traj && g_local_traj && workspace, "glamr_traj_local_to_global_backward: null argument");
  GLAMR_REQUIRE(g_trans || g_orient || g_orient_q, "glamr_traj_local_to_global_backward: at least one of g_trans, g_orient and g_orient_q must be given");
  GLAMR_REQUIRE((int64_t)T * 11 < 0x7fffffff, "glamr_traj_local_to_global_backward: sequence too long");
  hipLaunchKernelGGL(traj_global_bwd_kernel, dim3(n_seq), dim3(TGB_THREADS), 0, static_cast<hipStream_t>(stream), T, lens_dev, local_traj, g_trans, g_orient, g_orient_q,
                     g_local_traj, static_cast<float*>(workspace));
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}
