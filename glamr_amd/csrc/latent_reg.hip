// The latent regularisers of the latent-optimisation mode: motion_latent_reg and traj_latent_reg (loss_func.py:293-310).
// Per scene, value = sum over the scene's persons of sum z^2, divided by the scene's number of latent ROWS (infiller windows for the motion
// latent, persons for the trajectory latent); gradient g = fl(fl(weight / rows) * 2 z).  One launch serves both latents of a batch, one
// workgroup per scene (scene = max_persons consecutive slots, as in glamr_scene_batch).
//
// The latents are padded: meps (slots, n_win_max, 128) with n_win_slot[k] real rows in slot k, teps (slots, 128) with slot k real iff
// n_win_slot[k] > 0.  Padded rows are never READ (they may hold anything) and enter no sum and no count; their gradient rows are written as
// zero when the gradient is stored and left alone when it is added into a buffer that already holds the data terms' gradient.
//
// Summation order is fixed: every thread adds the float4 groups tid, tid + 256, ... of its scene in that order (x, y, z, w inside a group,
// one fused multiply-add each), the 64 lanes of a wave are folded by the butterfly 32, 16, ..., 1, and thread 0 adds the four wave partials in
// wave order.  No atomics: a repeat on the same inputs is bit-equal.  The gradient's product and the addition into the buffer are separate
// roundings (__fmul_rn / __fadd_rn: never contracted into one fma).
#include "common.hpp"

namespace glamr {
namespace {

constexpr int LR_THREADS = 256, LR_WAVES = LR_THREADS / 64, NZ4 = 128 / 4;

struct LatentRegArgs {
  int max_persons, n_win_max;
  const float4* meps; const float4* teps; const int32_t* n_win_slot;
  float weight[2]; int mode[2]; int add[2];
  float4* grad[2];
  float* values; float* history; int n_rows; const int32_t* row_index;
};

__device__ __forceinline__ float sq_acc(float acc, const float4& z) {
  acc = fmaf(z.x, z.x, acc); acc = fmaf(z.y, z.y, acc); acc = fmaf(z.z, z.z, acc); return fmaf(z.w, z.w, acc);
}
__device__ __forceinline__ float4 reg_grad(float c, const float4& z) {
  return make_float4(__fmul_rn(c, 2.0f * z.x), __fmul_rn(c, 2.0f * z.y), __fmul_rn(c, 2.0f * z.z), __fmul_rn(c, 2.0f * z.w));
}
__device__ __forceinline__ void put_grad(float4* g, bool add, const float4& v) {
  if (add) { const float4 o = *g; *g = make_float4(__fadd_rn(o.x, v.x), __fadd_rn(o.y, v.y), __fadd_rn(o.z, v.z), __fadd_rn(o.w, v.w)); }
  else *g = v;
}

__global__ __launch_bounds__(LR_THREADS) void latent_reg_kernel(LatentRegArgs a) {
  __shared__ float part[2][LR_WAVES];
  const int s = blockIdx.x, tid = threadIdx.x, P = a.max_persons, W = a.n_win_max;
  const int32_t* nw = a.n_win_slot + (size_t)s * P;
  // rows of the scene: windows (clamped to the padded extent: nothing outside the arrays is touched whatever the table holds) and persons
  int rows[2] = {0, 0};
  for (int p = 0; p < P; ++p) { const int n = min(max(nw[p], 0), W); rows[0] += n; rows[1] += n > 0; }
  float acc[2] = {0.0f, 0.0f};
  for (int t = 0; t < 2; ++t) {
    if (a.mode[t] == GLAMR_LATENT_REG_ABSENT) continue;
    const bool active = a.mode[t] == GLAMR_LATENT_REG_ACTIVE;
    const float c = (active && rows[t] > 0) ? __fdiv_rn(a.weight[t], (float)rows[t]) : 0.0f;
    const int per_slot = (t == 0 ? W : 1) * NZ4, total = P * per_slot;
    const float4* z = (t == 0 ? a.meps : a.teps) + (size_t)s * total;
    float4* g = active ? a.grad[t] + (size_t)s * total : nullptr;
    for (int i = tid; i < total; i += LR_THREADS) {
      const int p = i / per_slot, row = (i - p * per_slot) / NZ4;
      const bool real = row < min(max(nw[p], 0), W);
      if (real) {
        const float4 v = z[i];
        acc[t] = sq_acc(acc[t], v);
        if (active) put_grad(g + i, a.add[t] != 0, reg_grad(c, v));
      } else if (active && !a.add[t]) {
        g[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) { acc[0] += __shfl_xor(acc[0], off); acc[1] += __shfl_xor(acc[1], off); }
  if ((tid & 63) == 0) { part[0][tid >> 6] = acc[0]; part[1][tid >> 6] = acc[1]; }
  __syncthreads();
  if (tid == 0) {
    const int r = (a.history && a.row_index) ? *a.row_index : -1;
    for (int t = 0; t < 2; ++t) {
      if (a.mode[t] == GLAMR_LATENT_REG_ABSENT) continue;
      float sum = part[t][0];
      for (int w = 1; w < LR_WAVES; ++w) sum += part[t][w];
      const float value = rows[t] > 0 ? __fdiv_rn(sum, (float)rows[t]) : 0.0f;
      a.values[(size_t)s * 2 + t] = value;
      if (r >= 0 && r < a.n_rows) a.history[((size_t)s * a.n_rows + r) * 2 + t] = value;
    }
  }
}

bool mode_ok(int m) { return m == GLAMR_LATENT_REG_ABSENT || m == GLAMR_LATENT_REG_MONITOR || m == GLAMR_LATENT_REG_ACTIVE; }

}  // namespace
}  // namespace glamr

extern "C" int glamr_latent_reg(int n_scenes, int max_persons, int n_win_max, const float* meps, const float* teps, const int32_t* n_win_slot,
                                const int32_t* n_win_slot_host, float weight_motion, float weight_traj, int mode_motion, int mode_traj, int add_motion,
                                int add_traj, float* g_meps, float* g_teps, float* values, float* history, int n_rows, const int32_t* row_index, void* stream) {
  using namespace glamr;
  GLAMR_REQUIRE(n_scenes >= 0 && max_persons >= 1 && n_win_max >= 0, "glamr_latent_reg: bad geometry (n_scenes >= 0, max_persons >= 1, n_win_max >= 0)");
  GLAMR_REQUIRE(mode_ok(mode_motion) && mode_ok(mode_traj), "glamr_latent_reg: a mode must be GLAMR_LATENT_REG_ABSENT, _MONITOR or _ACTIVE");
  if (n_scenes == 0 || (mode_motion == GLAMR_LATENT_REG_ABSENT && mode_traj == GLAMR_LATENT_REG_ABSENT)) return GLAMR_OK;
  GLAMR_REQUIRE(n_win_slot && n_win_slot_host && values, "glamr_latent_reg: null argument");
  GLAMR_REQUIRE(mode_motion == GLAMR_LATENT_REG_ABSENT || (meps && n_win_max >= 1), "glamr_latent_reg: motion_latent_reg needs meps and n_win_max >= 1");
  GLAMR_REQUIRE(mode_traj == GLAMR_LATENT_REG_ABSENT || teps, "glamr_latent_reg: traj_latent_reg needs teps");
  GLAMR_REQUIRE(mode_motion != GLAMR_LATENT_REG_ACTIVE || g_meps, "glamr_latent_reg: an active motion_latent_reg needs g_meps");
  GLAMR_REQUIRE(mode_traj != GLAMR_LATENT_REG_ACTIVE || g_teps, "glamr_latent_reg: an active traj_latent_reg needs g_teps");
  GLAMR_REQUIRE(((reinterpret_cast<uintptr_t>(meps) | reinterpret_cast<uintptr_t>(teps) | reinterpret_cast<uintptr_t>(g_meps) | reinterpret_cast<uintptr_t>(g_teps)) & 15) == 0,
                "glamr_latent_reg: meps, teps, g_meps and g_teps must be 16-byte aligned");
  GLAMR_REQUIRE(!history || (row_index && n_rows >= 1), "glamr_latent_reg: a history needs row_index and n_rows >= 1");
  GLAMR_REQUIRE((int64_t)max_persons * (n_win_max + 1) * (128 / 4) < 0x7fffffff, "glamr_latent_reg: scene too large");
  const bool any_active = mode_motion == GLAMR_LATENT_REG_ACTIVE || mode_traj == GLAMR_LATENT_REG_ACTIVE;
  for (int s = 0; s < n_scenes; ++s) {
    int persons = 0;
    for (int p = 0; p < max_persons; ++p) {
      const int k = s * max_persons + p, n = n_win_slot_host[k];
      GLAMR_REQUIRE(n >= 0 && n <= n_win_max, "glamr_latent_reg: slot %d has %d windows (0 <= n_win_slot <= n_win_max = %d)", k, n, n_win_max);
      persons += n > 0;
    }
    GLAMR_REQUIRE(!any_active || persons >= 1, "glamr_latent_reg: scene %d has no person, but a regulariser is active", s);
  }
  LatentRegArgs a{max_persons, n_win_max, reinterpret_cast<const float4*>(meps), reinterpret_cast<const float4*>(teps), n_win_slot,
                  {weight_motion, weight_traj}, {mode_motion, mode_traj}, {add_motion, add_traj},
                  {reinterpret_cast<float4*>(g_meps), reinterpret_cast<float4*>(g_teps)}, values, history, n_rows, row_index};
  hipLaunchKernelGGL(latent_reg_kernel, dim3(n_scenes), dim3(LR_THREADS), 0, static_cast<hipStream_t>(stream), a);
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}
