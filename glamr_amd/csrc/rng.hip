// The priors' Gaussian latent draws from per-sequence Philox streams (rng_algo.hpp): every number is a function of
// (seed, sequence id, person id, prior, element index) and of nothing else -- not of the batch a sequence is in, its slot there, the number of
// windows the batch was padded to, or the GPU count.  Replaces the two torch.randn launches of a step (GlobalReconOptimizer.latent_source).
//
// One thread per Philox block: ~10 x (2 mul-lo + 2 mul-hi + 4 xor/add), two Box-Muller pairs, one 16-byte store; consecutive threads write
// consecutive 16 bytes.  The draw kernel runs in the "priors" segment of a pipelined step, beside resident workgroups of the other batch's
// optimiser stage, and follows nn_free.hpp's rules for that neighbourhood: no LDS, two waves per workgroup, well under 128 registers, no scratch.
//
// Uniform -> normal, Box-Muller on the word pairs (0,1) and (2,3): for (x, y), u = (x + 0.5) 2^-32, theta = 2 pi (y + 0.5) 2^-32,
// r = sqrt(-2 ln u), outputs r cos(theta), r sin(theta).  In fp32, without losing the ends of the range:
//   * -ln u: for x < 2^31, -logf of u = fma(float(x), 2^-32, 2^-33) (relative error 2^-24 in u, i.e. 6e-8 absolute in ln u); for x >= 2^31,
//     where u rounds towards 1 and ln u would lose everything (x = 0xffffffff: u rounds to 1, r to 0 instead of 2^-16), -log1pf(-v) of
//     v = 1 - u = (~x + 0.5) 2^-32, which is exact in the integers and small;
//   * theta: the two top bits of y are the quadrant, applied at the end by exact swaps and sign changes; the other 30 bits f give the angle
//     inside the quadrant in half turns, t = (f + 0.5) 2^-31 in (0, 1/2), and sincospif(t) takes half turns (no product with pi is rounded).
//     What is left is float(f): 2^-24 relative of an angle below pi / 2.
// OCML's precise logf / log1pf / sincospif and the correctly rounded sqrtf (no fast-math flag on this file).  Bound and measured maximum
// against float64: DESIGN.md 10, tests/test_philox_gpu.py.
#include "common.hpp"
#include "rng_algo.hpp"

namespace glamr {
namespace {

constexpr int RNG_THREADS = 128;

__device__ __forceinline__ void box_muller(uint32_t x, uint32_t y, float& a, float& b) {
  const float u = fmaf((float)x, 0x1p-32f, 0x1p-33f);
  const float v = fmaf((float)(~x), 0x1p-32f, 0x1p-33f);
  const float nl = (x & 0x80000000u) ? -log1pf(-v) : -logf(u);
  const float r = sqrtf(2.0f * nl);
  const uint32_t q = y >> 30, f = y & 0x3fffffffu;
  float s, c;
  sincospif(fmaf((float)f, 0x1p-31f, 0x1p-32f), &s, &c);
  // cos / sin of the angle plus q quarter turns
  const float cq = (q & 1u) ? -s : c, sq = (q & 1u) ? c : s;
  const float sign = (q & 2u) ? -1.0f : 1.0f;
  a = sign * (r * cq);
  b = sign * (r * sq);
}

__device__ __forceinline__ float4 normals_of(const rng::Block& k) {
  float4 o;
  box_muller(k.w[0], k.w[1], o.x, o.y);
  box_muller(k.w[2], k.w[3], o.z, o.w);
  return o;
}

__global__ __launch_bounds__(RNG_THREADS) void rng_bits_kernel(uint64_t seed, uint64_t seq_id, uint32_t sub, uint32_t first_block, int64_t n_blocks, uint4* out) {
  const int64_t i = (int64_t)blockIdx.x * RNG_THREADS + threadIdx.x;
  if (i >= n_blocks) return;
  const rng::Block k = rng::stream_block(seed, seq_id, sub, first_block + (uint32_t)i);
  out[i] = make_uint4(k.w[0], k.w[1], k.w[2], k.w[3]);
}

// the kernel's own uniform -> normal map on integers the caller chose (4 words in, 4 floats out per block)
__global__ __launch_bounds__(RNG_THREADS) void rng_box_muller_kernel(int64_t n_blocks, const uint4* bits, float4* out) {
  const int64_t i = (int64_t)blockIdx.x * RNG_THREADS + threadIdx.x;
  if (i >= n_blocks) return;
  const uint4 w = bits[i];
  out[i] = normals_of(rng::Block{{w.x, w.y, w.z, w.w}});
}

// elements [first_elem, first_elem + n) of one stream; thread i owns block first_elem / 4 + i.  A block that lies inside the range and whose
// four floats start at a 16-byte boundary of `out` goes out as one vector store; the (at most two) ragged blocks and unaligned outputs
// element by element, never outside [out, out + n).
__global__ __launch_bounds__(RNG_THREADS) void rng_normal_kernel(uint64_t seed, uint64_t seq_id, uint32_t sub, uint64_t first_elem, int64_t n, int64_t n_blocks, int vec_ok,
                                                                  float* out) {
  const int64_t i = (int64_t)blockIdx.x * RNG_THREADS + threadIdx.x;
  if (i >= n_blocks) return;
  const uint64_t block = first_elem / 4 + (uint64_t)i;
  const float4 v = normals_of(rng::stream_block(seed, seq_id, sub, (uint32_t)block));
  const int64_t o = (int64_t)(block * 4 - first_elem);             // index in `out` of the block's first value: -3 .. n - 1
  if (vec_ok && o >= 0 && o + 4 <= n) {
    *reinterpret_cast<float4*>(out + o) = v;
    return;
  }
  const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (o + j >= 0 && o + j < n) out[o + j] = e[j];
}

// Both latent arrays of every slot of a batch in one launch: per slot n_windows * 32 blocks of the infiller's (n_windows, 128) draws, then 32
// blocks of the trajectory predictor's 128.  The seed comes from device memory: a captured step is replayed under another seed by
// rewriting those two words (glamr_rng_set_seed), not by re-capturing.
__global__ __launch_bounds__(RNG_THREADS) void latents_draw_kernel(const uint32_t* __restrict__ seed_dev, const uint64_t* __restrict__ seq_ids,
                                                                    const int32_t* __restrict__ person_ids, int n_slots, int n_windows, float4* __restrict__ meps,
                                                                    float4* __restrict__ teps) {
  constexpr uint32_t BPW = rng::NZ / 4;                            // blocks per 128 values
  const uint32_t m_blocks = (uint32_t)n_windows * BPW, per_slot = m_blocks + BPW;
  const int64_t g = (int64_t)blockIdx.x * RNG_THREADS + threadIdx.x;
  if (g >= (int64_t)n_slots * per_slot) return;
  const uint32_t slot = (uint32_t)(g / per_slot), r = (uint32_t)(g - (int64_t)slot * per_slot);
  const bool traj = r >= m_blocks;
  const uint32_t block = traj ? r - m_blocks : r;
  float4* dst = traj ? teps + (size_t)slot * BPW + block : meps + (size_t)slot * m_blocks + block;
  const int32_t person = person_ids[slot];
  if (person < 0) {                                                // padding slot
    *dst = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const uint64_t seed = (uint64_t)seed_dev[0] | ((uint64_t)seed_dev[1] << 32);
  *dst = normals_of(rng::stream_block(seed, seq_ids[slot], rng::substream(person, traj ? rng::PRIOR_TRAJ : rng::PRIOR_INFILLER), block));
}

__global__ __launch_bounds__(64) void rng_set_seed_kernel(uint32_t* seed_dev, uint32_t lo, uint32_t hi) {
  if (threadIdx.x < 2) seed_dev[threadIdx.x] = threadIdx.x ? hi : lo;
}

inline unsigned grid_for(int64_t threads) { return (unsigned)((threads + RNG_THREADS - 1) / RNG_THREADS); }
constexpr int64_t MAX_BLOCKS = (int64_t)1 << 32;                    // blocks of one sub-stream

}  // namespace
}  // namespace glamr

using namespace glamr;

extern "C" int glamr_rng_bits(uint64_t seed, uint64_t seq_id, uint32_t sub, uint32_t first_block, int64_t n_blocks, uint32_t* out, void* stream) {
  GLAMR_REQUIRE(n_blocks >= 0, "glamr_rng_bits: negative n_blocks");
  GLAMR_REQUIRE((int64_t)first_block + n_blocks <= MAX_BLOCKS, "glamr_rng_bits: blocks [%u, %u + %lld) pass the 2^32 blocks of a sub-stream", first_block,
                first_block, (long long)n_blocks);
  if (n_blocks == 0) return GLAMR_OK;
  GLAMR_REQUIRE(out, "glamr_rng_bits: null argument");
  GLAMR_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "glamr_rng_bits: out must be 16-byte aligned");
  hipLaunchKernelGGL(rng_bits_kernel, dim3(grid_for(n_blocks)), dim3(RNG_THREADS), 0, static_cast<hipStream_t>(stream), seed, seq_id, sub, first_block, n_blocks,
                     reinterpret_cast<uint4*>(out));
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}

extern "C" int glamr_rng_box_muller(int64_t n_blocks, const uint32_t* bits, float* out, void* stream) {
  GLAMR_REQUIRE(n_blocks >= 0, "glamr_rng_box_muller: negative n_blocks");
  if (n_blocks == 0) return GLAMR_OK;
  GLAMR_REQUIRE(bits && out, "glamr_rng_box_muller: null argument");
  GLAMR_REQUIRE(((reinterpret_cast<uintptr_t>(bits) | reinterpret_cast<uintptr_t>(out)) & 15) == 0, "glamr_rng_box_muller: bits and out must be 16-byte aligned");
  hipLaunchKernelGGL(rng_box_muller_kernel, dim3(grid_for(n_blocks)), dim3(RNG_THREADS), 0, static_cast<hipStream_t>(stream), n_blocks,
                     reinterpret_cast<const uint4*>(bits), reinterpret_cast<float4*>(out));
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}

extern "C" int glamr_rng_normal(uint64_t seed, uint64_t seq_id, uint32_t sub, uint64_t first_elem, int64_t n, float* out, void* stream) {
  GLAMR_REQUIRE(n >= 0, "glamr_rng_normal: negative n");
  GLAMR_REQUIRE(first_elem <= (uint64_t)MAX_BLOCKS * 4 && (uint64_t)n <= (uint64_t)MAX_BLOCKS * 4 - first_elem,
                "glamr_rng_normal: elements [%llu, %llu + %lld) pass the 2^34 values of a sub-stream", (unsigned long long)first_elem, (unsigned long long)first_elem,
                (long long)n);
  if (n == 0) return GLAMR_OK;
  GLAMR_REQUIRE(out, "glamr_rng_normal: null argument");
  GLAMR_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "glamr_rng_normal: out must be 4-byte aligned");
  const int64_t n_blocks = (int64_t)((first_elem + (uint64_t)n + 3) / 4 - first_elem / 4);
  // out + o of a whole block is 16-byte aligned iff the address out WOULD have at element 4 * (first_elem / 4) is
  const int vec_ok = ((reinterpret_cast<uintptr_t>(out) - 4 * (uintptr_t)(first_elem & 3)) & 15) == 0;
  hipLaunchKernelGGL(rng_normal_kernel, dim3(grid_for(n_blocks)), dim3(RNG_THREADS), 0, static_cast<hipStream_t>(stream), seed, seq_id, sub, first_elem, n, n_blocks, vec_ok,
                     out);
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}

extern "C" int glamr_latents_draw(const uint64_t* seed_dev, const uint64_t* seq_ids, const int32_t* person_ids, int n_slots, int n_windows, float* meps, float* teps,
                                  void* stream) {
  GLAMR_REQUIRE(n_slots >= 0 && n_windows >= 0, "glamr_latents_draw: negative n_slots or n_windows");
  if (n_slots == 0) return GLAMR_OK;
  GLAMR_REQUIRE(seed_dev && seq_ids && person_ids && teps && (meps || n_windows == 0), "glamr_latents_draw: null argument");
  GLAMR_REQUIRE(((reinterpret_cast<uintptr_t>(meps) | reinterpret_cast<uintptr_t>(teps)) & 15) == 0, "glamr_latents_draw: meps and teps must be 16-byte aligned");
  GLAMR_REQUIRE((int64_t)n_windows * (rng::NZ / 4) < MAX_BLOCKS / 2, "glamr_latents_draw: n_windows too large");
  const int64_t threads = (int64_t)n_slots * ((int64_t)n_windows + 1) * (rng::NZ / 4);
  GLAMR_REQUIRE(threads / RNG_THREADS < 0x7fffffff, "glamr_latents_draw: batch too large for one launch");
  hipLaunchKernelGGL(latents_draw_kernel, dim3(grid_for(threads)), dim3(RNG_THREADS), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const uint32_t*>(seed_dev), seq_ids,
                     person_ids, n_slots, n_windows, reinterpret_cast<float4*>(meps), reinterpret_cast<float4*>(teps));
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}

extern "C" int glamr_rng_set_seed(uint64_t* seed_dev, uint64_t seed, void* stream) {
  GLAMR_REQUIRE(seed_dev, "glamr_rng_set_seed: null argument");
  hipLaunchKernelGGL(rng_set_seed_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), reinterpret_cast<uint32_t*>(seed_dev), (uint32_t)seed,
                     (uint32_t)(seed >> 32));
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}
