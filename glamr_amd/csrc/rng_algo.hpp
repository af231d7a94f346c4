// The counter-based generator behind the priors' latent draws: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
// as 1, 2, 3", SC'11) and the stream layout of DESIGN.md 10.  Integer arithmetic only, no HIP construct outside __HIPCC__ guards: the host
// test-suite compiles this header with g++ (tests/hostsim/rng_host.cpp) and compares it with a NumPy restatement (tests/philox_ref.py).
//
//   key     = the 64-bit seed, low word first
//   counter = (block, sub, seq_id low, seq_id high)
//     block : index of the 4-value block inside one (person, prior) array; element e of the array is output word e % 4 of block e / 4
//     sub   : 2 * person_id + prior        (prior 0 = motion infiller, 1 = trajectory predictor)
//     seq_id: 64-bit sequence id
// `block` is the only block counter: a range is never carried into `sub`.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GLAMR_RNG_HD __host__ __device__ __forceinline__
#else
#define GLAMR_RNG_HD inline
#endif

namespace glamr {
namespace rng {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // Weyl increments of the key
constexpr int PHILOX_ROUNDS = 10;
constexpr int PRIOR_INFILLER = 0, PRIOR_TRAJ = 1;
constexpr int NZ = 128;                                                    // latent width of both priors: 32 blocks per window / per trajectory draw

GLAMR_RNG_HD uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

struct Block {
  uint32_t w[4];
};

// philox4x32-10 of counter c under key (k0, k1)
GLAMR_RNG_HD Block philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < PHILOX_ROUNDS; ++r) {
    const uint32_t hi0 = mulhi32(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = mulhi32(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  return Block{{c0, c1, c2, c3}};
}

GLAMR_RNG_HD uint32_t substream(int32_t person_id, int prior) { return (uint32_t)person_id * 2u + (uint32_t)prior; }

// block `block` of sub-stream `sub` of sequence `seq_id` under `seed`
GLAMR_RNG_HD Block stream_block(uint64_t seed, uint64_t seq_id, uint32_t sub, uint32_t block) {
  return philox4x32_10(block, sub, (uint32_t)seq_id, (uint32_t)(seq_id >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

}  // namespace rng
}  // namespace glamr
