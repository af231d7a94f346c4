// TEST INFRASTRUCTURE: exposes the integer path of glamr_amd/csrc/rng_algo.hpp to Python (g++ build, host only) so it can be compared with
// the NumPy twin (tests/philox_ref.py).  Not part of the product library.
#include "../../glamr_amd/csrc/rng_algo.hpp"
using namespace glamr::rng;

// raw philox4x32-10: ctr (n, 4), key (n, 2) -> out (n, 4)
extern "C" void t_philox(int n, const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  for (int i = 0; i < n; ++i) {
    const Block b = philox4x32_10(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key[2 * i], key[2 * i + 1]);
    for (int j = 0; j < 4; ++j) out[4 * i + j] = b.w[j];
  }
}

// the stream layout: (seed, seq_id, sub, block) per row -> out (n, 4)
extern "C" void t_stream_blocks(int n, const uint64_t* seed, const uint64_t* seq_id, const uint32_t* sub, const uint32_t* block, uint32_t* out) {
  for (int i = 0; i < n; ++i) {
    const Block b = stream_block(seed[i], seq_id[i], sub[i], block[i]);
    for (int j = 0; j < 4; ++j) out[4 * i + j] = b.w[j];
  }
}

extern "C" uint32_t t_substream(int32_t person_id, int prior) { return substream(person_id, prior); }
