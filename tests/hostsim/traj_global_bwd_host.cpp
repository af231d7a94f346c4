// TEST INFRASTRUCTURE: the algorithm of glamr_amd/csrc/traj_global_bwd.hpp (what glamr_traj_local_to_global_backward launches) on the
// single-threaded host runtime of grecon_host.cpp, with host pointers.  Never loaded by the product.
//
// The runtime's scan is given the DEVICE's order of additions (DeviceRT::scan with 256 threads: Hillis-Steele inside each run of 64 elements,
// the runs' totals added in order, a carry per chunk of 256), not HostRT's serial loop.  The headings of the large-turn sequences are prefix
// sums of hundreds of radians: the serial fp32 loop accumulates one rounding of ~3e-5 rad per frame and ends 8 - 19 x above the fp32 autograd
// floor there (torch's CPU cumsum accumulates in double), the device's tree at most 4 x.  `serial` = 1 runs HostRT's loop (reported by the test).
#include "grecon_host.cpp"
#include "../../glamr_amd/csrc/traj_global_bwd.hpp"

struct DeviceOrderRT : HostRT {
  void scan(float* a, int n, int stride, bool reverse) const {
    const int BLOCK = 256, NW = BLOCK / 64;
    float carry = 0.f;
    for (int base = 0; base < n; base += BLOCK) {
      float x[BLOCK], red[NW];
      for (int j = 0; j < BLOCK; ++j) { const int i = base + j; x[j] = i < n ? a[(size_t)(reverse ? n - 1 - i : i) * stride] : 0.f; }
      for (int off = 1; off < 64; off <<= 1)
        for (int j = BLOCK - 1; j >= 0; --j) if ((j & 63) >= off) x[j] += x[j - off];      // (descending j: x[j - off] is still the previous round's)
      for (int w = 0; w < NW; ++w) red[w] = x[w * 64 + 63];
      float tot = 0.f;
      for (int w = 0; w < NW; ++w) tot += red[w];
      for (int j = 0; j < BLOCK; ++j) {
        const int i = base + j;
        float pre = carry;
        for (int w = 0; w < (j >> 6); ++w) pre += red[w];
        if (i < n) a[(size_t)(reverse ? n - 1 - i : i) * stride] = x[j] + pre;
      }
      carry += tot;
    }
  }
};

// lens: (n_seq) or null = T; the upstream arrays may be null; g_local_traj (n_seq, T, 11)
extern "C" int hostsim_traj_global_bwd(int n_seq, int T, const int32_t* lens, const float* local_traj, const float* g_trans, const float* g_orient, const float* g_orient_q,
                                       float* g_local_traj, int serial) {
  if (n_seq < 0 || T < 1 || !local_traj || !g_local_traj || !(g_trans || g_orient || g_orient_q)) return -1;
  std::vector<float> ws((size_t)T * glamr::TGB_WS_FLOATS_PER_FRAME);
  HostRT srt;
  DeviceOrderRT drt;
  for (int b = 0; b < n_seq; ++b) {
    const size_t f = (size_t)b * T;
    int n = lens ? lens[b] : T;
    n = n < 0 ? 0 : (n > T ? T : n);
    const float* gt = g_trans ? g_trans + f * 3 : nullptr;
    const float* go = g_orient ? g_orient + f * 3 : nullptr;
    const float* gq = g_orient_q ? g_orient_q + f * 4 : nullptr;
    if (serial) glamr::traj_global_bwd(srt, n, T, local_traj + f * 11, gt, go, gq, g_local_traj + f * 11, ws.data());
    else glamr::traj_global_bwd(drt, n, T, local_traj + f * 11, gt, go, gq, g_local_traj + f * 11, ws.data());
  }
  return 0;
}
