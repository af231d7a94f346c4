// TEST INFRASTRUCTURE (tests/test_rotmath_gpu.py builds and runs it; tests/test_rotmath_ref.py compiles it): every primitive of
// glamr_amd/csrc/rotmath.hpp on the device, one thread per row, under whatever flags this file is compiled with -- the library's default flags,
// those of grecon.hip, or -DGLAMR_ROTMATH_IEEE=1 with those of init.hip.  The rows, the fp64 reference and the tolerances live in
// tests/rotmath_ref_common.py.
//
//   rotmath_probe <in> <out>     (`rotmath_probe --table` prints the table alone, without touching a device)
//   <in>   int32 magic, int32 number of blocks, then per block: int32 primitive id, int32 rows n, n x NIN fp32 inputs and, for a primitive with a
//          backward, n x NOUT fp32 upstream gradients
//   <out>  per block, in the same order: n x NOUT fp32 forward values and, for a primitive with a backward, n x NIN fp32 input gradients
//          (accumulated into zeros, as tests/hostsim/rotmath_shim.cpp does)
// Every HIP call is checked; the first error ends the program with a non-zero status before anything else is launched.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../glamr_amd/csrc/rotmath.hpp"
using namespace glamr::rm;

#define CHECK(call)                                                                                   \
  do {                                                                                                \
    const hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) {                                                                           \
      std::fprintf(stderr, "rotmath_probe: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
      std::exit(1);                                                                                   \
    }                                                                                                 \
  } while (0)

typedef void (*kernel_t)(int, const float*, const float*, float*, float*);

#define PROBE(name, NIN, NOUT, HASB, FWD, BWD)                                                                          \
  __global__ void k_##name(int n, const float* __restrict__ x, const float* __restrict__ gout, float* __restrict__ out, \
                           float* __restrict__ gx) {                                                                    \
    const int i = blockIdx.x * blockDim.x + threadIdx.x;                                                                \
    if (i >= n) return;                                                                                                 \
    float xi[NIN], gi[NIN], oi[NOUT], go[NOUT];                                                                         \
    for (int k = 0; k < NIN; ++k) { xi[k] = x[(size_t)i * NIN + k]; gi[k] = 0.f; }                                      \
    for (int k = 0; k < NOUT; ++k) { oi[k] = 0.f; go[k] = HASB ? gout[(size_t)i * NOUT + k] : 0.f; }                     \
    FWD;                                                                                                                \
    BWD;                                                                                                                \
    for (int k = 0; k < NOUT; ++k) out[(size_t)i * NOUT + k] = oi[k];                                                   \
    if (HASB)                                                                                                           \
      for (int k = 0; k < NIN; ++k) gx[(size_t)i * NIN + k] = gi[k];                                                    \
  }

PROBE(rot6d_to_rotmat, 6, 9, 1, rot6d_to_rotmat(xi, oi), rot6d_to_rotmat_bwd(xi, go, gi))
PROBE(rotmat_to_quat, 9, 4, 1, rotmat_to_quat(xi, oi), rotmat_to_quat_bwd(xi, go, gi))
PROBE(quat_to_aa, 4, 3, 1, quat_to_aa(xi, oi), quat_to_aa_bwd(xi, go, gi))
PROBE(aa_to_quat, 3, 4, 1, aa_to_quat(xi, oi), aa_to_quat_bwd(xi, go, gi))
PROBE(aa_to_rotmat_k, 3, 9, 1, aa_to_rotmat_k(xi, oi), aa_to_rotmat_k_bwd(xi, go, gi))
PROBE(aa_to_rotmat_s, 3, 9, 1, aa_to_rotmat_s(xi, oi), aa_to_rotmat_s_bwd(xi, go, gi))
PROBE(rotmat_to_aa, 9, 3, 1, rotmat_to_aa(xi, oi), rotmat_to_aa_bwd(xi, go, gi))
PROBE(quat_mul, 8, 4, 1, quat_mul(xi, xi + 4, oi), quat_mul_bwd(xi, xi + 4, go, gi, gi + 4))
PROBE(atan2s, 2, 1, 1, oi[0] = atan2s(xi[0], xi[1]), atan2s_bwd(xi[0], xi[1], go[0], gi[0], gi[1]))
PROBE(normalize3, 3, 3, 1, normalize3(xi, oi), normalize3_bwd(xi, go, gi))
PROBE(quat_to_rotmat, 4, 9, 0, quat_to_rotmat(xi, oi), (void)go)
PROBE(quat_rotate, 7, 3, 0, quat_rotate(xi, xi + 4, oi), (void)go)
PROBE(quat_heading, 4, 1, 0, oi[0] = quat_heading(xi), (void)go)
PROBE(quat_heading_q, 4, 4, 0, quat_heading_q(xi, oi), (void)go)
PROBE(heading_quat, 1, 4, 1, heading_quat(xi[0], oi), gi[0] += heading_quat_bwd(xi[0], go))
PROBE(sdiv, 2, 1, 1, oi[0] = sdiv(xi[0], xi[1]), sdiv_bwd(xi[0], xi[1], go[0], gi[0], gi[1]))
PROBE(sqrt_clamped, 1, 1, 1, oi[0] = sqrt_clamped(xi[0], 1e-6f), gi[0] += sqrt_clamped_bwd(xi[0], 1e-6f, go[0]))
PROBE(mat3_mul, 18, 9, 1, mat3_mul(xi, xi + 9, oi), mat3_mul_bwd(xi, xi + 9, go, gi, gi + 9))
PROBE(quat_mul_plain, 8, 4, 0, quat_mul_plain(xi, xi + 4, oi), (void)go)
// the operand arrays: div_(n, d), sqrt_rn_(x), sincos_(x) -> (sin, cos)
PROBE(div, 2, 1, 0, oi[0] = div_(xi[0], xi[1]), (void)go)
PROBE(sqrt_rn, 1, 1, 0, oi[0] = sqrt_rn_(xi[0]), (void)go)
PROBE(sincos, 1, 2, 0, sincos_(xi[0], oi[0], oi[1]), (void)go)

struct Entry { const char* name; int nin, nout, hasb; kernel_t kernel; };
#define ENTRY(name, NIN, NOUT, HASB) {#name, NIN, NOUT, HASB, k_##name}
static const Entry TABLE[] = {
    ENTRY(rot6d_to_rotmat, 6, 9, 1), ENTRY(rotmat_to_quat, 9, 4, 1), ENTRY(quat_to_aa, 4, 3, 1),     ENTRY(aa_to_quat, 3, 4, 1),
    ENTRY(aa_to_rotmat_k, 3, 9, 1),  ENTRY(aa_to_rotmat_s, 3, 9, 1), ENTRY(rotmat_to_aa, 9, 3, 1),   ENTRY(quat_mul, 8, 4, 1),
    ENTRY(atan2s, 2, 1, 1),          ENTRY(normalize3, 3, 3, 1),     ENTRY(quat_to_rotmat, 4, 9, 0), ENTRY(quat_rotate, 7, 3, 0),
    ENTRY(quat_heading, 4, 1, 0),    ENTRY(quat_heading_q, 4, 4, 0), ENTRY(heading_quat, 1, 4, 1),   ENTRY(sdiv, 2, 1, 1),
    ENTRY(sqrt_clamped, 1, 1, 1),    ENTRY(mat3_mul, 18, 9, 1),      ENTRY(quat_mul_plain, 8, 4, 0), ENTRY(div, 2, 1, 0),
    ENTRY(sqrt_rn, 1, 1, 0),         ENTRY(sincos, 1, 2, 0),
};
static const int N_TABLE = (int)(sizeof(TABLE) / sizeof(TABLE[0]));
static const int MAGIC = 0x31504d52;          // "RMP1"
static const int MAX_ROWS = 1 << 22;

static void fail(const char* what) {
  std::fprintf(stderr, "rotmath_probe: %s\n", what);
  std::exit(1);
}
static void read_exact(void* p, size_t bytes, FILE* f) {
  if (bytes && std::fread(p, 1, bytes, f) != bytes) fail("input file is shorter than its blocks say");
}
static void write_exact(const void* p, size_t bytes, FILE* f) {
  if (bytes && std::fwrite(p, 1, bytes, f) != bytes) fail("cannot write the output file");
}

int main(int argc, char** argv) {
  for (int t = 0; t < N_TABLE; ++t) std::printf("table %d %s %d %d %d\n", t, TABLE[t].name, TABLE[t].nin, TABLE[t].nout, TABLE[t].hasb);
  if (argc == 2 && std::string(argv[1]) == "--table") return 0;
  if (argc != 3) fail("usage: rotmath_probe <in> <out> | --table");
  FILE* fin = std::fopen(argv[1], "rb");
  if (!fin) fail("cannot open the input file");
  FILE* fout = std::fopen(argv[2], "wb");
  if (!fout) fail("cannot open the output file");
  int head[2];
  read_exact(head, sizeof(head), fin);
  if (head[0] != MAGIC || head[1] < 0 || head[1] > 4096) fail("not a rotmath_probe input file");
  std::vector<float> hx, hg, ho, hgx;
  for (int b = 0; b < head[1]; ++b) {
    int bh[2];
    read_exact(bh, sizeof(bh), fin);
    const int id = bh[0], n = bh[1];
    if (id < 0 || id >= N_TABLE || n < 0 || n > MAX_ROWS) fail("block with an unknown primitive or a row count out of range");
    const Entry& e = TABLE[id];
    const size_t nx = (size_t)n * e.nin, no = (size_t)n * e.nout;
    hx.resize(nx); ho.resize(no);
    hg.resize(e.hasb ? no : 0); hgx.resize(e.hasb ? nx : 0);
    read_exact(hx.data(), nx * sizeof(float), fin);
    read_exact(hg.data(), hg.size() * sizeof(float), fin);
    if (n > 0) {
      float *dx = nullptr, *dg = nullptr, *dout = nullptr, *dgx = nullptr;
      CHECK(hipMalloc(&dx, nx * sizeof(float)));
      CHECK(hipMalloc(&dout, no * sizeof(float)));
      CHECK(hipMemcpy(dx, hx.data(), nx * sizeof(float), hipMemcpyHostToDevice));
      CHECK(hipMemset(dout, 0, no * sizeof(float)));
      if (e.hasb) {
        CHECK(hipMalloc(&dg, no * sizeof(float)));
        CHECK(hipMalloc(&dgx, nx * sizeof(float)));
        CHECK(hipMemcpy(dg, hg.data(), no * sizeof(float), hipMemcpyHostToDevice));
        CHECK(hipMemset(dgx, 0, nx * sizeof(float)));
      }
      e.kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0>>>(n, dx, dg, dout, dgx);
      CHECK(hipGetLastError());
      CHECK(hipDeviceSynchronize());
      CHECK(hipMemcpy(ho.data(), dout, no * sizeof(float), hipMemcpyDeviceToHost));
      if (e.hasb) CHECK(hipMemcpy(hgx.data(), dgx, nx * sizeof(float), hipMemcpyDeviceToHost));
      CHECK(hipFree(dx));
      CHECK(hipFree(dout));
      if (e.hasb) { CHECK(hipFree(dg)); CHECK(hipFree(dgx)); }
    }
    write_exact(ho.data(), no * sizeof(float), fout);
    write_exact(hgx.data(), hgx.size() * sizeof(float), fout);
    std::printf("block %d %s rows %d\n", b, e.name, n);
  }
  std::fclose(fin);
  if (std::fclose(fout) != 0) fail("cannot write the output file");
  std::printf("done %d blocks\n", head[1]);
  return 0;
}
