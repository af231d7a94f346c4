// glamr_sdf_penetration: the multi-person penetration term of the reference's loss_func_dict (loss_func.py:274-290), whose SDFLoss comes from
// a third-party package -- restated in DESIGN.md 18.  Four launches on the caller's stream:
//   sdf_boxes_kernel   one workgroup per (frame, person): bounding boxes of the frame's active persons, overlap flags, N_f
//   sdf_grid_kernel    the hot path: phi of every overlapping mesh, brute force over (voxel, face) pairs.  A workgroup owns 1024 voxels of one
//                      mesh, four per lane; the faces go through LDS in tiles of 256 records (sdf.hpp: face_record) that every lane reads at
//                      the same address (broadcast), so one record serves the lane's four voxels
//   sdf_sample_kernel  one workgroup per (frame, sampled person): trilinear samples of the other overlapping persons' grids at its vertices,
//                      robustifier, the gradient to its own vertices (stored: only that lane writes it) and the person's partial sum
//   sdf_finish_kernel  L_f = sum over the persons in index order / N_f^2
// Plain fp32, no atomics, every sum in a fixed order: two calls give the same bits.  Activity, boxes and the overlap decision stay on the
// device; the host side checks its arguments and launches, so the call can be recorded into a stream capture.
#include "common.hpp"
#include "sdf.hpp"

namespace glamr {
namespace {

constexpr int SDF_THREADS = 256;
constexpr int SDF_VOX_PER_LANE = 4;
constexpr int SDF_VOX_PER_BLOCK = SDF_THREADS * SDF_VOX_PER_LANE;
constexpr int SDF_TILE = 256;                 // faces per LDS tile: one record per thread and staging pass, 20 KiB
constexpr int SDF_MAX_PERSONS = 32;
constexpr float SDF_PI = 3.14159265358979323846f;

struct SdfWs {                                // carved out of the caller's workspace
  float* boxes;                               // (F, P, 6) lo, hi
  int* overlap;                               // (F, P)
  int* nf;                                    // (F)
  float* partial;                             // (F, P) per sampled person: sum of r(sample) over sources and vertices
  float* phi;                                 // (F, P, G, G, G)
};

size_t sdf_ws_carve(int F, int P, int G, char* base, SdfWs* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += align_up(bytes, 256); return p; };
  char* boxes = take((size_t)F * P * 6 * sizeof(float));
  char* overlap = take((size_t)F * P * sizeof(int));
  char* nf = take((size_t)F * sizeof(int));
  char* partial = take((size_t)F * P * sizeof(float));
  char* phi = take((size_t)F * P * G * G * G * sizeof(float));
  if (w) *w = SdfWs{reinterpret_cast<float*>(boxes), reinterpret_cast<int*>(overlap), reinterpret_cast<int*>(nf), reinterpret_cast<float*>(partial),
                    reinterpret_cast<float*>(phi)};
  return off;
}

// min / max of six values over the workgroup: wave shuffles, then the four waves' results through LDS.  min and max are exact, so the order
// does not matter.  Every thread returns with the result in v.
__device__ void block_minmax(float (&v)[6], float (*ex)[6]) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const float o = __shfl_xor(v[k], off, 64);
      v[k] = k < 3 ? fminf(v[k], o) : fmaxf(v[k], o);
    }
  const int wave = threadIdx.x >> 6;
  __syncthreads();                            // (ex may still be read from the previous person)
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 6; ++k) ex[wave][k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    float r = ex[0][k];
    for (int w = 1; w < SDF_THREADS / 64; ++w) r = k < 3 ? fminf(r, ex[w][k]) : fmaxf(r, ex[w][k]);
    v[k] = r;
  }
}

// grid (F * P).  Every workgroup of a frame needs every active person's box for its own flag, so it reduces them all (P times the reads of a
// pass that is a few microseconds); an inactive person's vertices are never read.
__global__ __launch_bounds__(SDF_THREADS) void sdf_boxes_kernel(const float* __restrict__ verts, const unsigned char* __restrict__ active, int P, int V,
                                                                 float* __restrict__ boxes, int* __restrict__ overlap, int* __restrict__ nf,
                                                                 float* __restrict__ boxes_out, int* __restrict__ overlap_out) {
  __shared__ float ex[SDF_THREADS / 64][6];
  __shared__ float sbox[SDF_MAX_PERSONS][6];
  const int p = blockIdx.x % P, f = blockIdx.x / P;
  const size_t fp = (size_t)f * P + p;
  const unsigned char* act = active + (size_t)f * P;
  for (int q = 0; q < P; ++q) {
    if (!act[q]) continue;                    // (uniform over the workgroup)
    const float* x = verts + ((size_t)f * P + q) * V * 3;
    const float inf = __builtin_huge_valf();
    float v[6] = {inf, inf, inf, -inf, -inf, -inf};
    for (int i = threadIdx.x; i < V; i += SDF_THREADS) {
      const float a = x[3 * i], b = x[3 * i + 1], c = x[3 * i + 2];
      v[0] = fminf(v[0], a); v[1] = fminf(v[1], b); v[2] = fminf(v[2], c);
      v[3] = fmaxf(v[3], a); v[4] = fmaxf(v[4], b); v[5] = fmaxf(v[5], c);
    }
    block_minmax(v, ex);
    if (threadIdx.x < 6) sbox[q][threadIdx.x] = v[threadIdx.x];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int mine = 0, count = 0;
    for (int a = 0; a < P; ++a) {
      if (!act[a]) continue;
      int hit = 0;
      for (int b = 0; b < P; ++b) hit |= (b != a && act[b] && sdf::boxes_overlap(sbox[a], sbox[b])) ? 1 : 0;
      count += hit;
      if (a == p) mine = hit;
    }
    overlap[fp] = mine;
    if (overlap_out) overlap_out[fp] = mine;
    if (p == 0) nf[f] = count;
  }
  if (threadIdx.x < 6) {
    const float b = act[p] ? sbox[p][threadIdx.x] : 0.f;
    boxes[fp * 6 + threadIdx.x] = b;
    if (boxes_out) boxes_out[fp * 6 + threadIdx.x] = b;
  }
}

// grid (F * P, ceil(G^3 / 1024)).  phi goes to `phi` (the workspace, or the caller's phi_out); a mesh that overlaps nothing exits at once and
// writes zeros only where the caller asked to see the grid.
__global__ __launch_bounds__(SDF_THREADS) void sdf_grid_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int V, int NF, int G,
                                                                float scale_factor, const float* __restrict__ boxes, const int* __restrict__ overlap,
                                                                float* __restrict__ phi, int zero_isolated) {
  __shared__ __attribute__((aligned(16))) float tile[SDF_TILE * sdf::FACE_FLOATS];
  const int mesh = blockIdx.x;
  const int G3 = G * G * G;
  const int vox0 = blockIdx.y * SDF_VOX_PER_BLOCK + threadIdx.x;
  float* out = phi + (size_t)mesh * G3;
  if (!overlap[mesh]) {
    if (zero_isolated)
#pragma unroll
      for (int j = 0; j < SDF_VOX_PER_LANE; ++j)
        if (vox0 + j * SDF_THREADS < G3) out[vox0 + j * SDF_THREADS] = 0.f;
    return;
  }
  const sdf::Norm nm = sdf::box_norm(boxes + (size_t)mesh * 6, scale_factor);
  const float* x = verts + (size_t)mesh * V * 3;
  float px[SDF_VOX_PER_LANE], py[SDF_VOX_PER_LANE], pz[SDF_VOX_PER_LANE], dmin2[SDF_VOX_PER_LANE], wsum[SDF_VOX_PER_LANE];
#pragma unroll
  for (int j = 0; j < SDF_VOX_PER_LANE; ++j) {
    const int vox = vox0 + j * SDF_THREADS;   // (past G^3: computed on a voxel outside the grid and not stored)
    const int kx = vox % G, ky = (vox / G) % G, kz = vox / (G * G);
    px[j] = sdf::voxel_centre(kx, G); py[j] = sdf::voxel_centre(ky, G); pz[j] = sdf::voxel_centre(kz, G);
    dmin2[j] = __builtin_huge_valf(); wsum[j] = 0.f;
  }
  for (int base = 0; base < NF; base += SDF_TILE) {
    const int nt = min(SDF_TILE, NF - base);
    __syncthreads();                          // the previous tile has been read
    if ((int)threadIdx.x < nt) {
      const int* fi = faces + (size_t)(base + threadIdx.x) * 3;
      float c[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int vi = min(max(fi[k], 0), V - 1);      // an index outside the mesh is clamped, never followed
        c[k][0] = (x[3 * vi] - nm.cx) / nm.s; c[k][1] = (x[3 * vi + 1] - nm.cy) / nm.s; c[k][2] = (x[3 * vi + 2] - nm.cz) / nm.s;
      }
      float r[sdf::FACE_FLOATS];
      sdf::face_record(c[0], c[1], c[2], r);
      float4* dst = reinterpret_cast<float4*>(tile + threadIdx.x * sdf::FACE_FLOATS);
#pragma unroll
      for (int k = 0; k < sdf::FACE_FLOATS / 4; ++k) dst[k] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
    }
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      float r[sdf::FACE_FLOATS];
      const float4* src = reinterpret_cast<const float4*>(tile + t * sdf::FACE_FLOATS);
#pragma unroll
      for (int k = 0; k < sdf::FACE_FLOATS / 4; ++k) {
        const float4 q = src[k];
        r[4 * k] = q.x; r[4 * k + 1] = q.y; r[4 * k + 2] = q.z; r[4 * k + 3] = q.w;
      }
      const float abx = r[3] - r[0], aby = r[4] - r[1], abz = r[5] - r[2];
      const float acx = r[6] - r[0], acy = r[7] - r[1], acz = r[8] - r[2];
      const float bcx = r[6] - r[3], bcy = r[7] - r[4], bcz = r[8] - r[5];
#pragma unroll
      for (int j = 0; j < SDF_VOX_PER_LANE; ++j)
        sdf::point_face(px[j], py[j], pz[j], r, abx, aby, abz, acx, acy, acz, bcx, bcy, bcz, dmin2[j], wsum[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < SDF_VOX_PER_LANE; ++j) {
    const int vox = vox0 + j * SDF_THREADS;
    if (vox < G3) out[vox] = wsum[j] > SDF_PI ? sqrtf(dmin2[j]) : 0.f;      // winding number > 1/2 (wsum holds half the solid angles)
  }
}

// grid (F * P): the workgroup samples person q = blockIdx.x % P of frame blockIdx.x / P in the grids of the frame's other overlapping persons.
__global__ __launch_bounds__(SDF_THREADS) void sdf_sample_kernel(const float* __restrict__ verts, int P, int V, int G, float scale_factor, float rho,
                                                                  const float* __restrict__ boxes, const int* __restrict__ overlap,
                                                                  const int* __restrict__ nf, const float* __restrict__ phi,
                                                                  float* __restrict__ g_verts, float* __restrict__ partial) {
  __shared__ float red[SDF_THREADS];
  __shared__ sdf::Norm snorm[SDF_MAX_PERSONS];
  const int q = blockIdx.x % P, f = blockIdx.x / P;
  const size_t fq = (size_t)f * P + q;
  const int* ov = overlap + (size_t)f * P;
  float* g = g_verts ? g_verts + fq * V * 3 : nullptr;
  if (!ov[q]) {                               // inactive or isolated: zeros, and its vertices are not read
    if (g)
      for (int i = threadIdx.x; i < V * 3; i += SDF_THREADS) g[i] = 0.f;
    if (threadIdx.x == 0) partial[fq] = 0.f;
    return;
  }
  if ((int)threadIdx.x < P && ov[threadIdx.x]) snorm[threadIdx.x] = sdf::box_norm(boxes + ((size_t)f * P + threadIdx.x) * 6, scale_factor);
  __syncthreads();
  const int n = nf[f];
  const float inv_n2 = 1.f / ((float)n * (float)n);
  const float* x = verts + fq * V * 3;
  const size_t G3 = (size_t)G * G * G;
  float acc = 0.f;
  for (int i = threadIdx.x; i < V; i += SDF_THREADS) {
    const float vx = x[3 * i], vy = x[3 * i + 1], vz = x[3 * i + 2];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int p = 0; p < P; ++p) {
      if (p == q || !ov[p]) continue;
      const sdf::Norm nm = snorm[p];
      float dx, dy, dz, dr;
      const float val = sdf::trilinear(phi + ((size_t)f * P + p) * G3, G, (vx - nm.cx) / nm.s, (vy - nm.cy) / nm.s, (vz - nm.cz) / nm.s, dx, dy, dz);
      acc += sdf::robust(val, rho, dr);
      const float k = dr / nm.s;
      gx += k * dx; gy += k * dy; gz += k * dz;
    }
    if (g) { g[3 * i] = gx * inv_n2; g[3 * i + 1] = gy * inv_n2; g[3 * i + 2] = gz * inv_n2; }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = SDF_THREADS / 2; s >= 1; s >>= 1) {      // a fixed tree
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[fq] = red[0];
}

__global__ void sdf_finish_kernel(int F, int P, const int* __restrict__ nf, const float* __restrict__ partial, float* __restrict__ loss) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const int n = nf[f];
  float s = 0.f;
  for (int q = 0; q < P; ++q) s += partial[(size_t)f * P + q];
  loss[f] = n > 0 ? s / ((float)n * (float)n) : 0.f;
}

bool sdf_sizes_ok(int F, int P, int V, int NF, int G) {
  return F >= 0 && P >= 1 && P <= SDF_MAX_PERSONS && V >= 1 && NF >= 1 && G >= 2 && G <= 64 && (int64_t)F * P < (1 << 24) &&
         (int64_t)V * 3 < 0x7fffffff && (int64_t)NF * 3 < 0x7fffffff;
}

}  // namespace
}  // namespace glamr

extern "C" size_t glamr_sdf_workspace_bytes(int n_frames, int n_persons, int n_verts, int n_faces, int grid) {
  if (!glamr::sdf_sizes_ok(n_frames, n_persons, n_verts, n_faces, grid) || n_frames == 0) return 0;
  return glamr::sdf_ws_carve(n_frames, n_persons, grid, nullptr, nullptr);
}

extern "C" int glamr_sdf_penetration(const float* verts, const unsigned char* active, const int* faces, int F, int P, int V, int NF, int grid,
                                     float scale_factor, float rho, float* loss, float* g_verts, float* phi_out, float* boxes_out, int* overlap_out,
                                     void* ws, void* stream) {
  using namespace glamr;
  GLAMR_REQUIRE(sdf_sizes_ok(F, P, V, NF, grid), "glamr_sdf_penetration: bad sizes (0 <= F, F * P < 2^24, 1 <= P <= 32, V >= 1, NF >= 1, 2 <= grid <= 64)");
  GLAMR_REQUIRE(scale_factor > -1.f && rho >= 0.f, "glamr_sdf_penetration: scale_factor must exceed -1 and rho must not be negative (0 switches the robustifier off)");
  if (F == 0) return GLAMR_OK;
  GLAMR_REQUIRE(verts && active && faces && loss && ws, "glamr_sdf_penetration: NULL argument (verts, active, faces, loss, ws)");
  GLAMR_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "glamr_sdf_penetration: the workspace must be 16-byte aligned");
  SdfWs w;
  sdf_ws_carve(F, P, grid, static_cast<char*>(ws), &w);
  float* phi = phi_out ? phi_out : w.phi;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(SDF_THREADS), per_person(F * P);
  const int G3 = grid * grid * grid;
  hipLaunchKernelGGL(sdf_boxes_kernel, per_person, block, 0, s, verts, active, P, V, w.boxes, w.overlap, w.nf, boxes_out, overlap_out);
  GLAMR_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(sdf_grid_kernel, dim3(F * P, (G3 + SDF_VOX_PER_BLOCK - 1) / SDF_VOX_PER_BLOCK), block, 0, s, verts, faces, V, NF, grid, scale_factor,
                     w.boxes, w.overlap, phi, phi_out ? 1 : 0);
  GLAMR_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(sdf_sample_kernel, per_person, block, 0, s, verts, P, V, grid, scale_factor, rho, w.boxes, w.overlap, w.nf, phi, g_verts, w.partial);
  GLAMR_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(sdf_finish_kernel, dim3((F + 63) / 64), dim3(64), 0, s, F, P, w.nf, w.partial, loss);
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}
