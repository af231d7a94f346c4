// TEST INFRASTRUCTURE: the arithmetic of glamr_amd/csrc/sdf.hpp (what glamr_sdf_penetration launches) on the host, in the kernels' order of
// operations -- boxes and flags, the grid, the sample with its 256-lane strided sums and fixed tree, the pass over the persons -- with host
// pointers and the entry point's argument checks.  Never loaded by the product.
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>
#include "../../glamr_amd/csrc/sdf.hpp"

using namespace glamr::sdf;

// 0, or -1 (GLAMR_E_INVALID).  Outputs as the entry point's; phi_out / boxes_out / overlap_out / g_verts may be NULL.
extern "C" int hostsim_sdf_penetration(const float* verts, const unsigned char* active, const int* faces, int F, int P, int V, int NF, int G,
                                       float scale_factor, float rho, float* loss, float* g_verts, float* phi_out, float* boxes_out, int* overlap_out) {
  if (F < 0 || P < 1 || P > 32 || V < 1 || NF < 1 || G < 2 || G > 64 || !(scale_factor > -1.f) || !(rho >= 0.f)) return -1;
  if (F == 0) return 0;
  if (!verts || !active || !faces || !loss) return -1;
  const size_t G3 = (size_t)G * G * G;
  const float inf = std::numeric_limits<float>::infinity();
  std::vector<float> boxes((size_t)P * 6), phi((size_t)P * G3), partial(P), rec((size_t)NF * FACE_FLOATS);
  std::vector<int> flag(P);
  for (int f = 0; f < F; ++f) {
    const unsigned char* act = active + (size_t)f * P;
    for (int p = 0; p < P; ++p) {
      float* b = &boxes[(size_t)p * 6];
      for (int k = 0; k < 6; ++k) b[k] = 0.f;
      if (!act[p]) continue;
      for (int k = 0; k < 3; ++k) { b[k] = inf; b[3 + k] = -inf; }
      const float* x = verts + ((size_t)f * P + p) * V * 3;
      for (int i = 0; i < V; ++i)
        for (int k = 0; k < 3; ++k) { b[k] = fminf(b[k], x[3 * i + k]); b[3 + k] = fmaxf(b[3 + k], x[3 * i + k]); }
    }
    int n = 0;
    for (int p = 0; p < P; ++p) {
      flag[p] = 0;
      if (!act[p]) continue;
      for (int q = 0; q < P; ++q) flag[p] |= (q != p && act[q] && boxes_overlap(&boxes[(size_t)p * 6], &boxes[(size_t)q * 6])) ? 1 : 0;
      n += flag[p];
    }
    for (int p = 0; p < P; ++p) {
      if (boxes_out) for (int k = 0; k < 6; ++k) boxes_out[((size_t)f * P + p) * 6 + k] = boxes[(size_t)p * 6 + k];
      if (overlap_out) overlap_out[(size_t)f * P + p] = flag[p];
      float* ph = &phi[(size_t)p * G3];
      if (flag[p]) {
        const Norm nm = box_norm(&boxes[(size_t)p * 6], scale_factor);
        const float* x = verts + ((size_t)f * P + p) * V * 3;
        for (int t = 0; t < NF; ++t) {
          float c[3][3];
          for (int k = 0; k < 3; ++k) {
            int vi = faces[3 * t + k];
            vi = vi < 0 ? 0 : (vi > V - 1 ? V - 1 : vi);
            c[k][0] = (x[3 * vi] - nm.cx) / nm.s; c[k][1] = (x[3 * vi + 1] - nm.cy) / nm.s; c[k][2] = (x[3 * vi + 2] - nm.cz) / nm.s;
          }
          face_record(c[0], c[1], c[2], &rec[(size_t)t * FACE_FLOATS]);
        }
        for (size_t vox = 0; vox < G3; ++vox) {
          const int kx = (int)(vox % G), ky = (int)((vox / G) % G), kz = (int)(vox / ((size_t)G * G));
          const float px = voxel_centre(kx, G), py = voxel_centre(ky, G), pz = voxel_centre(kz, G);
          float dmin2 = inf, wsum = 0.f;
          for (int t = 0; t < NF; ++t) {
            const float* r = &rec[(size_t)t * FACE_FLOATS];
            point_face(px, py, pz, r, r[3] - r[0], r[4] - r[1], r[5] - r[2], r[6] - r[0], r[7] - r[1], r[8] - r[2], r[6] - r[3], r[7] - r[4], r[8] - r[5],
                       dmin2, wsum);
          }
          ph[vox] = wsum > 3.14159265358979323846f ? sqrtf(dmin2) : 0.f;
        }
      } else {
        for (size_t vox = 0; vox < G3; ++vox) ph[vox] = 0.f;
      }
      if (phi_out) for (size_t vox = 0; vox < G3; ++vox) phi_out[((size_t)f * P + p) * G3 + vox] = ph[vox];
    }
    const float inv_n2 = n > 0 ? 1.f / ((float)n * (float)n) : 0.f;
    for (int q = 0; q < P; ++q) {
      float* g = g_verts ? g_verts + ((size_t)f * P + q) * V * 3 : nullptr;
      partial[q] = 0.f;
      if (!flag[q]) {
        if (g) for (int i = 0; i < V * 3; ++i) g[i] = 0.f;
        continue;
      }
      const float* x = verts + ((size_t)f * P + q) * V * 3;
      float red[256];
      for (int lane = 0; lane < 256; ++lane) {
        float acc = 0.f;
        for (int i = lane; i < V; i += 256) {
          float gx = 0.f, gy = 0.f, gz = 0.f;
          for (int p = 0; p < P; ++p) {
            if (p == q || !flag[p]) continue;
            const Norm nm = box_norm(&boxes[(size_t)p * 6], scale_factor);
            float dx, dy, dz, dr;
            const float val = trilinear(&phi[(size_t)p * G3], G, (x[3 * i] - nm.cx) / nm.s, (x[3 * i + 1] - nm.cy) / nm.s, (x[3 * i + 2] - nm.cz) / nm.s, dx, dy, dz);
            acc += robust(val, rho, dr);
            const float k = dr / nm.s;
            gx += k * dx; gy += k * dy; gz += k * dz;
          }
          if (g) { g[3 * i] = gx * inv_n2; g[3 * i + 1] = gy * inv_n2; g[3 * i + 2] = gz * inv_n2; }
        }
        red[lane] = acc;
      }
      for (int s = 128; s >= 1; s >>= 1)
        for (int lane = 0; lane < s; ++lane) red[lane] += red[lane + s];
      partial[q] = red[0];
    }
    float s = 0.f;
    for (int q = 0; q < P; ++q) s += partial[q];
    loss[f] = n > 0 ? s / ((float)n * (float)n) : 0.f;
  }
  return 0;
}
