// The arithmetic of the multi-person penetration term (glamr_sdf_penetration): box normalisation, the per-face record the grid
// kernel stages, one (voxel, face) evaluation -- squared distance to the triangle and its solid angle --, the trilinear sample with zero
// padding and its coordinate gradient, and the robustifier.  Plain fp32, host and device, so the same lines can be run against fp64 on the
// CPU.  sdf.hip holds the kernels.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define GLAMR_SDF_HD __host__ __device__ inline
#else
#define GLAMR_SDF_HD inline
#endif

namespace glamr {
namespace sdf {

constexpr int FACE_FLOATS = 20;      // a, b, c, n | 1/|ab|^2, 1/|ac|^2, 1/|bc|^2, 1/|n|^2 | |ab|^2, ab.ac, |ac|^2, |n|^2: five 16-byte reads

struct Norm { float cx, cy, cz, s; };

// c = (lo + hi) / 2, s = (1 + scale_factor) / 2 . max_axis(hi - lo): the frame the grid of a mesh lives in
GLAMR_SDF_HD Norm box_norm(const float* box, float scale_factor) {
  const float ex = box[3] - box[0], ey = box[4] - box[1], ez = box[5] - box[2];
  Norm n;
  n.cx = (box[0] + box[3]) * 0.5f; n.cy = (box[1] + box[4]) * 0.5f; n.cz = (box[2] + box[5]) * 0.5f;
  n.s = ((1.f + scale_factor) * 0.5f) * fmaxf(ex, fmaxf(ey, ez));
  return n;
}

// closed intervals on all three axes (a NaN box overlaps nothing)
GLAMR_SDF_HD bool boxes_overlap(const float* p, const float* q) {
  return p[0] <= q[3] && q[0] <= p[3] && p[1] <= q[4] && q[1] <= p[4] && p[2] <= q[5] && q[2] <= p[5];
}

// The record of one face from its three corners in normalised coordinates.  A face without area gets |n|^2 = -1 (its interior test can never
// pass) and reciprocals of 0 for edges without length (the edge then stands for its first corner): no division by zero reaches a voxel.
GLAMR_SDF_HD void face_record(const float* a, const float* b, const float* c, float* r) {
  const float abx = b[0] - a[0], aby = b[1] - a[1], abz = b[2] - a[2];
  const float acx = c[0] - a[0], acy = c[1] - a[1], acz = c[2] - a[2];
  const float bcx = c[0] - b[0], bcy = c[1] - b[1], bcz = c[2] - b[2];
  const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
  const float d00 = abx * abx + aby * aby + abz * abz, d01 = abx * acx + aby * acy + abz * acz, d11 = acx * acx + acy * acy + acz * acz;
  const float dbc = bcx * bcx + bcy * bcy + bcz * bcz, nn = nx * nx + ny * ny + nz * nz;
  r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = b[0]; r[4] = b[1]; r[5] = b[2]; r[6] = c[0]; r[7] = c[1]; r[8] = c[2];
  r[9] = nx; r[10] = ny; r[11] = nz;
  r[12] = d00 > 0.f ? 1.f / d00 : 0.f; r[13] = d11 > 0.f ? 1.f / d11 : 0.f; r[14] = dbc > 0.f ? 1.f / dbc : 0.f;
  const bool flat = !(nn > 0.f);
  r[15] = flat ? 0.f : 1.f / nn;
  r[16] = d00; r[17] = d01; r[18] = d11; r[19] = flat ? -1.f : nn;
}

// atan2 to ~1e-5 relative: an odd degree-11 polynomial on [0, 1] and the three reflections.  The winding number only has to be right to
// within 1/2 (sum of |error| <= 2.3e-5 . sum |omega|); the distance carries the accuracy, not this.
GLAMR_SDF_HD float atan2_cheap(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = fmaxf(fmaxf(ax, ay), 1e-37f), mn = fminf(ax, ay);
  const float t = mn / mx, t2 = t * t;
  float p = -0.01172120f;
  p = p * t2 + 0.05265332f; p = p * t2 - 0.11643287f; p = p * t2 + 0.19354346f; p = p * t2 - 0.33262347f; p = p * t2 + 0.99997726f;
  float r = p * t;
  r = ay > ax ? 1.57079632679489661923f - r : r;
  r = x < 0.f ? 3.14159265358979323846f - r : r;
  return y < 0.f ? -r : r;
}

// squared distance from the point to the segment start + t e, t in [0, 1]; S = start - point
GLAMR_SDF_HD float seg_dist2(float Sx, float Sy, float Sz, float ex, float ey, float ez, float inv_ee) {
  float t = -(Sx * ex + Sy * ey + Sz * ez) * inv_ee;
  t = fminf(fmaxf(t, 0.f), 1.f);
  const float rx = Sx + t * ex, ry = Sy + t * ey, rz = Sz + t * ez;
  return rx * rx + ry * ry + rz * rz;
}

// One (point, face) evaluation.  Distance: the minimum over the three edges (each covers its two corners) and, where the foot of the
// perpendicular lies inside the triangle, the plane -- all seven regions of the point-triangle problem.  Solid angle: Van Oosterom-Strackee,
// omega = 2 atan2(A.(B x C), |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|) with A.(B x C) = A.n.  e_* are the face's edge vectors b-a, c-a, c-b.
GLAMR_SDF_HD void point_face(float px, float py, float pz, const float* r, float abx, float aby, float abz, float acx, float acy, float acz,
                             float bcx, float bcy, float bcz, float& dmin2, float& wsum) {
  const float Ax = r[0] - px, Ay = r[1] - py, Az = r[2] - pz;
  const float Bx = r[3] - px, By = r[4] - py, Bz = r[5] - pz;
  const float Cx = r[6] - px, Cy = r[7] - py, Cz = r[8] - pz;
  float d2 = seg_dist2(Ax, Ay, Az, abx, aby, abz, r[12]);
  d2 = fminf(d2, seg_dist2(Ax, Ay, Az, acx, acy, acz, r[13]));
  d2 = fminf(d2, seg_dist2(Bx, By, Bz, bcx, bcy, bcz, r[14]));
  const float h = Ax * r[9] + Ay * r[10] + Az * r[11];                         // A . n: height over the plane times |n|, and the triple product
  const float d1 = -(Ax * abx + Ay * aby + Az * abz), d2b = -(Ax * acx + Ay * acy + Az * acz);
  const float vn = r[18] * d1 - r[17] * d2b, wn = r[16] * d2b - r[17] * d1;     // barycentric coordinates times |n|^2
  const float plane = h * h * r[15];
  d2 = (vn >= 0.f && wn >= 0.f && vn + wn <= r[19]) ? fminf(d2, plane) : d2;
  dmin2 = fminf(dmin2, d2);
  const float la = sqrtf(Ax * Ax + Ay * Ay + Az * Az), lb = sqrtf(Bx * Bx + By * By + Bz * Bz), lc = sqrtf(Cx * Cx + Cy * Cy + Cz * Cz);
  const float ab = Ax * Bx + Ay * By + Az * Bz, bc = Bx * Cx + By * Cy + Bz * Cz, ca = Cx * Ax + Cy * Ay + Cz * Az;
  wsum += atan2_cheap(h, la * lb * lc + ab * lc + bc * la + ca * lb);           // half the solid angle
}

// voxel centre k of a grid of G cells over [-1, 1]
GLAMR_SDF_HD float voxel_centre(int k, int G) { return -1.f + (float)(2 * k + 1) / (float)G; }

GLAMR_SDF_HD float phi_at(const float* phi, int G, int x, int y, int z) {
  return (x >= 0 && x < G && y >= 0 && y < G && z >= 0 && z < G) ? phi[((size_t)z * G + y) * G + x] : 0.f;
}

// F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=False) of one point u in normalised coordinates (u[0] indexes the last
// axis) and d value / d u, constant inside a cell.
GLAMR_SDF_HD float trilinear(const float* phi, int G, float ux, float uy, float uz, float& gx, float& gy, float& gz) {
  const float fx = ((ux + 1.f) * G - 1.f) * 0.5f, fy = ((uy + 1.f) * G - 1.f) * 0.5f, fz = ((uz + 1.f) * G - 1.f) * 0.5f;
  gx = gy = gz = 0.f;
  if (!(fx > -1.f && fx < (float)G && fy > -1.f && fy < (float)G && fz > -1.f && fz < (float)G)) return 0.f;      // (also NaN)
  const float x0f = floorf(fx), y0f = floorf(fy), z0f = floorf(fz);
  const int x0 = (int)x0f, y0 = (int)y0f, z0 = (int)z0f;
  const float tx = fx - x0f, ty = fy - y0f, tz = fz - z0f, sx = 1.f - tx, sy = 1.f - ty, sz = 1.f - tz;
  const float c000 = phi_at(phi, G, x0, y0, z0), c100 = phi_at(phi, G, x0 + 1, y0, z0), c010 = phi_at(phi, G, x0, y0 + 1, z0),
              c110 = phi_at(phi, G, x0 + 1, y0 + 1, z0), c001 = phi_at(phi, G, x0, y0, z0 + 1), c101 = phi_at(phi, G, x0 + 1, y0, z0 + 1),
              c011 = phi_at(phi, G, x0, y0 + 1, z0 + 1), c111 = phi_at(phi, G, x0 + 1, y0 + 1, z0 + 1);
  const float half_g = 0.5f * G;
  gx = half_g * (((c100 - c000) * sy + (c110 - c010) * ty) * sz + ((c101 - c001) * sy + (c111 - c011) * ty) * tz);
  gy = half_g * (((c010 - c000) * sx + (c110 - c100) * tx) * sz + ((c011 - c001) * sx + (c111 - c101) * tx) * tz);
  gz = half_g * (((c001 - c000) * sx + (c101 - c100) * tx) * sy + ((c011 - c010) * sx + (c111 - c110) * tx) * ty);
  return ((c000 * sx + c100 * tx) * sy + (c010 * sx + c110 * tx) * ty) * sz + ((c001 * sx + c101 * tx) * sy + (c011 * sx + c111 * tx) * ty) * tz;
}

// r(x) = x^2 / (x^2 + rho^2) and its derivative; rho = 0: the identity
GLAMR_SDF_HD float robust(float x, float rho, float& dr) {
  if (rho == 0.f) { dr = 1.f; return x; }
  const float r2 = rho * rho, den = x * x + r2;
  dr = 2.f * x * r2 / (den * den);
  return x * x / den;
}

}  // namespace sdf
}  // namespace glamr
