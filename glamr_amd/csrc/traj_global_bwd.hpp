// Vector-Jacobian product of traj_local2global_heading (traj_pred/utils/traj_utils.py:65-88, local_heading=True, 6D local orientation)
// followed by quaternion_to_angle_axis -- the map traj_to_global2_kernel (nets.hip) computes -- for ONE sequence, written against the block
// runtime (thread id, barrier, rt.scan): DeviceRT on the device (traj_global_bwd.hip), the single-threaded host runtime of tests/hostsim on
// the CPU.  DESIGN.md 14.
//
// Forward, rows t in [0, n):   theta_t = atan2s(L[t][10], L[t][9]),  h_t = sum_{s <= t} theta_s,
//   d_0 = L[0][0:2],  d_t = R(h_{t-1}) L[t][0:2]  (t >= 1),   trans_t = (sum_{s <= t} d_s, L[t][2]),
//   q_t = (heading_quat(h_t) (x) rotmat_to_quat(rot6d_to_rotmat(L[t][3:9]))) (x) base,   orient_t = quat_to_aa(q_t).
// Reverse, nothing taped (theta and its prefix sum are recomputed from L):
//   columns 0-1   S_t = sum_{s >= t} g_trans_s[0:2];  row t >= 1 gets R(h_{t-1})^T S_t, row 0 gets S_0
//   column 2      g_trans_t[2]
//   columns 3-8   g_q = g_orient_q + quat_to_aa_bwd(q, g_orient), back through the two products (base is a constant), rotmat_to_quat_bwd and
//                 rot6d_to_rotmat_bwd
//   g_h[t]        = S_{t+1} . dR/dh(h_t) L[t+1][0:2]  (t + 1 < n)  +  heading_quat_bwd(h_t, .) of the first product's left factor
//   columns 9-10  atan2s_bwd at (L[t][10], L[t][9]) of sum_{s >= t} g_h[s]
// Every per-frame operator is rotmath.hpp's.  Frame t is handled by thread t mod nthreads in every phase and writes only its own elements
// (the dR/dh term of row t + 1 is computed by frame t, which reads row t + 1); every sum is one of the four scans: no atomics, a fixed order.
// Rows at or beyond n are never read from the upstream arrays and are written as zeros.
//
// Optional world heading offset (the optimiser's world_dheading step, global_recon_model.py:459-465): with `wdh` given, g_orient
// is the gradient of  aa(q_z(wdh[t]) (x) aa_to_quat(orient_t))  instead of orient_t: it is taken back through world_dheading_bwd first, and
// g_wdh[t] (rows [0, n), written only where g_orient is given) receives the offset's own gradient.  The translation and g_orient_q are
// unaffected.  Without `wdh` (the default) nothing of this is evaluated.
#pragma once
#include "rotmath.hpp"

namespace glamr {

constexpr int TGB_WS_FLOATS_PER_FRAME = 4;      // h, S_x, S_y, g_h

// out = quat_to_aa(angle_axis_to_quaternion((0, 0, w)) (x) aa_to_quat(base)) for an upstream gradient ga of `out`: returns d/dw and, with
// g_base given, ADDS d/d base to it
GLAMR_HD float world_dheading_bwd(const float base[3], float w, const float ga[3], float* g_base) {
  float qz[4], qb[4], qo[4];
  rm::heading_quat(w, qz);
  rm::aa_to_quat(base, qb);
  rm::quat_mul(qz, qb, qo);
  float gqo[4] = {0.f, 0.f, 0.f, 0.f}, gqz[4] = {0.f, 0.f, 0.f, 0.f}, gqb[4] = {0.f, 0.f, 0.f, 0.f};
  rm::quat_to_aa_bwd(qo, ga, gqo);
  rm::quat_mul_bwd(qz, qb, gqo, gqz, g_base ? gqb : nullptr);
  if (g_base) rm::aa_to_quat_bwd(base, gqb, g_base);
  return rm::heading_quat_bwd(w, gqz);
}

// L, gL: [T][11];  g_trans, g_orient: [T][3] or null;  g_orient_q: [T][4] or null;  ws: [4][T] floats of this sequence;  0 <= n <= T;
// wdh, g_wdh: [n] or null
template <class RT>
GLAMR_HD void traj_global_bwd(RT& rt, int n, int T, const float* L, const float* g_trans, const float* g_orient, const float* g_orient_q, float* gL, float* ws,
                              const float* wdh = nullptr, float* g_wdh = nullptr) {
  const int tid = rt.tid(), nt = rt.nthreads();
  float* h = ws;
  float* Sx = ws + T;
  float* Sy = ws + 2 * (size_t)T;
  float* gh = ws + 3 * (size_t)T;
  // a sequence of at most one frame per thread keeps its row in registers between the phases (copied, never addressed: a pointer to `row`
  // would put it into scratch memory)
  const bool one = T <= nt;
  float row[11];
  if (one && tid < n)
    for (int c = 0; c < 11; ++c) row[c] = L[(size_t)tid * 11 + c];
  auto fetch = [&](int t, float (&r)[11]) {
    if (one) { for (int c = 0; c < 11; ++c) r[c] = row[c]; }
    else { for (int c = 0; c < 11; ++c) r[c] = L[(size_t)t * 11 + c]; }
  };

  for (int t = tid; t < T; t += nt) {
    if (t >= n) {
      for (int c = 0; c < 11; ++c) gL[(size_t)t * 11 + c] = 0.0f;
      continue;
    }
    float r[11];
    fetch(t, r);
    h[t] = rm::atan2s(r[10], r[9]);
    Sx[t] = g_trans ? g_trans[(size_t)t * 3 + 0] : 0.0f;
    Sy[t] = g_trans ? g_trans[(size_t)t * 3 + 1] : 0.0f;
  }
  rt.sync();
  rt.scan(h, n, 1, false);
  if (g_trans) {
    rt.scan(Sx, n, 1, true);
    rt.scan(Sy, n, 1, true);
  }

  for (int t = tid; t < n; t += nt) {
    float r[11];
    fetch(t, r);
    float* g = gL + (size_t)t * 11;
    const float ht = h[t];
    // translation: own columns 0-2, and the heading term of the NEXT row's displacement
    float sx = Sx[t], sy = Sy[t];
    if (t > 0) {
      float s, c;
      rm::sincos_(h[t - 1], s, c);
      const float a = c * sx + s * sy, b = c * sy - s * sx;
      sx = a; sy = b;
    }
    g[0] = sx; g[1] = sy;
    g[2] = g_trans ? g_trans[(size_t)t * 3 + 2] : 0.0f;
    float ght = 0.0f;
    if (t + 1 < n) {
      float s, c;
      rm::sincos_(ht, s, c);
      const float dx = L[(size_t)(t + 1) * 11], dy = L[(size_t)(t + 1) * 11 + 1];
      ght = Sx[t + 1] * (-dx * s - dy * c) + Sy[t + 1] * (dx * c - dy * s);
    }
    // orientation
    float g6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (g_orient || g_orient_q) {
      const float base[4] = {0.5f, 0.5f, 0.5f, 0.5f};
      float hq[4], R[9], lq[4], q1[4], q[4];
      rm::heading_quat(ht, hq);
      rm::rot6d_to_rotmat(r + 3, R);
      rm::rotmat_to_quat(R, lq);
      rm::quat_mul(hq, lq, q1);
      rm::quat_mul(q1, base, q);
      float gq[4] = {0.f, 0.f, 0.f, 0.f};
      if (g_orient_q) for (int c = 0; c < 4; ++c) gq[c] = g_orient_q[(size_t)t * 4 + c];
      if (g_orient) {
        float ga[3] = {g_orient[(size_t)t * 3], g_orient[(size_t)t * 3 + 1], g_orient[(size_t)t * 3 + 2]};
        if (wdh) {
          float aa[3], gb[3] = {0.f, 0.f, 0.f};
          rm::quat_to_aa(q, aa);
          const float gw = world_dheading_bwd(aa, wdh[t], ga, gb);
          if (g_wdh) g_wdh[t] = gw;
          for (int c = 0; c < 3; ++c) ga[c] = gb[c];
        }
        rm::quat_to_aa_bwd(q, ga, gq);
      }
      float gq1[4] = {0.f, 0.f, 0.f, 0.f}, ghq[4] = {0.f, 0.f, 0.f, 0.f}, glq[4] = {0.f, 0.f, 0.f, 0.f};
      rm::quat_mul_bwd(q1, base, gq, gq1, nullptr);
      rm::quat_mul_bwd(hq, lq, gq1, ghq, glq);
      ght += rm::heading_quat_bwd(ht, ghq);
      float gR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      rm::rotmat_to_quat_bwd(R, glq, gR);
      rm::rot6d_to_rotmat_bwd(r + 3, gR, g6);
    }
    for (int c = 0; c < 6; ++c) g[3 + c] = g6[c];
    gh[t] = ght;
  }
  rt.sync();
  rt.scan(gh, n, 1, true);

  for (int t = tid; t < n; t += nt) {
    float r[11];
    fetch(t, r);
    float gy = 0.0f, gx = 0.0f;
    rm::atan2s_bwd(r[10], r[9], gh[t], gy, gx);
    gL[(size_t)t * 11 + 9] = gx;
    gL[(size_t)t * 11 + 10] = gy;
  }
}

}  // namespace glamr
