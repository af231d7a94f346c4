// Taped forward and explicit backward of the trajectory predictor's inference pass (TrajPredVAE.inference, traj_pred_vae.py:20-92, 202-334,
// 524-548): the vector-Jacobian product of (joint rows, latent draw) -> infer_out_local_traj_tp, weights constant.  The reference never takes
// this gradient: get_pred_trajectory_base clones traj_local_pred after .detach() (global_recon_model.py:396), so `traj_latent` sits in its
// parameter list with a gradient of None.  This is the attached alternative: optimising the predictor's latent, or the sensitivity of the
// predicted local trajectory to the infilled motion.
//
// Included by nets.hip INSIDE its anonymous namespace, after traj_pass.  The forward IS traj_pass (the same kernels on the same route, fused
// ones included) on the distinct slots of a tape arena, with the TAPE instances of the recurrence kernels, which also store every step's
// post-activation gates and cell state (LSTM_TAPE x 128 floats per step, direction and layer: 10 KB per frame and sequence).  What the fused
// two-layer row kernels leave on chip -- the 512-wide hidden rows of in_mlp, out_mlp and the decoder MLP -- is recomputed by the backward with
// one GEMM each (their ReLU masks are all it needs).  The backward walks the layers in reverse; linear layers: dX = dY W through lin_bwd of
// nets_tape.hpp (transposed weights made once per handle; on the fp16 matrix cores every gradient row is scaled by a power of two before the
// split and scaled back after: no range analysis bounds a gradient); the recurrences: the two BPTT kernels below.  Every sum has a fixed order.

// ---- BPTT of one bi-LSTM layer ------------------------------------------------------------------------------------------------------------
// Per step, walking each direction in the reverse of its forward order, from the tape (i f g o post-activation, c; c_prev = the c of the step
// before):   dh = dH[t] + dh_rec,  do = dh tanh c,  dc += dh o (1 - tanh^2 c),  di = dc g,  df = dc c_prev,  dg = dc i,  dc_prev = dc f,
// pre-activation gradients  di i (1 - i), df f (1 - f), dg (1 - g^2), do o (1 - o)  -> dG[t] (what the input projection's backward multiplies),
// and  dh_rec[128] = dgates[512] . W_hh  for the step before.
struct LstmBwdArgs {
  const float* tape;     // [n_seq][max_len][2][LSTM_TAPE][128]
  const float* dH;       // [n_seq][max_len][256]: upstream gradient of the layer's output rows
  const float* Whh_f;    // [512][128]
  const float* Whh_b;
  const int* lens;
  float* dG;             // [n_seq][max_len][1024]: gradient of the gate pre-activations (rows >= lens are not written: zeroed by the caller)
  int max_len;
};

// plain fp32: one 512-thread workgroup per (sequence, direction), as lstm_kernel.  Thread (k, part) keeps column k of rows [128 part, 128 part + 128)
// of W_hh in registers; the four partial sums of a column are added in the order of the gates.
__global__ __launch_bounds__(512) void lstm_bwd_kernel(LstmBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float sdg[512];
  __shared__ float spart[4][128];
  const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x, k = tid & 127, part = tid >> 7;
  const int n = a.lens[b];
  const float* Wcol = (dir ? a.Whh_b : a.Whh_f) + (size_t)part * 128 * 128 + k;
  float w[128];
#pragma unroll
  for (int j = 0; j < 128; ++j) w[j] = Wcol[(size_t)j * 128];
  float dc = 0.f, dh_rec = 0.f;
  for (int s = n - 1; s >= 0; --s) {
    const int t = dir ? (n - 1 - s) : s;
    if (tid < 128) {
      const float* tp = a.tape + lstm_tape_off(b, a.max_len, t, dir) + tid;
      const float ig = tp[0], fg = tp[128], gg = tp[256], og = tp[384], c = tp[512];
      const float cp = s > 0 ? a.tape[lstm_tape_off(b, a.max_len, dir ? t + 1 : t - 1, dir) + 512 + tid] : 0.f;
      const float dh = a.dH[((size_t)b * a.max_len + t) * 256 + dir * 128 + tid] + dh_rec;
      const float tc = tanhf(c);
      const float d_o = dh * tc;
      dc += dh * og * (1.0f - tc * tc);
      const float pi = dc * gg * ig * (1.0f - ig), pf = dc * cp * fg * (1.0f - fg), pg = dc * ig * (1.0f - gg * gg), po = d_o * og * (1.0f - og);
      dc *= fg;
      sdg[tid] = pi; sdg[128 + tid] = pf; sdg[256 + tid] = pg; sdg[384 + tid] = po;
      float* gp = a.dG + ((size_t)b * a.max_len + t) * 1024 + dir * 512 + tid;
      gp[0] = pi; gp[128] = pf; gp[256] = pg; gp[384] = po;
    }
    if (s == 0) break;                     // (uniform: nothing reads a recurrent gradient before the first step)
    __syncthreads();
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 128; j += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(sdg + part * 128 + j);
      acc = fmaf(w[j], v[0], acc); acc = fmaf(w[j + 1], v[1], acc); acc = fmaf(w[j + 2], v[2], acc); acc = fmaf(w[j + 3], v[3], acc);
    }
    spart[part][k] = acc;
    __syncthreads();
    if (tid < 128) dh_rec = ((spart[0][tid] + spart[1][tid]) + spart[2][tid]) + spart[3][tid];
  }
}

// Large batches, on the matrix cores: one 512-thread workgroup walks 16 sequences of one direction together, the mirror image of
// lstm_mfma_kernel.  Per step dh_rec[16 x 128] = dgates[16 x 512] . W_hh as v_mfma_f32_16x16x32_f16 with both operands split in two fp16
// planes (three products per accumulator): wave w owns hidden units [16 w, 16 w + 16), one 16 x 16 output tile over 16 k steps; its
// fragments of W_hh^T (16 k steps x 2 planes x 8 halves: lane (n, q) holds rows 32 j + 8 q .. + 7 of column 16 w + n) stay in 128 registers
// for the whole launch.  The gate gradients are lane-local: lane (n, q) receives dh_rec of unit 16 w + n for sequences 4 q .. 4 q + 3, the
// very (unit, sequence) pairs whose gates it reads from the tape.  dgates live in LDS already split, rows padded to 520 halves (the A operand
// of a step is 32 ds_read_b128: lane = sequence n, quarter q supplies the same k as on the B side).
// A gradient has no a-priori range, so each sequence's 512 gate gradients of a step are scaled by a power of two before the split -- 2^-e,
// e = ilogb(largest |entry|) - 14, as the RS instances of gemm_free_kernel do per row -- and dh_rec is scaled back by 2^e (both exact: the
// result does not depend on the gradient's magnitude).  The largest entry of a row is spread over the 8 waves: 16-lane shuffles, one partial
// per wave through LDS and a FIRST barrier; the split halves are written after it (every wave has finished reading the previous step's by
// then: one LDS buffer) and a SECOND barrier precedes the products.  Tape and upstream rows of the next step are requested before the
// products of this one.
constexpr int LSTM_BWD_GS = 520;      // halves per LDS row of one plane
__global__ __launch_bounds__(512) void lstm_bwd_mfma_kernel(LstmBwdArgs a, int n_seq) {
  GLAMR_CRITICAL_PATH_PRIO();
  __shared__ __attribute__((aligned(16))) _Float16 sg[2][16][LSTM_BWD_GS];      // [plane][sequence][gate row]
  __shared__ float smax[8][16];
  const int dir = blockIdx.y, s0 = blockIdx.x * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int u0 = wave * 16;
  const float* Whh = dir ? a.Whh_b : a.Whh_f;
  f16x8 wh[16], wl[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = Whh[(size_t)(32 * j + 8 * q + e) * 128 + u0 + n];
    split8(x, wh[j], wl[j]);
  }
  int len[4], seq[4], maxlen = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int sq = s0 + 4 * q + r;
    len[r] = sq < n_seq ? a.lens[sq] : 0;
    seq[r] = min(sq, n_seq - 1);
  }
  for (int m = 0; m < 16; ++m) { const int sq = s0 + m; if (sq < n_seq) maxlen = max(maxlen, a.lens[sq]); }
  // what step s needs of sequence r: gates and upstream gradient of its frame, the cell state of the step before (zero outside the sequence)
  float gate[4][4], up[4], cn[4], cc[4];
  auto frame = [&](int s, int r) { return dir ? (len[r] - 1 - s) : s; };
  auto fetch = [&](int s) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool act = s >= 0 && s < len[r];
      const size_t off = act ? lstm_tape_off(seq[r], a.max_len, frame(s, r), dir) + u0 + n : 0;
#pragma unroll
      for (int g = 0; g < 4; ++g) gate[g][r] = act ? a.tape[off + g * 128] : 0.f;
      up[r] = act ? a.dH[((size_t)seq[r] * a.max_len + frame(s, r)) * 256 + dir * 128 + u0 + n] : 0.f;
      const bool actp = s - 1 >= 0 && s - 1 < len[r];
      cn[r] = actp ? a.tape[lstm_tape_off(seq[r], a.max_len, frame(s - 1, r), dir) + 512 + u0 + n] : 0.f;
    }
  };
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int s = maxlen - 1;
    cc[r] = (s >= 0 && s < len[r]) ? a.tape[lstm_tape_off(seq[r], a.max_len, frame(s, r), dir) + 512 + u0 + n] : 0.f;
  }
  fetch(maxlen - 1);
  float dc[4] = {0.f, 0.f, 0.f, 0.f}, dh_rec[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s = maxlen - 1; s >= 0; --s) {
    float pg[4][4], mx[4];
    int ex[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ig = gate[0][r], fg = gate[1][r], gg = gate[2][r], og = gate[3][r];
      if (s < len[r]) {
        const float dh = up[r] + dh_rec[r];
        const float tc = fast_tanh(cc[r]);
        const float d_o = dh * tc;
        dc[r] += dh * og * (1.0f - tc * tc);
        pg[0][r] = dc[r] * gg * ig * (1.0f - ig);
        pg[1][r] = dc[r] * cn[r] * fg * (1.0f - fg);
        pg[2][r] = dc[r] * ig * (1.0f - gg * gg);
        pg[3][r] = d_o * og * (1.0f - og);
        dc[r] *= fg;
        float* gp = a.dG + ((size_t)seq[r] * a.max_len + frame(s, r)) * 1024 + dir * 512 + u0 + n;
#pragma unroll
        for (int g = 0; g < 4; ++g) gp[g * 128] = pg[g][r];
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) pg[g][r] = 0.f;
        dc[r] = 0.f;
      }
      cc[r] = cn[r];
      mx[r] = fmaxf(fmaxf(fabsf(pg[0][r]), fabsf(pg[1][r])), fmaxf(fabsf(pg[2][r]), fabsf(pg[3][r])));
    }
    if (s == 0) break;                     // (uniform: nothing reads a recurrent gradient before the first step)
    fetch(s - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], off));      // the 16 lanes of a quarter: the units of this wave
      if (n == 0) smax[wave][4 * q + r] = mx[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 4 * q + r;
      float v = smax[0][m];
#pragma unroll
      for (int w = 1; w < 8; ++w) v = fmaxf(v, smax[w][m]);
      ex[r] = (v > 0.f && v < INFINITY) ? ilogbf(v) - 14 : 0;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float x = ldexpf(pg[g][r], -ex[r]);
        const _Float16 hh = (_Float16)x;
        sg[0][m][g * 128 + u0 + n] = hh;
        sg[1][m][g * 128 + u0 + n] = (_Float16)(x - (float)hh);
      }
    }
    __syncthreads();
    f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
    // the two small products first; two accumulators (even / odd k steps) so that consecutive MFMAs do not wait for each other
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const f16x8 ah = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(&sg[0][n][32 * j + 8 * q]));
      const f16x8 al = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(&sg[1][n][32 * j + 8 * q]));
      acc[j & 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, wh[j], acc[j & 1], 0, 0, 0);
      acc[(j + 1) & 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wl[j], acc[(j + 1) & 1], 0, 0, 0);
      acc[j & 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wh[j], acc[j & 1], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dh_rec[r] = ldexpf(acc[0][r] + acc[1][r], ex[r]);
  }
}

void bilstm_bwd(const Plan& p, const float* tape, const float* dH, float* const hh[2], const int* lens, float* dG, int max_len, int B) {
  LstmBwdArgs la{tape, dH, hh[0], hh[1], lens, dG, max_len};
  if (B >= 512 && !p.fp32) hipLaunchKernelGGL(lstm_bwd_mfma_kernel, dim3((B + 15) / 16, 2), dim3(512), 0, p.st, la, B);      // the forward's own threshold
  else hipLaunchKernelGGL(lstm_bwd_kernel, dim3(B, 2), dim3(512), 0, p.st, la);
}

// ---- the small kernels of the backward ------------------------------------------------------------------------------------------------
// upstream rows (n_seq, max_len, 11) -> [MT][64]: zero past a sequence's end, in the padding columns and on the four pinned entries of row 0
// (columns 0, 1, 9, 10 are constants: DataDecoder :319-327)
__global__ void traj_g_in_kernel(const float* g, int max_len, const int* lens, float* draw) {
  const int b = blockIdx.x, t = blockIdx.y, c = threadIdx.x;
  const bool pinned = t == 0 && (c < 2 || c == 9 || c == 10);
  draw[((size_t)b * max_len + t) * 64 + c] = (c < 11 && t < lens[b] && !pinned) ? g[((size_t)b * max_len + t) * 11 + c] : 0.0f;
}
// out[b][c] = sum over the sequence's frames of d[b][t][c], in frame order (the row bias W_z z + b is shared by all frames of a sequence)
__global__ void seq_sum_kernel(const float* d, int max_len, const int* lens, int ld, float* out) {
  const int b = blockIdx.x, c = blockIdx.y * blockDim.x + threadIdx.x, n = lens[b];
  if (c >= ld) return;
  const float* p = d + (size_t)b * max_len * ld + c;
  float s = 0.f;
  int t = 0;
  for (; t + 8 <= n; t += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(t + u) * ld];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; t < n; ++t) s += p[(size_t)t * ld];
  out[(size_t)b * ld + c] = s;
}
// z = mu + eps exp(0.5 logvar), pz row = [mu | logvar]: d mu = dz, d logvar = dz eps 0.5 exp(0.5 logvar), d eps = dz exp(0.5 logvar)
__global__ void reparam_traj_bwd_kernel(const float* pz, const float* eps, const float* dz, float* dpz, float* deps) {
  const int b = blockIdx.x, k = threadIdx.x;
  const float sd = expf(0.5f * pz[(size_t)b * D + NZ + k]), g = dz[(size_t)b * NZ + k];
  dpz[(size_t)b * D + k] = g;
  dpz[(size_t)b * D + NZ + k] = g * eps[(size_t)b * NZ + k] * 0.5f * sd;
  deps[(size_t)b * NZ + k] = g * sd;
}
// mean over the sequence's OWN frames: every one of them receives d mean / len
__global__ void masked_mean_bwd_kernel(const float* dmean, int max_len, const int* lens, float* dctx) {
  const int b = blockIdx.x, t = blockIdx.y, k = threadIdx.x, n = lens[b];
  if (t < n) dctx[((size_t)b * max_len + t) * D + k] += dmean[(size_t)b * D + k] / (float)n;
}
__global__ void joints_out_bwd_kernel(const float* dx, int max_len, const int* lens, float* g_joint_pos) {
  const int b = blockIdx.x, t = blockIdx.y, c = threadIdx.x;
  if (c < 69) g_joint_pos[((size_t)b * max_len + t) * 69 + c] = t < lens[b] ? dx[((size_t)b * max_len + t) * XLD + c] : 0.0f;
}

// ---- tape layout ------------------------------------------------------------------------------------------------------------------------
struct TrajTape {
  TrajSlots s;                                                   // what the forward keeps
  float *pose;                                                   // [B][max_len][96] body-pose rows (in_body_pose callers: the FK kernel's input)
  float *hid, *dA, *dB, *dC, *draw, *dx;                         // backward: recomputed hidden rows [MT][512]; gradients [MT][1024], [MT][256] x 2, [MT][64], [MT][96]
  float *dzrow, *dz, *dpz, *dpr2, *dpr1, *dmean;                 // per sequence
  int* lens;
  size_t total;
};
TrajTape traj_tape_layout(int B, int max_len, char* base) {
  TrajTape t{};
  size_t off = 0;
  // (+ 32 rows per buffer, as ws_layout: kernels that work in whole row blocks stay inside the arena)
  auto take = [&](size_t nfloats) { float* p = reinterpret_cast<float*>(base + off); off = align_up(off + (nfloats + 32 * 1024) * sizeof(float), 256); return p; };
  const size_t MT = (size_t)B * max_len, NB = (size_t)B;
  TrajSlots& s = t.s;
  s.x = take(MT * XLD); s.h0 = take(MT * D); s.h1 = take(MT * D); s.h2 = take(MT * D); s.ctx = take(MT * D);
  s.g = take(MT * 1024); s.tmp = take(MT * D); s.dec = take(MT * D);
  s.mean = take(NB * D); s.pr1 = take(NB * FF); s.pr2 = take(NB * D); s.pz = take(NB * D); s.z = take(NB * NZ); s.zrow = take(NB * FF);
  s.raw = take(MT * 64); s.scr = take(MT * 3);
  for (int l = 0; l < 2; ++l) s.lstm[l] = take(MT * 2 * LSTM_TAPE * 128);
  t.pose = take(MT * XLD);
  t.hid = take(MT * FF); t.dA = s.g;                              // (the forward's scratch rows are free once it has run)
  t.dB = take(MT * D); t.dC = take(MT * D); t.draw = s.raw; t.dx = take(MT * XLD);
  t.dzrow = take(NB * FF); t.dz = take(NB * NZ); t.dpz = take(NB * D); t.dpr2 = take(NB * D); t.dpr1 = take(NB * FF); t.dmean = take(NB * D);
  t.lens = reinterpret_cast<int*>(take(NB + 64));
  t.total = off;
  return t;
}

// the layers the backward multiplies with, transposed once per handle (the first time a tape is asked for)
int traj_transposes(glamr_nets* h) {
  const Lin* layers[] = {&h->t_in1, &h->t_in2, &h->t_ih[0], &h->t_ih[1], &h->t_out1, &h->t_out2, &h->t_pr1, &h->t_pr2, &h->t_pz, &h->t_dz, &h->t_dctx, &h->t_d2, &h->t_dfc};
  for (const Lin* L : layers)
    if (!transposed(h, *L)) return fail(GLAMR_E_HIP, "could not build the transposed weights of a layer");
  return GLAMR_OK;
}

// dX = act'(.) dY W into a zeroed dX (lin_bwd accumulates)
int lin_bwd0(const TapeCtx& c, const Lin& L, float* dY, int ldy, const float* Y, int act, float* dX, int ldx, int M) {
  GLAMR_HIP_CHECK(hipMemsetAsync(dX, 0, (size_t)M * ldx * sizeof(float), c.p.st));
  return lin_bwd(c, L, dY, ldy, Y, act, dX, ldx, M);
}

// ---- backward: g (n_seq, max_len, 11) -> g_eps (n_seq, 128) [, g_joint_pos (n_seq, max_len, 69)] -------------------------------------------
int traj_backward_pass(glamr_nets* h, const Plan& p, const TrajTape& t, int B, int max_len, const float* eps, const float* g, float* g_eps, float* g_joint_pos) {
  const int MT = B * max_len;
  hipStream_t st = p.st;
  const TrajSlots& s = t.s;
  const TapeCtx c{h, p, nullptr};
  // decoder: out_fc, out_mlp on [z | ctx]
  hipLaunchKernelGGL(traj_g_in_kernel, dim3(B, max_len), dim3(64), 0, st, g, max_len, t.lens, t.draw);
  RC(lin_bwd0(c, h->t_dfc, t.draw, 64, nullptr, ACT_NONE, t.dB, D, MT));
  RC(lin(p, h->t_dctx, s.ctx, D, t.hid, FF, MT, ACT_RELU, {.rowbias = s.zrow, .rpg = max_len, .ldrb = FF}));
  RC(lin_bwd0(c, h->t_d2, t.dB, D, s.dec, ACT_RELU, t.dA, FF, MT));
  RC(lin_bwd0(c, h->t_dctx, t.dA, FF, t.hid, ACT_RELU, t.dC, D, MT));      // d ctx, decoder path; t.dA is now d(W_ctx ctx + W_z z + b)
  hipLaunchKernelGGL(seq_sum_kernel, dim3(B, FF / 128), dim3(128), 0, st, t.dA, max_len, t.lens, FF, t.dzrow);
  RC(lin_bwd0(c, h->t_dz, t.dzrow, FF, nullptr, ACT_NONE, t.dz, NZ, B));
  // reparameterisation -> d eps, and d mu / d logvar into the prior
  hipLaunchKernelGGL(reparam_traj_bwd_kernel, dim3(B), dim3(NZ), 0, st, s.pz, eps, t.dz, t.dpz, g_eps);
  if (!g_joint_pos) return GLAMR_OK;
  RC(lin_bwd0(c, h->t_pz, t.dpz, D, nullptr, ACT_NONE, t.dpr2, D, B));
  RC(lin_bwd0(c, h->t_pr2, t.dpr2, D, s.pr2, ACT_RELU, t.dpr1, FF, B));
  RC(lin_bwd0(c, h->t_pr1, t.dpr1, FF, s.pr1, ACT_RELU, t.dmean, D, B));
  hipLaunchKernelGGL(masked_mean_bwd_kernel, dim3(B, max_len), dim3(D), 0, st, t.dmean, max_len, t.lens, t.dC);
  // context encoder: out_mlp
  RC(lin(p, h->t_out1, s.h2, D, t.hid, FF, MT, ACT_RELU));
  RC(lin_bwd0(c, h->t_out2, t.dC, D, s.ctx, ACT_RELU, t.dA, FF, MT));
  RC(lin_bwd0(c, h->t_out1, t.dA, FF, t.hid, ACT_RELU, t.dB, D, MT));       // d h2
  // the two bi-LSTM layers: BPTT, then the input projection
  float* dH[2] = {t.dC, t.dB};      // upstream of layer l
  float* dIn[2] = {t.dB, t.dC};     // gradient of its input rows
  for (int l = 1; l >= 0; --l) {
    GLAMR_HIP_CHECK(hipMemsetAsync(t.dA, 0, (size_t)MT * 1024 * sizeof(float), st));
    bilstm_bwd(p, s.lstm[l], dH[l], h->t_hh[l], t.lens, t.dA, max_len, B);
    RC(lin_bwd0(c, h->t_ih[l], t.dA, 1024, nullptr, ACT_NONE, dIn[l], D, MT));
  }
  // in_mlp
  RC(lin(p, h->t_in1, s.x, XLD, t.hid, FF, MT, ACT_RELU));
  RC(lin_bwd0(c, h->t_in2, t.dB, D, s.h0, ACT_RELU, t.dA, FF, MT));
  RC(lin_bwd0(c, h->t_in1, t.dA, FF, t.hid, ACT_RELU, t.dx, XLD, MT));
  hipLaunchKernelGGL(joints_out_bwd_kernel, dim3(B, max_len), dim3(XLD), 0, st, t.dx, max_len, t.lens, g_joint_pos);
  return GLAMR_OK;
}
