// wk_ctc_bwd.hip -- the backward pass of the fp32 GRU-CTC head (wk_ctc.hip):
// from the gradient at the logits (what wk_ctc_loss writes) to the gradient of
// every GRU_CTC_Model parameter, in wk_ctc_create's blob order.
//
// The function differentiated is the one wk_ctc_forward computes in fp32 (the
// eval-mode module: no dropout).  wk_ctc_forward_train keeps the features, the
// encoder output x0, both layers' gate inputs gi = x W_ih^T and outputs y0, y1;
// the gates are recomputed here from them, outside the recurrence.
//
// Kernels (all fp32; every matrix product on v_mfma_f32_16x16x4_f32):
//   ctc_bwd_gemm_kernel     C[M][N] = sum_k A(m, k) B(k, n) with element strides
//                           for both operands: the TN (weight gradients: the
//                           reduction runs over the rows), NN (input gradients)
//                           and NT (recomputed W_hh h, encoder pre-activations)
//                           forms.  A reduction over the rows is split across
//                           workgroups into partial tiles...
//   ctc_bwd_reduce_kernel   ... which this kernel adds in split order.
//   ctc_bwd_colsum_kernel   bias gradients: column sums, accumulated in double.
//   ctc_bwd_shift_kernel    h_prev [rows][256]: y at t - 1 (forward half) and at
//                           t + 1 (reverse half), 0 at the sequence end.
//   ctc_bwd_gates_kernel    r, z, n recomputed per (row, direction, unit) and
//                           folded into the five factors a BPTT step multiplies by.
//   ctc_gru_bptt_kernel     the recurrence backward in time, after the shape of
//                           ctc_gru_kernel: a persistent workgroup per (16
//                           utterances, direction), W_hh^T as A fragments in VGPRs.
//   ctc_bwd_layernorm_kernel  ReLU mask + LayerNorm backward, one wave per row.
//   ctc_bwd_norm_kernel     2-norm of the gradient blob, in double, fixed order.
// No kernel uses a floating-point atomic and every sum has a fixed order: equal
// inputs give equal bits.  No workgroup waits on another.
#include <math.h>

#include "wk_ctc_handle.h"

using namespace wk;

namespace {

// ---------------------------------------------------------------------------
// Block GEMM, 64 x 64 tile, 4 waves of 32 x 32 (2 x 2 accumulators of 16 x 16).
// A(m, k) = A[m sam + k sak], B(k, n) = B[k sbk + n sbn]; AK / BK: the operand's
// k stride is 1 (threads of a staging load then run along k, else along m / n).
// K goes in chunks of 16 through LDS images [k][m], [k][n] (pitch 80: the four
// 16-lane groups of a fragment read land on distinct banks); the next chunk's
// global loads are in flight during this chunk's MFMAs.  Rows, columns and k
// past the end read 0 and are never stored.  blockIdx.z = the K split: split z
// covers k in [z kper, (z + 1) kper) and, with more than one split, writes its
// tile to part[z][M][N] instead of C.
// ---------------------------------------------------------------------------
constexpr int kBgT = 64, kBgK = 16, kBgP = 80;

template <bool KF>
__device__ __forceinline__ void bg_load(const float* __restrict__ p, int64_t so, int64_t sk, int o0, int olim, int64_t k0,
                                        int64_t k1, int tid, float (&v)[4]) {
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int e = tid + 256 * h;
    const int k = KF ? (e & 15) : (e >> 6), o = KF ? (e >> 4) : (e & 63);
    const int64_t kk = k0 + k;
    const int oo = o0 + o;
    v[h] = (kk < k1 && oo < olim) ? p[(int64_t)oo * so + kk * sk] : 0.0f;
  }
}
template <bool KF>
__device__ __forceinline__ void bg_store(float* s, int tid, const float (&v)[4]) {
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int e = tid + 256 * h;
    const int k = KF ? (e & 15) : (e >> 6), o = KF ? (e >> 4) : (e & 63);
    s[k * kBgP + o] = v[h];
  }
}

template <bool AK, bool BK>
__global__ __launch_bounds__(256) void ctc_bwd_gemm_kernel(const float* __restrict__ A, int64_t sam, int64_t sak,
                                                           const float* __restrict__ B, int64_t sbk, int64_t sbn,
                                                           float* __restrict__ C, int64_t ldc, int M, int N, int64_t K,
                                                           int64_t kper, float* __restrict__ part) {
  __shared__ float As[kBgK * kBgP], Bs[kBgK * kBgP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, q = lane >> 4, wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * kBgT, n0 = blockIdx.y * kBgT;
  const int64_t kb = (int64_t)blockIdx.z * kper;
  const int64_t ke = kb + kper < K ? kb + kper : K;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float va[4], vb[4];
  bg_load<AK>(A, sam, sak, m0, M, kb, ke, tid, va);
  bg_load<BK>(B, sbn, sbk, n0, N, kb, ke, tid, vb);
  for (int64_t k0 = kb; k0 < ke; k0 += kBgK) {
    bg_store<AK>(As, tid, va);
    bg_store<BK>(Bs, tid, vb);
    __syncthreads();
    if (k0 + kBgK < ke) {
      bg_load<AK>(A, sam, sak, m0, M, k0 + kBgK, ke, tid, va);
      bg_load<BK>(B, sbn, sbk, n0, N, k0 + kBgK, ke, tid, vb);
    }
#pragma unroll
    for (int s = 0; s < kBgK / 4; ++s) {
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = As[(4 * s + q) * kBgP + 32 * wm + 16 * i + li];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = Bs[(4 * s + q) * kBgP + 32 * wn + 16 * j + li];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma4(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
  // D of a 16 x 16 tile: lane holds rows 4q .. 4q + 3, column li
  float* out = gridDim.z > 1 ? part + (int64_t)blockIdx.z * M * N : C;
  const int64_t ld = gridDim.z > 1 ? (int64_t)N : ldc;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + 32 * wn + 16 * j + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + 32 * wm + 16 * i + 4 * q + r;
        if (row < M && col < N) out[(int64_t)row * ld + col] = acc[i][j][r];
      }
    }
}

// C[m][n] = part[0][m][n] + part[1][m][n] + ... in that order.
__global__ __launch_bounds__(256) void ctc_bwd_reduce_kernel(const float* __restrict__ part, int splits, int M, int N,
                                                             float* __restrict__ C, int64_t ldc) {
  const int64_t mn = (int64_t)M * N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < mn; i += (int64_t)gridDim.x * 256) {
    float s = part[i];
    for (int z = 1; z < splits; ++z) s += part[(int64_t)z * mn + i];
    C[(i / N) * ldc + i % N] = s;
  }
}

// out[n] = sum over rows of X[row ld + n]: 64 columns x 16 row groups per
// block, each thread a strided chain in double, the 16 chains added in order.
__global__ __launch_bounds__(1024) void ctc_bwd_colsum_kernel(const float* __restrict__ X, int64_t rows, int64_t ld, int N,
                                                              float* __restrict__ out) {
  __shared__ double sm[16][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + c;
  double s = 0.0;
  if (n < N)
    for (int64_t r = g; r < rows; r += 16) s += (double)X[r * ld + n];
  sm[g][c] = s;
  __syncthreads();
  if (g == 0 && n < N) {
    double t = sm[0][c];
#pragma unroll
    for (int i = 1; i < 16; ++i) t += sm[i][c];
    out[n] = (float)t;
  }
}

// h_prev of both directions: [rows][fwd 128 | rev 128] = y[b][t - 1][fwd], y[b][t + 1][rev], 0 outside the sequence.
__global__ __launch_bounds__(256) void ctc_bwd_shift_kernel(const float* __restrict__ y, int64_t rows, int T,
                                                            float* __restrict__ hprev) {
  const int64_t n = rows * (2 * kH / 4);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / (2 * kH / 4);
    const int c4 = (int)(i % (2 * kH / 4));
    const int t = (int)(row % T);
    const bool rev = c4 >= kH / 4;
    const bool in = rev ? t + 1 < T : t > 0;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (in) v = *reinterpret_cast<const float4*>(y + (rev ? row + 1 : row - 1) * (2 * kH) + 4 * c4);
    *reinterpret_cast<float4*>(hprev + row * (2 * kH) + 4 * c4) = v;
  }
}

// The gate activations of ctc_gru_kernel (wk_ctc_gru.hip).
__device__ __forceinline__ float sigm(float v) { return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }
__device__ __forceinline__ float tanh_fast(float v) { return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(__expf(2.0f * v) + 1.0f), 1.0f); }

// The factors of one BPTT step, per (row, direction, unit), from gi = x W_ih^T,
// gh = W_hh h_prev (both without bias) and h_prev:
//   coef[row][dir][0] = (h_prev - n) z (1 - z)    dz = dh * it
//   coef[row][dir][1] = (1 - z) (1 - n^2)         dn = dh * it
//   coef[row][dir][2] = (W_hn h_prev + b_hn) r (1 - r)   dr = dn * it
//   coef[row][dir][3] = r                         da_h's n part = dn * it
//   coef[row][dir][4] = z                         the carry dh * it
constexpr int kCoef = 5;
__global__ __launch_bounds__(256) void ctc_bwd_gates_kernel(const float* __restrict__ gi, const float* __restrict__ gh,
                                                            const float* __restrict__ hprev, const float* __restrict__ bih,
                                                            const float* __restrict__ bhh, int64_t rows,
                                                            float* __restrict__ coef) {
  const int64_t n = rows * 2 * kH;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / (2 * kH);
    const int d = (int)(i % (2 * kH)) / kH, u = (int)(i % kH);
    const float* g = gi + row * (6 * kH) + d * 3 * kH;
    const float* h = gh + row * (6 * kH) + d * 3 * kH;
    const float* bi = bih + d * 3 * kH;
    const float* bh = bhh + d * 3 * kH;
    const float r = sigm(g[u] + bi[u] + h[u] + bh[u]);
    const float z = sigm(g[kH + u] + bi[kH + u] + h[kH + u] + bh[kH + u]);
    const float hn = h[2 * kH + u] + bh[2 * kH + u];
    const float c = tanh_fast(g[2 * kH + u] + bi[2 * kH + u] + r * hn);
    const float hp = hprev[row * (2 * kH) + d * kH + u];
    float* o = coef + (row * 2 + d) * (kCoef * kH) + u;
    o[0] = (hp - c) * z * (1.0f - z);
    o[kH] = (1.0f - z) * (1.0f - c * c);
    o[2 * kH] = hn * r * (1.0f - r);
    o[3 * kH] = r;
    o[4 * kH] = z;
  }
}

// ---------------------------------------------------------------------------
// BPTT of one GRU layer, both directions in the grid: workgroup (x, dir) owns
// utterances 16 x .. 16 x + 15 of direction dir and walks its T steps backward
// in time (forward direction: t = T - 1 .. 0; reverse: t = 0 .. T - 1).  With
// dh the gradient at the state h_t (the layer's upstream gradient dy[b][t] plus
// what step t + 1 carried back):
//   dn = dh (1 - z)(1 - n^2), dz = dh (h_prev - n) z (1 - z), dr = dn (W_hn h_prev + b_hn) r (1 - r)
//   da_i = [dr, dz, dn], da_h = [dr, dz, dn r], dh_prev = dh z + W_hh^T da_h
// Wave w owns units 16 w .. 16 w + 15: its 16 rows of W_hh^T [128][384] are 96
// A fragments in VGPRs; a step's da_h goes through LDS as the B operand [k =
// gate row][batch] (two images: one barrier per step), D = W_hh^T da_h lands
// on the lane that holds the same (unit, utterance) elements' dh, so the carry
// stays in registers.  The factors (ctc_bwd_gates_kernel) and dy of the next
// step are loaded before this step's MFMAs.  The loop is bounded by T and the
// only synchronisation is the workgroup's barrier.
// ---------------------------------------------------------------------------
constexpr int kBpBatch = 16, kBpWaves = kH / 16, kBpThreads = 64 * kBpWaves, kBpKS = 3 * kH / 4, kBpP = 17;

__global__ __launch_bounds__(kBpThreads) void ctc_gru_bptt_kernel(const float* __restrict__ coef, const float* __restrict__ dy,
                                                                  const float* __restrict__ whht_pk, int64_t B, int T,
                                                                  float* __restrict__ da_i, float* __restrict__ da_h) {
  __shared__ float dah[2][3 * kH * kBpP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y;
  const int n = lane & 15, q = lane >> 4;
  const int u0 = 16 * wave + 4 * q;   // the lane's units u0 .. u0 + 3 of utterance slot n
  const int64_t b = (int64_t)blockIdx.x * kBpBatch + n;
  const bool live = b < B;
  float wt[kBpKS];
  {
    const float* p = whht_pk + ((size_t)dir * kBpWaves + wave) * kBpKS * 64 + lane;
#pragma unroll
    for (int s = 0; s < kBpKS; ++s) wt[s] = p[s * 64];
  }
  const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 cf[kCoef], dyv;
  auto load_step = [&](int step) {
    const int sc = step < T ? step : T - 1;
    const int t = dir == 0 ? T - 1 - sc : sc;
    const int64_t row = (live ? b : 0) * T + t;
    const float* cp = coef + (row * 2 + dir) * (kCoef * kH) + u0;
#pragma unroll
    for (int k = 0; k < kCoef; ++k) cf[k] = live ? *reinterpret_cast<const float4*>(cp + k * kH) : zero4;
    dyv = live ? *reinterpret_cast<const float4*>(dy + row * (2 * kH) + dir * kH + u0) : zero4;
  };
  load_step(0);
  float dh[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int cur = 0;
  for (int step = 0; step < T; ++step) {
    const int t = dir == 0 ? T - 1 - step : step;
    const float cz[4] = {cf[0].x, cf[0].y, cf[0].z, cf[0].w}, cn[4] = {cf[1].x, cf[1].y, cf[1].z, cf[1].w};
    const float cr[4] = {cf[2].x, cf[2].y, cf[2].z, cf[2].w}, gr[4] = {cf[3].x, cf[3].y, cf[3].z, cf[3].w};
    const float gz[4] = {cf[4].x, cf[4].y, cf[4].z, cf[4].w}, up[4] = {dyv.x, dyv.y, dyv.z, dyv.w};
    float dr[4], dz[4], dn[4], dnr[4], carry[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float d = dh[i] + up[i];
      dn[i] = d * cn[i];
      dz[i] = d * cz[i];
      dr[i] = dn[i] * cr[i];
      dnr[i] = dn[i] * gr[i];
      carry[i] = d * gz[i];
      dah[cur][(u0 + i) * kBpP + n] = dr[i];
      dah[cur][(kH + u0 + i) * kBpP + n] = dz[i];
      dah[cur][(2 * kH + u0 + i) * kBpP + n] = dnr[i];
    }
    if (live) {
      const int64_t o = ((int64_t)b * T + t) * (6 * kH) + dir * 3 * kH + u0;
      *reinterpret_cast<float4*>(da_i + o) = make_float4(dr[0], dr[1], dr[2], dr[3]);
      *reinterpret_cast<float4*>(da_i + o + kH) = make_float4(dz[0], dz[1], dz[2], dz[3]);
      *reinterpret_cast<float4*>(da_i + o + 2 * kH) = make_float4(dn[0], dn[1], dn[2], dn[3]);
      *reinterpret_cast<float4*>(da_h + o) = make_float4(dr[0], dr[1], dr[2], dr[3]);
      *reinterpret_cast<float4*>(da_h + o + kH) = make_float4(dz[0], dz[1], dz[2], dz[3]);
      *reinterpret_cast<float4*>(da_h + o + 2 * kH) = make_float4(dnr[0], dnr[1], dnr[2], dnr[3]);
    }
    __syncthreads();
    load_step(step + 1);   // (past the last step: the last step's again, unused)
    // W_hh^T da_h: A = this wave's 16 units x k, B = da_h[k][batch]; four accumulators hide the MFMA latency
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* bp = dah[cur] + q * kBpP + n;
#pragma unroll
    for (int s = 0; s < kBpKS; ++s) acc[s & 3] = mfma4(wt[s], bp[4 * s * kBpP], acc[s & 3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) dh[i] = carry[i] + ((acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]));
    cur ^= 1;   // the other image: a wave still reading this one is at most one barrier behind
  }
}

// ---------------------------------------------------------------------------
// Encoder backward, one wave per row (lane: columns lane and lane + 64).  pre =
// feats W_enc^T (no bias) is recomputed by the GEMM; the ReLU mask is the saved
// output x0 > 0 (gradient 0 at a pre-activation <= 0, torch's convention).
//   a = pre + b, xh = (a - mean) rstd (biased variance, eps 1e-5)
//   dyl = mask ? dx0 : 0, dxh = dyl gamma
//   dpre = rstd (dxh - mean(dxh) - xh mean(dxh xh))
// Outputs: dpre in place of pre, dyl (column sums: d beta), dyl xh (d gamma).
// ---------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void ctc_bwd_layernorm_kernel(float* __restrict__ pre, const float* __restrict__ bias,
                                                                const float* __restrict__ gamma, const float* __restrict__ x0,
                                                                const float* __restrict__ dx0, int64_t rows,
                                                                float* __restrict__ dyl_out, float* __restrict__ dgx_out) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
  const float b0 = bias[lane], b1 = bias[lane + 64], g0 = gamma[lane], g1 = gamma[lane + 64];
  for (int64_t row = wv; row < rows; row += nw) {
    const int64_t o = row * kH + lane;
    const float a0 = pre[o] + b0, a1 = pre[o + 64] + b1;
    const float mean = wave_sum(a0 + a1) * (1.0f / kH);
    const float c0 = a0 - mean, c1 = a1 - mean;
    const float rstd = 1.0f / sqrtf(wave_sum(__builtin_fmaf(c0, c0, c1 * c1)) * (1.0f / kH) + 1e-5f);
    const float xh0 = c0 * rstd, xh1 = c1 * rstd;
    const float dl0 = x0[o] > 0.0f ? dx0[o] : 0.0f, dl1 = x0[o + 64] > 0.0f ? dx0[o + 64] : 0.0f;
    const float dx0h = dl0 * g0, dx1h = dl1 * g1;
    const float m1 = wave_sum(dx0h + dx1h) * (1.0f / kH);
    const float m2 = wave_sum(__builtin_fmaf(dx0h, xh0, dx1h * xh1)) * (1.0f / kH);
    pre[o] = rstd * (dx0h - m1 - xh0 * m2);
    pre[o + 64] = rstd * (dx1h - m1 - xh1 * m2);
    dyl_out[o] = dl0;
    dyl_out[o + 64] = dl1;
    dgx_out[o] = dl0 * xh0;
    dgx_out[o + 64] = dl1 * xh1;
  }
}

// sqrt(sum g^2) in double: thread i adds elements i, i + 1024, ... in order, then a fixed tree over the threads.
__global__ __launch_bounds__(1024) void ctc_bwd_norm_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ out) {
  __shared__ double sm[1024];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const double v = (double)g[i];
    s += v * v;
  }
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)sqrt(sm[0]);
}

// ---- host ---------------------------------------------------------------------
struct Split {
  int splits;
  int64_t kper;
};
// The K split of a GEMM: a function of its shape alone (equal shapes, equal
// summation order on every device).  About 1024 workgroups where the tile
// grid alone gives fewer, at least 256 k per split, kper a multiple of the chunk.
Split gemm_split(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = ((M + kBgT - 1) / kBgT) * ((N + kBgT - 1) / kBgT);
  int64_t s = 1024 / tiles;
  if (s > (K + 255) / 256) s = (K + 255) / 256;
  if (s < 1) s = 1;
  int64_t kper = (K + s - 1) / s;
  kper = (kper + kBgK - 1) / kBgK * kBgK;
  return {(int)((K + kper - 1) / kper), kper};
}

struct Operand {
  const float* p;
  int64_t s_outer, s_k;   // element strides: along m (A) or n (B), and along k
};

// The partials workspace: the training workspace's, at its capacity.
struct Part {
  float* p;
  size_t floats;
};

// C[M][N] (row pitch ldc) = A B on st.  (A split that the workspace could not hold is not made.)
void gemm(hipStream_t st, int M, int N, int64_t K, Operand a, Operand b, float* C, int64_t ldc, Part pt) {
  Split sp = gemm_split(M, N, K);
  if (sp.splits > 1 && (size_t)sp.splits * M * N > pt.floats) sp = {1, K};
  float* part = pt.p;
  const dim3 g((unsigned)((M + kBgT - 1) / kBgT), (unsigned)((N + kBgT - 1) / kBgT), (unsigned)sp.splits);
  const bool ak = a.s_k == 1, bk = b.s_k == 1;
  if (ak && bk)
    hipLaunchKernelGGL((ctc_bwd_gemm_kernel<true, true>), g, dim3(256), 0, st, a.p, a.s_outer, a.s_k, b.p, b.s_k, b.s_outer, C,
                       ldc, M, N, K, sp.kper, part);
  else if (ak)
    hipLaunchKernelGGL((ctc_bwd_gemm_kernel<true, false>), g, dim3(256), 0, st, a.p, a.s_outer, a.s_k, b.p, b.s_k, b.s_outer, C,
                       ldc, M, N, K, sp.kper, part);
  else
    hipLaunchKernelGGL((ctc_bwd_gemm_kernel<false, false>), g, dim3(256), 0, st, a.p, a.s_outer, a.s_k, b.p, b.s_k, b.s_outer,
                       C, ldc, M, N, K, sp.kper, part);
  if (sp.splits > 1) {
    const int64_t mn = (int64_t)M * N;
    hipLaunchKernelGGL(ctc_bwd_reduce_kernel, dim3((unsigned)((mn + 255) / 256 < 4096 ? (mn + 255) / 256 : 4096)), dim3(256), 0,
                       st, part, sp.splits, M, N, C, ldc);
  }
}

void colsum(hipStream_t st, const float* X, int64_t rows, int64_t ld, int N, float* out) {
  hipLaunchKernelGGL(ctc_bwd_colsum_kernel, dim3((unsigned)((N + 63) / 64)), dim3(1024), 0, st, X, rows, ld, N, out);
}

unsigned grid_for(int64_t n, int n_cu) {
  const int64_t blocks = (n + 255) / 256;
  return (unsigned)(blocks < 8 * (int64_t)n_cu ? blocks : 8 * (int64_t)n_cu);
}

}  // namespace

namespace wk {

// W_hh [2 dir][384][128] -> ctc_gru_bptt_kernel's A fragments of W_hh^T: [dir][8 unit tiles][96 k-steps][64 lanes],
// lane l of (tile tl, k-step s) holds W_hh[4 s + (l >> 4)][16 tl + (l & 15)].
std::vector<float> ctc_pack_whht(const float* whh) {
  std::vector<float> pk((size_t)2 * kBpWaves * kBpKS * 64);
  size_t o = 0;
  for (int d = 0; d < 2; ++d)
    for (int tl = 0; tl < kBpWaves; ++tl)
      for (int s = 0; s < kBpKS; ++s)
        for (int ln = 0; ln < 64; ++ln) pk[o++] = whh[((size_t)d * 3 * kH + 4 * s + (ln >> 4)) * kH + 16 * tl + (ln & 15)];
  return pk;
}

size_t ctc_bwd_part_floats(int V, int64_t rows) {
  // every product of launch_ctc_backward, {M, N, K}: the weight gradients (K = rows), then the products over the rows
  const int64_t shapes[9][3] = {{V, 2 * kH, rows}, {3 * kH, 2 * kH, rows}, {3 * kH, kH, rows},     {kH, kMels, rows}, {rows, 2 * kH, V},
                                {rows, 3 * kH, kH}, {rows, 2 * kH, 6 * kH}, {rows, kH, 6 * kH},    {rows, kH, kMels}};
  size_t need = 1;
  for (const auto& s : shapes) {
    const Split sp = gemm_split(s[0], s[1], s[2]);
    const size_t n = sp.splits > 1 ? (size_t)sp.splits * s[0] * s[1] : 0;
    if (n > need) need = n;
  }
  return need;
}

void launch_ctc_backward(const CtcBwd& a, hipStream_t st) {
  const CtcTrainWs& s = a.ws;
  const CtcWeights& w = a.w;
  const int64_t rows = a.B * a.T;
  const int V = a.V, H = kH;
  const CtcBlob blob = ctc_blob(V);
  auto g = [&](int seg) { return a.grads + blob.off[seg]; };   // a segment's gradient
  const Part part{s.part, ctc_bwd_part_floats(V, (int64_t)s.rows)};

  // output layer: db = sum g, dW = g^T y1, dy1 = g W
  colsum(st, a.dlogits, rows, V, V, g(kSegOutB));
  gemm(st, V, 2 * H, rows, {a.dlogits, 1, V}, {s.y[1], 1, 2 * H}, g(kSegOutW), 2 * H, part);
  gemm(st, (int)rows, 2 * H, V, {a.dlogits, V, 1}, {w.out_w, 1, 2 * H}, s.dya, 2 * H, part);
  for (int l = 1; l >= 0; --l) {
    const int din = l == 0 ? H : 2 * H;
    const float* x = l == 0 ? s.x0 : s.drop.on[1] ? s.y0d : s.y[0];
    const float* dy = l == 1 ? s.dya : s.dyb;
    float* dx = l == 1 ? s.dyb : s.dya;
    hipLaunchKernelGGL(ctc_bwd_shift_kernel, dim3(grid_for(rows * (2 * H / 4), a.n_cu)), dim3(256), 0, st, s.y[l].get(), rows, a.T,
                       s.hprev.get());
    for (int d = 0; d < 2; ++d)   // gh = h_prev W_hh^T
      gemm(st, (int)rows, 3 * H, H, {s.hprev + d * H, 2 * H, 1}, {w.whh[l] + (size_t)d * 3 * H * H, H, 1}, s.gh + d * 3 * H,
           6 * H, part);
    hipLaunchKernelGGL(ctc_bwd_gates_kernel, dim3(grid_for(rows * 2 * H, a.n_cu)), dim3(256), 0, st, s.gi[l].get(), s.gh.get(),
                       s.hprev.get(), w.bih[l].get(), w.bhh[l].get(), rows, s.coef.get());
    hipLaunchKernelGGL(ctc_gru_bptt_kernel, dim3((unsigned)((a.B + kBpBatch - 1) / kBpBatch), 2), dim3(kBpThreads), 0, st,
                       s.coef.get(), dy, w.whht_pk[l].get(), a.B, a.T, s.da_i.get(), s.da_h.get());
    for (int d = 0; d < 2; ++d) {
      gemm(st, 3 * H, din, rows, {s.da_i + d * 3 * H, 1, 6 * H}, {x, 1, din}, g(ctc_gru_seg(l, d, kGruWih)), din, part);
      gemm(st, 3 * H, H, rows, {s.da_h + d * 3 * H, 1, 6 * H}, {s.hprev + d * H, 1, 2 * H}, g(ctc_gru_seg(l, d, kGruWhh)), H, part);
      colsum(st, s.da_i + d * 3 * H, rows, 6 * H, 3 * H, g(ctc_gru_seg(l, d, kGruBih)));
      colsum(st, s.da_h + d * 3 * H, rows, 6 * H, 3 * H, g(ctc_gru_seg(l, d, kGruBhh)));
    }
    // dx = da_i [rows][fwd 384 | rev 384] W_ih [fwd rows; rev rows]: both directions' shares in one product
    gemm(st, (int)rows, din, 6 * H, {s.da_i, 6 * H, 1}, {w.wih[l], 1, din}, dx, din, part);
    // the layer's input went through dropout site l: dx <- s m dx (site 0: x0 > 0 below already implies m; s is still due)
    if (s.drop.on[l]) launch_ctc_dropout_bwd(s.drop, l, dx, rows, a.n_cu, st);
  }
  // encoder (dx0 = s.dya [rows][128])
  gemm(st, (int)rows, H, kMels, {s.feats, kMels, 1}, {w.enc_w, kMels, 1}, s.pre, H, part);
  hipLaunchKernelGGL(ctc_bwd_layernorm_kernel, dim3(grid_for(rows * 64, a.n_cu)), dim3(256), 0, st, s.pre.get(), w.enc_b.get(),
                     w.ln_g.get(), s.x0.get(), s.dya.get(), rows, s.t0.get(), s.t1.get());
  colsum(st, s.t1, rows, H, H, g(kSegLnG));
  colsum(st, s.t0, rows, H, H, g(kSegLnB));
  colsum(st, s.pre, rows, H, H, g(kSegEncB));
  gemm(st, H, kMels, rows, {s.pre, 1, H}, {s.feats, 1, kMels}, g(kSegEncW), kMels, part);
  if (a.norm) hipLaunchKernelGGL(ctc_bwd_norm_kernel, dim3(1), dim3(1024), 0, st, a.grads, blob.off[kCtcSegs], a.norm);
}

void launch_ctc_bwd_norm(const float* g, int64_t n, float* out, hipStream_t st) {
  hipLaunchKernelGGL(ctc_bwd_norm_kernel, dim3(1), dim3(1024), 0, st, g, n, out);
}

}  // namespace wk
