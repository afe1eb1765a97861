// wk_ctc_dense.hip -- the dense layers of the GRU-CTC head (wk_ctc.hip) that are
// not the fused fp16 output kernels: X2a, the encoder Linear 80->128 + LayerNorm
// + ReLU (ctc.py:125-130), and the GEMM behind every materialised [rows][N] tensor.
//
// Kernels:
//   ctc_encoder_kernel    Linear 80->128 as fp32 MFMA tiles of 16 rows, LayerNorm
//                         by in-register + 16-lane shuffle sums.
//   ctc_encoder16_kernel  the same on v_mfma_f32_16x16x32_f16 (fp16 mode): fp16
//                         time-major rows out, optionally z-scoring raw rows as
//                         they load (wk_ctc_transcribe).
//   ctc_gemm_nt_kernel    the GEMMs that materialise a [rows][N] tensor (the fp32
//                         parity mode's input projections and output layer, the
//                         fp16 A/B path's projections): 128 x 128 MFMA block
//                         tiles over LDS-staged K chunks, fp32 or fp16 operands,
//                         fp32 accumulate.  ARGMAX mode (fp32 decode without
//                         log-probs): no C, each row's first argmax by a 64-bit
//                         atomicMax; ctc_keys_to_best_kernel decodes the keys.
//   ctc_convert_kernel    element-wise fp16 <-> fp32 copy (attribution paths).
// Host: ctc_gemm_nt, ctc_gemm_argmax (shape checks + launch), the launchers.
#include <math.h>

#include <type_traits>

#include "wk_ctc_dev.h"

using namespace wk;

namespace {

// ---------------------------------------------------------------------------
// X2a: encoder Linear(80,128) + LayerNorm(128) + ReLU, one wave per row
// ---------------------------------------------------------------------------
// Linear 80 -> 128 on the matrix cores: a wave takes 16 rows at a time, D =
// x[16 rows][80] . W^T as 8 column tiles x 20 K-steps of v_mfma_f32_16x16x4f32
// (B fragments from an LDS copy of W laid out [k-step][tile][lane], so each
// read is one conflict-free ds_read_b32).  The lane then holds rows 4 (l>>4) + i
// of column 16 ct + (l & 15): LayerNorm's row sums are 8 in-register adds and
// a 16-lane shuffle reduction.  (Was one wave per row on the VALU: 1.19 ms per
// 4096 utterances.)
__global__ __launch_bounds__(256) void ctc_encoder_kernel(const float* __restrict__ in, int64_t rows,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ out) {
  constexpr int KS = kMels / 4, CT = kH / 16;           // 20 K-steps, 8 column tiles
  __shared__ float wf[KS][CT][64];                      // B[k = 4 s + (l>>4)][col = 16 ct + (l&15)] = W[col][k]
  __shared__ float pb[3][kH];                           // bias, gamma, beta
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < KS * CT * 64; i += 256) {
    const int st = i / (CT * 64), ct = (i / 64) % CT, l = i & 63;
    wf[st][ct][l] = w[(16 * ct + (l & 15)) * kMels + 4 * st + (l >> 4)];
  }
  for (int i = tid; i < kH; i += 256) {
    pb[0][i] = bias[i];
    pb[1][i] = gamma[i];
    pb[2][i] = beta[i];
  }
  __syncthreads();
  const int li = lane & 15, lg = lane >> 4;
  const int64_t nblk = (rows + 15) / 16;
  for (int64_t blk = (int64_t)blockIdx.x * 4 + wv; blk < nblk; blk += (int64_t)gridDim.x * 4) {
    const int64_t r0 = blk * 16;
    const int64_t ra = r0 + li;                          // this lane's A row
    float xa[KS];
#pragma unroll
    for (int st = 0; st < KS; ++st) xa[st] = ra < rows ? in[ra * kMels + 4 * st + lg] : 0.0f;
    f32x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int st = 0; st < KS; ++st)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma4(xa[st], wf[st][ct][lane], acc[ct]);
    float mean[4], rs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s1 = 0.0f;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        acc[ct][i] += pb[0][16 * ct + li];
        s1 += acc[ct][i];
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) s1 += __shfl_xor(s1, o, 64);
      mean[i] = s1 * (1.0f / kH);
      float s2 = 0.0f;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const float d = acc[ct][i] - mean[i];
        s2 = __builtin_fmaf(d, d, s2);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) s2 += __shfl_xor(s2, o, 64);
      rs[i] = 1.0f / sqrtf(s2 * (1.0f / kH) + 1e-5f);   // biased variance, as nn.LayerNorm
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = r0 + 4 * lg + i;
      if (r < rows) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int col = 16 * ct + li;
          out[r * kH + col] = fmaxf(__builtin_fmaf((acc[ct][i] - mean[i]) * rs[i], pb[1][col], pb[2][col]), 0.0f);
        }
      }
    }
  }
}

// fp16 mode (precision 1, "fp16 GEMM operands"): the same Linear 80 -> 128 +
// LayerNorm + ReLU on v_mfma_f32_16x16x32_f16 -- K = 80 in 3 steps (the last
// half zero), 24 MFMAs of 16 cycles per 16 rows instead of 160 fp32 MFMAs of 32
// (the fp32 kernel above ran at ~1/5 of the HBM rate).  W is the A operand and
// the rows the B operand, so a lane ends with 4 consecutive output columns of
// one row per column tile: LayerNorm's sums are in-lane plus two shuffles, and
// each tile leaves as one 8-byte store.  W fragments come from LDS per block
// (24 KB; keeping them in VGPRs would cost 96 registers and the occupancy).
// Output rows are time-major (row t B + b for input row b T + t): the fp16
// path keeps every [rows][.] tensor after the encoder in that order, so that a
// GRU step's 16 utterances are 16 adjacent rows of the gate inputs and outputs.
// NORM (wk_ctc_transcribe): the input rows are raw log-mel; each is z-scored
// with its utterance's zs = {mean, 1/std} (ctc_zstats_kernel) as it is loaded.
template <bool NORM>
__global__ __launch_bounds__(256) void ctc_encoder16_kernel(const float* __restrict__ in, int64_t rows,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int B, int T,
                                                            const float2* __restrict__ zs, __half* __restrict__ out) {
  constexpr int KS = 3, CT = kH / 16;
  __shared__ __attribute__((aligned(16))) h8 wf[KS][CT][64];   // A[col 16 ct + (l&15)][k = 32 s + 8 (l>>4) + j]
  __shared__ __attribute__((aligned(16))) float pb[3][kH];      // bias, gamma, beta
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < KS * CT * 64; i += 256) {
    const int st = i / (CT * 64), ct = (i / 64) % CT, l = i & 63;
    h8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 32 * st + 8 * (l >> 4) + j;
      v[j] = (_Float16)(k < kMels ? w[(16 * ct + (l & 15)) * kMels + k] : 0.0f);
    }
    wf[st][ct][l] = v;
  }
  for (int i = tid; i < kH; i += 256) {
    pb[0][i] = bias[i];
    pb[1][i] = gamma[i];
    pb[2][i] = beta[i];
  }
  __syncthreads();
  const int li = lane & 15, lg = lane >> 4;
  const int64_t nblk = (rows + 15) / 16;
  // Loads and stores go through buffer resources (rows past the end read 0 /
  // drop), so the loop has no branch: the next block's rows are loaded before
  // this block's compute and stores, and the compiler's vmcnt waits for those
  // loads only, not for the stores behind them (with guarded accesses it
  // waited for everything: ~60 % of wave-cycles were waits, PMC).
  const __amdgpu_buffer_rsrc_t irs = make_rsrc(in, (uint32_t)(rows * kMels * 4));   // < 2^31 B (host check)
  const __amdgpu_buffer_rsrc_t ors = make_rsrc(out, (uint32_t)(rows * kH * 2));
  // one block of input rows in flight per wave (a block's compute is
  // far shorter than the HBM latency)
  float4 xr[KS][2];
  auto load_blk = [&](int64_t blk, float4 (&x)[KS][2]) __attribute__((always_inline)) {
    const int64_t r = blk * 16 + li;
#pragma unroll
    for (int st = 0; st < KS; ++st) {
      const int k0 = 32 * st + 8 * lg;
      const int off = r < rows && k0 < kMels ? (int)(r * kMels + k0) * 4 : 0x7FFFFFE0;   // past num_records: 0
      x[st][0] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(irs, off, 0, 0));
      x[st][1] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(irs, off + 16, 0, 0));
    }
  };
  const int64_t G = (int64_t)gridDim.x * 4;
  auto body = [&](int64_t blk, float4 (&x)[KS][2]) __attribute__((always_inline)) {
    const int64_t r = blk * 16 + li;   // this lane's row
    const int rr = r < rows ? (int)r : 0;   // rows < 2^31 (host check)
    const int ub = rr / T, ut = rr - ub * T;
    h8 xb[KS];
    if constexpr (NORM) {
      const float2 z = zs[ub];
#pragma unroll
      for (int st = 0; st < KS; ++st) {
        const float4 a = x[st][0], b = x[st][1];
        xb[st] = h8{(_Float16)((a.x - z.x) * z.y), (_Float16)((a.y - z.x) * z.y), (_Float16)((a.z - z.x) * z.y),
                     (_Float16)((a.w - z.x) * z.y), (_Float16)((b.x - z.x) * z.y), (_Float16)((b.y - z.x) * z.y),
                     (_Float16)((b.z - z.x) * z.y), (_Float16)((b.w - z.x) * z.y)};
      }
    } else {
#pragma unroll
      for (int st = 0; st < KS; ++st) {
        const float4 a = x[st][0], b = x[st][1];
        xb[st] = h8{(_Float16)a.x, (_Float16)a.y, (_Float16)a.z, (_Float16)a.w,
                     (_Float16)b.x, (_Float16)b.y, (_Float16)b.z, (_Float16)b.w};
      }
    }
    load_blk(blk + G, x);   // the wave's next block into the same registers (past the end: zeros, unused)
    f32x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = *reinterpret_cast<const f32x4*>(&pb[0][16 * ct + 4 * lg]);   // + bias
    int wl = lane;
    asm volatile("" : "+v"(wl));   // W fragments re-read per block, not hoisted into 96 VGPRs
#pragma unroll
    for (int st = 0; st < KS; ++st)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[st][ct][wl], xb[st], acc[ct], 0, 0, 0);
    // acc[ct][i] = row r, column 16 ct + 4 lg + i; the row's 128 columns are in lanes li + 16 q
    float s1 = 0.0f;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) s1 += (acc[ct][0] + acc[ct][1]) + (acc[ct][2] + acc[ct][3]);
    s1 = sum_rows4(s1);
    const float mean = s1 * (1.0f / kH);
    float s2 = 0.0f;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = acc[ct][i] - mean;
        s2 = __builtin_fmaf(d, d, s2);
      }
    s2 = sum_rows4(s2);
    const float rs = 1.0f / sqrtf(s2 * (1.0f / kH) + 1e-5f);   // biased variance, as nn.LayerNorm
    const int orow = r < rows ? (ut * B + ub) * (kH * 2) : 0x7FFFFE00;   // time-major output row (bytes); past the end: dropped
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int c0 = 16 * ct + 4 * lg;
      const f32x4 g = *reinterpret_cast<const f32x4*>(&pb[1][c0]);
      const f32x4 bt = *reinterpret_cast<const f32x4*>(&pb[2][c0]);
      _Float16 y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] = (_Float16)fmaxf(__builtin_fmaf((acc[ct][i] - mean) * rs, g[i], bt[i]), 0.0f);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, y), ors,
                                            orow + c0 * 2, 0, 0);
    }
  };
  int64_t blk = (int64_t)blockIdx.x * 4 + wv;
  load_blk(blk, xr);
  for (; blk < nblk; blk += G) body(blk, xr);
}
// ---------------------------------------------------------------------------
// Plain GEMM C[M][N] = A[M][K] W[N][K]^T, fp32 accumulate, for the paths that
// materialise a [rows][N] tensor: the fp32 parity mode's input projections (N =
// 768) and output layer (N = V, ctc.py:146), and the fp16 A/B path's
// projections (WAKEWORD_CTC_GEMM=1).  fp32 operands on v_mfma_f32_16x16x4_f32
// (exact fp32 products and sums), fp16 on v_mfma_f32_16x16x16_f16.
// Block tile 128 rows x 128 columns, 4 waves of 64 x 64 (4 x 4 accumulators
// of 16 x 16).  K goes in chunks of 64 bytes per row (16 fp32 / 32 fp16): the
// block stages a chunk of its A rows and W rows in LDS (double-buffered, one
// barrier per chunk; the next chunk's global loads are in flight during this
// chunk's MFMAs), and a lane reads its fragments as 16-byte pieces: lane
// group q = lane >> 4 holds piece q of a row (E = 4 fp32 / 8 fp16 k), and MFMA
// step s takes element s (fp32) or elements 4s .. 4s + 3 (fp16) of it -- the
// same k permutation in A and W, so the chunk is complete after its steps.
// Rows past M and columns past N read a clamped row and are never stored.
// K is a multiple of the chunk.  LDS rows are 64 bytes with their four 16-byte
// pieces swizzled (gemm_piece): the fragment reads are bank-conflict-free.
// ---------------------------------------------------------------------------
constexpr int kGemmBM = 128, kGemmBN = 128, kGemmPitch = 4;   // LDS row pitch in 16-byte pieces (swizzled, below)
// piece q of LDS row n sits at q ^ ((n >> 1) & 3): each 16-lane group of a
// fragment ds_read_b128 (rows li, pieces q) then covers all 64 banks (brute-forced).
__device__ __forceinline__ int gemm_piece(int n, int q) { return q ^ ((n >> 1) & 3); }

// Element-wise fp16 <-> fp32 copy (the WAKEWORD_CTC_MIX attribution paths).
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void ctc_convert_kernel(const TI* __restrict__ in, TO* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if constexpr (std::is_same<TO, __half>::value) out[i] = __float2half((float)in[i]);
    else out[i] = (float)in[i];
  }
}

// ARGMAX (fp32 decode, no log-probs): C is not written; each row's first
// argmax of (A W^T)[row] + bias over the block's columns goes to keys[row] by a
// 64-bit atomicMax on {order-preserving float bits, ~column} (the larger logit
// wins, an equal logit keeps the smaller column, as torch.argmax), so the
// [rows][V] fp32 logits never exist (19.7 GB written and read back at config
// 5 before).  keys must be zeroed first; ctc_keys_to_best_kernel decodes them.
__device__ __forceinline__ unsigned long long argmax_key(float v, int col) {
  unsigned u = __float_as_uint(v);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)col);
}

__global__ __launch_bounds__(256) void ctc_keys_to_best_kernel(const unsigned long long* __restrict__ keys,
                                                               int64_t rows, int* __restrict__ best) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < rows) best[r] = (int)(0xFFFFFFFFu - (unsigned)(keys[r] & 0xFFFFFFFFull));
}

template <typename TI, typename TO, bool ARGMAX = false>
__global__ __launch_bounds__(256) void ctc_gemm_nt_kernel(const TI* __restrict__ A, const TI* __restrict__ W,
                                                          TO* __restrict__ C, int64_t M, int N, int K,
                                                          const float* __restrict__ bias = nullptr,
                                                          unsigned long long* __restrict__ keys = nullptr) {
  constexpr bool F16 = std::is_same<TI, __half>::value;
  constexpr int E = 16 / (int)sizeof(TI), KC = 4 * E;
  __shared__ uint4 As[2][kGemmBM * kGemmPitch], Ws[2][kGemmBN * kGemmPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, q = lane >> 4, wm = wave >> 1, wn = wave & 1;
  const int64_t r0 = (int64_t)blockIdx.x * kGemmBM;
  const int c0 = blockIdx.y * kGemmBN;
  // cooperative staging: thread tid moves pieces p = tid and tid + 256 of each
  // operand (row p >> 2, piece p & 3 of the chunk)
  const uint4* ga[2];
  const uint4* gw[2];
  int so[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int p = tid + 256 * h, row = p >> 2, pc = p & 3;
    const int64_t ra = r0 + row < M ? r0 + row : M - 1;
    const int cw = c0 + row < N ? c0 + row : N - 1;
    ga[h] = reinterpret_cast<const uint4*>(A + ra * K) + pc;
    gw[h] = reinterpret_cast<const uint4*>(W + (int64_t)cw * K) + pc;
    so[h] = row * kGemmPitch + gemm_piece(row, pc);
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const int nch = K / KC;
  uint4 pa[2], pw[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    pa[h] = ga[h][0];
    pw[h] = gw[h][0];
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    As[0][so[h]] = pa[h];
    Ws[0][so[h]] = pw[h];
  }
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const int buf = c & 1;
    {   // next chunk's pieces (the last chunk re-loads itself: unconditional loads keep pa / pw in
        // registers -- under a branch the compiler staged them through scratch and waited at once)
      const int cn = c + 1 < nch ? c + 1 : c;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        pa[h] = ga[h][4 * cn];
        pw[h] = gw[h][4 * cn];
      }
    }
    uint4 a[4], w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = As[buf][(64 * wm + 16 * i + li) * kGemmPitch + gemm_piece(li, q)];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = Ws[buf][(64 * wn + 16 * j + li) * kGemmPitch + gemm_piece(li, q)];
    if constexpr (F16) {
      typedef _Float16 h4v __attribute__((ext_vector_type(4)));
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint2 au = st ? make_uint2(a[i].z, a[i].w) : make_uint2(a[i].x, a[i].y);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint2 wu = st ? make_uint2(w[j].z, w[j].w) : make_uint2(w[j].x, w[j].y);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(h4v, au), __builtin_bit_cast(h4v, wu),
                                                              acc[i][j], 0, 0, 0);
          }
        }
    } else {
#pragma unroll
      for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float av = __uint_as_float(st == 0 ? a[i].x : st == 1 ? a[i].y : st == 2 ? a[i].z : a[i].w);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float wv = __uint_as_float(st == 0 ? w[j].x : st == 1 ? w[j].y : st == 2 ? w[j].z : w[j].w);
            acc[i][j] = mfma4(av, wv, acc[i][j]);
          }
        }
    }
    if (c + 1 < nch) {   // buffer buf ^ 1 was last read in chunk c - 1, before the barrier below it
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        As[buf ^ 1][so[h]] = pa[h];
        Ws[buf ^ 1][so[h]] = pw[h];
      }
    }
    __syncthreads();
  }
  if constexpr (ARGMAX) {
    float bj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = c0 + 64 * wn + 16 * j + li;
      bj[j] = col < N ? bias[col] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float bv = -INFINITY;
        int bc = 0x7FFFFFFF;
#pragma unroll
        for (int j = 0; j < 4; ++j) {   // this lane's columns, increasing
          const int col = c0 + 64 * wn + 16 * j + li;
          const float v = acc[i][j][r] + bj[j];
          if (col < N && v > bv) { bv = v; bc = col; }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {   // the 16 column lanes of the row: first maximum
          const float ov = __shfl_xor(bv, o, 64);
          const int oc = __shfl_xor(bc, o, 64);
          if (ov > bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
        }
        const int64_t row = r0 + 64 * wm + 16 * i + 4 * q + r;
        if (li == 0 && row < M && bc < N) atomicMax(keys + row, argmax_key(bv, bc));
      }
    return;
  }
  // D of a 16 x 16 tile: lane holds rows 4q .. 4q + 3, column li
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = c0 + 64 * wn + 16 * j + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = r0 + 64 * wm + 16 * i + 4 * q + r;
        if (row < M && col < N) {
          if constexpr (std::is_same<TO, __half>::value) C[row * N + col] = __float2half(acc[i][j][r]);
          else C[row * N + col] = acc[i][j][r];
        }
      }
    }
}

}  // namespace

namespace wk {

wk_status ctc_gemm_nt(hipStream_t st, int64_t M, int64_t N, int64_t K, const void* A, const void* W, void* C, bool f16,
                      bool c16) {
  if (M <= 0) return WK_OK;
  if (K % (f16 ? 32 : 16) != 0 || N > INT32_MAX || K > INT32_MAX || (M + kGemmBM - 1) / kGemmBM > INT32_MAX)
    return fail(WK_ERR_UNSUPPORTED, "ctc gemm: K must be a multiple of 16 (fp32) / 32 (fp16)");
  const dim3 g((unsigned)((M + kGemmBM - 1) / kGemmBM), (unsigned)((N + kGemmBN - 1) / kGemmBN));
  if (f16 && c16)
    hipLaunchKernelGGL((ctc_gemm_nt_kernel<__half, __half>), g, dim3(256), 0, st, (const __half*)A, (const __half*)W,
                       (__half*)C, M, (int)N, (int)K);
  else if (f16)
    hipLaunchKernelGGL((ctc_gemm_nt_kernel<__half, float>), g, dim3(256), 0, st, (const __half*)A, (const __half*)W,
                       (float*)C, M, (int)N, (int)K);
  else
    hipLaunchKernelGGL((ctc_gemm_nt_kernel<float, float>), g, dim3(256), 0, st, (const float*)A, (const float*)W,
                       (float*)C, M, (int)N, (int)K);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? WK_OK : hip_fail(e, "ctc gemm launch");
}

wk_status ctc_gemm_argmax(hipStream_t st, int64_t M, int64_t N, int64_t K, const float* A, const float* W,
                          const float* bias, unsigned long long* keys, int* best) {
  if (M <= 0) return WK_OK;
  if (K % 16 != 0 || N > INT32_MAX || K > INT32_MAX || (M + kGemmBM - 1) / kGemmBM > INT32_MAX)
    return fail(WK_ERR_UNSUPPORTED, "ctc gemm: K must be a multiple of 16");
  hipError_t e = hipMemsetAsync(keys, 0, sizeof(unsigned long long) * M, st);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
  const dim3 g((unsigned)((M + kGemmBM - 1) / kGemmBM), (unsigned)((N + kGemmBN - 1) / kGemmBN));
  hipLaunchKernelGGL((ctc_gemm_nt_kernel<float, float, true>), g, dim3(256), 0, st, A, W, (float*)nullptr, M, (int)N,
                     (int)K, bias, keys);
  hipLaunchKernelGGL(ctc_keys_to_best_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, keys, M, best);
  e = hipGetLastError();
  return e == hipSuccess ? WK_OK : hip_fail(e, "ctc gemm-argmax launch");
}

void launch_ctc_encoder(bool f16, const float* feats, int B, int T, const float* w, const float* bias, const float* gamma,
                        const float* beta, const float2* zs, void* out, int n_cu, hipStream_t st) {
  const int64_t rows = (int64_t)B * T;
  // two 4-wave workgroups per CU: 3 or more measured slower (0.187 -> 0.21-0.22 ms, profiles/r05g_ctc_ab.txt)
  const dim3 g((int)((rows + 63) / 64 < 2 * n_cu ? (rows + 63) / 64 : 2 * n_cu));
  if (!f16)
    hipLaunchKernelGGL(ctc_encoder_kernel, g, dim3(256), 0, st, feats, rows, w, bias, gamma, beta, (float*)out);
  else if (zs)
    hipLaunchKernelGGL(ctc_encoder16_kernel<true>, g, dim3(256), 0, st, feats, rows, w, bias, gamma, beta, B, T, zs, (__half*)out);
  else
    hipLaunchKernelGGL(ctc_encoder16_kernel<false>, g, dim3(256), 0, st, feats, rows, w, bias, gamma, beta, B, T,
                       (const float2*)nullptr, (__half*)out);
}

void launch_ctc_convert(const __half* in, float* out, int64_t n, int n_cu, hipStream_t st) {
  hipLaunchKernelGGL((ctc_convert_kernel<__half, float>), dim3(2 * n_cu), dim3(256), 0, st, in, out, n);
}
void launch_ctc_convert(const float* in, __half* out, int64_t n, int n_cu, hipStream_t st) {
  hipLaunchKernelGGL((ctc_convert_kernel<float, __half>), dim3(2 * n_cu), dim3(256), 0, st, in, out, n);
}

}  // namespace wk
