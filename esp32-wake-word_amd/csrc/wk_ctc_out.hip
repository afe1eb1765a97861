// wk_ctc_out.hip -- X2c / X3 of the GRU-CTC head (wk_ctc.hip): Linear 256->V,
// log_softmax, per-frame argmax and the greedy CTC decode (ctc.py:143-152,
// 453-471).
//
// Kernels:
//   ctc_argmax_kernel        one wave per row of materialised logits: bias,
//                            max/argmax (first index), log-sum-exp, optional
//                            log_softmax output.
//   ctc_out_argmax16_kernel  fp16 mode: output layer + first argmax fused on
//                            v_mfma_f32_16x16x32_f16, W tiles by LDS-DMA, the
//                            logits never in HBM (LOGITS: also stored as fp16
//                            for the log_softmax); KEYED (V <= 4096): the
//                            column rides in the value's low mantissa bits and
//                            the runner-up is tracked for the re-score.
//   ctc_out_decode16_kernel  its decode-only KEYED form with the fold moved in
//                            among the MFMAs (57 % of the config-5 step).
//   ctc_rescore_kernel       near-tie rows of the two kernels above decided
//                            again between their top-2 columns in fp32.
//   ctc_pred_kernel          best[] -> batch-major per-frame argmax.
//   ctc_greedy_kernel        one wave per utterance: drop blanks, collapse repeats.
// out_load_a, out_dma_offsets and out_row_reduce are the three blocks the two
// fused kernels share.
#include <float.h>
#include <math.h>

#include <type_traits>

#include "wk_ctc_dev.h"

using namespace wk;

namespace {

// ---------------------------------------------------------------------------
// X2c / X3: bias + log_softmax + argmax, one wave per row; greedy collapse
// ---------------------------------------------------------------------------
// Online softmax state of one lane: running max (first index on ties, as
// torch.max) and the sum of exp rescaled to it.
struct SoftmaxAcc {
  float mx = -INFINITY, s = 0.0f;
  int arg = 0x7fffffff;
  __device__ __forceinline__ void push(float y, int v) {
    if (y > mx) {
      s = s * __expf(mx - y) + 1.0f;
      mx = y;
      arg = v;
    } else {
      s += __expf(y - mx);
    }
  }
};

// tm_B > 0: logits rows are time-major (t tm_B + b); log_probs stays [b][t].
template <typename LT>
__global__ __launch_bounds__(256) void ctc_argmax_kernel(const LT* __restrict__ logits, const float* __restrict__ bias,
                                                         int64_t rows, int V, float* __restrict__ log_probs,
                                                         int* __restrict__ best, int tm_B = 0, int T = 0) {
  constexpr int NV = 16 / (int)sizeof(LT);   // elements per 16-byte load
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;   // wave-uniform
  const LT* x = logits + r * V;
  SoftmaxAcc acc;
  if (V % NV == 0) {   // rows are 16-byte aligned: one 16-byte load per lane per step
    for (int c = lane; c < V / NV; c += 64) {
      LT e[NV];
      float bb[NV];
      *reinterpret_cast<uint4*>(e) = reinterpret_cast<const uint4*>(x)[c];
#pragma unroll
      for (int q = 0; q < NV / 4; ++q) *reinterpret_cast<float4*>(bb + 4 * q) = reinterpret_cast<const float4*>(bias)[c * (NV / 4) + q];
      float y[NV];
      float lm = -INFINITY;
      int li = 0;
#pragma unroll
      for (int i = 0; i < NV; ++i) {   // chunk max (first index) ...
        y[i] = (float)e[i] + bb[i];
        if (y[i] > lm) { lm = y[i]; li = i; }
      }
      float ls = 0.0f;
#pragma unroll
      for (int i = 0; i < NV; ++i) ls += __expf(y[i] - lm);   // ... independent exps, then one merge
      if (lm > acc.mx) {
        acc.s = acc.s * __expf(acc.mx - lm) + ls;
        acc.mx = lm;
        acc.arg = c * NV + li;
      } else {
        acc.s += ls * __expf(lm - acc.mx);
      }
    }
  } else {
    for (int v = lane; v < V; v += 64) acc.push((float)x[v] + bias[v], v);
  }
  float mx = acc.mx, s = acc.s;
  int arg = acc.arg;
  for (int m = 32; m >= 1; m >>= 1) {
    const float om = __shfl_xor(mx, m, 64), os = __shfl_xor(s, m, 64);
    const int oa = __shfl_xor(arg, m, 64);
    const float nm = fmaxf(mx, om);
    s = (mx == -INFINITY ? 0.0f : s * __expf(mx - nm)) + (om == -INFINITY ? 0.0f : os * __expf(om - nm));
    if (om > mx || (om == mx && oa < arg)) arg = oa;
    mx = nm;
  }
  if (log_probs) {
    const float lse = mx + logf(s);
    const int64_t orow = tm_B > 0 ? (r % tm_B) * T + r / tm_B : r;
    for (int v = lane; v < V; v += 64) log_probs[orow * V + v] = (float)x[v] + bias[v] - lse;
  }
  if (lane == 0 && best) best[r] = arg;
}

// decode_predictions' per-frame argmax (ctc.py:454) in batch-major order:
// pred[b][t] from the output layer's best[] (time-major rows in fp16 mode).
__global__ __launch_bounds__(256) void ctc_pred_kernel(const int* __restrict__ best, int64_t B, int T, int tm,
                                                       int* __restrict__ pred) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= B * (int64_t)T) return;
  const int64_t b = r / T, t = r - b * T;
  pred[r] = best[tm ? t * B + b : r];
}

// decode_predictions (ctc.py:453-471): drop blanks (0) and collapse repeats,
// prev starting at the blank (ctc.py:462).  One wave per utterance, 64 frames
// at a time: a frame is kept when tok != 0 and tok != tok[t-1]; its output slot
// is the count kept so far plus the kept lanes below it (ballot + mbcnt).
// (One thread per utterance walking its T frames serially took 0.17 ms per
// 4096 utterances: strided, dependent loads.)
// tm: best is time-major (frame t of utterance b at t B + b).
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const int* __restrict__ best, int64_t B, int T,
                                                         int* __restrict__ tokens, int* __restrict__ lengths,
                                                         int tm = 0) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const int64_t ts = tm ? B : 1;   // frame stride
  const int* p = best + (tm ? b : b * T);
  int* o = tokens + b * T;
  int n = 0;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    const int tok = t < T ? p[t * ts] : 0;
    const int prev = t == 0 ? 0 : (t < T ? p[(t - 1) * ts] : 0);
    const bool keep = tok != 0 && tok != prev;
    const uint64_t m = __ballot(keep);
    const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
    if (keep) o[n + below] = tok;
    n += __popcll(m);
  }
  for (int t = n + lane; t < T; t += 64) o[t] = -1;
  if (lane == 0) lengths[b] = n;
}

// ---------------------------------------------------------------------------
// X2 output layer + X3 argmax, fused (fp16 mode): best[r] = first argmax over
// v of (y[r] . W[v] + b[v]) with y [rows][256] and W [V][256] in fp16, fp32
// accumulation on v_mfma_f32_16x16x32_f16 -- the [rows][V] logits never touch
// HBM (they were 2 x 9.9 GB of traffic per 4096 utterances).  A workgroup owns
// kOutRows rows: each of its kOutWaves waves keeps its 16 kOutRF rows' A
// fragments in VGPRs (kOutRF row tiles x 8 K-steps) and walks V in 64-column tiles of W staged through
// a double-buffered LDS image (512-byte rows, 16-byte chunks XOR-swizzled: a
// B-fragment ds_read_b128 is conflict-free), one barrier per tile.  Each lane keeps
// a running (max, index) for its 4 RF rows over its columns, visited in increasing
// order, then 16-lane shuffles pick the first maximum (torch.max semantics).
// LOGITS = true also stores the fp16 logits (bias included) for the log_softmax
// kernel; the argmax is this kernel's in both cases and both variants
// accumulate identically (bias as the first MFMA's C operand, the same K
// order), so tokens do not depend on log-probs being requested.
// ---------------------------------------------------------------------------
// Double-buffered W tiles of 64 columns, 3 row tiles per wave, 8 waves (a
// four-buffer ring with the LDS-DMA two tiles ahead, 32- and 128-column tiles,
// 12 waves were measured slower: DESIGN 5.3).
constexpr int kOutNB = 2, kOutAhead = 1;
constexpr int kOutK = 2 * kH, kOutBN = 64, kOutCF = kOutBN / 16, kOutPitch = kOutK, kOutRF = 3, kOutWaves = 8;
// W tile rows are 512 B with their 16-byte chunks XOR-swizzled by the row's
// low 4 bits (chunk c of row n at c ^ (n & 15)): a ds_read_b128 B fragment
// (row 16 cf + li, chunk 4 st + lg) then hits 16 distinct 4-bank windows in
// each of the instruction's four lane groups.  (With the former padded pitch
// of 264 halfs, 42 % of the kernel's LDS cycles were bank conflicts, PMC.)
__device__ __forceinline__ int out_chunk(int n, int c) { return c ^ (n & 15); }
// (RF = 3, 48 rows per wave: each B fragment read from LDS feeds 3 MFMAs -- the
// LDS bytes per MFMA were the limit at RF = 2; 246 VGPRs, still 2 waves per
// SIMD: +3 % utterances/s.)
constexpr int out_rf(bool logits) { return logits ? 2 : kOutRF; }
constexpr int out_rows(bool logits) { return 16 * out_rf(logits) * kOutWaves; }
// KEYED (V <= 4096, so 4 NT <= 256): the running maximum carries its column
// in the value's low 8 mantissa bits, so the epilogue is one VALU per value
// (v_and_or_b32) and one v_max3_f32 per two values instead of compare + two
// selects per value.  The tag is 255 - (4 tile + cf): among values whose
// upper 24 bits agree, an earlier column makes the larger tagged value when
// they are positive, so equal logits keep the first index, as torch.argmax
// does (ctc.py:454).  Between negative values the tag orders the other way
// (round 4 spread the sign into the tag with a v_perm_b32 first: two VALU per
// value); such a tie is within 2^-15 of the row's maximum, which makes the
// row a near-tie that ctc_rescore_kernel decides again in fp32 with the
// first-index rule.  The column is 16 (4 tile + cf) + li.  A tagged value
// moves by < 2^-15 of itself: the first maximum is exact except between
// logits that agree to within that (fp16 operands already put ~1e-3 of noise
// on every logit); the tokens stay a function of the row alone.
// m = max(m, k0, k1) on the tagged values (fmaxf would first canonicalise
// each of them: they come from integer ops).  The tags are applied in C++, so
// the compiler still places the wait states for reading MFMA results.
__device__ __forceinline__ float out_max3(float m, float k0, float k1) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(k0), "v"(k1));
  return r;
}
// mask = 0xffffff00 (in a VGPR: VOP3 takes no literal), tag in an SGPR
__device__ __forceinline__ float out_tag(float x, unsigned mask, unsigned tag) {
  return __builtin_bit_cast(float, (__builtin_bit_cast(unsigned, x) & mask) | tag);
}
// Runner-up tracking (KEYED): the second largest of {m, k0, k1} is their
// median; the row's running second maximum is max(m2, med3(m, k0, k1)), and
// over four values max3(m2, med3(m, k0, k1), med3(max3(m, k0, k1), k2, k3)).
__device__ __forceinline__ float out_med3(float a, float b, float c) {
  float r;
  asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// Near-tie re-scoring (decision parity): a row whose top-2 tagged
// logits are closer than this is re-decided between those two columns in fp32
// (ctc_rescore_kernel).  The fp16 operands move a logit by ~3e-4 rms here
// (256 products of fp16-rounded weights); the margin test is generous.
__device__ __forceinline__ bool out_near_tie(float m1, float m2) {
  return m1 - m2 < 4e-3f + 2e-3f * fabsf(m1);
}

// The column block (4 tile + cf) of a tagged value.
__device__ __forceinline__ int out_untag(float m) { return (int)(255u - (__builtin_bit_cast(unsigned, m) & 255u)); }

// A fragments of a wave's 16 RF rows: rows row0 + 16 rf + li, k = 32 st + 8 lg .. +7 (rows past the end: 0).
template <int RF>
__device__ __forceinline__ void out_load_a(h8 (&a)[RF][8], const __half* __restrict__ y, int64_t row0, int64_t rows, int li,
                                           int lg) {
#pragma unroll
  for (int rf = 0; rf < RF; ++rf) {
    const int64_t r = row0 + 16 * rf + li;
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      uint4 v = make_uint4(0, 0, 0, 0);
      // Non-temporal: the once-read y rows do not evict the W tiles every
      // workgroup re-reads from L2 (PMC: 851 -> 681 MB per launch against
      // 638 MB algorithmic, same time; profiles/r05c_*_ctc_hbm_traffic.json).
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      if (r < rows) {
        const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(y + r * kOutK + 32 * st + 8 * lg));
        v = make_uint4(t[0], t[1], t[2], t[3]);
      }
      a[rf][st] = __builtin_bit_cast(h8, v);
    }
  }
}

// W tile -> LDS by DMA (buffer_load ... lds) in 1 KB pieces (two 512-byte
// rows), dealt to the first NW waves of the workgroup: piece q = wave x pieces
// per wave + i covers rows 2 q and 2 q + 1; lane L writes position L & 31 of
// its row, so it loads global chunk (L & 31) ^ (row & 15) -- the swizzle is in
// the global addresses.  A lane's offsets within a tile are tile-invariant:
// computed once, the tile's base goes in the scalar offset.  (Waves past NW get
// wave 0's offsets and never issue.)
template <int NW>
__device__ __forceinline__ void out_dma_offsets(int (&off)[kOutBN * kOutK * 2 / 1024 / NW], int wvu, int lane) {
  constexpr int PER = kOutBN * kOutK * 2 / 1024 / NW;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int q = (NW == kOutWaves || wvu < NW ? wvu : 0) * PER + i, rr = 2 * q + (lane >> 5), c = (lane & 31) ^ (rr & 15);
    off[i] = rr * (kOutK * 2) + 16 * c;
  }
}

// A row's first maximum (m, column k) across its 16 column lanes (torch.max
// semantics: an equal value keeps the smaller column) and, KEYED, the merged
// runner-up (m2, k2); lane li == 0 stores best[r] and, for a near-tie, the
// runner-up's column in best2[r] (else -1).
template <bool KEYED>
__device__ __forceinline__ void out_row_reduce(float m, int k, float m2, int k2, int li, int64_t r, int64_t rows,
                                               int* __restrict__ best, int* __restrict__ best2) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int ok = __shfl_xor(k, o, 64);
    const bool other_wins = om > m || (om == m && ok < k);
    if (KEYED) {
      const float om2 = __shfl_xor(m2, o, 64);
      const int ok2 = __shfl_xor(k2, o, 64);
      // the merged runner-up: the loser of the two maxima, or the larger runner-up
      const float lm = other_wins ? m : om;
      const int lk = other_wins ? k : ok;
      const bool r_other = om2 > m2 || (om2 == m2 && ok2 < k2);
      const float rm = r_other ? om2 : m2;
      const int rk = r_other ? ok2 : k2;
      const bool use_loser = lm > rm || (lm == rm && lk < rk);
      m2 = use_loser ? lm : rm;
      k2 = use_loser ? lk : rk;
    }
    if (other_wins) { m = om; k = ok; }
  }
  if (li == 0 && r < rows) {
    best[r] = k;
    best2[r] = KEYED && m2 > -INFINITY && out_near_tie(m, m2) ? k2 : -1;
  }
}

template <bool LOGITS, bool KEYED>
__global__ __launch_bounds__(kOutWaves * 64) void ctc_out_argmax16_kernel(const __half* __restrict__ y,
                                                                          const __half* __restrict__ w,
                                                                          const float* __restrict__ bias, int64_t rows,
                                                                          int V, __half* __restrict__ logits,
                                                                          int* __restrict__ best,
                                                                          int* __restrict__ best2) {
  constexpr int kOutRF = out_rf(LOGITS), kOutRows = out_rows(LOGITS);
  __shared__ __attribute__((aligned(1024))) _Float16 bt[kOutNB][kOutBN * kOutPitch];   // (EARLYDMA: row addresses XOR the chunk)
  // the tile's bias, staged with its W rows (an L2 load per column in the
  // epilogue stalled it); replicated x4 so one ds_read_b128 is an MFMA C operand
  __shared__ f32x4 bsh[kOutNB][kOutBN];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const bool wave0 = __builtin_amdgcn_readfirstlane(wv) < (kOutBN + 63) / 64;   // the waves that stage the tile's bias
  const int64_t row0 = (int64_t)blockIdx.x * kOutRows + 16 * kOutRF * wv;
  h8 a[kOutRF][8];
  out_load_a<kOutRF>(a, y, row0, rows, li, lg);
  const int NT = (V + kOutBN - 1) / kOutBN;
  // W tile nt -> registers: 64 rows x 32 16-byte chunks, 4 per thread.  Buffer
  // loads: rows past V come back 0 from the range check, no branch per load.
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(w, (uint32_t)V * kOutK * 2);
  const __amdgpu_buffer_rsrc_t brs = make_rsrc(bias, (uint32_t)V * 4);
  float pb = 0.0f;
  // W tile nt -> bt[nt & 1] by LDS-DMA (buffer_load ... lds), issued by waves
  // 0-3 after their MFMA phase: instruction i of wave w fills 1 KB = rows
  // 2 (8 w + i) and +1 (out_dma_offsets).  The compiler makes every LDS read
  // after an LDS-DMA wait for it, so no wave issues one before its own
  // B-fragment reads of the period; the target buffer was last read in the
  // previous period, and the explicit vmcnt(0) before the closing barrier
  // completes the DMA.
  const int wvu = __builtin_amdgcn_readfirstlane(wv);
  constexpr int kDmaWaves = 4, kDmaPer = kOutBN * kOutK * 2 / 1024 / kDmaWaves;   // waves 0-3 (leading) issue the DMA
  int dma_off[kDmaPer];
  out_dma_offsets<kDmaWaves>(dma_off, wvu, lane);
  auto dma_piece = [&](int nt, int i) {
    const int q = wvu * kDmaPer + i;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)&bt[nt & (kOutNB - 1)][q * 512], 16,
                                             dma_off[i], nt * (kOutBN * kOutK * 2), 0, 0);
  };
  auto dma_w = [&](int nt) {
    if (wvu >= kDmaWaves) return;
#pragma unroll
    for (int i = 0; i < kDmaPer; ++i) dma_piece(nt, i);
  };
  auto fetch = [&](int nt) {   // the tile's bias (W comes by dma_w)
    if (wave0) pb = buf_load(brs, 4 * (nt * kOutBN + tid), 0);
  };
  auto stash = [&](int buf) {
    if (wave0 && tid < kOutBN) bsh[buf][tid] = f32x4{pb, pb, pb, pb};
  };
  fetch(0);
  stash(0);
  dma_w(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  float mx[kOutRF][4], mx2[kOutRF][4];   // (mx2: KEYED runner-up)
  int ix[kOutRF][4];
  unsigned kmask;   // (KEYED) out_tag's mask, in a VGPR (VOP3 takes no literal)
  asm("v_mov_b32 %0, 0xffffff00" : "=v"(kmask));
#pragma unroll
  for (int rf = 0; rf < kOutRF; ++rf)
#pragma unroll
    for (int i = 0; i < 4; ++i) { mx[rf][i] = -INFINITY; mx2[rf][i] = -INFINITY; ix[rf][i] = 0; }
  // Skew: the second half of the waves (4-7, each the partner of
  // a first-half wave on the same SIMD) runs one tile behind in its epilogue:
  // per tile it finishes tile nt - 1's argmax first, then issues tile nt's
  // MFMAs, while the first half issues tile nt's MFMAs and then its epilogue.
  // The barrier keeps all waves on one tile; the skew puts one wave's epilogue
  // VALU beside its partner's MFMAs instead of both SIMD waves alternating
  // all-MFMA and all-VALU phases in step.
  // lagging: waves 4-7, one of the two waves of each SIMD
  const bool lag = (__builtin_amdgcn_readfirstlane(wv) >> 2) & 1;
  // The bias is the MFMAs' initial C operand (one ds_read_b128 of the
  // replicated bias per column tile), so the epilogue is compare + select.
  f32x4 acc[kOutRF][kOutCF];
  // (FULL: every column of the tile is < V -- all tiles but a ragged last
  // one -- so the per-lane bound check and its exec-mask blocks go)
  auto epilogue_t = [&](int tile, auto full) __attribute__((always_inline)) {
    // column v = 64 tile + 16 cf + li, rows row0 + 16 rf + 4 lg + i
#pragma unroll
    for (int cf = 0; cf < kOutCF; ++cf) {
      const int v = tile * kOutBN + 16 * cf + li;
      if (KEYED) {
        const unsigned tag = 255u - (unsigned)(kOutCF * tile + cf);
        if (LOGITS) {
#pragma unroll
          for (int rf = 0; rf < kOutRF; ++rf)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int64_t r = row0 + 16 * rf + 4 * lg + i;
              if ((decltype(full)::value || v < V) && r < rows) logits[r * V + v] = __float2half(acc[rf][cf][i]);
            }
        }
        static_assert(kOutCF == 4, "the epilogue folds the tile's four column blocks at once");
        if (cf == kOutCF - 1) {   // all four column blocks: four tagged values per two v_max3_f32
#pragma unroll
          for (int rf = 0; rf < kOutRF; ++rf)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float x[4];
#pragma unroll
              for (int c = 0; c < 4; ++c) {   // (-FLT_MAX past V: tagged -inf would be a NaN)
                x[c] = acc[rf][c][i];
                if (!decltype(full)::value) x[c] = tile * kOutBN + 16 * c + li < V ? x[c] : -FLT_MAX;
              }
              const float t0 = out_tag(x[0], kmask, tag + 3), t1 = out_tag(x[1], kmask, tag + 2);
              const float t2 = out_tag(x[2], kmask, tag + 1), t3 = out_tag(x[3], kmask, tag);
              const float m = mx[rf][i], a = out_med3(m, t0, t1), m1 = out_max3(m, t0, t1);
              const float b = out_med3(m1, t2, t3);
              mx[rf][i] = out_max3(m1, t2, t3);
              mx2[rf][i] = out_max3(mx2[rf][i], a, b);
            }
        }
      } else if (decltype(full)::value || v < V) {
#pragma unroll
        for (int rf = 0; rf < kOutRF; ++rf)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float z = acc[rf][cf][i];
            if (z > mx[rf][i]) { mx[rf][i] = z; ix[rf][i] = v; }
            if (LOGITS) {
              const int64_t r = row0 + 16 * rf + 4 * lg + i;
              if (r < rows) logits[r * V + v] = __float2half(acc[rf][cf][i]);
            }
          }
      }
    }
  };
  auto epilogue = [&](int tile) __attribute__((always_inline)) {
    if ((tile + 1) * kOutBN <= V) epilogue_t(tile, std::true_type{});
    else epilogue_t(tile, std::false_type{});
  };
  for (int nt = 0; nt < NT; ++nt) {
    if (nt + kOutAhead < NT) fetch(nt + kOutAhead);
    const _Float16* b = bt[nt & (kOutNB - 1)];
    if (lag && nt > 0) epilogue(nt - 1);
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      h8 bf[kOutCF];
#pragma unroll
      for (int cf = 0; cf < kOutCF; ++cf)
        bf[cf] = *reinterpret_cast<const h8*>(b + (16 * cf + li) * kOutPitch + 8 * out_chunk(li, 4 * st + lg));
      if (st == 0) {
#pragma unroll
        for (int cf = 0; cf < kOutCF; ++cf) {
          const f32x4 c0 = bsh[nt & (kOutNB - 1)][16 * cf + li];
#pragma unroll
          for (int rf = 0; rf < kOutRF; ++rf)
            acc[rf][cf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[rf][0], bf[cf], c0, 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int rf = 0; rf < kOutRF; ++rf)
#pragma unroll
          for (int cf = 0; cf < kOutCF; ++cf)
            acc[rf][cf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[rf][st], bf[cf], acc[rf][cf], 0, 0, 0);
      }
    }
    if (!lag && nt + kOutAhead < NT) {   // after this wave's last LDS read of the period
      stash((nt + kOutAhead) & (kOutNB - 1));
      dma_w(nt + kOutAhead);
    }
    if (!lag) epilogue(nt);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // LDS-DMA done (the barrier's own wait omits it)
    __syncthreads();
  }
  if (lag && NT > 0) epilogue(NT - 1);
  // first maximum across the 16 column lanes of each row
#pragma unroll
  for (int rf = 0; rf < kOutRF; ++rf)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float m = mx[rf][i], m2 = mx2[rf][i];   // (m2: KEYED runner-up)
      out_row_reduce<KEYED>(m, KEYED ? 16 * out_untag(m) + li : ix[rf][i], m2, KEYED ? 16 * out_untag(m2) + li : -1, li,
                            row0 + 16 * rf + 4 * lg + i, rows, best, best2);
    }
}

// Decode-only form of the kernel above (KEYED, no logits: wk_ctc_transcribe's
// path), with the epilogue moved in among the MFMAs.  A tile's four
// column blocks are computed in two halves (blocks 0-1, then 2-3); each half's
// 48 MFMAs carry the fold of the OTHER half's finished accumulators (blocks
// 2-3 of the previous tile, then blocks 0-1 of this one), one item per k-step
// with a sched_barrier after each, so the fold's VALU goes into the cycles a
// v_mfma_f32_16x16x32_f16 leaves (8 of its 16) with no second accumulator set.
// Both waves of a SIMD run the same schedule (no skew).  The next tile's W
// goes into the other LDS buffer by DMA at the start of the period (separate
// arrays: the compiler sees they cannot alias, so no read waits for it).
// Columns past V get bias -1e30 and read W rows of 0, so no tile needs a
// bound check; the first tile's dummy fold reads accumulators preset to -1e30.
// Tokens are the same as ctc_out_argmax16_kernel<false, true>'s (same
// accumulation order per logit, same tags; the folds take exact max/median).
__global__ __launch_bounds__(kOutWaves * 64) void ctc_out_decode16_kernel(const __half* __restrict__ y,
                                                                          const __half* __restrict__ w,
                                                                          const float* __restrict__ bias, int64_t rows,
                                                                          int V, int* __restrict__ best,
                                                                          int* __restrict__ best2) {
  constexpr int RF = kOutRF, kRows = 16 * RF * kOutWaves;
  // Two separate W buffers (and bias buffers), selected at compile time: the
  // compiler then knows the LDS-DMA into one cannot alias the B-fragment reads
  // of the other, so a period can start the next tile's DMA and still read its
  // own tile without waiting for it (with one array it waits at the first read).
  __shared__ __attribute__((aligned(1024))) _Float16 bt0[kOutBN * kOutPitch];
  __shared__ __attribute__((aligned(1024))) _Float16 bt1[kOutBN * kOutPitch];
  __shared__ f32x4 bsh0[kOutBN], bsh1[kOutBN];   // the tile's bias x4 (an MFMA C operand)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wvu = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kRows + 16 * RF * wvu;
  h8 a[RF][8];
  out_load_a<RF>(a, y, row0, rows, li, lg);
  const int NT = (V + kOutBN - 1) / kOutBN;
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(w, (uint32_t)V * kOutK * 2);
  const __amdgpu_buffer_rsrc_t brs = make_rsrc(bias, (uint32_t)V * 4);
  // W tiles by LDS-DMA (as above), 4 pieces per wave, all 8 waves
  constexpr int kDmaPer = kOutBN * kOutK * 2 / 1024 / kOutWaves;
  int dma_off[kDmaPer];
  out_dma_offsets<kOutWaves>(dma_off, wvu, lane);
  auto dma_w = [&](_Float16* dst, int nt) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < kDmaPer; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)&dst[(wvu * kDmaPer + i) * 512],
                                               16, dma_off[i], nt * (kOutBN * kOutK * 2), 0, 0);
  };
  float pb = 0.0f;
  auto fetch = [&](int nt) {   // wave 0: the tile's bias (used at stash: no wait here)
    if (wvu == 0) pb = buf_load(brs, 4 * (nt * kOutBN + lane), 0);
  };
  auto stash = [&](f32x4* dst, int nt) {   // -1e30 past V
    const float v = nt * kOutBN + lane < V ? pb : -1e30f;
    if (wvu == 0) dst[lane] = f32x4{v, v, v, v};
  };
  fetch(0);
  stash(bsh0, 0);
  dma_w(bt0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  float mx[RF][4], mx2[RF][4];
  f32x4 acc[RF][kOutCF];
#pragma unroll
  for (int rf = 0; rf < RF; ++rf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { mx[rf][i] = -INFINITY; mx2[rf][i] = -INFINITY; }
#pragma unroll
    for (int cf = 2; cf < kOutCF; ++cf) acc[rf][cf] = f32x4{-1e30f, -1e30f, -1e30f, -1e30f};   // the first dummy fold
  }
  unsigned kmask;   // out_tag's mask, in a VGPR (VOP3 takes no literal)
  asm("v_mov_b32 %0, 0xffffff00" : "=v"(kmask));
  float carry[RF][4];   // a tile's blocks 0-1 median, folded with its blocks 2-3 (the runner-up, 4 values at once)
#pragma unroll
  for (int rf = 0; rf < RF; ++rf)
#pragma unroll
    for (int i = 0; i < 4; ++i) carry[rf][i] = -INFINITY;
  // One half: blocks 2h and 2h + 1 of the tile in (b, bs) (16 steps of one B
  // fragment x RF MFMAs; fragments read two steps ahead), with the fold of
  // blocks 2eh, 2eh + 1 of tile etile (12 items of 5 VALU) spread one item per
  // step; a sched_barrier after each step keeps that order.
  auto half = [&](const _Float16* b, const f32x4* bs, int h, int etile, int eh) __attribute__((always_inline)) {
    auto frag = [&](int s) -> h8 {
      const int cf = 2 * h + (s >> 3), st = s & 7;
      return *reinterpret_cast<const h8*>(b + (16 * cf + li) * kOutPitch + 8 * out_chunk(li, 4 * st + lg));
    };
    const unsigned tag = 255u - (unsigned)(kOutCF * etile + 2 * eh);   // block 2eh; block 2eh + 1: tag - 1
    constexpr int PD = 4;   // fragment prefetch distance in steps (2: +1.5 % time; profiles/r05p_dec16_variants_ab.txt)
    f32x4 c0 = bs[16 * (2 * h) + li];
    h8 ring[PD + 1];
#pragma unroll
    for (int q = 0; q < PD; ++q) ring[q] = frag(q);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int cf = 2 * h + (s >> 3), st = s & 7;
      if (s + PD < 16) ring[(s + PD) % (PD + 1)] = frag(s + PD);
      if (s == 8) c0 = bs[16 * cf + li];
      const h8 bf = ring[s % (PD + 1)];
#pragma unroll
      for (int rf = 0; rf < RF; ++rf)
        acc[rf][cf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[rf][st], bf, st == 0 ? c0 : acc[rf][cf], 0, 0, 0);
      if (s < RF * 4) {   // fold item s: row block rf, row i
        const int rf = s >> 2, i = s & 3;
        const float t0 = out_tag(acc[rf][2 * eh][i], kmask, tag), t1 = out_tag(acc[rf][2 * eh + 1][i], kmask, tag - 1);
        const float m = mx[rf][i];
        if (eh == 0) {   // one runner-up update per tile: blocks 0-1's median waits for blocks 2-3's (-1 VALU / 4 logits)
          carry[rf][i] = out_med3(m, t0, t1);
        } else {
          mx2[rf][i] = out_max3(mx2[rf][i], carry[rf][i], out_med3(m, t0, t1));
        }
        mx[rf][i] = out_max3(m, t0, t1);
      }
      __builtin_amdgcn_sched_barrier(0);   // (without: the compiler clusters the fold, +1.5-3 % time)
    }
  };
  // One period: tile nt from (b, bs); the next tile's W and bias go into (nb, nbs)
  // at its start (the other buffers were last read in the previous period).
  auto period = [&](const _Float16* b, const f32x4* bs, _Float16* nb, f32x4* nbs, int nt) __attribute__((always_inline)) {
    const bool more = nt + 1 < NT;
    if (more) {   // (the pieces spread among the MFMAs, one per 4 steps, or s_setprio 1 for waves 4-7: within +-1 %)
      fetch(nt + 1);
      dma_w(nb, nt + 1);
    }
    half(b, bs, 0, nt > 0 ? nt - 1 : 0, 1);   // blocks 0-1 || fold of the previous tile's blocks 2-3
    half(b, bs, 1, nt, 0);                    // blocks 2-3 || fold of this tile's blocks 0-1
    if (more) stash(nbs, nt + 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // LDS-DMA done (the barrier's own wait omits it)
    __syncthreads();
  };
  for (int nt = 0; nt < NT; nt += 2) {
    period(bt0, bsh0, bt1, bsh1, nt);
    if (nt + 1 < NT) period(bt1, bsh1, bt0, bsh0, nt + 1);
  }
  {   // the last tile's blocks 2-3
    const unsigned tag = 255u - (unsigned)(kOutCF * (NT - 1) + 2);
#pragma unroll
    for (int rf = 0; rf < RF; ++rf)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float t0 = out_tag(acc[rf][2][i], kmask, tag), t1 = out_tag(acc[rf][3][i], kmask, tag - 1);
        const float m = mx[rf][i];
        mx2[rf][i] = out_max3(mx2[rf][i], carry[rf][i], out_med3(m, t0, t1));
        mx[rf][i] = out_max3(m, t0, t1);
      }
  }
  // first maximum across the 16 column lanes of each row
#pragma unroll
  for (int rf = 0; rf < RF; ++rf)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float m = mx[rf][i], m2 = mx2[rf][i];
      out_row_reduce<true>(m, 16 * out_untag(m) + li, m2, 16 * out_untag(m2) + li, li, row0 + 16 * rf + 4 * lg + i, rows, best,
                           best2);
    }
}

// Near-tie re-scoring after the fp16 output kernels (V <= 4096): a row whose
// top-2 logits came within out_near_tie of each other is decided between those
// two columns again with fp32 weights (y is the fp16 GRU output, widened
// exactly): bias + sum_k y[k] W[c][k] in fp32, the larger wins, an exact tie
// keeps the smaller column (torch.argmax).  Rows with best2 < 0 keep their fp16
// decision.  A wave takes 64 consecutive rows, finds the flagged ones with a
// ballot and re-scores them one at a time with all 64 lanes (4 k per lane, a
// shuffle-tree sum): the flagged rows are a few percent, and one thread per row
// walking a 256-long dependent FMA chain had cost ~0.11 ms per batch.
__global__ __launch_bounds__(256) void ctc_rescore_kernel(const __half* __restrict__ y, const float* __restrict__ w,
                                                          const float* __restrict__ bias, int64_t rows,
                                                          int* __restrict__ best, const int* __restrict__ best2) {
  const int lane = threadIdx.x & 63;
  const int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
  if (base >= rows) return;   // (wave-uniform)
  const int64_t r = base + lane;
  const int c2l = r < rows ? best2[r] : -1;
  uint64_t mask = __ballot(c2l >= 0);
  while (mask) {   // (wave-uniform)
    const int j = __builtin_ctzll(mask);
    mask &= mask - 1;
    const int64_t rj = base + j;
    const int c2 = __shfl(c2l, j, 64), c1 = best[rj];
    const __half2* yr = reinterpret_cast<const __half2*>(y + rj * (2 * kH)) + 2 * lane;
    const float4 w1 = reinterpret_cast<const float4*>(w + (int64_t)c1 * (2 * kH))[lane];
    const float4 w2 = reinterpret_cast<const float4*>(w + (int64_t)c2 * (2 * kH))[lane];
    const float2 ya = __half22float2(yr[0]), yb = __half22float2(yr[1]);
    float s1 = __builtin_fmaf(ya.x, w1.x, __builtin_fmaf(ya.y, w1.y, __builtin_fmaf(yb.x, w1.z, yb.y * w1.w)));
    float s2 = __builtin_fmaf(ya.x, w2.x, __builtin_fmaf(ya.y, w2.y, __builtin_fmaf(yb.x, w2.z, yb.y * w2.w)));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o, 64);
      s2 += __shfl_xor(s2, o, 64);
    }
    s1 += bias[c1];
    s2 += bias[c2];
    if (lane == 0 && (s2 > s1 || (s2 == s1 && c2 < c1))) best[rj] = c2;
  }
}

}  // namespace

namespace wk {

void launch_ctc_argmax(bool f16, const void* logits, const float* bias, int64_t rows, int V, float* log_probs, int* best,
                       int tm_B, int T, hipStream_t st) {
  const dim3 g((unsigned)((rows + 3) / 4));
  if (f16)
    hipLaunchKernelGGL(ctc_argmax_kernel<__half>, g, dim3(256), 0, st, (const __half*)logits, bias, rows, V, log_probs, best,
                       tm_B, T);
  else
    hipLaunchKernelGGL(ctc_argmax_kernel<float>, g, dim3(256), 0, st, (const float*)logits, bias, rows, V, log_probs, best,
                       tm_B, T);
}

void launch_ctc_out16(const __half* y, const __half* w16, const float* bias, int64_t rows, int V, __half* logits, int* best,
                      int* best2, bool fold, hipStream_t st) {
  const bool keyed = ctc_out_keyed(V);
  const int br = out_rows(logits != nullptr);
  const dim3 og((unsigned)((rows + br - 1) / br)), blk(kOutWaves * 64);
  if (logits)
    hipLaunchKernelGGL((keyed ? ctc_out_argmax16_kernel<true, true> : ctc_out_argmax16_kernel<true, false>), og, blk, 0, st, y,
                       w16, bias, rows, V, logits, best, best2);
  else if (keyed && fold)   // the decode-only kernel, the fold among the MFMAs
    hipLaunchKernelGGL(ctc_out_decode16_kernel, og, blk, 0, st, y, w16, bias, rows, V, best, best2);
  else
    hipLaunchKernelGGL((keyed ? ctc_out_argmax16_kernel<false, true> : ctc_out_argmax16_kernel<false, false>), og, blk, 0, st,
                       y, w16, bias, rows, V, (__half*)nullptr, best, best2);
}

void launch_ctc_rescore(const __half* y, const float* w, const float* bias, int64_t rows, int* best, const int* best2,
                        hipStream_t st) {
  hipLaunchKernelGGL(ctc_rescore_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, y, w, bias, rows, best, best2);
}

void launch_ctc_greedy(const int* best, int64_t B, int T, int* tokens, int* lengths, int tm, hipStream_t st) {
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, best, B, T, tokens, lengths, tm);
}

void launch_ctc_pred(const int* best, int64_t B, int T, int tm, int* pred, hipStream_t st) {
  hipLaunchKernelGGL(ctc_pred_kernel, dim3((unsigned)((B * (int64_t)T + 255) / 256)), dim3(256), 0, st, best, B, T, tm, pred);
}

}  // namespace wk
