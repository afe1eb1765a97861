// wk_ctc_cer.hip -- batched edit distance between hypotheses and references
// with its split into substitutions, deletions and insertions, the oracle
// hypothesis of an N-best list and the corpus totals an error rate is made of.
//
// Pair (b, h) compares hypothesis h of utterance b (N tokens) with reference b
// (M tokens).  D[i][j] is the cheapest alignment of the first i hypothesis
// tokens with the first j reference tokens under additive costs: match 0,
// insertion (a hypothesis token alone) and deletion (a reference token alone)
// 2^16, substitution 2^16 + 1.  D[N][M] = d * 2^16 + s: the Levenshtein
// distance and the fewest substitutions among the alignments that reach it;
// ins - del = N - M gives the rest.  All of it is integer, so every output is
// defined bit for bit, whatever the lane layout.
//
// Two launches on the caller's stream, no host synchronisation, no atomics,
// no floating point:
//   pairs   one wave per pair, the hypotheses of one utterance adjacent in the
//           grid so that they share its reference in L2.  The reference sits in
//           registers, lane l holding columns l C + 1 .. l C + C (C = 1, 2, 4,
//           8 or 16 by max_ref_len, a template parameter: no dynamic register
//           indexing), and the wave walks the hypothesis one token per row.
//           The row is kept as w_j = D[i][j] - j DEL, in which the deletion
//           chain D[i][j] = min(tmp_j, D[i][j-1] + DEL) is a prefix minimum:
//             tmp_j = min(w'_j + INS, w'_{j-1} + (r_j == h_i ? -DEL : SUB - DEL))
//             w_j   = min_{k <= j} tmp_k
//           (w' the row before; column 0, i INS, never wins the chain: D[i-1][1]
//           <= D[i-1][0] + DEL makes tmp_1 <= D[i][0] + DEL).  That is an
//           in-lane scan over C values and one wave-wide exclusive prefix-min:
//           DPP row shifts inside each row of 16 lanes, the three row ends
//           through v_readlane.  w'_{j-1} of a lane's first column comes from
//           one DPP wave shift whose fill-in for lane 0 is column 0.
//           Hypothesis words are loaded 64 per lane-wide load, the next chunk
//           in flight, and handed out with v_readlane in the order of the set
//           bits of a keep mask: the lanes below the length, or with `collapse`
//           the ballot of label != 0 && label != the label before (the last
//           label carried across chunks), so the collapsed hypothesis is never
//           stored.  Columns beyond M compute values nobody reads: a column
//           only feeds higher ones.
//   reduce  one block: per utterance the oracle hypothesis, the smallest
//           (d, s, h); the two totals rows as int64 sums, combined by a fixed
//           tree (integer sums: any order gives the same bits).
// The workspace holds (N, M) per pair and nothing proportional to
// hyp_stride * max_ref_len: no DP matrix, no back-pointers.
#include "wakeword.h"
#include "wk_ctc_lattice_dev.h"

namespace wk {
namespace {

constexpr int kCerMaxHypStride = 32767;      // d <= 32767: d * 2^16 + s is a positive int32
constexpr int kCerMaxRefLen = 1024;          // 64 lanes x 16 columns
constexpr int kCerMaxHyp = 64;
constexpr int64_t kCerMaxPairs = (int64_t)1 << 24;     // batch * n_hyp
constexpr int64_t kCerMaxWords = (int64_t)1 << 30;     // batch * n_hyp * hyp_stride
constexpr int kCerIns = 1 << 16, kCerDel = 1 << 16, kCerSub = (1 << 16) + 1;
constexpr int kCerInf = 0x7FFFFFFF;
constexpr int kCerReduceBlock = 1024;

bool cer_shape_ok(int64_t batch, int32_t n_hyp, int32_t hyp_stride, int32_t max_ref_len) {
  return batch > 0 && n_hyp >= 1 && n_hyp <= kCerMaxHyp && hyp_stride >= 1 && hyp_stride <= kCerMaxHypStride &&
         max_ref_len >= 1 && max_ref_len <= kCerMaxRefLen && batch <= kCerMaxPairs && batch * n_hyp <= kCerMaxPairs &&
         batch * n_hyp * hyp_stride <= kCerMaxWords;
}

int64_t cer_bytes(int64_t batch, int32_t n_hyp) {       // (N, M) [batch][n_hyp]
  return round_up_256(8 * batch * n_hyp);
}

// v of the lane `n` below in the same row of 16 lanes (row_shr:n); kCerInf where there is none.
template <int N> __device__ __forceinline__ int min_row_shr(int v) {
  return min(v, __builtin_amdgcn_update_dpp(kCerInf, v, 0x110 + N, 0xF, 0xF, false));
}

// min over the lanes below this one (kCerInf in lane 0).  All 64 lanes active.
__device__ __forceinline__ int wave_prefix_min_excl(int m, int lane) {
  int v = prev_lane(kCerInf, m);
  v = min_row_shr<1>(v);
  v = min_row_shr<2>(v);
  v = min_row_shr<4>(v);
  v = min_row_shr<8>(v);                       // inclusive inside each row of 16
  const int e0 = __builtin_amdgcn_readlane(v, 15);
  const int e1 = min(e0, __builtin_amdgcn_readlane(v, 31));
  const int e2 = min(e1, __builtin_amdgcn_readlane(v, 47));
  const int row = lane >> 4;
  const int below = row == 0 ? kCerInf : row == 1 ? e0 : row == 2 ? e1 : e2;
  return min(v, below);
}

template <int C>
__global__ __launch_bounds__(64) void ctc_cer_pairs_kernel(const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len,
                                                           int n_hyp, int hyp_stride, const int32_t* __restrict__ ref,
                                                           int ref_stride, const int32_t* __restrict__ ref_len, int max_ref_len,
                                                           int collapse, int32_t* __restrict__ nm, int32_t* __restrict__ stats) {
  const int lane = threadIdx.x;
  const int64_t pair = blockIdx.x;                 // b * n_hyp + h: one utterance's hypotheses are adjacent
  const int64_t b = blockIdx.x / (unsigned)n_hyp;  // (pairs <= 2^24: a 32-bit divide)
  const int M = __builtin_amdgcn_readfirstlane(min(max(ref_len[b], 0), max_ref_len));
  const int len = __builtin_amdgcn_readfirstlane(hyp_len ? min(max(hyp_len[pair], 0), hyp_stride) : hyp_stride);

  // lane l's reference tokens r_{l C + 1 + q}, q < C (0 beyond M: those columns are never read)
  const int32_t* r = ref + b * ref_stride;
  int rt[C], w[C];
#pragma unroll
  for (int q = 0; q < C; ++q) {
    const int j = lane * C + q;
    rt[q] = j < M ? r[j] : 0;
    w[q] = 0;                                      // row 0: D[0][j] = j DEL
  }

  const int32_t* hp = hyp + pair * hyp_stride;
  int N = 0;                                       // rows done = tokens of the hypothesis so far
  int carry = 0;                                   // collapse: the label of the frame before this chunk
  int next = lane < len ? hp[lane] : 0;
  for (int t0 = 0; t0 < len; t0 += 64) {
    int cur = next;
    asm volatile("" : "+v"(cur));                  // this chunk has arrived before the next one's load is issued, so that
    const int tn = t0 + 64 + lane;                 // load alone is in flight during the rows and nothing waits for it
    next = tn < len ? hp[tn] : 0;
    uint64_t keep;
    if (collapse) {
      const int before = prev_lane(carry, cur);    // (lane 0: the carry)
      keep = __ballot(t0 + lane < len && cur != 0 && cur != before);
      carry = __builtin_amdgcn_readlane(cur, 63);  // (only read when a next chunk exists: this one was full)
    } else {
      keep = __ballot(t0 + lane < len);
    }
    while (keep) {                                 // (wave-uniform)
      const int src = __builtin_ctzll(keep);
      keep &= keep - 1;
      const int h = __builtin_amdgcn_readlane(cur, src);
      // D[i-1][l C] - (l C) DEL for the lane's first column; lane 0: column 0 of the row before, N INS
      const int left = prev_lane(N * kCerIns, w[C - 1]);
      int p[C];
#pragma unroll
      for (int q = 0; q < C; ++q) {
        const int diag = (q == 0 ? left : w[q - 1]) + (rt[q] == h ? -kCerDel : kCerSub - kCerDel);
        const int tmp = min(w[q] + kCerIns, diag);
        p[q] = q == 0 ? tmp : min(p[q - 1], tmp);
      }
      const int below = wave_prefix_min_excl(p[C - 1], lane);
#pragma unroll
      for (int q = 0; q < C; ++q) w[q] = min(p[q], below);
      ++N;
    }
  }

  // D[N][M]: column M is lane (M - 1) / C, register (M - 1) % C; M = 0 is column 0
  int key = N * kCerIns;
  if (M > 0) {
    const int q_m = (M - 1) % C;
    int v = w[0];
#pragma unroll
    for (int q = 1; q < C; ++q) v = q == q_m ? w[q] : v;
    key = __builtin_amdgcn_readlane(v, (M - 1) / C) + M * kCerDel;
  }
  if (lane == 0) {
    const int d = key >> 16, s = key & 0xFFFF;
    const int del = (d - s - (N - M)) / 2;         // d = s + del + ins, ins - del = N - M
    stats[4 * pair] = d;
    stats[4 * pair + 1] = s;
    stats[4 * pair + 2] = del;
    stats[4 * pair + 3] = d - s - del;
    nm[2 * pair] = N;
    nm[2 * pair + 1] = M;
  }
}

// d_best and d_totals from the pairs' stats.  One block; thread i takes
// utterances i, i + blockDim, ...; the sums are integers, so the tree's order
// does not show in the result.
__global__ __launch_bounds__(kCerReduceBlock) void ctc_cer_reduce_kernel(const int32_t* __restrict__ stats,
                                                                         const int32_t* __restrict__ nm, int64_t batch, int n_hyp,
                                                                         int32_t* __restrict__ best, int64_t* __restrict__ totals) {
  __shared__ int64_t part[kCerReduceBlock];
  int64_t acc[2][7] = {};
  for (int64_t b = threadIdx.x; b < batch; b += kCerReduceBlock) {
    const int32_t* st = stats + 4 * b * n_hyp;
    int best_h = 0, best_key = (st[0] << 16) | st[1];
    for (int h = 1; h < n_hyp; ++h) {
      const int key = (st[4 * h] << 16) | st[4 * h + 1];
      if (key < best_key) best_key = key, best_h = h;        // strictly smaller: ties keep the lower index
    }
    if (best) best[b] = best_h;
    for (int row = 0; row < 2; ++row) {
      const int h = row ? best_h : 0;
      for (int k = 0; k < 4; ++k) acc[row][k] += st[4 * h + k];
      acc[row][4] += nm[2 * (b * n_hyp + h) + 1];
      acc[row][5] += nm[2 * (b * n_hyp + h)];
      acc[row][6] += st[4 * h] > 0;
    }
  }
  if (!totals) return;                             // (uniform)
  for (int row = 0; row < 2; ++row)
    for (int k = 0; k < 7; ++k) {
      __syncthreads();
      part[threadIdx.x] = acc[row][k];
      __syncthreads();
      for (int n = kCerReduceBlock / 2; n > 0; n >>= 1) {
        if ((int)threadIdx.x < n) part[threadIdx.x] += part[threadIdx.x + n];
        __syncthreads();
      }
      if (threadIdx.x == 0) totals[8 * row + k] = part[0];
    }
  if (threadIdx.x == 0) totals[7] = totals[15] = batch;
}

}  // namespace
}  // namespace wk

using wk::invalid;

extern "C" {

int64_t wk_ctc_cer_workspace_bytes(int64_t batch, int32_t n_hyp, int32_t hyp_stride, int32_t max_ref_len) {
  if (!wk::cer_shape_ok(batch, n_hyp, hyp_stride, max_ref_len)) return 0;
  return wk::cer_bytes(batch, n_hyp);
}

wk_status wk_ctc_cer(const int32_t* d_hyp, const int32_t* d_hyp_lengths_or_null, int64_t batch, int32_t n_hyp,
                     int32_t hyp_stride, const int32_t* d_ref, int32_t ref_stride, const int32_t* d_ref_lengths,
                     int32_t max_ref_len, int32_t collapse, void* d_workspace, int32_t* d_stats,
                     int32_t* d_best_or_null, int64_t* d_totals_or_null, int32_t device, void* stream) {
  if (!d_hyp || !d_ref || !d_ref_lengths || !d_workspace || !d_stats) return invalid("wk_ctc_cer: null pointer");
  if (!collapse && !d_hyp_lengths_or_null) return invalid("wk_ctc_cer: d_hyp_lengths is required unless collapse is set");
  if (batch <= 0 || n_hyp <= 0 || hyp_stride <= 0 || max_ref_len <= 0)
    return invalid("wk_ctc_cer: batch, n_hyp, hyp_stride and max_ref_len must be positive");
  if (hyp_stride > wk::kCerMaxHypStride) return invalid("wk_ctc_cer: hyp_stride > 32767");
  if (max_ref_len > wk::kCerMaxRefLen) return invalid("wk_ctc_cer: max_ref_len > 1024");
  if (ref_stride < max_ref_len) return invalid("wk_ctc_cer: ref_stride < max_ref_len");
  if (n_hyp > wk::kCerMaxHyp) return invalid("wk_ctc_cer: n_hyp > 64");
  if (batch > wk::kCerMaxPairs || batch * n_hyp > wk::kCerMaxPairs) return invalid("wk_ctc_cer: batch * n_hyp > 2^24");
  if (batch * n_hyp * hyp_stride > wk::kCerMaxWords) return invalid("wk_ctc_cer: batch * n_hyp * hyp_stride > 2^30");
  if ((uintptr_t)d_workspace & 15) return invalid("wk_ctc_cer: d_workspace must be 16-byte aligned");
  if (device < 0) return invalid("wk_ctc_cer: device < 0");
  int32_t* nm = (int32_t*)d_workspace;
  hipStream_t st = (hipStream_t)stream;
  return wk::on_device(device, [&]() -> wk_status {
    const dim3 grid((unsigned)(batch * n_hyp));
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(64), 0, st, d_hyp, d_hyp_lengths_or_null, n_hyp, hyp_stride, d_ref, ref_stride,
                         d_ref_lengths, max_ref_len, collapse, nm, d_stats);
    };
    if (max_ref_len <= 64) launch(wk::ctc_cer_pairs_kernel<1>);
    else if (max_ref_len <= 128) launch(wk::ctc_cer_pairs_kernel<2>);
    else if (max_ref_len <= 256) launch(wk::ctc_cer_pairs_kernel<4>);
    else if (max_ref_len <= 512) launch(wk::ctc_cer_pairs_kernel<8>);
    else launch(wk::ctc_cer_pairs_kernel<16>);
    if (d_best_or_null || d_totals_or_null)
      hipLaunchKernelGGL(wk::ctc_cer_reduce_kernel, dim3(1), dim3(wk::kCerReduceBlock), 0, st, (const int32_t*)d_stats,
                         (const int32_t*)nm, batch, n_hyp, d_best_or_null, d_totals_or_null);
    return wk::ctc_launched("wk_ctc_cer");
  });
}

}  // extern "C"
