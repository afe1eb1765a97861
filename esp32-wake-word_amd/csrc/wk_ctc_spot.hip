// wk_ctc_spot.hip -- CTC keyword spotting: for every (utterance, keyword) pair
// the best score of the keyword over all segments of the utterance, the
// segment, and optionally the per-frame trace, from [B][T][V] fp32 log-probs,
// blank = 0.
//
// Keyword w_0..w_{S-1} has L = 2S-1 states, even j emitting w_{j/2}, odd j the
// blank (no outer blanks: a span is tight).  With x_t(j) = lp_t(l_j), or
// lp_t(l_j) - max_v lp_t(v) with `normalize` (-inf stays -inf),
//   a_{-1}(j) = -inf
//   a_t(0) = x_t(0) + max(a_{t-1}(0), 0)            the keyword may start at any frame
//   a_t(j) = x_t(j) + max(a_{t-1}(j), a_{t-1}(j-1), [a_{t-1}(j-2)])
// (third term: j even, j >= 2, w_{j/2} != w_{j/2-1}), e_t = a_t(L-1), score =
// max_{t < Tb} e_t at the first frame that attains it.  Every state carries the
// frame at which its path entered state 0 (-1 while its value is -inf).  Ties:
// stay, then j-1, then j-2 (at state 0: stay, then enter); a candidate replaces
// the best only if strictly greater.  max is exact and every add or subtract
// rounds once, so the result is defined bit for bit, whatever the lane layout.
//
// Two launches on the caller's stream (one without `normalize`), no host
// synchronisation, no atomics:
//   rowmax   a wave per frame t < Tb: 16-byte loads (RowSplit,
//            wk_ctc_lattice_dev.h), a DPP reduction (wave_max), g[b][t];
//   recur    one wave per (utterance, keyword), the keywords of one utterance
//            adjacent in the grid so that they share its rows in L2.  Lane j
//            holds state j and its carried start frame; the values of states
//            j-1 and j-2 come from one and two DPP wave shifts, whose fill-in
//            for lane 0 is the entry (value 0, start t).  Nothing is gathered
//            to memory: lane j reads lp[b][t][l_j] straight from the row, and
//            as the addresses do not depend on the recurrence a group of
//            kSpotGroup rows is in flight.  g_t is read 64 frames per load (one
//            per lane) and handed out with v_readlane.  The running (best,
//            start, end) stays in each lane's registers -- lane L-1's is the
//            result, written once.  e_t is collected in LDS, one store per
//            step that nothing waits for, and goes out as one coalesced row
//            per kSpotTrace frames.
//            States j >= L compute values nobody reads: a state only feeds
//            higher ones.
#include <math.h>

#include "wakeword.h"
#include "wk_ctc_lattice_dev.h"

namespace wk {
namespace {

constexpr int kSpotMaxLen = 32;              // L = 63 states: one lane each
constexpr int64_t kSpotMaxPairs = (int64_t)1 << 24;    // batch * n_keywords
constexpr int kSpotGroup = 16;               // rows in flight per wave
constexpr int kSpotTrace = 64;               // frames per stored trace row (and per g load): one per lane

int64_t ctc_spot_bytes(int64_t batch, int32_t T) {      // g [batch][T]
  return round_up_256(4 * batch * T);
}

// ---- row maximum --------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_spot_rowmax_kernel(const float* __restrict__ lp, const int32_t* __restrict__ in_len,
                                                              int64_t rows, int T, int V, float* __restrict__ g) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= rows) return;                                   // (wave-uniform)
  const int b = (int)(row / T), t = (int)(row % T);
  const int Tb = in_len ? min(max(in_len[b], 0), T) : T;
  if (t >= Tb) return;
  const float* p = lp + row * V;
  const RowSplit r = row_split(p, V);
  float m = lane < r.head ? p[lane] : neg_inf();
#pragma unroll 4
  for (int q = lane; q < r.nq; q += 64) {
    const float4 v = r.q4[q];
    m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
  }
  if (r.tail0 + lane < V) m = fmaxf(m, p[r.tail0 + lane]);
  m = wave_max(m);
  if (lane == 0) g[row] = m;
}

// ---- recurrence ---------------------------------------------------------------------
template <bool NORM, bool TRACE>
__global__ __launch_bounds__(64) void ctc_spot_recur_kernel(const float* __restrict__ lp, const int32_t* __restrict__ in_len,
                                                            const int32_t* __restrict__ kw, int kw_stride,
                                                            const int32_t* __restrict__ kw_len, int T, int V, int K, int max_len,
                                                            const float* __restrict__ g, float* __restrict__ scores,
                                                            int32_t* __restrict__ spans, float* __restrict__ trace) {
  constexpr int PF = kSpotGroup;
  const int lane = threadIdx.x;
  const int64_t pair = blockIdx.x;                 // b * K + k: one utterance's keywords are adjacent
  const int b = (int)(pair / K), k = (int)(pair % K);
  const int Tb = __builtin_amdgcn_readfirstlane(in_len ? min(max(in_len[b], 0), T) : T);
  const int S = __builtin_amdgcn_readfirstlane(min(max(kw_len[k], 0), max_len));
  const int L = 2 * S - 1;

  // lane j's column l_j and whether state j may be entered from j-2
  const int32_t* w = kw + (int64_t)k * kw_stride;
  const int i = lane >> 1;
  int col = 0;
  bool bad = false, skip = false;
  if (!(lane & 1) && i < S) {
    const int v = w[i];
    bad = v < 1 || v >= V;
    col = bad ? 0 : v;                             // (never an index when out of range)
    if (i >= 1) skip = v != w[i - 1];
  }
  const bool ok = S > 0 && Tb > 0 && __ballot(bad) == 0;      // wave-uniform

  float best = neg_inf();       // this lane's running maximum of a_t(lane), the first frame that attains it
  int best_start = -1, best_end = -1;
  float* tr = TRACE ? trace + pair * T : nullptr;
  __shared__ float chunk[TRACE ? 3 * kSpotTrace : 1];      // 64 frames of e_t, then the lanes' scratch words
  int t_fill = 0;
  if (ok) {
    // Row t of the utterance, clamped to its last: the rows read ahead of Tb - 1
    // stay inside [batch][T] and are never used.
    const float* rows = lp + (int64_t)b * T * V;
    const auto row = [&](int t) { return rows + (int64_t)min(t, T - 1) * V; };
    const float* gp = NORM ? g + (int64_t)b * T : nullptr;
    float gcur = 0.0f, gnext = 0.0f;               // lane i: g of frame 64 c + i, this chunk's and the next's
    if (NORM) {
      gcur = gp[min(lane, T - 1)];
      gnext = gp[min(kSpotTrace + lane, T - 1)];
    }
    float buf[PF];
#pragma unroll
    for (int q = 0; q < PF; ++q) buf[q] = row(q)[col];

    float a = neg_inf();
    int start = -1;
    // The trace: every step lane L-1 drops e_t into chunk[t % 64] with one LDS
    // store that nothing waits for (the other lanes store into scratch words of
    // their own, so the store needs no branch); every 64 frames the chunk goes
    // out as one coalesced row.
    float* const slot = lane == L - 1 ? chunk : chunk + kSpotTrace + lane;
    const auto step = [&](int t, float raw) {
      float x = raw;
      if (NORM) {
        const float gt = read_lane(gcur, t & (kSpotTrace - 1));
        x = raw == neg_inf() ? raw : raw - gt;
      }
      const float p1 = prev_lane(0.0f, a);         // state j-1; for state 0 the entry: value 0 ...
      const int s1 = prev_lane(t, start);          // ... starting at this frame
      const float p2 = prev_lane(neg_inf(), p1);
      const int s2 = prev_lane(-1, s1);
      float m = a;
      int ms = start;
      if (p1 > m) m = p1, ms = s1;
      if (skip && p2 > m) m = p2, ms = s2;
      a = x + m;
      start = a == neg_inf() ? -1 : ms;
      if (a > best) best = a, best_start = start, best_end = t + 1;
      if (TRACE) slot[t & (kSpotTrace - 1)] = a;   // lane L-1: e_t into the chunk; the others: into their own scratch
    };
    const auto store_chunk = [&](int t0, int n) {  // frames t0 .. t0+n-1 of the trace, one per lane
      __builtin_amdgcn_wave_barrier();             // (one wave, and the LDS serves a wave's accesses in order)
      const float e = chunk[lane];
      __builtin_amdgcn_wave_barrier();
      if (lane < n) tr[t0 + lane] = e;
    };
    const auto next_g = [&](int step0) {           // at the first step of a chunk of 64 frames
      if (NORM && step0 > 0 && (step0 & (kSpotTrace - 1)) == 0) {
        gcur = gnext;
        gnext = gp[min(step0 + kSpotTrace + lane, T - 1)];
      }
    };
    int step0 = 0;
    for (; step0 + PF <= Tb; step0 += PF) {
      next_g(step0);
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        step(step0 + q, buf[q]);
        buf[q] = row(step0 + PF + q)[col];
      }
      if (TRACE && ((step0 + PF) & (kSpotTrace - 1)) == 0) store_chunk(step0 + PF - kSpotTrace, kSpotTrace);
    }
    next_g(step0);
#pragma unroll
    for (int q = 0; q < PF; ++q)                   // the last Tb % PF steps: their rows are in buf
      if (step0 + q < Tb) step(step0 + q, buf[q]);
    if (TRACE) {
      const int t0 = Tb & ~(kSpotTrace - 1);       // the chunk the loop has not stored
      store_chunk(t0, Tb - t0);
      t_fill = Tb;
    }
  }
  if (lane == (ok ? L - 1 : 0)) {
    scores[pair] = best;
    spans[2 * pair] = best_start;
    spans[2 * pair + 1] = best_end;
  }
  if (TRACE)
    for (int t = t_fill + lane; t < T; t += 64) tr[t] = neg_inf();
}

}  // namespace
}  // namespace wk

using wk::invalid;

extern "C" {

int64_t wk_ctc_spot_workspace_bytes(int64_t batch, int32_t T, int32_t n_keywords, int32_t max_keyword_len) {
  if (batch <= 0 || T <= 0 || n_keywords <= 0 || max_keyword_len < 1 || max_keyword_len > wk::kSpotMaxLen ||
      batch > wk::kCtcMaxFrames || batch * T > wk::kCtcMaxFrames || batch * n_keywords > wk::kSpotMaxPairs)
    return 0;
  return wk::ctc_spot_bytes(batch, T);
}

wk_status wk_ctc_spot(const float* d_log_probs, int64_t batch, int32_t T, int32_t vocab, const int32_t* d_input_lengths_or_null,
                      const int32_t* d_keywords, int32_t keyword_stride, const int32_t* d_keyword_lengths, int32_t n_keywords,
                      int32_t max_keyword_len, int32_t normalize, void* d_workspace, float* d_scores, int32_t* d_spans,
                      float* d_frame_scores_or_null, int32_t device, void* stream) {
  if (!d_log_probs || !d_keywords || !d_keyword_lengths || !d_workspace || !d_scores || !d_spans)
    return invalid("wk_ctc_spot: null pointer");
  if (batch <= 0 || T <= 0 || vocab <= 0 || n_keywords <= 0)
    return invalid("wk_ctc_spot: batch, T, vocab and n_keywords must be positive");
  if (max_keyword_len < 1 || max_keyword_len > wk::kSpotMaxLen) return invalid("wk_ctc_spot: max_keyword_len must be in [1, 32]");
  if (keyword_stride < max_keyword_len) return invalid("wk_ctc_spot: keyword_stride < max_keyword_len");
  if (vocab > wk::kCtcMaxVocab) return invalid("wk_ctc_spot: vocab > 65536");
  if (batch > wk::kCtcMaxFrames || batch * T > wk::kCtcMaxFrames) return invalid("wk_ctc_spot: batch * T > 2^28");
  if (batch * n_keywords > wk::kSpotMaxPairs) return invalid("wk_ctc_spot: batch * n_keywords > 2^24");
  if ((uintptr_t)d_workspace & 15) return invalid("wk_ctc_spot: d_workspace must be 16-byte aligned");
  if (device < 0) return invalid("wk_ctc_spot: device < 0");
  float* g = (float*)d_workspace;
  hipStream_t st = (hipStream_t)stream;
  return wk::on_device(device, [&]() -> wk_status {
    const int64_t rows = batch * T;
    if (normalize)
      hipLaunchKernelGGL(wk::ctc_spot_rowmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, d_log_probs,
                         d_input_lengths_or_null, rows, T, vocab, g);
    const dim3 grid((unsigned)(batch * n_keywords));
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(64), 0, st, d_log_probs, d_input_lengths_or_null, d_keywords, keyword_stride,
                         d_keyword_lengths, T, vocab, n_keywords, max_keyword_len, g, d_scores, d_spans, d_frame_scores_or_null);
    };
    if (normalize) {
      if (d_frame_scores_or_null) launch(wk::ctc_spot_recur_kernel<true, true>);
      else launch(wk::ctc_spot_recur_kernel<true, false>);
    } else {
      if (d_frame_scores_or_null) launch(wk::ctc_spot_recur_kernel<false, true>);
      else launch(wk::ctc_spot_recur_kernel<false, false>);
    }
    return wk::ctc_launched("wk_ctc_spot");
  });
}

}  // extern "C"
