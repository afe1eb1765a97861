// wk_ctc_align.hip -- CTC forced alignment: the best (Viterbi) path of a known
// label sequence through [B][T][V] fp32 log-probs, blank = 0.
//
// With l' the label sequence interleaved with blanks (L = 2S+1 states) and
// Tb = clamp(input_length, 0, T),
//   a_0(0) = lp_0(0),  a_0(1) = lp_0(l'_1),  a_0(s >= 2) = -inf
//   a_t(s) = lp_t(l'_s) + max(a_{t-1}(s), a_{t-1}(s-1), [a_{t-1}(s-2)])
// (the third term only for a label state whose label differs from the one two
// states back: wk_ctc_loss's lattice with max in place of lse), score =
// max(a_{Tb-1}(L-1), a_{Tb-1}(L-2)), and the path follows the back-pointers from
// that state.  Ties: among equal predecessors s, then s-1, then s-2 (a
// candidate replaces the best only if strictly greater); at the exit L-1 when
// a(L-1) >= a(L-2).  max is exact and the add rounds once, so the result is
// defined bit for bit by the recurrence, whatever the lane layout.
//
// Four launches on the caller's stream, no host synchronisation, no atomics:
//   prep     one block per utterance: the lattice's inputs (lengths, labels:
//            wk_ctc_lattice_dev.h), the spans preset to -1;
//   gather   lp_t(l'_s) into a dense [B][T][Ls] buffer (wk_ctc_lattice_dev.h);
//   recur    one wave per utterance on the register-row layout of
//            wk_ctc_lattice_dev.h, the gathered rows loaded a group of steps
//            ahead.  Per step a lane packs its R two-bit back-pointers into
//            one word and stores it: one coalesced row of 64 words per (b, t);
//            no alpha row is stored.  The same wave then
//            walks the path back: lane i re-loads word i of a group of rows (the
//            addresses do not depend on the path, so the loads run ahead), and
//            each step is a v_readlane at the uniform index s / R and scalar
//            arithmetic -- no memory access on the dependent chain.  The states
//            of 64 frames are collected one per lane and stored as one row;
//   emit     one thread per (b, t): token, log-prob and, where a label's run of
//            frames begins or ends, its span.
#include <math.h>

#include "wakeword.h"
#include "wk_ctc_lattice_dev.h"

namespace wk {
namespace {

constexpr int kBackChunk = 64;               // frames per backtrace chunk: one back-pointer row per register, one state per lane
constexpr int kPadRows = 128;                // back-pointer rows of slack between lpg and bp (below)

struct CtcAlignWs {
  float* lpg;        // [batch][T][ls] gathered log-probs
  uint32_t* bp;      // [batch][T][64] back-pointers: lane i's word holds 2 bits per state i*R + j.
                     // kPadRows rows (32 KiB) of slack lie between lpg and bp: the recursion's row loads
                     // run a prefetch group past an utterance's last row (at most 16 KiB past
                     // lpg's end) and the backtrace's up to 127 rows before its first (before bp's start),
                     // so neither needs a clamped address; what they read there is never used
  int32_t *meta, *lab;   // [batch][4]: Tb, S, labels valid, (spare); [batch][smax]
  int ls, smax;
  int64_t bytes;
};

CtcAlignWs ctc_align_layout(void* base, int64_t batch, int32_t T, int32_t max_label_len) {
  CtcAlignWs w;
  w.ls = ctc_lattice_row(max_label_len);
  w.smax = max_label_len > 0 ? max_label_len : 1;
  const int64_t frames = batch * T;
  w.lpg = (float*)base;
  w.bp = (uint32_t*)(w.lpg + frames * w.ls) + kPadRows * 64;
  w.meta = (int32_t*)(w.bp + frames * 64);
  w.lab = w.meta + 4 * batch;
  w.bytes = round_up_256((int64_t)4 * (frames * w.ls + (frames + kPadRows) * 64 + 4 * batch + batch * w.smax));
  return w;
}

// ---- prep -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_align_prep_kernel(const int32_t* __restrict__ labels, int label_stride,
                                                             const int32_t* __restrict__ in_len,
                                                             const int32_t* __restrict__ lab_len, int T, int V, int max_label_len,
                                                             int32_t* __restrict__ spans, CtcAlignWs w) {
  const int b = blockIdx.x, i = threadIdx.x;
  const LatticePrep p = lattice_prep_labels(labels, label_stride, in_len, lab_len, T, V, max_label_len, w);
  if (spans && i < max_label_len) {          // emit overwrites the labels an alignment places
    spans[((int64_t)b * max_label_len + i) * 2] = -1;
    spans[((int64_t)b * max_label_len + i) * 2 + 1] = -1;
  }
  lattice_prep_meta(p.Tb, p.S, __syncthreads_or(p.bad), w);
}

// ---- recursion and backtrace ------------------------------------------------------
// One step: a <- x + max(a, the neighbours'), x the gathered row (-inf at s >= L,
// which keeps those states at -inf).  Returns the lane's back-pointers, two
// bits per state: how far back (0, 1 or 2 states) the maximum lies.
template <int R> __device__ __forceinline__ uint32_t ctc_align_step(float (&a)[R], const float (&x)[R], const bool (&skip)[R]) {
  const LatticeNb<R> n = lattice_neighbours<R, false>(a);
  uint32_t word = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    float best = a[j];
    uint32_t k = 0;
    if (n.n1[j] > best) best = n.n1[j], k = 1;
    if (!(R % 2 == 0 && j % 2 == 0)) {      // (an even state is a blank: two terms)
      if (skip[j] && n.n2[j] > best) best = n.n2[j], k = 2;
    }
    a[j] = x[j] + best;
    word |= k << (2 * j);
  }
  return word;
}

// The forward pass of one utterance on one wave (all 64 lanes active): writes
// the back-pointer row of every t < Tb and leaves a_{Tb-1} in a.  Row t + PF is
// loaded into the register row t leaves free, so PF rows are in flight; every
// load and store of the main loop is unconditional and unclamped (the rows past
// Tb - 1 it touches lie in the workspace, CtcAlignWs, and are never used), so an
// address is a running pointer plus an immediate and the wait in front of a
// step is a count that leaves the younger loads and stores in flight.
template <int R>
__device__ __forceinline__ void ctc_align_forward(const float* __restrict__ lpg, uint32_t* bp, const int32_t* __restrict__ lab,
                                                  int Tb, int S, int lane, float (&a)[R]) {
  constexpr int LS = 64 * R;
  constexpr int PF = R <= 2 ? 16 : 8;      // rows in flight: 8 KiB (R <= 4) or 16 KiB (R = 8) per wave
  const int L = 2 * S + 1;
  bool skip[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int s = lane * R + j, i = s >> 1;
    skip[j] = s < L && (s & 1) && i >= 1 && lab[i] != lab[i - 1];
    a[j] = s == 0 ? 0.0f : neg_inf();      // the row before the first: x + 0 = x exactly, so a_0 is as defined
  }
  const float* src = lpg + lane * R;
  uint32_t* dst = bp + lane;
  float buf[PF][R];
#pragma unroll
  for (int k = 0; k < PF; ++k) ld_row<R>(src + (int64_t)k * LS, buf[k]);
  const auto group = [&](int step0) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      dst[(int64_t)(step0 + k) * 64] = ctc_align_step<R>(a, buf[k], skip);
      ld_row<R>(src + (int64_t)(step0 + PF + k) * LS, buf[k]);
    }
  };
  // The first group stands outside the loop: the loop is then entered with the
  // memory operations in flight that its own iterations leave.
  int step0 = 0;
  if (PF <= Tb) {
    group(0);
    for (step0 = PF; step0 + PF <= Tb; step0 += PF) group(step0);
  }
#pragma unroll
  for (int k = 0; k < PF; ++k)      // the last Tb % PF steps: their rows are in buf
    if (step0 + k < Tb) dst[(int64_t)(step0 + k) * 64] = ctc_align_step<R>(a, buf[k], skip);
}

template <int R>
__global__ __launch_bounds__(64) void ctc_align_recur_kernel(int T, CtcAlignWs w, int32_t* __restrict__ states,
                                                             float* __restrict__ score) {
  constexpr int LOG_R = R == 1 ? 0 : R == 2 ? 1 : R == 4 ? 2 : 3;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = __builtin_amdgcn_readfirstlane(w.meta[4 * b]);
  const int S = __builtin_amdgcn_readfirstlane(w.meta[4 * b + 1]);
  const int ok = __builtin_amdgcn_readfirstlane(w.meta[4 * b + 2]);
  const int64_t frame0 = (int64_t)b * T;
  uint32_t* bp = w.bp + frame0 * 64;
  int32_t* st = states + frame0;

  int s = -1;                   // the path's state, wave-uniform; -1: no alignment
  float best = neg_inf();
  if (ok && Tb > 0) {
    float a[R];
    ctc_align_forward<R>(w.lpg + frame0 * (64 * R), bp, w.lab + (int64_t)b * w.smax, Tb, S, lane, a);
    // the two exit states, L-1 (the trailing blank) and L-2 (none when S = 0)
    const int L = 2 * S + 1;
    float e1 = neg_inf(), e2 = neg_inf();
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int q = lane * R + j;
      if (q == L - 1) e1 = a[j];
      if (q == L - 2) e2 = a[j];
    }
    e1 = __shfl(e1, (L - 1) >> LOG_R);
    e2 = __shfl(e2, max(L - 2, 0) >> LOG_R);
    const bool last = e1 >= e2;
    best = last ? e1 : e2;
    // (S = 0: e2 = -inf, so L-2 is chosen only with best = -inf, which is no alignment)
    s = __builtin_amdgcn_readfirstlane(best == neg_inf() ? -1 : last ? L - 1 : L - 2);
  }
  if (lane == 0) score[b] = best;

  // Backtrace, a chunk of 64 frames at a time from the last: step k of chunk c is
  // frame Tb-1 - 64 c - k.  Register k holds this lane's word of that frame's row
  // (the word the lane wrote itself: same thread, same address, program order)
  // and is re-loaded with the next chunk's as soon as the step has read it, so 64
  // rows are in flight and no address depends on the path.  A step reads word
  // s / R of its row with v_readlane and steps back by the two bits of state s,
  // clamped so that s stays in [0, L) on any input; lane k keeps the state of
  // step k and the chunk is stored as one row.  The last chunk's steps before
  // frame 0 read the slack in front of bp: s is not used after frame 0, and
  // those lanes do not store.
  int t_fill = 0;
  if (s >= 0) {
    constexpr int G = kBackChunk;
    const uint32_t* src = bp + (int64_t)(Tb - 1) * 64 + lane;
    uint32_t row[G];
#pragma unroll
    for (int k = 0; k < G; ++k) row[k] = src[-(int64_t)k * 64];
    for (int t0 = Tb - 1; t0 >= 0; t0 -= G) {      // t0: the frame of step 0
      src -= G * 64;
      int mine = 0;
#pragma unroll
      for (int k = 0; k < G; ++k) {
        mine = lane == k ? s : mine;
        const uint32_t word = read_lane(row[k], s >> LOG_R);
        row[k] = src[-(int64_t)k * 64];
        const int back = (int)((word >> (2 * (s & (R - 1)))) & 3u);
        s -= min(back, s);
      }
      const int t = t0 - lane;
      if (t >= 0) st[t] = mine;
    }
    t_fill = Tb;
  }
  for (int t = t_fill + lane; t < T; t += 64) st[t] = -1;
}

// ---- emit -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_align_emit_kernel(const int32_t* __restrict__ states, int T, int max_label_len,
                                                             int64_t frames, int32_t* __restrict__ tokens,
                                                             float* __restrict__ frame_lp, int32_t* __restrict__ spans,
                                                             CtcAlignWs w) {
  const int64_t bt = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (bt >= frames) return;
  const int b = (int)(bt / T), t = (int)(bt % T);
  const int s = states[bt];
  if (s < 0) {
    if (tokens) tokens[bt] = -1;
    if (frame_lp) frame_lp[bt] = 0.0f;
    return;
  }
  const int i = s >> 1;
  if (tokens) tokens[bt] = (s & 1) ? w.lab[(int64_t)b * w.smax + i] : 0;
  if (frame_lp) frame_lp[bt] = w.lpg[bt * w.ls + s];
  if (spans && (s & 1) && i < max_label_len) {
    // a label's frames are one contiguous run: its first frame writes the start, its last the end
    const int prev = t > 0 ? states[bt - 1] : -1;
    const int next = t + 1 < T ? states[bt + 1] : -1;      // -1 from Tb on
    int32_t* sp = spans + ((int64_t)b * max_label_len + i) * 2;
    if (prev != s) sp[0] = t;
    if (next != s) sp[1] = t + 1;
  }
}

}  // namespace
}  // namespace wk

using wk::invalid;

extern "C" {

int64_t wk_ctc_align_workspace_bytes(int64_t batch, int32_t T, int32_t max_label_len) {
  if (!wk::ctc_lattice_shape_ok(batch, T, max_label_len)) return 0;
  return wk::ctc_align_layout(nullptr, batch, T, max_label_len).bytes;
}

wk_status wk_ctc_align(const float* d_log_probs, int64_t batch, int32_t T, int32_t vocab, const int32_t* d_labels,
                       int32_t label_stride, const int32_t* d_input_lengths, const int32_t* d_label_lengths,
                       int32_t max_label_len, void* d_workspace, int32_t* d_states, int32_t* d_frame_tokens_or_null,
                       float* d_frame_lp_or_null, int32_t* d_spans_or_null, float* d_score, int32_t device, void* stream) {
  if (!d_log_probs || !d_labels || !d_input_lengths || !d_label_lengths || !d_workspace || !d_states || !d_score)
    return invalid("wk_ctc_align: null pointer");
  if (batch <= 0 || T <= 0 || vocab <= 0) return invalid("wk_ctc_align: batch, T and vocab must be positive");
  if (max_label_len < 0 || label_stride < max_label_len) return invalid("wk_ctc_align: label_stride < max_label_len");
  if (max_label_len > wk::kCtcLatticeMaxLabels) return invalid("wk_ctc_align: max_label_len > 255");
  if (vocab > wk::kCtcMaxVocab) return invalid("wk_ctc_align: vocab > 65536");
  if (batch * T > wk::kCtcMaxFrames || batch > wk::kCtcMaxFrames) return invalid("wk_ctc_align: batch * T > 2^28");
  if ((uintptr_t)d_workspace & 15) return invalid("wk_ctc_align: d_workspace must be 16-byte aligned");
  if (device < 0) return invalid("wk_ctc_align: device < 0");
  const wk::CtcAlignWs w = wk::ctc_align_layout(d_workspace, batch, T, max_label_len);
  hipStream_t st = (hipStream_t)stream;
  return wk::on_device(device, [&]() -> wk_status {
    hipLaunchKernelGGL(wk::ctc_align_prep_kernel, dim3((unsigned)batch), dim3(256), 0, st, d_labels, label_stride,
                       d_input_lengths, d_label_lengths, T, vocab, max_label_len, d_spans_or_null, w);
    wk::launch_lattice_gather(d_log_probs, batch, T, vocab, w, st);
    wk::dispatch_R(w.ls, [&](auto r) {
      hipLaunchKernelGGL(wk::ctc_align_recur_kernel<decltype(r)::value>, dim3((unsigned)batch), dim3(64), 0, st, T, w, d_states,
                         d_score);
    });
    if (d_frame_tokens_or_null || d_frame_lp_or_null || d_spans_or_null) {
      const int64_t frames = batch * T;
      hipLaunchKernelGGL(wk::ctc_align_emit_kernel, dim3((unsigned)((frames + 255) / 256)), dim3(256), 0, st, d_states, T,
                         max_label_len, frames, d_frame_tokens_or_null, d_frame_lp_or_null, d_spans_or_null, w);
    }
    return wk::ctc_launched("wk_ctc_align");
  });
}

}  // extern "C"
