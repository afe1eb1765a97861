// wk_ctc_lattice_dev.h -- what the units that work on [B][T][V] fp32 log-probs
// share (internal): wk_ctc_loss.hip, wk_ctc_align.hip, wk_ctc_beam.hip,
// wk_ctc_spot.hip and wk_ctc_cer.hip.  One wave holds a row of lattice states
// (or beam slots, or DP columns) in registers, one or R per lane; this header
// has the lane moves and the log-space sums those recurrences are written in,
// the register-row layout of the label lattice with its gather and prep steps
// (loss and align), the split of a V-wide row into aligned 16-byte loads (beam
// and spot), and the host-side limits the five entry points share (their
// launch-error tail, ctc_launched, is in wk_kernels.h with the handle units').
// Each kernel's own layout constants and its tie rule stay in its unit, as
// wk_ctc_dev.h prescribes; wave_max is beside wave_sum in wk_common.h.
#pragma once
#include <string>
#include <type_traits>

#include "wk_common.h"
#include "wk_kernels.h"

namespace wk {

// ---- host side ----------------------------------------------------------------------
constexpr int kCtcMaxVocab = 65536;                    // a token is 16 bits of a node word, a chain code, a column index
constexpr int64_t kCtcMaxFrames = (int64_t)1 << 28;    // batch * T: one block (or wave) per frame fits a grid
constexpr int kCtcLatticeMaxLabels = 255;              // L = 511 states: 8 registers per lane

inline int64_t round_up_256(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

// ---- lanes --------------------------------------------------------------------------
__device__ __forceinline__ float neg_inf() { return -__builtin_inff(); }

// The previous (wave_shr:1) / next (wave_shl:1) lane's v; `fill` in the lane that has none.
__device__ __forceinline__ int prev_lane(int fill, int v) { return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xF, 0xF, false); }
__device__ __forceinline__ int next_lane(int fill, int v) { return __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xF, 0xF, false); }
__device__ __forceinline__ float prev_lane(float fill, float v) {
  return __int_as_float(prev_lane(__float_as_int(fill), __float_as_int(v)));
}
__device__ __forceinline__ float next_lane(float fill, float v) {
  return __int_as_float(next_lane(__float_as_int(fill), __float_as_int(v)));
}

// v of lane `lane` (wave-uniform), in every lane: v_readlane.
__device__ __forceinline__ int read_lane(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float read_lane(float v, int lane) { return __int_as_float(read_lane(__float_as_int(v), lane)); }
__device__ __forceinline__ uint32_t read_lane(uint32_t v, int lane) { return (uint32_t)read_lane((int)v, lane); }
__device__ __forceinline__ int64_t read_lane(int64_t v, int lane) {
  const uint32_t lo = read_lane((uint32_t)v, lane), hi = read_lane((uint32_t)((uint64_t)v >> 32), lane);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// ln(e^a + e^b) and ln(e^a + e^b + e^c), -inf when every term is.  The largest
// term's exponential is 1 exactly, so it is not computed: max / med / min are
// one instruction each where an exponential is a double-cost one.  (All -inf:
// the differences are NaN and the select drops them.)
__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b), n = fminf(a, b);
  const float r = m + wk_logf(1.0f + __expf(n - m));
  return m == neg_inf() ? m : r;
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c), d = __builtin_amdgcn_fmed3f(a, b, c), n = fminf(fminf(a, b), c);
  const float r = m + wk_logf(1.0f + __expf(d - m) + __expf(n - m));
  return m == neg_inf() ? m : r;
}

// ---- a V-wide row in 16-byte loads ----------------------------------------------------
// Row p[0 .. V) as a head of single elements [0, head) up to the first 16-byte
// boundary, nq quads q4[0 .. nq) and a tail [tail0, V): ids 0 .. V-1 in order,
// no byte outside the row touched.
struct RowSplit {
  int head, nq, tail0;
  const float4* q4;
};
__device__ __forceinline__ RowSplit row_split(const float* p, int V) {
  const int head = min((int)((4 - (((uintptr_t)p >> 2) & 3)) & 3), V);
  const int nq = (V - head) >> 2;
  return {head, nq, head + 4 * nq, reinterpret_cast<const float4*>(p + head)};
}

// ---- the label lattice in registers (loss, align) ---------------------------------------
// With l' the labels interleaved with blanks, L = 2S+1 states.  A row of the
// lattice is ls = 64 R floats, R in {1, 2, 4, 8}: lane i of the one wave that
// runs the recursion holds the consecutive states i R .. i R + R - 1.
//
// A unit's workspace struct `Ws` carries the lattice's inputs under these names:
//   float* lpg      [batch][T][ls] gathered log-probs lp_t(l'_s), -inf at s >= L
//   int32_t* meta   [batch][4]     Tb, S, labels valid, (the unit's)
//   int32_t* lab    [batch][smax]  the labels, 0 for one outside [1, V)
//   int ls, smax
// The kernels take it by value, so the struct's layout is the unit's own.

// States per row; 0 beyond kCtcLatticeMaxLabels.
inline int ctc_lattice_row(int max_label_len) {
  const int L = 2 * max_label_len + 1;
  for (int r = 1; r <= 8; r *= 2)
    if (L <= 64 * r) return 64 * r;
  return 0;
}
inline bool ctc_lattice_shape_ok(int64_t batch, int32_t T, int32_t max_label_len) {
  return batch > 0 && T > 0 && max_label_len >= 0 && max_label_len <= kCtcLatticeMaxLabels && batch * T <= kCtcMaxFrames;
}
// f(std::integral_constant<int, R>) for the R of a row of ls floats.
template <typename F> void dispatch_R(int ls, F f) {
  switch (ls / 64) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}
inline int ls_shift(int ls) {      // log2(ls)
  int shift = 6;
  while ((1 << shift) < ls) ++shift;
  return shift;
}

template <int R> __device__ __forceinline__ void ld_row(const float* p, float (&r)[R]) {
  if constexpr (R == 1) {
    r[0] = p[0];
  } else if constexpr (R == 2) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    r[0] = v.x;
    r[1] = v.y;
  } else {
#pragma unroll
    for (int k = 0; k < R / 4; ++k) {
      const float4 v = reinterpret_cast<const float4*>(p)[k];
      r[4 * k] = v.x, r[4 * k + 1] = v.y, r[4 * k + 2] = v.z, r[4 * k + 3] = v.w;
    }
  }
}
template <int R> __device__ __forceinline__ void st_row(float* p, const float (&r)[R]) {
  if constexpr (R == 1) {
    p[0] = r[0];
  } else if constexpr (R == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(r[0], r[1]);
  } else {
#pragma unroll
    for (int k = 0; k < R / 4; ++k) reinterpret_cast<float4*>(p)[k] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
  }
}

// What a step combines a[j] with: n1[j], n2[j] = states s-1, s-2 (REV: s+1,
// s+2) of row a.  They are the lane's own registers but for two values that
// come from the neighbouring lane by a DPP wave shift (-inf past the ends).
template <int R> struct LatticeNb {
  float n1[R], n2[R];
};
template <int R, bool REV> __device__ __forceinline__ LatticeNb<R> lattice_neighbours(const float (&a)[R]) {
  LatticeNb<R> n;
  if constexpr (!REV) {
    const float p1 = prev_lane(neg_inf(), a[R - 1]);
    const float p2 = R >= 2 ? prev_lane(neg_inf(), a[R >= 2 ? R - 2 : 0]) : prev_lane(neg_inf(), p1);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      n.n1[j] = j >= 1 ? a[j >= 1 ? j - 1 : 0] : p1;
      n.n2[j] = j >= 2 ? a[j >= 2 ? j - 2 : 0] : (j == 1 ? p1 : p2);
    }
  } else {
    const float q1 = next_lane(neg_inf(), a[0]);
    const float q2 = R >= 2 ? next_lane(neg_inf(), a[R >= 2 ? 1 : 0]) : next_lane(neg_inf(), q1);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      n.n1[j] = j + 1 < R ? a[j + 1 < R ? j + 1 : 0] : q1;
      n.n2[j] = j + 2 < R ? a[j + 2 < R ? j + 2 : 0] : (j + 2 == R ? q1 : q2);
    }
  }
  return n;
}

// The common half of a prep kernel (one block of 256 threads per utterance,
// blockIdx.x), in two steps around the kernel's own __syncthreads_or(bad):
// lattice_prep_labels clamps the lengths and validates and copies thread i's
// label; lattice_prep_meta writes meta[0..2].
struct LatticePrep {
  int Tb, S;      // clamp(input_length, 0, T), clamp(label_length, 0, max_label_len)
  int bad, v;     // thread i < S: its label is outside [1, V); the label, 0 when bad (never an index)
};
template <typename Ws>
__device__ __forceinline__ LatticePrep lattice_prep_labels(const int32_t* labels, int label_stride, const int32_t* in_len,
                                                           const int32_t* lab_len, int T, int V, int max_label_len, const Ws& w) {
  const int b = blockIdx.x, i = threadIdx.x;
  LatticePrep p = {min(max(in_len[b], 0), T), min(max(lab_len[b], 0), max_label_len), 0, 0};
  if (i < p.S) {
    p.v = labels[(int64_t)b * label_stride + i];
    p.bad = p.v < 1 || p.v >= V;
    if (p.bad) p.v = 0;
    w.lab[(int64_t)b * w.smax + i] = p.v;
  }
  return p;
}
template <typename Ws> __device__ __forceinline__ void lattice_prep_meta(int Tb, int S, int any_bad, const Ws& w) {
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    w.meta[4 * b + 0] = Tb;
    w.meta[4 * b + 1] = S;
    w.meta[4 * b + 2] = !any_bad;
  }
}

// lp_t(l'_s) into the dense [B][T][ls] buffer, parallel over t, so the recursion
// never waits on a strided load from a V-wide row.
template <typename Ws>
__global__ __launch_bounds__(256) void ctc_lattice_gather_kernel(const float* __restrict__ lp, int T, int V, int ls_shift,
                                                                 int64_t total, Ws w) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;                                        // total = batch * T * ls
  const int s = (int)(idx & (w.ls - 1));
  const int64_t bt = idx >> ls_shift;
  const int b = (int)(bt / T), t = (int)(bt % T);
  const int Tb = w.meta[4 * b], S = w.meta[4 * b + 1];
  if (t >= Tb) return;
  if (s > 2 * S) {                 // past the last state: -inf, which the recursion relies on
    w.lpg[idx] = neg_inf();
    return;
  }
  const int v = (s & 1) ? w.lab[(int64_t)b * w.smax + (s >> 1)] : 0;
  w.lpg[idx] = lp[bt * V + v];
}
template <typename Ws> void launch_lattice_gather(const float* lp, int64_t batch, int T, int V, const Ws& w, hipStream_t st) {
  const int64_t total = batch * T * w.ls;
  hipLaunchKernelGGL(ctc_lattice_gather_kernel<Ws>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, lp, T, V,
                     ls_shift(w.ls), total, w);
}

}  // namespace wk
