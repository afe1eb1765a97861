// wk_ctc_loss.hip -- CTC loss and its gradient (nn.CTCLoss(blank=0), ctc.py:369,
// :380-425) on [B][T][V] fp32 log-probs, fp32 arithmetic in log space.
//
// With l' the label sequence interleaved with blanks (L = 2S+1 states),
//   alpha_t(s) = lp_t(l'_s) + lse(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2)])
//   beta_t(s)  = lp_t(l'_s) + lse(beta_{t+1}(s),  beta_{t+1}(s+1),  [beta_{t+1}(s+2)])
// (the third term only for a label state whose label differs from the one two
// states away), nll = -lse(alpha_{T-1}(L-1), alpha_{T-1}(L-2)), and
//   g[t][v] = exp(lp_t(v)) - exp(lse_{s: l'_s = v}(alpha_t(s) + beta_t(s)) + nll - lp_t(v)),
// torch's native CTC backward convention (both alpha and beta include lp_t).
//
// Five launches on the caller's stream, no host synchronisation:
//   prep     one block per utterance: the lattice's inputs (lengths, labels:
//            wk_ctc_lattice_dev.h), and the states of one class chained in
//            index order;
//   gather   lp_t(l'_s) into a dense [B][T][Ls] buffer (wk_ctc_lattice_dev.h);
//   recur    one wave per (utterance, direction) on the register-row layout of
//            wk_ctc_lattice_dev.h -- no LDS, no barrier; the gathered rows are
//            loaded a group of steps ahead;
//   grad     one block per (b, t): alpha + beta staged in LDS, each class's
//            states summed by one lane in index order (the blank's by one wave,
//            a fixed butterfly), the V-wide row written with 16-byte accesses;
//   finish   nll -> d_nll, and the reduction in double in a fixed order.
// Nothing is accumulated with atomics: two calls give the same bits.
#include <math.h>

#include "wakeword.h"
#include "wk_ctc_lattice_dev.h"

namespace wk {
namespace {

constexpr int kFirst = 0x10000;             // chain code: bit 16 = first state of its class, low 16 = next + 1

struct CtcLossWs {
  float *lpg, *alpha, *beta, *nll;
  int32_t *meta, *lab, *chain;
  int ls, smax;      // floats per (b, t) row of lpg / alpha / beta; ints per utterance of lab / chain
  int64_t bytes;
};

CtcLossWs ctc_loss_layout(void* base, int64_t batch, int32_t T, int32_t max_label_len) {
  CtcLossWs w;
  w.ls = ctc_lattice_row(max_label_len);
  w.smax = max_label_len > 0 ? max_label_len : 1;
  const int64_t rows = batch * T * w.ls;
  float* f = (float*)base;
  w.lpg = f;
  w.alpha = f + rows;
  w.beta = f + 2 * rows;
  w.nll = f + 3 * rows;
  w.meta = (int32_t*)(w.nll + batch);
  w.lab = w.meta + 4 * batch;
  w.chain = w.lab + batch * w.smax;
  w.bytes = round_up_256((int64_t)sizeof(float) * (3 * rows + batch) + (int64_t)sizeof(int32_t) * (4 * batch + 2 * batch * w.smax));
  return w;
}

// ---- prep -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_loss_prep_kernel(const int32_t* __restrict__ labels, int label_stride,
                                                            const int32_t* __restrict__ in_len,
                                                            const int32_t* __restrict__ lab_len, int T, int V, int max_label_len,
                                                            CtcLossWs w) {
  __shared__ int sl[256];
  const int b = blockIdx.x, i = threadIdx.x;
  const LatticePrep p = lattice_prep_labels(labels, label_stride, in_len, lab_len, T, V, max_label_len, w);
  const int S = p.S, v = p.v;
  sl[i] = i < S ? v : -1;
  const int any_bad = __syncthreads_or(p.bad);
  if (i < S) {
    int first = kFirst, next = 0;
    for (int j = 0; j < i; ++j)
      if (sl[j] == v) first = 0;
    for (int j = S - 1; j > i; --j)
      if (sl[j] == v) next = j + 1;
    w.chain[(int64_t)b * w.smax + i] = first | next;
  }
  lattice_prep_meta(p.Tb, S, any_bad, w);
  if (i == 0) w.meta[4 * b + 3] = 0;
}

// ---- recursion --------------------------------------------------------------------
// One step of the recursion: a <- x + lse(a, the neighbours'), x the gathered row
// (-inf at s >= L, which keeps those states at -inf).
template <int R, bool REV>
__device__ __forceinline__ void ctc_loss_step(float (&a)[R], const float (&x)[R], const bool (&skip)[R]) {
  const LatticeNb<R> n = lattice_neighbours<R, REV>(a);
#pragma unroll
  for (int j = 0; j < R; ++j) {
    if (R % 2 == 0 && j % 2 == 0)      // s = lane R + j is even: a blank, two terms
      a[j] = x[j] + lse2(a[j], n.n1[j]);
    else
      a[j] = x[j] + lse3(a[j], n.n1[j], skip[j] ? n.n2[j] : neg_inf());
  }
}

// One direction of one utterance on one wave (all 64 lanes active).  Writes
// out[t][s] for t < Tb and every s < 64 R (-inf at s >= L) and returns, in every
// lane, lse of the last row's two final states (forward: -nll).
//
// Steps run in groups of PF.  A group's rows were loaded while the group before
// ran (PF to 2 PF - 1 steps ahead), and inside the main loop every load and
// store is unconditional (a load past the end re-reads the last row), so the
// wait in front of a group is a count that leaves the stores just issued in
// flight; with a branch around either it becomes a wait for everything, and
// each group pays a store's round trip.
template <int R, bool REV>
__device__ __forceinline__ float ctc_loss_recur(const float* __restrict__ lpg, float* __restrict__ out,
                                                const int32_t* __restrict__ lab, int Tb, int S, int lane) {
  constexpr int LS = 64 * R;
  constexpr int PF = R <= 2 ? 8 : 4;
  const int L = 2 * S + 1;
  bool valid[R], skip[R];
  float a[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int s = lane * R + j, i = s >> 1;
    valid[j] = s < L;
    skip[j] = false;
    if (valid[j] && (s & 1)) skip[j] = REV ? (i + 1 < S && lab[i] != lab[i + 1]) : (i >= 1 && lab[i] != lab[i - 1]);
    // the row before the first: all mass on the entry state
    a[j] = s == (REV ? L - 1 : 0) ? 0.0f : neg_inf();
  }
  if (Tb > 0) {
    const float* src = lpg + lane * R;
    float* dst = out + lane * R;
    const auto row = [&](int step) { return (int64_t)(REV ? Tb - 1 - step : step) * LS; };
    float buf[PF][R];
#pragma unroll
    for (int k = 0; k < PF; ++k) ld_row<R>(src + row(min(k, Tb - 1)), buf[k]);
    const auto group = [&](int step0) {
      float cur[PF][R];
#pragma unroll
      for (int k = 0; k < PF; ++k) {
#pragma unroll
        for (int j = 0; j < R; ++j) cur[k][j] = buf[k][j];
        ld_row<R>(src + row(min(step0 + PF + k, Tb - 1)), buf[k]);
      }
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        ctc_loss_step<R, REV>(a, cur[k], skip);
        st_row<R>(dst + row(step0 + k), a);
      }
    };
    // The first group stands outside the loop: the loop is then entered with the
    // memory operations in flight that its own iterations leave (loads, then
    // stores), and the count in front of a group holds on both paths.
    int step0 = 0;
    if (PF <= Tb) {
      group(0);
      for (step0 = PF; step0 + PF <= Tb; step0 += PF) group(step0);
    }
#pragma unroll
    for (int k = 0; k < PF; ++k) {      // the last Tb % PF steps: their rows are in buf
      if (step0 + k < Tb) {
        ctc_loss_step<R, REV>(a, buf[k], skip);
        st_row<R>(dst + row(step0 + k), a);
      }
    }
  }
  // lse over the two exit states (forward: L-1, L-2; backward: 0, 1), butterflies in a fixed order
  float m = neg_inf();
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int s = lane * R + j;
    const bool fin = valid[j] && (REV ? s <= 1 : s >= L - 2);
    if (!fin) a[j] = neg_inf();
    m = fmaxf(m, a[j]);
  }
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  const float mm = m == neg_inf() ? 0.0f : m;
  float sum = 0.0f;
#pragma unroll
  for (int j = 0; j < R; ++j) sum += __expf(a[j] - mm);
  for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
  return mm + wk_logf(sum);
}

template <int R>
__global__ __launch_bounds__(64) void ctc_loss_recur_kernel(int T, CtcLossWs w) {
  const int b = blockIdx.x >> 1, lane = threadIdx.x;
  const bool rev = blockIdx.x & 1;
  const int Tb = __builtin_amdgcn_readfirstlane(w.meta[4 * b]);
  const int S = __builtin_amdgcn_readfirstlane(w.meta[4 * b + 1]);
  const int ok = __builtin_amdgcn_readfirstlane(w.meta[4 * b + 2]);
  if (!ok) {     // a label outside [1, V): no alignment
    if (!rev && lane == 0) w.nll[b] = __builtin_inff();
    return;
  }
  const int64_t row0 = (int64_t)b * T * (64 * R);
  const int32_t* lab = w.lab + (int64_t)b * w.smax;
  if (rev) {
    (void)ctc_loss_recur<R, true>(w.lpg + row0, w.beta + row0, lab, Tb, S, lane);
  } else {
    const float ll = ctc_loss_recur<R, false>(w.lpg + row0, w.alpha + row0, lab, Tb, S, lane);
    if (lane == 0) w.nll[b] = -ll;
  }
}

// ---- gradient ---------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void ctc_loss_grad_kernel(const float* __restrict__ lp, float* __restrict__ grad, int T, int V,
                                                            int64_t batch, int mean, float grad_scale, CtcLossWs w) {
  __shared__ float ab[2 * kCtcLatticeMaxLabels + 2];
  __shared__ int chain[256];
  __shared__ float blank_lcab;
  const int64_t bt = blockIdx.x;
  const int b = (int)(bt / T), t = (int)(bt % T), tid = threadIdx.x;
  const int Tb = w.meta[4 * b], S = w.meta[4 * b + 1];
  const float nll = w.nll[b];
  const float* __restrict__ row = lp + bt * V;
  float* __restrict__ g = grad + bt * V;
  if (t >= Tb || !(nll < __builtin_inff())) {      // padding frames; an utterance without an alignment
    if constexpr (VEC) {
      for (int i = tid; i < V / 4; i += 256) reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int i = tid; i < V; i += 256) g[i] = 0.0f;
    }
    return;
  }
  const float scale = grad_scale * (mean ? 1.0f / ((float)batch * (float)max(S, 1)) : 1.0f);
  const int L = 2 * S + 1;
  const int64_t r0 = bt * w.ls;
  for (int s = tid; s < L; s += 256) ab[s] = w.alpha[r0 + s] + w.beta[r0 + s];
  chain[tid] = tid < S ? w.chain[(int64_t)b * w.smax + tid] : 0;
  __syncthreads();

  // lse of alpha + beta over the states of one class: a label's by the lane of
  // its first occurrence along the chain, the blank's (even states) by wave 3
  float lcab = neg_inf();
  bool leader = false;
  int cls = 0;
  if (tid < S && (chain[tid] & kFirst)) {
    leader = true;
    cls = w.lab[(int64_t)b * w.smax + tid];
    float m = neg_inf();
    for (int j = tid; j >= 0; j = (chain[j] & 0xFFFF) - 1) m = fmaxf(m, ab[2 * j + 1]);
    if (m > neg_inf()) {
      float sum = 0.0f;
      for (int j = tid; j >= 0; j = (chain[j] & 0xFFFF) - 1) sum += __expf(ab[2 * j + 1] - m);
      lcab = m + wk_logf(sum);
    }
  }
  if (tid >= 192) {
    const int lane = tid - 192;
    float m = neg_inf();
    for (int i = lane; i <= S; i += 64) m = fmaxf(m, ab[2 * i]);
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const float mm = m == neg_inf() ? 0.0f : m;
    float sum = 0.0f;
    for (int i = lane; i <= S; i += 64) sum += __expf(ab[2 * i] - mm);
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) blank_lcab = mm + wk_logf(sum);
  }

  if constexpr (VEC) {
    for (int i = tid; i < V / 4; i += 256) {
      const float4 x = reinterpret_cast<const float4*>(row)[i];
      reinterpret_cast<float4*>(g)[i] = make_float4(scale * __expf(x.x), scale * __expf(x.y), scale * __expf(x.z), scale * __expf(x.w));
    }
  } else {
    for (int i = tid; i < V; i += 256) g[i] = scale * __expf(row[i]);
  }
  __syncthreads();      // the row's plain values are written; the label classes and the blank overwrite theirs
  if (leader) {
    const float x = row[cls];
    g[cls] = scale * (__expf(x) - __expf(lcab + nll - x));
  }
  if (tid == 0) {
    const float x = row[0];
    g[0] = scale * (__expf(x) - __expf(blank_lcab + nll - x));
  }
}

// ---- finish -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_loss_finish_kernel(int64_t batch, int reduction, int zero_infinity, CtcLossWs w,
                                                              float* __restrict__ d_nll, float* __restrict__ d_loss) {
  __shared__ double part[256];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int64_t b = tid; b < batch; b += 256) {
    float n = w.nll[b];
    if (zero_infinity && !(n < __builtin_inff())) n = 0.0f;
    d_nll[b] = n;
    acc += reduction == WK_CTC_REDUCTION_MEAN ? (double)n / (double)max(w.meta[4 * b + 1], 1) : (double)n;
  }
  part[tid] = acc;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  if (tid == 0) d_loss[0] = (float)(reduction == WK_CTC_REDUCTION_MEAN ? part[0] / (double)batch : part[0]);
}

}  // namespace
}  // namespace wk

using wk::invalid;

extern "C" {

int64_t wk_ctc_loss_workspace_bytes(int64_t batch, int32_t T, int32_t max_label_len) {
  if (!wk::ctc_lattice_shape_ok(batch, T, max_label_len)) return 0;
  return wk::ctc_loss_layout(nullptr, batch, T, max_label_len).bytes;
}

wk_status wk_ctc_loss(const float* d_log_probs, int64_t batch, int32_t T, int32_t vocab, const int32_t* d_labels,
                      int32_t label_stride, const int32_t* d_input_lengths, const int32_t* d_label_lengths,
                      int32_t max_label_len, int32_t reduction, int32_t zero_infinity, float grad_scale, void* d_workspace,
                      float* d_nll, float* d_loss, float* d_grad_or_null, int32_t device, void* stream) {
  if (!d_log_probs || !d_labels || !d_input_lengths || !d_label_lengths || !d_workspace || !d_nll || !d_loss)
    return invalid("wk_ctc_loss: null pointer");
  if (batch <= 0 || T <= 0 || vocab <= 0) return invalid("wk_ctc_loss: batch, T and vocab must be positive");
  if (max_label_len < 0 || label_stride < max_label_len) return invalid("wk_ctc_loss: label_stride < max_label_len");
  if (reduction != WK_CTC_REDUCTION_NONE && reduction != WK_CTC_REDUCTION_SUM && reduction != WK_CTC_REDUCTION_MEAN)
    return invalid("wk_ctc_loss: bad reduction");
  if (max_label_len > wk::kCtcLatticeMaxLabels) return invalid("wk_ctc_loss: max_label_len > 255");
  if (vocab > wk::kCtcMaxVocab) return invalid("wk_ctc_loss: vocab > 65536");
  if (batch * T > wk::kCtcMaxFrames || batch > wk::kCtcMaxFrames) return invalid("wk_ctc_loss: batch * T > 2^28");
  if ((uintptr_t)d_workspace & 15) return invalid("wk_ctc_loss: d_workspace must be 16-byte aligned");
  if (device < 0) return invalid("wk_ctc_loss: device < 0");
  const wk::CtcLossWs w = wk::ctc_loss_layout(d_workspace, batch, T, max_label_len);
  hipStream_t st = (hipStream_t)stream;
  return wk::on_device(device, [&]() -> wk_status {
    hipLaunchKernelGGL(wk::ctc_loss_prep_kernel, dim3((unsigned)batch), dim3(256), 0, st, d_labels, label_stride, d_input_lengths,
                       d_label_lengths, T, vocab, max_label_len, w);
    wk::launch_lattice_gather(d_log_probs, batch, T, vocab, w, st);
    wk::dispatch_R(w.ls, [&](auto r) {
      hipLaunchKernelGGL(wk::ctc_loss_recur_kernel<decltype(r)::value>, dim3((unsigned)(2 * batch)), dim3(64), 0, st, T, w);
    });
    if (d_grad_or_null) {
      const bool vec = vocab % 4 == 0 && !(((uintptr_t)d_log_probs | (uintptr_t)d_grad_or_null) & 15);
      const int mean = reduction == WK_CTC_REDUCTION_MEAN;
      if (vec)
        hipLaunchKernelGGL(wk::ctc_loss_grad_kernel<true>, dim3((unsigned)(batch * T)), dim3(256), 0, st, d_log_probs,
                           d_grad_or_null, T, vocab, batch, mean, grad_scale, w);
      else
        hipLaunchKernelGGL(wk::ctc_loss_grad_kernel<false>, dim3((unsigned)(batch * T)), dim3(256), 0, st, d_log_probs,
                           d_grad_or_null, T, vocab, batch, mean, grad_scale, w);
    }
    hipLaunchKernelGGL(wk::ctc_loss_finish_kernel, dim3(1), dim3(256), 0, st, batch, reduction, zero_infinity, w, d_nll, d_loss);
    return wk::ctc_launched("wk_ctc_loss");
  });
}

}  // extern "C"
