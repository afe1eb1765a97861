// wk_ctc_optim.hip -- the optimiser half of the GRU-CTC training step
// (ctc.py:368, :401-402: clip_grad_norm_(5.0) then optim.Adam(lr=1e-3)) on the
// weights as a wk_ctc handle keeps them, fp32:
//
//   ctc_adam_kernel     clip + Adam on the handle's per-tensor buffers, in place
//   ctc_refresh_kernel  whh_pk[l] and whht_pk[l] again from the updated whh[l]
//   ctc_blob_kernel     the blob <-> the per-tensor buffers (wk_ctc_weights / wk_ctc_set_weights)
//
// A handle's weights are not a blob: wk_ctc_create splits it into per-tensor
// buffers (CtcSegTable names them in blob order) and derives the two fragment
// layouts of W_hh on the host.  The gradient and the moments stay in blob
// order; a workgroup row (blockIdx.y) is one segment, so the segment is uniform
// and every element of every buffer is written by exactly one thread.  No
// atomics; loops are bounded by the segment's length.
#include "wk_ctc_dev.h"

namespace {
using namespace wk;

// A workgroup row's walk over its segment's `len` elements: vec(i) for each
// group of four starting at element i (every segment starts on a multiple of
// 4 floats in the blob and on 16 bytes in its buffer), then one(i) for the
// scalar tail -- which is the whole segment when VEC is off (a caller's blob
// pointer that is not 16-byte aligned).
template <bool VEC, typename F4, typename F1>
__device__ __forceinline__ void for_segment(int64_t len, F4 vec, F1 one) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  const int64_t nv = VEC ? len >> 2 : 0;
  for (int64_t i = tid; i < nv; i += nth) vec(4 * i);
  for (int64_t i = 4 * nv + tid; i < len; i += nth) one(i);
}

// One element of torch.optim.Adam (non-amsgrad, L2 weight decay) after clip_grad_norm_'s scaling.
__device__ __forceinline__ void adam_one(float& p, float& m, float& v, float g, float coef, const CtcAdamArgs& a) {
  g *= coef;
  g += a.weight_decay * p;
  m = a.beta1 * m + a.one_minus_beta1 * g;
  v = a.beta2 * v + a.one_minus_beta2 * (g * g);
  p -= a.step_size * m / (sqrtf(v) / a.sqrt_bc2 + a.eps);
}

template <bool VEC>
__global__ __launch_bounds__(256) void ctc_adam_kernel(const CtcSegTable tab, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, const float* __restrict__ norm,
                                                       const CtcAdamArgs a) {
  const CtcSeg s = tab.s[blockIdx.y];
  // clip_grad_norm_: min(1, max_norm / (norm + 1e-6)); a NaN norm stays NaN (the comparison is false), as torch's clamp
  float coef = 1.0f;
  if (norm) {
    const float c = a.max_norm / (norm[0] + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;
  }
  float* __restrict__ p = s.p;
  const float* gs = g + s.off;
  float *ms = m + s.off, *vs = v + s.off;
  for_segment<VEC>(
      s.len,
      [&](int64_t i) {
        float4 pp = *reinterpret_cast<const float4*>(p + i), mm = *reinterpret_cast<const float4*>(ms + i);
        float4 vv = *reinterpret_cast<const float4*>(vs + i);
        const float4 gg = *reinterpret_cast<const float4*>(gs + i);
        adam_one(pp.x, mm.x, vv.x, gg.x, coef, a);
        adam_one(pp.y, mm.y, vv.y, gg.y, coef, a);
        adam_one(pp.z, mm.z, vv.z, gg.z, coef, a);
        adam_one(pp.w, mm.w, vv.w, gg.w, coef, a);
        *reinterpret_cast<float4*>(p + i) = pp;
        *reinterpret_cast<float4*>(ms + i) = mm;
        *reinterpret_cast<float4*>(vs + i) = vv;
      },
      [&](int64_t i) {
        float pp = p[i], mm = ms[i], vv = vs[i];
        adam_one(pp, mm, vv, gs[i], coef, a);
        p[i] = pp;
        ms[i] = mm;
        vs[i] = vv;
      });
}

// TO_BLOB: blob[off + i] = buffer[i] (gather); else buffer[i] = blob[off + i] (scatter).
template <bool VEC, bool TO_BLOB>
__global__ __launch_bounds__(256) void ctc_blob_kernel(const CtcSegTable tab, float* __restrict__ blob_out,
                                                       const float* __restrict__ blob_in) {
  const CtcSeg s = tab.s[blockIdx.y];
  const float* src = TO_BLOB ? s.p : blob_in + s.off;
  float* dst = TO_BLOB ? blob_out + s.off : s.p;
  for_segment<VEC>(
      s.len, [&](int64_t i) { *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i); },
      [&](int64_t i) { dst[i] = src[i]; });
}

// The two fragment layouts of W_hh [2 dir][384][128], one output element per
// thread (a gather: the writes are coalesced), by the host packers' formulas:
//   y = 0, 1: whh_pk[y]   [dir][24 tiles][32 k-steps][64 lanes]  = whh[dir][16 tl + (l & 15)][4 s + (l >> 4)]   (pack_frag, E = 1)
//   y = 2, 3: whht_pk[y-2] [dir][8 tiles][96 k-steps][64 lanes]  = whh[dir][4 s + (l >> 4)][16 tl + (l & 15)]   (ctc_pack_whht)
constexpr int kWhhFloats = 2 * 3 * kH * kH;
static_assert(kWhhFloats % 256 == 0 && kWhhFloats == 2 * 24 * 32 * 64 && kWhhFloats == 2 * 8 * 96 * 64, "fragment layouts");
__global__ __launch_bounds__(256) void ctc_refresh_kernel(const CtcWhhSet w) {
  const int layer = blockIdx.y & 1;
  const bool transposed = blockIdx.y >= 2;
  const float* __restrict__ whh = layer ? w.whh[1] : w.whh[0];
  float* __restrict__ out = transposed ? (layer ? w.whht_pk[1] : w.whht_pk[0]) : (layer ? w.whh_pk[1] : w.whh_pk[0]);
  const int o = blockIdx.x * 256 + threadIdx.x;   // < kWhhFloats: the grid is exact
  const int ln = o & 63, t = o >> 6;
  int row, col;
  if (!transposed) {
    const int s = t & 31, tl = (t >> 5) % 24, d = t / (32 * 24);
    row = d * 3 * kH + 16 * tl + (ln & 15);
    col = 4 * s + (ln >> 4);
  } else {
    const int s = t % 96, tl = (t / 96) & 7, d = t / (96 * 8);
    row = d * 3 * kH + 4 * s + (ln >> 4);
    col = 16 * tl + (ln & 15);
  }
  out[o] = whh[row * kH + col];
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One workgroup row per segment; enough columns for the longest one at a few vectors per thread.
dim3 seg_grid(const CtcSegTable& tab, int n_cu) {
  int64_t longest = 1;
  for (const CtcSeg& s : tab.s) longest = s.len > longest ? s.len : longest;
  const int64_t want = (longest / 4 + 255) / 256, cap = 2 * (int64_t)n_cu;
  return dim3((unsigned)(want < cap ? want : cap), kCtcSegs);
}

}  // namespace

namespace wk {

void launch_ctc_adam(const CtcSegTable& tab, const float* g, float* m, float* v, const float* norm, const CtcAdamArgs& a,
                     int n_cu, hipStream_t st) {
  if (aligned16(g))   // (m, v and the handle's buffers are hipMalloc blocks)
    hipLaunchKernelGGL(ctc_adam_kernel<true>, seg_grid(tab, n_cu), dim3(256), 0, st, tab, g, m, v, norm, a);
  else
    hipLaunchKernelGGL(ctc_adam_kernel<false>, seg_grid(tab, n_cu), dim3(256), 0, st, tab, g, m, v, norm, a);
}

void launch_ctc_refresh(const CtcWhhSet& w, hipStream_t st) {
  hipLaunchKernelGGL(ctc_refresh_kernel, dim3(kWhhFloats / 256, 4), dim3(256), 0, st, w);
}

void launch_ctc_gather(const CtcSegTable& tab, float* blob, int n_cu, hipStream_t st) {
  if (aligned16(blob))
    hipLaunchKernelGGL((ctc_blob_kernel<true, true>), seg_grid(tab, n_cu), dim3(256), 0, st, tab, blob, nullptr);
  else
    hipLaunchKernelGGL((ctc_blob_kernel<false, true>), seg_grid(tab, n_cu), dim3(256), 0, st, tab, blob, nullptr);
}

void launch_ctc_scatter(const CtcSegTable& tab, const float* blob, int n_cu, hipStream_t st) {
  if (aligned16(blob))
    hipLaunchKernelGGL((ctc_blob_kernel<true, false>), seg_grid(tab, n_cu), dim3(256), 0, st, tab, nullptr, blob);
  else
    hipLaunchKernelGGL((ctc_blob_kernel<false, false>), seg_grid(tab, n_cu), dim3(256), 0, st, tab, nullptr, blob);
}

}  // namespace wk
