// wk_ctc_dropout.hip -- train-mode dropout of the GRU-CTC head (ctc.py:131,
// :140) on gfx950: masks from a counter-based generator, applied in the
// training forward and made again, not stored, in the backward.
//
// The addressing (wakeword.h has the full statement): element e = row * width
// + unit of site s under (seed, offset) takes word e % 4 of
//   philox4x32_10(counter = (q low, q high, offset low, offset high | s << 31), key = (seed low, seed high)),  q = e / 4,
// and is kept iff word >= thr = floor(p 2^32); a kept element is multiplied by
// scale = 1.0f / (1.0f - p), a dropped one becomes 0.
//
// One thread makes one Philox block, i.e. four adjacent elements: both widths
// (128, 256) are multiples of 4, so a row is whole blocks, a block never
// straddles two rows, and a block is one 16-byte load and one 16-byte store.
// Every loop is bounded by the block count n4 = rows * width / 4; each element
// is written by one thread; there are no atomics.
#include <cmath>

#include "wk_ctc_dev.h"
#include "wk_philox.h"

namespace wk {
namespace {

// One site of one call, as the kernels take it (by value).
struct DropSite {
  uint2 key;
  uint32_t c2, c3;   // the counter's words 2 and 3: the offset and the site
  uint32_t thr;
  float scale;
};

__device__ __forceinline__ uint4 drop_words(const DropSite& d, int64_t q) {
  return philox4x32_10(make_uint4((uint32_t)q, (uint32_t)((uint64_t)q >> 32), d.c2, d.c3), d.key);
}

__device__ __forceinline__ float4 drop4(const DropSite& d, int64_t q, float4 v) {
  const uint4 w = drop_words(d, q);
  return make_float4(w.x >= d.thr ? v.x * d.scale : 0.0f, w.y >= d.thr ? v.y * d.scale : 0.0f,
                     w.z >= d.thr ? v.z * d.scale : 0.0f, w.w >= d.thr ? v.w * d.scale : 0.0f);
}

// Forward: out = scale * mask * in over n4 blocks of four.  in == out (site 0, in place) is allowed: no __restrict__.
__global__ __launch_bounds__(256) void ctc_dropout_fwd_kernel(const float* in, float* out, int64_t n4, DropSite d) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += step)
    reinterpret_cast<float4*>(out)[q] = drop4(d, q, reinterpret_cast<const float4*>(in)[q]);
}

// Backward: dx <- scale * mask * dx in place, the forward's mask made again.
__global__ __launch_bounds__(256) void ctc_dropout_bwd_kernel(float* __restrict__ dx, int64_t n4, DropSite d) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += step) {
    float4* p = reinterpret_cast<float4*>(dx) + q;
    *p = drop4(d, q, *p);
  }
}

// Mask export: bytes, 1 = kept.  (The caller's buffer has no alignment rule: four byte stores.)
__global__ __launch_bounds__(256) void ctc_dropout_mask_kernel(uint8_t* __restrict__ mask, int64_t n4, DropSite d) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += step) {
    const uint4 w = drop_words(d, q);
    uint8_t* m = mask + 4 * q;
    m[0] = w.x >= d.thr;
    m[1] = w.y >= d.thr;
    m[2] = w.z >= d.thr;
    m[3] = w.w >= d.thr;
  }
}

DropSite drop_site(const CtcDrop& d, int site) {
  return {make_uint2((uint32_t)d.seed, (uint32_t)(d.seed >> 32)), (uint32_t)d.offset,
          (uint32_t)(d.offset >> 32) | ((uint32_t)site << 31), d.thr[site], d.scale[site]};
}

int64_t blocks4(int site, int64_t rows) { return rows * (kCtcDropWidth[site] / 4); }

unsigned drop_grid(int64_t n4, int n_cu) {
  const int64_t blocks = (n4 + 255) / 256;
  return (unsigned)(blocks < 8 * (int64_t)n_cu ? blocks : 8 * (int64_t)n_cu);
}

}  // namespace

CtcDrop ctc_drop(const wk_ctc_dropout& d) {
  CtcDrop r{};
  r.seed = d.seed;
  r.offset = d.offset;
  const float p[2] = {d.p_enc, d.p_gru};
  for (int s = 0; s < 2; ++s) {
    r.on[s] = p[s] > 0.0f;
    r.thr[s] = (uint32_t)std::floor((double)p[s] * 4294967296.0);   // p < 1 as a float: below 2^32
    r.scale[s] = 1.0f / (1.0f - p[s]);
  }
  return r;
}

void launch_ctc_dropout_fwd(const CtcDrop& d, int site, const float* in, float* out, int64_t rows, int n_cu, hipStream_t st) {
  const int64_t n4 = blocks4(site, rows);
  hipLaunchKernelGGL(ctc_dropout_fwd_kernel, dim3(drop_grid(n4, n_cu)), dim3(256), 0, st, in, out, n4, drop_site(d, site));
}

void launch_ctc_dropout_bwd(const CtcDrop& d, int site, float* dx, int64_t rows, int n_cu, hipStream_t st) {
  const int64_t n4 = blocks4(site, rows);
  hipLaunchKernelGGL(ctc_dropout_bwd_kernel, dim3(drop_grid(n4, n_cu)), dim3(256), 0, st, dx, n4, drop_site(d, site));
}

void launch_ctc_dropout_mask(const CtcDrop& d, int site, uint8_t* mask, int64_t rows, int n_cu, hipStream_t st) {
  const int64_t n4 = blocks4(site, rows);
  if (!d.on[site]) {
    (void)hipMemsetAsync(mask, 1, (size_t)n4 * 4, st);
    return;
  }
  hipLaunchKernelGGL(ctc_dropout_mask_kernel, dim3(drop_grid(n4, n_cu)), dim3(256), 0, st, mask, n4, drop_site(d, site));
}

}  // namespace wk
