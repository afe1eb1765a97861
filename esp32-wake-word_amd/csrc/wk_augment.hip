// wk_augment.hip -- wk_augment_batch: extract_features' waveform stage
// (extract_mfcc.py:7-45, :90-121, :157-169) for a batch of clips on gfx950:
// pad_audio, the speed / volume variants of augment_audio_waveform and
// add_random_noise.  include/wakeword.h has the full statement of row r = i*K + v.
//
// One workgroup of 1024 threads makes one output row: thread t owns the Philox
// blocks q = t + 1024 k, i.e. samples 4q..4q+3, so a wave's loads and stores are
// 1 KiB runs of 16-byte pieces.  With the SNR stage off the row streams through
// (its own instantiation, without the row's LDS); with it on, b and z wait in LDS
// (2 x 64 KiB) for the row's two powers, so the clip is read once and the noise
// made once.  All noise is a function of its address (stream, row, sample), so
// a pad sample that the interpolation reads is made again where it is read,
// never stored.  The row's two powers are summed per thread in sample order,
// across the wave by a butterfly (every lane ends with the same sum) and across
// the 16 waves by one thread in wave order: a fixed order, no atomics.
//
// Bounds: every clip read is at an index < lim = min(clamp(len, 0, in_len),
// out_len) <= in_len <= in_stride; every store is at j < out_len of row < rows.
#include <cmath>

#include "wk_kernels.h"
#include "wk_philox.h"
#include "wk_status.h"

namespace wk {
namespace {

constexpr int kAugThreads = 1024;
static_assert(WK_AUG_MAX_LEN % 4 == 0 && 2 * WK_AUG_MAX_LEN * 4 + 1024 <= 160 * 1024, "b and z of one row fit one CU's LDS");

struct AugVariant {
  float speed, volume;
  int32_t m;     // (int)((double)out_len * speed): the resampled length
  float scale;   // (float)out_len / (float)m
};

struct AugArgs {
  const void* audio;
  const int32_t* len;
  float* out;
  int64_t rows, in_stride;
  int32_t in_len, out_len, K;
  float pad_noise, snr_noise, snr_lo, snr_hi;
  uint2 key;
  uint32_t epoch;
  AugVariant var[WK_AUG_MAX_VARIANTS];
};

// The build fuses a * b + c in the backend (-ffp-contract=fast), whatever the source says.  The interpolation's
// source position and blend, and the SNR stage's sum, round every operation on its own, as the host's wk_augment and
// the reference's torch lines do (a fused src moves by an ulp of ~4000, i.e. the weights by 2e-4): such a product
// passes through an empty asm statement, which the fusion cannot see through.
__device__ __forceinline__ float rounded(float v) {
  asm("" : "+v"(v));
  return v;
}

// The two Gaussians of a word pair: rho cos(2 pi u2), rho sin(2 pi u2).
__device__ __forceinline__ float2 gauss_pair(uint32_t wa, uint32_t wb) {
  const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f, u2 = (float)(wb >> 8) * 0x1p-24f;   // (exact: 24-bit integers)
  const float rho = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  return make_float2(rho * c, rho * s);
}

// The key goes through a vector register: its ten round keys are then two adds per round in the vector unit, not
// twenty scalar registers held over the whole row loop (which, with the library functions' constants, no longer fit).
__device__ __forceinline__ uint4 aug_words(const AugArgs& p, uint32_t q, uint32_t row, uint32_t stream) {
  uint2 key = p.key;
  asm volatile("" : "+v"(key.x), "+v"(key.y));
  return philox4x32_10(make_uint4(q, row, p.epoch, stream), key);
}

// Samples 4q..4q+3 of a stream.
__device__ __forceinline__ void gauss4(const AugArgs& p, uint32_t q, uint32_t row, uint32_t stream, float g[4]) {
  const uint4 w = aug_words(p, q, row, stream);
  const float2 a = gauss_pair(w.x, w.y), b = gauss_pair(w.z, w.w);
  g[0] = a.x, g[1] = a.y, g[2] = b.x, g[3] = b.y;
}

// The pair that holds sample j of a stream (samples j & ~1 and j | 1).
__device__ __forceinline__ float2 gauss_pair_at(const AugArgs& p, uint32_t j, uint32_t row, uint32_t stream) {
  const uint4 w = aug_words(p, j >> 2, row, stream);
  return (j & 2u) ? gauss_pair(w.z, w.w) : gauss_pair(w.x, w.y);
}

template <bool I16>
__device__ __forceinline__ float clip_sample(const void* x, int32_t j) {
  if (I16) return (float)static_cast<const int16_t*>(x)[j] * (1.0f / 32768.0f);
  return static_cast<const float*>(x)[j];
}

// Four adjacent clip samples j0..j0+3, all below lim: one 16-byte (8-byte for int16) load where the address allows.
template <bool I16>
__device__ __forceinline__ void clip_sample4(const void* x, int32_t j0, float v[4]) {
  if (I16) {
    const int16_t* s = static_cast<const int16_t*>(x) + j0;
    if (((uintptr_t)s & 7) == 0) {
      const short4 t = *reinterpret_cast<const short4*>(s);
      v[0] = (float)t.x * (1.0f / 32768.0f), v[1] = (float)t.y * (1.0f / 32768.0f);
      v[2] = (float)t.z * (1.0f / 32768.0f), v[3] = (float)t.w * (1.0f / 32768.0f);
      return;
    }
  } else {
    const float* s = static_cast<const float*>(x) + j0;
    if (((uintptr_t)s & 15) == 0) {
      const float4 t = *reinterpret_cast<const float4*>(s);
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = clip_sample<I16>(x, j0 + e);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// One row's facts, uniform over the workgroup.
struct AugRow {
  const void* x;       // the clip
  uint32_t r, clip;    // the Philox rows of streams 1-3 and of stream 0
  int32_t lim;         // a[j] is the clip below lim = min(len, out_len), the pad from there
  AugVariant var;
};

// Steps 1-3 for samples 4q..4q+3 (4q < out_len; entries at or beyond out_len are made but never used).
template <bool I16>
__device__ __forceinline__ void augment4(const AugArgs& p, const AugRow& w, int32_t q, float b[4]) {
  const int32_t j0 = 4 * q, n_out = p.out_len;
  const bool pad_on = p.pad_noise > 0.0f;
  float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (w.var.speed == 1.0f) {
    if (j0 + 3 < w.lim) {
      clip_sample4<I16>(w.x, j0, b);
    } else {
      if (pad_on) gauss4(p, (uint32_t)q, w.clip, 0u, g);
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = j0 + e < w.lim ? clip_sample<I16>(w.x, j0 + e) : p.pad_noise * g[e];
    }
  } else {
    b[0] = b[1] = b[2] = b[3] = 0.0f;
    if (pad_on && j0 + 3 >= w.var.m) gauss4(p, (uint32_t)q, w.r, 1u, g);   // the pad behind the resampled clip
    // (kept as a loop: one copy of the interpolation and its two generators)
#pragma unroll 1
    for (int e = 0; e < 4; ++e) {
      float val;
      const int32_t j = j0 + e;
      if (j >= w.var.m) {
        val = p.pad_noise * (e == 0 ? g[0] : e == 1 ? g[1] : e == 2 ? g[2] : g[3]);
      } else {
      // F.interpolate(mode='linear', align_corners=False), every operation rounded on its own (as wk_augment)
      float src = rounded(w.var.scale * ((float)j + 0.5f)) - 0.5f;
      src = src < 0.0f ? 0.0f : src;
      int32_t i0 = (int32_t)src;
      i0 = i0 < n_out - 1 ? i0 : n_out - 1;   // (never taken for a valid m; keeps the reads in bounds by construction)
      const int32_t i1 = i0 + (i0 < n_out - 1 ? 1 : 0);
      const float l1 = src - (float)i0, l0 = 1.0f - l1;
      float a0 = i0 < w.lim ? clip_sample<I16>(w.x, i0) : 0.0f;
      float a1 = i1 < w.lim ? clip_sample<I16>(w.x, i1) : 0.0f;
      if (pad_on && i1 >= w.lim) {   // a pad sample: made again from its address
        const float2 g1 = gauss_pair_at(p, (uint32_t)i1, w.clip, 0u);
        a1 = p.pad_noise * ((i1 & 1) ? g1.y : g1.x);
        if (i0 >= w.lim) {
          const float2 g0 = (i0 >> 1) == (i1 >> 1) ? g1 : gauss_pair_at(p, (uint32_t)i0, w.clip, 0u);
          a0 = p.pad_noise * ((i0 & 1) ? g0.y : g0.x);
        }
      }
      val = rounded(l0 * a0) + rounded(l1 * a1);
      }
      b[0] = e == 0 ? val : b[0], b[1] = e == 1 ? val : b[1], b[2] = e == 2 ? val : b[2], b[3] = e == 3 ? val : b[3];
    }
  }
  if (w.var.volume != 1.0f) {
#pragma unroll
    for (int e = 0; e < 4; ++e) b[e] = fminf(1.0f, fmaxf(-1.0f, b[e] * w.var.volume));
  }
}

__device__ __forceinline__ void store4(float* o, int32_t j0, int32_t n_out, bool vec, const float v[4]) {
  if (vec) {
    *reinterpret_cast<float4*>(o + j0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j0 + e < n_out) o[j0 + e] = v[e];
  }
}

// SNR = false is the kernel of snr_noise == 0: the same row loop without the row's LDS, so that two workgroups
// share a CU and twice the loads are in flight (the stream is bound by those).
template <bool I16, bool SNR>
__global__ __launch_bounds__(kAugThreads) void augment_kernel(const AugArgs p) {
  // The SNR stage's row: b and z wait here for the two powers.  A thread reads back only what it wrote.
  constexpr int kRowBlocks = SNR ? WK_AUG_MAX_LEN / 4 : 1;
  __shared__ float4 s_b[kRowBlocks], s_z[kRowBlocks];
  __shared__ float s_part[2][kAugThreads / 64];
  __shared__ float s_gain;
  __shared__ AugVariant s_var[WK_AUG_MAX_VARIANTS];   // (indexed per row: from LDS, not from 64 scalar registers)
  const int tid = threadIdx.x;
  if (tid < p.K) s_var[tid] = p.var[tid];
  __syncthreads();
  const int32_t n_out = p.out_len, n_q = (n_out + 3) >> 2;
  const bool vec_out = (n_out & 3) == 0 && ((uintptr_t)p.out & 15) == 0;
  for (int64_t row = blockIdx.x; row < p.rows; row += gridDim.x) {
    const int64_t clip = row / p.K;
    AugRow w;
    w.var = s_var[(int)(row - clip * p.K)];
    w.r = (uint32_t)row, w.clip = (uint32_t)clip;
    w.x = static_cast<const char*>(p.audio) + clip * p.in_stride * (I16 ? 2 : 4);
    int32_t len = p.len ? p.len[clip] : p.in_len;
    len = len < 0 ? 0 : (len > p.in_len ? p.in_len : len);   // (a device value: clamped, never trusted)
    w.lim = len < n_out ? len : n_out;
    float* o = p.out + row * (int64_t)n_out;

    int32_t q_first = tid;
    if (!SNR && w.var.speed == 1.0f) {
      // A plain row (the clip itself, or a volume variant) is a copy, and the stream is bound by the loads in flight
      // (DESIGN 5.14): the blocks that lie wholly inside the clip go four at a time, a thread's four loads issued
      // before its first store.  The boundary block and the pad are left to the loop below.
      const int32_t n_full = w.lim >> 2;   // blocks q < n_full: 4q + 3 < lim
#pragma unroll 1
      for (int32_t q0 = tid; q0 < n_full; q0 += 4 * kAugThreads) {
        float b[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (q0 + k * kAugThreads < n_full) clip_sample4<I16>(w.x, 4 * (q0 + k * kAugThreads), b[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int32_t q = q0 + k * kAugThreads;
          if (q < n_full) {
            if (w.var.volume != 1.0f) {
#pragma unroll
              for (int e = 0; e < 4; ++e) b[k][e] = fminf(1.0f, fmaxf(-1.0f, b[k][e] * w.var.volume));
            }
            store4(o, 4 * q, n_out, vec_out, b[k]);
          }
        }
      }
      q_first = n_full + tid;
    }

    float ps = 0.0f, pn = 0.0f;
#pragma unroll 1
    for (int32_t q = q_first; q < n_q; q += kAugThreads) {
      float b[4];
      augment4<I16>(p, w, q, b);
      if (!SNR) {   // a stream: read, blend, write
        store4(o, 4 * q, n_out, vec_out, b);
        continue;
      }
      float g[4], z[4];
      gauss4(p, (uint32_t)q, w.r, 2u, g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        z[e] = p.snr_noise * g[e];
        if (4 * q + e < n_out) {   // (the last block's tail is not part of the row)
          ps += b[e] * b[e];
          pn += z[e] * z[e];
        }
      }
      s_b[q] = make_float4(b[0], b[1], b[2], b[3]);
      s_z[q] = make_float4(z[0], z[1], z[2], z[3]);
    }
    if (!SNR) continue;
    ps = wave_sum(ps);
    pn = wave_sum(pn);
    if ((tid & 63) == 0) s_part[0][tid >> 6] = ps, s_part[1][tid >> 6] = pn;
    __syncthreads();
    if (tid == 0) {
      float sp = 0.0f, sn = 0.0f;
      for (int k = 0; k < kAugThreads / 64; ++k) sp += s_part[0][k], sn += s_part[1][k];
      const float Ps = sp / (float)n_out, Pn = sn / (float)n_out;
      const float u = (float)(aug_words(p, 0u, w.r, 3u).x >> 8) * 0x1p-24f;
      const float snr_db = p.snr_lo + u * (p.snr_hi - p.snr_lo);
      const float snr = exp10f(snr_db / 20.0f);
      s_gain = Pn > 0.0f ? sqrtf(Ps / (Pn * snr)) : 1.0f;
    }
    __syncthreads();   // (the next row's s_part writes come after every thread has passed this barrier)
    const float gain = s_gain;
#pragma unroll 1
    for (int32_t q = tid; q < n_q; q += kAugThreads) {
      const float4 b = s_b[q], z = s_z[q];
      const float v[4] = {fminf(1.0f, fmaxf(-1.0f, b.x + rounded(z.x * gain))),
                          fminf(1.0f, fmaxf(-1.0f, b.y + rounded(z.y * gain))),
                          fminf(1.0f, fmaxf(-1.0f, b.z + rounded(z.z * gain))),
                          fminf(1.0f, fmaxf(-1.0f, b.w + rounded(z.w * gain)))};
      store4(o, 4 * q, n_out, vec_out, v);
    }
  }
}

bool finite_pos(float v) { return std::isfinite(v) && v > 0.0f; }
bool finite_nonneg(float v) { return std::isfinite(v) && v >= 0.0f; }

}  // namespace
}  // namespace wk

extern "C" wk_status wk_augment_batch(const void* d_audio, int32_t dtype, const int32_t* d_len_or_null, int64_t n,
                                      int32_t in_len, int64_t in_stride, const wk_aug_variant* variants,
                                      int32_t n_variants, const wk_aug_spec* spec, int32_t out_len, float* d_out,
                                      void* stream) {
  using wk::invalid;
  if (!d_audio || !d_out || !variants || !spec) return invalid("wk_augment_batch: null pointer");
  if (dtype != WK_DTYPE_F32 && dtype != WK_DTYPE_I16) return invalid("wk_augment_batch: bad dtype");
  if (n < 0 || in_len < 0 || in_stride < in_len) return invalid("wk_augment_batch: bad n, in_len or in_stride");
  if (n_variants < 1 || n_variants > WK_AUG_MAX_VARIANTS) return invalid("wk_augment_batch: n_variants outside [1, 16]");
  if (out_len < 1 || out_len > WK_AUG_MAX_LEN) return invalid("wk_augment_batch: out_len outside [1, WK_AUG_MAX_LEN]");
  if (!wk::finite_nonneg(spec->pad_noise) || !wk::finite_nonneg(spec->snr_noise))
    return invalid("wk_augment_batch: negative or non-finite noise level");
  if (!std::isfinite(spec->snr_lo_db) || !std::isfinite(spec->snr_hi_db) || spec->snr_lo_db > spec->snr_hi_db)
    return invalid("wk_augment_batch: bad snr range");
  if (n >= ((int64_t)1 << 32) / n_variants + (((int64_t)1 << 32) % n_variants != 0))
    return invalid("wk_augment_batch: n * n_variants must be below 2^32");
  wk::AugArgs a{};
  for (int v = 0; v < n_variants; ++v) {
    const float speed = variants[v].speed, volume = variants[v].volume;
    if (!wk::finite_pos(speed) || !wk::finite_pos(volume)) return invalid("wk_augment_batch: speed and volume must be positive and finite");
    const double md = (double)out_len * (double)speed;   // (range-checked before the cast)
    if (!(md >= 1.0) || !(md < 2147483648.0)) return invalid("wk_augment_batch: int(out_len * speed) outside [1, 2^31)");
    const int32_t m = (int32_t)md;
    a.var[v] = {speed, volume, m, (float)out_len / (float)m};
  }
  if (n == 0) return WK_OK;
  a.audio = d_audio, a.len = d_len_or_null, a.out = d_out;
  a.rows = n * n_variants, a.in_stride = in_stride;
  a.in_len = in_len, a.out_len = out_len, a.K = n_variants;
  a.pad_noise = spec->pad_noise, a.snr_noise = spec->snr_noise, a.snr_lo = spec->snr_lo_db, a.snr_hi = spec->snr_hi_db;
  a.key = make_uint2((uint32_t)spec->seed, (uint32_t)(spec->seed >> 32));
  a.epoch = spec->epoch;
  const unsigned grid = (unsigned)(a.rows < (1 << 20) ? a.rows : (1 << 20));   // (rows beyond it: the kernel's row loop)
  const bool i16 = dtype == WK_DTYPE_I16, snr = a.snr_noise > 0.0f;
  auto kernel = i16 ? (snr ? wk::augment_kernel<true, true> : wk::augment_kernel<true, false>)
                    : (snr ? wk::augment_kernel<false, true> : wk::augment_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(wk::kAugThreads), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? WK_OK : wk::hip_fail(e, "augment launch");
}
