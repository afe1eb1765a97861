// wk_quant.hip -- calibration of the int8 network's activation exponents
// (ml_models/main.py:71-129, quantize_model_esp: esp-ppq observes the float
// network on calibration clips and picks a power-of-2 scale per tensor).
//
// wk_calib_kernel: one fp32 forward of the xiaoa CNN per clip, convolutions in
// direct form on v_mfma_f32_16x16x4f32 (the observed values are defined as the
// direct convolution's, not the inference path's Winograd): the forward of
// wk_direct_dev.h, which the training step runs too.  One workgroup of 8 waves
// walks clips wg, wg + grid, ...; a clip's activations stay in LDS ([t + 1][ci]
// images with zero guard rows), every pre-pool value of a layer is in an
// accumulator of exactly one lane.  Seven tensors are observed per clip
// (kCalibPerClip): the input (13 x 63), conv1 / conv2 / conv3 after ReLU and
// before the pool (32 x 63, 64 x 31, 128 x 15), GAP (128), classifier.0 after
// ReLU (64), the logit (1).  The MFMA tiles cover 64 / 32 / 16 columns: the
// lanes of columns t = 63, 31, 15 hold padding and count nothing, and the guard
// rows are never read as values.
//
// A power-of-2 quantiser needs no sort for a percentile: |x| goes to the bin of
// the smallest exponent that holds it, b = min{e : |x| <= 127 * 2^e}, read off
// the float's bits (hold_exp, wk_quant_rule.h: the rule the host applies to the
// weights).  32 bins per tensor, e in [-24, 7], clamped (zeros lowest).
//
// Counting.  The values of one tensor fall into a handful of bins, so a plain
// ds_add per lane would serialise on a few addresses.  Each wave instead peels
// its distinct bins: the first uncounted lane's bin is broadcast, a ballot finds
// every lane in that bin, and one lane adds the population count to the
// workgroup's LDS counter -- one LDS atomic per distinct bin per value-row of a
// wave (3 to 6 here), no same-address conflicts inside a wave, and one set of
// 224 counters per workgroup rather than per wave.  Maxima are unsigned maxima
// of the bit patterns, kept per lane in registers and merged once at the end.
// Each workgroup writes its counters once to its own slot of the workspace;
// wk_calib_sum_kernel adds the slots into 64-bit totals.  No floating-point
// atomics and no global atomics: integer sums, identical between calls.
//
// The C entry points of the int8 spec (wk_quant_spec_default, wk_set_quant,
// wk_get_quant, wk_quant_weights) and of calibration, with its host step (the
// percentile read off the totals), are at the end of this file.
#include <math.h>

#include "wk_direct_dev.h"
#include "wk_handle.h"
#include "wk_quant_rule.h"

namespace wk {
namespace {

constexpr int kNT = WK_QUANT_TENSORS, kNB = WK_QUANT_BINS;

// Workspace: the 64-bit totals ([7][32] counts, then the 7 maxima as bit patterns of |x|), fragment-major
// forward weights, then one slot of kCalibSlot 32-bit words per workgroup (7 x 32 counts, 7 maxima).
// Workgroup g walks clips g, g + grid, ...; grid = min(batch, kCalibGridCap).
constexpr int kCalibTotals = kNT * kNB + kNT;
constexpr int kCalibSlot = kNT * kNB + 8;
constexpr int kCalibGridCap = 512;
constexpr size_t kCalibTotalsBytes = (kCalibTotals * 8 + 255) & ~(size_t)255;

// Count one value per lane into the tensor's 32 LDS counters; idx < 0: this
// lane has no value.  Every lane of the wave must call it together.
__device__ __forceinline__ void wave_count(unsigned* cnt, int idx, int lane) {
  unsigned long long todo = __ballot(idx >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int b = __shfl(idx, leader, 64);
    const unsigned long long same = __ballot(idx == b);
    if (lane == leader) atomicAdd(&cnt[b], (unsigned)__popcll(same));
    todo &= ~same;
  }
}

__device__ __forceinline__ void observe(unsigned* cnt, unsigned& mx, float v, bool valid, int lane) {
  if (valid) mx = max(mx, __float_as_uint(v) & 0x7FFFFFFFu);
  wave_count(cnt, valid ? hold_exp(v) + 24 : -1, lane);   // bin 0..31 = exponent -24..7
}

// conv_layer_tile's epilogue: ReLU, observe the tile's pre-pool values (columns
// t >= TV are tile padding), maxpool(2) into the next image (TN pooled steps).
template <int TV, int TN>
__device__ __forceinline__ void epi_observe_pool(const f32x4& acc, unsigned* cnt, unsigned& mx, float* prow, int t,
                                                 int lane) {
  float pv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float y = fmaxf(acc[r], 0.0f);
    observe(cnt, mx, y, t < TV, lane);
    pv[r] = fmaxf(y, swap_adjacent(y));
  }
  if (!(lane & 1) && (t >> 1) < TN) *reinterpret_cast<float4*>(prow) = make_float4(pv[0], pv[1], pv[2], pv[3]);
}

__global__ __launch_bounds__(kDirectBlock) void wk_calib_kernel(const float* __restrict__ feats, int64_t batch,
                                                                const float* __restrict__ w, const float* __restrict__ pk,
                                                                unsigned* __restrict__ slots) {
  __shared__ __attribute__((aligned(16))) float sm[kDirectLdsFloats];
  __shared__ unsigned cnt[kCalibSlot];   // [7][32] counts, then the 7 maxima
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int i = tid; i < kCalibSlot; i += kDirectBlock) cnt[i] = 0u;
  float f1[16];
  direct_setup<kDirectLdsFloats>(sm, w, tid, f1);
  unsigned mx[kNT];
#pragma unroll
  for (int k = 0; k < kNT; ++k) mx[k] = 0u;
  // observed tensor L = conv layer L after ReLU, before the pool
  auto observe_pool = [&mx](auto layer, const f32x4& acc, int t, int /*c0*/, int l, float* prow) {
    constexpr int L = decltype(layer)::value;
    epi_observe_pool<kConvSteps[L - 1], kConvSteps[L]>(acc, cnt + L * kNB, mx[L], prow, t, l);
  };

  for (int64_t clip = blockIdx.x; clip < batch; clip += gridDim.x) {
    // ---- input: [13][63] -> X[t + 1][ci]
    const float* x = feats + clip * (13 * 63);
#pragma unroll
    for (int base = 0; base < 13 * 63; base += kDirectBlock) {
      const int i = base + tid;
      const bool ok = i < 13 * 63;
      const float v = ok ? x[i] : 0.0f;
      if (ok) {
        const int ci = i / 63, t = i - 63 * ci;
        sm[sX + (t + 1) * kXP + ci] = v;
      }
      observe(cnt + 0 * kNB, mx[0], v, ok, lane);
    }
    const float* pkc = per_clip_base(pk);
    __syncthreads();
    // ---- conv1, conv2, conv3: one tile per wave
    conv_layer_tile<1>(pkc, sm, wave, lane, observe_pool);
    __syncthreads();
    conv_layer_tile<2>(pkc, sm, wave, lane, observe_pool);
    __syncthreads();
    conv_layer_tile<3>(pkc, sm, wave, lane, observe_pool);
    __syncthreads();
    // ---- mean over the 7 pooled steps (waves 0 and 1)
    if (wave < 2) observe(cnt + 4 * kNB, mx[4], gap_channel(sm, tid), true, lane);
    __syncthreads();
    // ---- classifier.0 + ReLU (g: the G values read, which only the trainer uses)
    float g[16];
    classifier0(sm, tid, f1, g);
    __syncthreads();
    // ---- classifier.2 (wave 0).  The next clip's writes to sH come five barriers later.
    if (wave == 0) {
      float hv;
      const float z = classifier2(sm, lane, hv);
      observe(cnt + 5 * kNB, mx[5], hv, true, lane);
      observe(cnt + 6 * kNB, mx[6], z, lane == 0, lane);
    }
  }

  // ---- this workgroup's slot
#pragma unroll
  for (int k = 0; k < kNT; ++k) atomicMax(&cnt[kNT * kNB + k], mx[k]);
  __syncthreads();
  for (int i = tid; i < kCalibSlot; i += kDirectBlock) slots[(size_t)blockIdx.x * kCalibSlot + i] = cnt[i];
}

// Totals: element i of every slot, summed (counts) or maximised (the 7 bit patterns) in 64 bits.
__global__ void wk_calib_sum_kernel(const unsigned* __restrict__ slots, int nslots, unsigned long long* __restrict__ tot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kCalibTotals) return;
  unsigned long long v = 0;
  if (i < kNT * kNB) {
    for (int p = 0; p < nslots; ++p) v += slots[(size_t)p * kCalibSlot + i];
  } else {
    for (int p = 0; p < nslots; ++p) {
      const unsigned long long m = slots[(size_t)p * kCalibSlot + i];
      v = m > v ? m : v;
    }
  }
  tot[i] = v;
}

size_t calibrate_workspace_bytes(int64_t batch) {
  const int64_t grid = batch < kCalibGridCap ? batch : kCalibGridCap;
  return kCalibTotalsBytes + sizeof(float) * kDirectFwdPacked + sizeof(uint32_t) * kCalibSlot * (size_t)grid;
}

// Queues the pack, count and sum kernels; the totals are at the start of the workspace afterwards.
hipError_t launch_calibrate(const float* w, const float* feats, int64_t batch, void* workspace, hipStream_t stream) {
  unsigned long long* tot = (unsigned long long*)workspace;
  float* pk = (float*)((char*)workspace + kCalibTotalsBytes);
  unsigned* slots = (unsigned*)(pk + kDirectFwdPacked);
  const int grid = (int)(batch < kCalibGridCap ? batch : kCalibGridCap);
  const hipError_t e = launch_pack_direct(w, pk, kDirectFwdPacked, stream);
  if (e != hipSuccess) return e;
  wk_calib_kernel<<<grid, kDirectBlock, 0, stream>>>(feats, batch, w, pk, slots);
  wk_calib_sum_kernel<<<1, 256, 0, stream>>>(slots, grid, tot);
  return hipGetLastError();
}

}  // namespace
}  // namespace wk

using wk::hip_fail;
using wk::invalid;
using wk::on_device;

// ---------------------------------------------------------------------------
// Post-training int8 quantisation: the spec, and calibration's host step.
// ---------------------------------------------------------------------------
extern "C" {

wk_status wk_quant_spec_default(wk_quant_spec* out) {
  if (!out) return invalid("wk_quant_spec_default: null out");
  *out = wk_quant_spec{-4, {-8, -9, -9, -9, -9}, {-5, -5, -4, -5, -4, -3}};
  return WK_OK;
}

wk_status wk_set_quant(wk_handle* h, const wk_quant_spec* spec) {
  if (!spec) return invalid("wk_set_quant: null spec");
  wk::Int8Params p;
  if (const char* why = wk::int8_params(*spec, &p)) return invalid(why);
  if (!h) return invalid("wk_set_quant: null handle");
  if (h->cfg.precision != WK_PREC_INT8 || !h->d_int8) return invalid("wk_set_quant: not a WK_PREC_INT8 handle with weights");
  std::vector<int8_t> q(wk::kNumInt8Weights);
  wk::quantize_int8_weights(h->h_w.data(), spec->e_w, q.data());
  return on_device(h->cfg.device, [&]() -> wk_status {
    // launches already queued (on any stream) still read the old bytes: drain them first
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "wk_set_quant: sync");
    if ((e = hipMemcpy(h->d_int8, q.data(), q.size(), hipMemcpyHostToDevice)) != hipSuccess)
      return hip_fail(e, "wk_set_quant: hipMemcpy(int8 weights)");
    h->quant = *spec;
    h->qp = p;
    return WK_OK;
  });
}

wk_status wk_get_quant(wk_handle* h, wk_quant_spec* out) {
  if (!h || !out) return invalid("wk_get_quant: null argument");
  if (h->cfg.precision != WK_PREC_INT8) return invalid("wk_get_quant: not a WK_PREC_INT8 handle");
  *out = h->quant;
  return WK_OK;
}

wk_status wk_quant_weights(const float* host_weights, const wk_quant_spec* spec, int8_t* out) {
  if (!host_weights || !spec || !out) return invalid("wk_quant_weights: null argument");
  for (int i = 0; i < 5; ++i)
    if (spec->e_w[i] < -32 || spec->e_w[i] > 32) return invalid("wk_quant_weights: weight exponent outside [-32, 32]");
  wk::quantize_int8_weights(host_weights, spec->e_w, out);
  return WK_OK;
}

wk_status wk_calibrate_workspace_bytes(int64_t batch, size_t* bytes) {
  if (!bytes) return invalid("wk_calibrate_workspace_bytes: null bytes");
  *bytes = 0;
  if (batch < 1) return invalid("wk_calibrate_workspace_bytes: batch < 1");
  *bytes = wk::calibrate_workspace_bytes(batch);
  return WK_OK;
}

wk_status wk_calibrate(wk_handle* h, const float* d_feats, int64_t batch, double percentile, int32_t pin_e_in,
                       void* d_workspace, size_t workspace_bytes, wk_quant_spec* out, wk_calib_stats* stats_or_null,
                       void* stream) {
  if (!h) return invalid("wk_calibrate: null handle");
  if (!h->d_weights) return invalid("wk_calibrate: handle created without weights");
  if (!d_feats || !out || batch < 1) return invalid("wk_calibrate: null pointer or batch < 1");
  if (!(percentile > 0.0)) return invalid("wk_calibrate: percentile must be > 0");
  if (pin_e_in != WK_QUANT_CALIBRATE_INPUT && (pin_e_in < -32 || pin_e_in > 32))
    return invalid("wk_calibrate: pinned input exponent outside [-32, 32]");
  if (!d_workspace || ((uintptr_t)d_workspace & 255) || workspace_bytes < wk::calibrate_workspace_bytes(batch))
    return invalid("wk_calibrate: workspace null, not 256-byte aligned or below wk_calibrate_workspace_bytes");
  unsigned long long tot[wk::kCalibTotals];
  const wk_status st = on_device(h->cfg.device, [&]() -> wk_status {
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = wk::launch_calibrate(h->d_weights, d_feats, batch, d_workspace, s);
    if (e != hipSuccess) return hip_fail(e, "calibrate launch");
    if ((e = hipMemcpyAsync(tot, d_workspace, sizeof(tot), hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
      return hip_fail(e, "wk_calibrate: read back");
    return WK_OK;
  });
  if (st != WK_OK) return st;
  int e_t[WK_QUANT_TENSORS];
  for (int t = 0; t < WK_QUANT_TENSORS; ++t) {
    const unsigned long long* c = tot + t * WK_QUANT_BINS;
    const int64_t n = wk::kCalibPerClip[t] * batch;
    // the smallest bin whose cumulative count reaches k = ceil(percentile / 100 * n); >= 100: the maximum's bin
    int64_t k = percentile >= 100.0 ? n : (int64_t)ceil(percentile / 100.0 * (double)n);
    k = k < 1 ? 1 : (k > n ? n : k);
    int64_t cum = 0;
    int b = 0;
    for (; b < WK_QUANT_BINS - 1; ++b)
      if ((cum += (int64_t)c[b]) >= k) break;
    e_t[t] = b - 24;
    if (stats_or_null) {
      for (int i = 0; i < WK_QUANT_BINS; ++i) stats_or_null->counts[t][i] = (int64_t)c[i];
      const uint32_t mb = (uint32_t)tot[WK_QUANT_TENSORS * WK_QUANT_BINS + t];
      memcpy(&stats_or_null->max_abs[t], &mb, 4);
    }
  }
  if (stats_or_null) stats_or_null->n_clips = batch;
  out->e_in = pin_e_in != WK_QUANT_CALIBRATE_INPUT ? pin_e_in : e_t[0];
  for (int i = 0; i < 6; ++i) out->e_act[i] = e_t[1 + i];
  static const int off[6] = {wk::kOffW1, wk::kOffW2, wk::kOffW3, wk::kOffF1, wk::kOffF2, wk::kNumWeights};
  for (int i = 0; i < 5; ++i) {
    float m = 0.0f;
    for (int j = off[i]; j < off[i + 1]; ++j) m = fmaxf(m, fabsf(h->h_w[j]));
    out->e_w[i] = wk::hold_exp(m);
  }
  return WK_OK;
}

}  // extern "C"
