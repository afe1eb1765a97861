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
#include "wk_direct_dev.h"
#include "wk_quant_rule.h"

namespace wk {
namespace {

constexpr int kNT = WK_QUANT_TENSORS, kNB = WK_QUANT_BINS;

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

}  // namespace

size_t calibrate_workspace_bytes(int64_t batch) {
  const int64_t grid = batch < kCalibGridCap ? batch : kCalibGridCap;
  return kCalibTotalsBytes + sizeof(float) * kDirectFwdPacked + sizeof(uint32_t) * kCalibSlot * (size_t)grid;
}

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

}  // namespace wk
