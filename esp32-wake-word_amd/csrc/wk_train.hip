// wk_train.hip -- one training step of the xiaoa CNN (LightweightKWS,
// ml_models/src/wakeModel.py:4-34, num_classes = 1) as the reference's
// train_model runs it (ml_models/main.py:13-64): forward, BCE-with-logits,
// backward to the five weight tensors, AdamW.  fp32 throughout.
//
// wk_train_grad_kernel: one workgroup of 8 waves walks its clips (clip = wg,
// wg + grid, ...) one at a time.  A clip's activations never leave LDS:
//   X  [t+1][ci]  the input, transposed, one zero row of conv padding each side
//   P1 [t+1][ci]  pooled conv1 output (31 x 32), P2 likewise (15 x 64)
//   R1/R2/R3 [t+1][co]  per pre-pool position: 1 where the pool pair's gradient
//       goes (the larger element, the first on a tie, none if the maximum is
//       <= 0: ReLU), else 0; the backward pass multiplies the pooled gradient in,
//       so the same buffer then holds dY, the pre-activation gradient.
// Each convolution is three implicit GEMMs on v_mfma_f32_16x16x4f32 (direct
// form, not the forward path's Winograd: the pool decision needs the very
// pre-activations torch compares):
//   forward  Y[co][t]   = sum_{tap,ci} W[co][ci][tap] P[t + tap - 1][ci]
//   data     dP[ci][t]  = sum_{tap,co} W[co][ci][tap] dY[t + 1 - tap][co]
//   weight   dW[co][ci][tap] += sum_t dY[t][co] P[t + tap - 1][ci]
// The weight-gradient tiles stay in the wave's accumulators over all clips of
// the workgroup (conv3: 12 tiles per wave, conv2: 3, conv1: 1 in waves 0-5)
// and are written once, to the workgroup's slot of the trainer's workspace;
// wk_train_reduce_kernel sums the slots in a fixed order (no atomics: two
// calls give the same bits).  HBM traffic per clip is the 3276 bytes of
// features, 4 of label and 4 of logit; the workspace costs 160 KB per
// workgroup per call, not per clip.
// The forward pass is wk_direct_dev.h's (calibration runs the same one); its A
// operands and the data pass's come from a fragment-major copy of the weights
// that wk_pack_direct_kernel rebuilds at the start of every call (the weights
// change every step): forward order and transposed (data-gradient) order.
#include "wk_direct_dev.h"

#include <math.h>

#include <memory>
#include <new>

#include "wk_devmem.h"

namespace wk {
namespace {

constexpr int kSlot = kNumWeights + 32;   // floats per workgroup slot: gradients, then the loss sum at [kNumWeights]

// fragment-major weights (floats): the forward A fragments (wk_direct_dev.h),
// then the data-gradient A fragments [ci tile][step][64], step = tap * COUT/4 +
// cb, lane l: ci = 16 tile + (l & 15), co = 4 cb + (l >> 4).
constexpr int kTbW2 = kDirectFwdPacked;         // [2][48][64]
constexpr int kTbW3 = kTbW2 + 2 * 48 * 64;      // [4][96][64]
constexpr int kTrainPacked = kTbW3 + 4 * 96 * 64;

// LDS map (floats): the forward's images, then the backward pass's.
constexpr int sR1 = kDirectLdsFloats;        // [66][36]
constexpr int sR2 = sR1 + 66 * kP1P;         // [34][68]
constexpr int sR3 = sR2 + 34 * kP2P;         // [18][132]
constexpr int sD2 = sR3 + 18 * kP3P;         // [16][68]   first K half of dP2
constexpr int sD1 = sD2 + 16 * kP2P;         // [32][36]   first K half of dP1
constexpr int sDG = sD1 + 32 * kP1P;         // [4][128]   dG partial sums
constexpr int kLdsFloats = sDG + 512;
static_assert(kLdsFloats * 4 <= 64 * 1024, "static LDS limit");

// The first n floats of the fragment-major copy: kDirectFwdPacked (forward
// order only) or kTrainPacked.
__global__ void wk_pack_direct_kernel(const float* __restrict__ w, float* __restrict__ pk, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int base, cin, cout, inner;   // inner: channels of the K dimension (padded)
  bool fwd;
  int wbase;
  if (i < kDfW2) { base = kDfW1; cin = 13; cout = 32; inner = 16; fwd = true; wbase = kOffW1; }
  else if (i < kDfW3) { base = kDfW2; cin = 32; cout = 64; inner = 32; fwd = true; wbase = kOffW2; }
  else if (i < kTbW2) { base = kDfW3; cin = 64; cout = 128; inner = 64; fwd = true; wbase = kOffW3; }
  else if (i < kTbW3) { base = kTbW2; cin = 32; cout = 64; inner = 64; fwd = false; wbase = kOffW2; }
  else { base = kTbW3; cin = 64; cout = 128; inner = 128; fwd = false; wbase = kOffW3; }
  const int j = i - base, l = j & 63, ns = 3 * inner / 4;
  const int s = (j >> 6) % ns, tile = (j >> 6) / ns, tap = s / (inner / 4), cb = s % (inner / 4);
  const int a = 16 * tile + (l & 15), b = 4 * cb + (l >> 4);
  const int co = fwd ? a : b, ci = fwd ? b : a;
  pk[i] = (ci < cin && co < cout) ? w[wbase + (co * cin + ci) * 3 + tap] : 0.0f;
}

// conv_layer_tile's epilogue: maxpool(2) + ReLU of a forward tile, the route
// flags of its 16 positions and the pooled values.  Lane l holds
// y[co0 .. co0 + 3][t]; the pool partner t ^ 1 is lane l ^ 1.  TN = pooled
// steps (the floor pool drops the rest).
template <int TN>
__device__ __forceinline__ void epi_route_pool(const f32x4& acc, float* rrow, float* prow, int t, int lane) {
  const bool odd = lane & 1;
  const bool valid = (t >> 1) < TN;
  float rv[4], pv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float y = acc[r], o = swap_adjacent(y);
    const float a = odd ? o : y, b = odd ? y : o;   // a: first of the pair
    const float m = fmaxf(a, b);
    const bool mine = odd ? (b > a) : (a >= b);
    rv[r] = (valid && m > 0.0f && mine) ? 1.0f : 0.0f;
    pv[r] = fmaxf(m, 0.0f);
  }
  *reinterpret_cast<float4*>(rrow) = make_float4(rv[0], rv[1], rv[2], rv[3]);
  if (!odd && valid) *reinterpret_cast<float4*>(prow) = make_float4(pv[0], pv[1], pv[2], pv[3]);
}

// Half of the K range of one data-gradient tile.  wb: the tile's fragments +
// lane; rr: the lane's B element at tap 0, cb 0 = R row ti + 2, column l >> 4.
template <int COUT, int PR>
__device__ __forceinline__ f32x4 dgrad_half(const float* __restrict__ wb, const float* rr, int kh) {
  constexpr int NS = 3 * COUT / 4, HALF = NS / 2, PER_TAP = COUT / 4;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 8
  for (int i = 0; i < HALF; ++i) {
    const int s = kh * HALF + i, tap = s / PER_TAP, cb = s % PER_TAP;
    acc = mfma4(wb[s * 64], rr[4 * cb - tap * PR], acc);
  }
  return acc;
}

// Second half of a data-gradient tile: add the first half (d, [ti][ci]) and
// multiply into the route flags of pre-pool rows 2 ti, 2 ti + 1 -> dY.
template <int PD, int PR>
__device__ __forceinline__ void dgrad_finish(const f32x4& acc, const float* d, float* R, int ti, int c0) {
  const float4 h = *reinterpret_cast<const float4*>(d + ti * PD + c0);
  const float4 tot = make_float4(h.x + acc[0], h.y + acc[1], h.z + acc[2], h.w + acc[3]);
#pragma unroll
  for (int k = 1; k <= 2; ++k) {
    float4* p = reinterpret_cast<float4*>(R + (2 * ti + k) * PR + c0);
    const float4 f = *p;
    *p = make_float4(f.x * tot.x, f.y * tot.y, f.z * tot.z, f.w * tot.w);
  }
}

__device__ __forceinline__ void store_dw_tile(const f32x4& acc, float* dst, int cin, int co0, int ci, int tap) {
  if (ci < cin) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[((co0 + r) * cin + ci) * 3 + tap] = acc[r];
  }
}

__global__ __launch_bounds__(kDirectBlock) void wk_train_grad_kernel(
    const float* __restrict__ feats, const float* __restrict__ labels, int64_t batch, const float* __restrict__ w,
    const float* __restrict__ pk, float* __restrict__ part, float* __restrict__ logits) {
  __shared__ __attribute__((aligned(16))) float sm[kLdsFloats];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 15, q = lane >> 4;
  const float inv_b = 1.0f / (float)batch;

  // classifier.0: thread (o, part) owns F1[o][16 part .. +16] and its gradient
  const int fo = tid >> 3, fpart = tid & 7;
  float f1[16], df1[16];
  direct_setup<kLdsFloats>(sm, w, tid, f1);
#pragma unroll
  for (int j = 0; j < 16; ++j) df1[j] = 0.0f;
  float df2 = 0.0f, loss = 0.0f;
  f32x4 dw3[12], dw2[3], dw1;
#pragma unroll
  for (int n = 0; n < 12; ++n) dw3[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int n = 0; n < 3; ++n) dw2[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  dw1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  auto route_pool = [](auto layer, const f32x4& acc, int t, int c0, int l, float* prow) {
    constexpr int L = decltype(layer)::value;
    constexpr int R = L == 1 ? sR1 : L == 2 ? sR2 : sR3, PITCH = L == 1 ? kP1P : L == 2 ? kP2P : kP3P;
    epi_route_pool<kConvSteps[L]>(acc, sm + R + (t + 1) * PITCH + c0, prow, t, l);
  };

  for (int64_t clip = blockIdx.x; clip < batch; clip += gridDim.x) {
    // ---- input: [13][63] -> X[t + 1][ci]
    const float* x = feats + clip * (13 * 63);
    for (int i = tid; i < 13 * 63; i += kDirectBlock) {
      const int ci = i / 63, t = i - 63 * ci;
      sm[sX + (t + 1) * kXP + ci] = x[i];
    }
    const float y = labels[clip];
    const float* pkc = per_clip_base(pk);
    __syncthreads();

    // ---- forward conv1, conv2, conv3: the route image of layer L is R_L[t + 1][co]
    conv_layer_tile<1>(pkc, sm, wave, lane, route_pool);
    __syncthreads();
    conv_layer_tile<2>(pkc, sm, wave, lane, route_pool);
    __syncthreads();
    conv_layer_tile<3>(pkc, sm, wave, lane, route_pool);
    __syncthreads();
    // ---- mean over the 7 pooled steps
    if (tid < 128) gap_channel(sm, tid);
    __syncthreads();
    // ---- classifier.0 + ReLU: 8 threads per output row
    float g[16];
    classifier0(sm, tid, f1, g);
    __syncthreads();
    // ---- classifier.2, loss, dz: every wave computes the same z
    float hv;
    const float z = classifier2(sm, lane, hv);
    const float dz = (1.0f / (1.0f + expf(-z)) - y) * inv_b;
    if (tid == 0) {
      loss += fmaxf(z, 0.0f) - z * y + log1pf(expf(-fabsf(z)));
      if (logits) logits[clip] = z;
    }
    if (wave == 0) df2 = fmaf(dz, hv, df2);
    {
      const float dh = sm[sH + fo] > 0.0f ? dz * sm[sF2 + fo] : 0.0f;
#pragma unroll
      for (int j = 0; j < 16; ++j) df1[j] = fmaf(dh, g[j], df1[j]);
      // dG[k] = sum_o F1[o][k] dh[o]: 4 partial sums of 16 rows each
      const int k = tid & 127, oq = tid >> 7;
      float s = 0.0f;
#pragma unroll
      for (int o = 16 * oq; o < 16 * oq + 16; ++o) {
        const float d = sm[sH + o] > 0.0f ? dz * sm[sF2 + o] : 0.0f;
        s = fmaf(w[kOffF1 + o * 128 + k], d, s);
      }
      sm[sDG + oq * 128 + k] = s;
    }
    __syncthreads();
    // ---- dY3 = route * dG / 7 (pre-pool rows 0..13)
    for (int i = tid; i < 14 * 128; i += kDirectBlock) {
      const int t = i >> 7, co = i & 127;
      const float dg = ((sm[sDG + co] + sm[sDG + 128 + co]) + (sm[sDG + 256 + co] + sm[sDG + 384 + co])) / 7.0f;
      sm[sR3 + (t + 1) * kP3P + co] *= dg;
    }
    __syncthreads();
    // ---- conv3 weight gradient (wave = co tile; 3 taps x 4 ci tiles) and the
    // first K half of dP2
    {
      const float* dy = sm + sR3 + (q + 1) * kP3P + 16 * wave + ln;
      const float* pin = sm + sP2 + q * kP2P + ln;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float a = dy[4 * s * kP3P];
#pragma unroll
        for (int n = 0; n < 12; ++n)
          dw3[n] = mfma4(a, pin[(4 * s + n / 4) * kP2P + 16 * (n % 4)], dw3[n]);
      }
    }
    const int kh = wave >> 2;
    f32x4 dp;
    {
      const int mt = wave & 3;
      dp = dgrad_half<128, kP3P>(pkc + kTbW3 + mt * 96 * 64 + lane, sm + sR3 + (ln + 2) * kP3P + q, kh);
      if (kh == 0)
        *reinterpret_cast<float4*>(sm + sD2 + ln * kP2P + 16 * mt + 4 * q) = make_float4(dp[0], dp[1], dp[2], dp[3]);
    }
    __syncthreads();
    if (kh == 1) dgrad_finish<kP2P, kP2P>(dp, sm + sD2, sm + sR2, ln, 16 * (wave & 3) + 4 * q);
    __syncthreads();
    // ---- conv2 weight gradient (co tile = wave & 3, ci tile = wave >> 2, 3
    // taps) and the first K half of dP1 (ci tile = wave & 1, t tile = bit 1)
    {
      const float* dy = sm + sR2 + (q + 1) * kP2P + 16 * (wave & 3) + ln;
      const float* pin = sm + sP1 + q * kP1P + 16 * (wave >> 2) + ln;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const float a = dy[4 * s * kP2P];
#pragma unroll
        for (int n = 0; n < 3; ++n) dw2[n] = mfma4(a, pin[(4 * s + n) * kP1P], dw2[n]);
      }
    }
    const int mt1 = wave & 1, ti1 = 16 * ((wave >> 1) & 1) + ln;
    {
      dp = dgrad_half<64, kP2P>(pkc + kTbW2 + mt1 * 48 * 64 + lane, sm + sR2 + (ti1 + 2) * kP2P + q, kh);
      if (kh == 0)
        *reinterpret_cast<float4*>(sm + sD1 + ti1 * kP1P + 16 * mt1 + 4 * q) = make_float4(dp[0], dp[1], dp[2], dp[3]);
    }
    __syncthreads();
    if (kh == 1) dgrad_finish<kP1P, kP1P>(dp, sm + sD1, sm + sR1, ti1, 16 * mt1 + 4 * q);
    __syncthreads();
    // ---- conv1 weight gradient: waves 0-5, co tile = wave & 1, tap = wave >> 1
    if (wave < 6) {
      const float* dy = sm + sR1 + (q + 1) * kP1P + 16 * (wave & 1) + ln;
      const float* pin = sm + sX + (q + (wave >> 1)) * kXP + ln;
#pragma unroll
      for (int s = 0; s < 16; ++s) dw1 = mfma4(dy[4 * s * kP1P], pin[4 * s * kXP], dw1);
    }
    __syncthreads();
  }

  // ---- this workgroup's slot: gradients in blob order, then the loss sum
  float* dst = part + (size_t)blockIdx.x * kSlot;
#pragma unroll
  for (int n = 0; n < 12; ++n) store_dw_tile(dw3[n], dst + kOffW3, 64, 16 * wave + 4 * q, 16 * (n % 4) + ln, n / 4);
#pragma unroll
  for (int n = 0; n < 3; ++n) store_dw_tile(dw2[n], dst + kOffW2, 32, 16 * (wave & 3) + 4 * q, 16 * (wave >> 2) + ln, n);
  if (wave < 6) store_dw_tile(dw1, dst + kOffW1, 13, 16 * (wave & 1) + 4 * q, ln, wave >> 1);
#pragma unroll
  for (int j = 0; j < 16; ++j) dst[kOffF1 + fo * 128 + 16 * fpart + j] = df1[j];
  if (wave == 0) dst[kOffF2 + lane] = df2;
  if (tid == 0) dst[kNumWeights] = loss;
}

// Fixed-order sum of the workgroup slots: element i of every slot, four
// interleaved chains combined at the end.  Element kNumWeights is the loss.
__global__ void wk_train_reduce_kernel(const float* __restrict__ part, int nparts, int64_t batch,
                                       float* __restrict__ grads, float* __restrict__ grads2, float* __restrict__ d_loss) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > kNumWeights) return;
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int p = 0;
  for (; p + 4 <= nparts; p += 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += part[(size_t)(p + k) * kSlot + i];
  }
  for (int k = 0; p < nparts; ++p, ++k) s[k] += part[(size_t)p * kSlot + i];
  const float v = (s[0] + s[1]) + (s[2] + s[3]);
  if (i == kNumWeights) {
    *d_loss = v / (float)batch;
  } else {
    grads[i] = v;
    if (grads2) grads2[i] = v;
  }
}

// torch.optim.AdamW's update (decoupled weight decay first), in its order.
__global__ void wk_train_adamw_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                      const float* __restrict__ g, float decay, float beta1, float beta2,
                                      float step_size, float bc2_sqrt, float eps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kNumWeights) return;
  const float gi = g[i];
  float pi = p[i] * decay;
  const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
  const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
  pi -= step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
  p[i] = pi;
  m[i] = mi;
  v[i] = vi;
}

}  // namespace

hipError_t launch_pack_direct(const float* w, float* pk, int count, hipStream_t stream) {
  wk_pack_direct_kernel<<<(count + 255) / 256, 256, 0, stream>>>(w, pk, count);
  return hipGetLastError();
}

}  // namespace wk

struct wk_trainer {
  int device = 0;
  int grid_cap = 512;        // workgroups per gradient launch
  wk::DevBuf<float> d_w;      // [WK_NUM_WEIGHTS] current weights
  wk::DevBuf<float> d_pk;     // fragment-major copy (launch_pack_direct)
  wk::DevBuf<float> d_g;      // last gradients
  wk::DevBuf<float> d_m;      // AdamW first / second moments
  wk::DevBuf<float> d_v;
  wk::DevBuf<float> d_part;   // [part_slots][kSlot] workgroup partial sums
  int64_t part_slots = 0;
  int64_t steps = 0;
  bool have_grads = false;
};

using wk::hip_fail;
using wk::invalid;

extern "C" {

wk_status wk_trainer_create(int32_t device, const float* host_weights, wk_trainer** out) {
  if (!out) return invalid("wk_trainer_create: null out");
  *out = nullptr;
  if (!host_weights) return invalid("wk_trainer_create: null weights");
  if (device < 0) return invalid("wk_trainer_create: bad device");
  return wk::on_device(device, [&]() -> wk_status {
    std::unique_ptr<wk_trainer> t(new (std::nothrow) wk_trainer);   // (a failed create frees it here, device current)
    if (!t) return WK_ERR_NO_MEMORY;
    t->device = device;
    hipError_t e;
    const size_t nb = sizeof(float) * wk::kNumWeights;
    int cu = 256;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0)
      t->grid_cap = 2 * cu;
    if ((e = t->d_w.alloc(wk::kNumWeights)) != hipSuccess || (e = t->d_g.alloc(wk::kNumWeights)) != hipSuccess ||
        (e = t->d_m.alloc(wk::kNumWeights)) != hipSuccess || (e = t->d_v.alloc(wk::kNumWeights)) != hipSuccess ||
        (e = t->d_pk.alloc(wk::kTrainPacked)) != hipSuccess)
      return e == hipErrorOutOfMemory ? wk::fail(WK_ERR_NO_MEMORY, "wk_trainer_create: hipMalloc") : hip_fail(e, "wk_trainer_create: hipMalloc");
    if ((e = hipMemcpy(t->d_w, host_weights, nb, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemset(t->d_m, 0, nb)) != hipSuccess || (e = hipMemset(t->d_v, 0, nb)) != hipSuccess ||
        (e = hipDeviceSynchronize()) != hipSuccess)
      return hip_fail(e, "wk_trainer_create: upload");
    *out = t.release();
    return WK_OK;
  });
}

wk_status wk_trainer_destroy(wk_trainer* t) {
  if (!t) return invalid("wk_trainer_destroy: null trainer");
  const wk_status s = wk::on_device(t->device, [&]() -> wk_status {
    (void)hipDeviceSynchronize();
    delete t;
    return WK_OK;
  });
  if (s != WK_OK) delete t;   // the device could not be made current: the object goes all the same
  return WK_OK;
}

wk_status wk_trainer_grad(wk_trainer* t, const float* d_feats, const float* d_labels, int64_t batch, float* d_loss,
                          float* d_logits_or_null, float* d_grads_or_null, void* stream) {
  if (!t) return invalid("wk_trainer_grad: null trainer");
  if (!d_feats || !d_labels || !d_loss) return invalid("wk_trainer_grad: null pointer");
  if (batch < 1) return invalid("wk_trainer_grad: batch < 1");
  return wk::on_device(t->device, [&]() -> wk_status {
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    const int grid = (int)(batch < t->grid_cap ? batch : t->grid_cap);
    if (grid > t->part_slots) {   // workspace grows on the first call with a larger batch (then reused)
      if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "wk_trainer_grad: sync");
      t->part_slots = 0;
      if ((e = t->d_part.alloc((size_t)grid * wk::kSlot)) != hipSuccess)
        return e == hipErrorOutOfMemory ? wk::fail(WK_ERR_NO_MEMORY, "wk_trainer_grad: workspace") : hip_fail(e, "wk_trainer_grad: workspace");
      t->part_slots = grid;
    }
    if ((e = wk::launch_pack_direct(t->d_w, t->d_pk, wk::kTrainPacked, st)) != hipSuccess)
      return hip_fail(e, "wk_trainer_grad launch");
    wk::wk_train_grad_kernel<<<grid, wk::kDirectBlock, 0, st>>>(d_feats, d_labels, batch, t->d_w, t->d_pk, t->d_part,
                                                               d_logits_or_null);
    wk::wk_train_reduce_kernel<<<(wk::kNumWeights + 1 + 255) / 256, 256, 0, st>>>(t->d_part, grid, batch, t->d_g,
                                                                                 d_grads_or_null, d_loss);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "wk_trainer_grad launch");
    t->have_grads = true;
    return WK_OK;
  });
}

wk_status wk_trainer_step(wk_trainer* t, const wk_adamw* opt, const float* d_grads_or_null, void* stream) {
  if (!t) return invalid("wk_trainer_step: null trainer");
  if (!opt) return invalid("wk_trainer_step: null optimizer parameters");
  if (!std::isfinite(opt->lr) || !std::isfinite(opt->eps)) return invalid("wk_trainer_step: lr / eps not finite");
  if (!d_grads_or_null && !t->have_grads) return invalid("wk_trainer_step: no gradients (call wk_trainer_grad or pass them)");
  return wk::on_device(t->device, [&]() -> wk_status {
    const int64_t step = t->steps + 1;
    const double bc1 = 1.0 - pow((double)opt->beta1, (double)step);
    const double bc2 = 1.0 - pow((double)opt->beta2, (double)step);
    wk::wk_train_adamw_kernel<<<(wk::kNumWeights + 255) / 256, 256, 0, (hipStream_t)stream>>>(
        t->d_w, t->d_m, t->d_v, d_grads_or_null ? d_grads_or_null : t->d_g,
        (float)(1.0 - (double)opt->lr * (double)opt->weight_decay), opt->beta1, opt->beta2,
        (float)((double)opt->lr / bc1), (float)sqrt(bc2), opt->eps);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "wk_trainer_step launch");
    t->steps = step;
    return WK_OK;
  });
}

wk_status wk_trainer_weights(wk_trainer* t, float* d_out, void* stream) {
  if (!t) return invalid("wk_trainer_weights: null trainer");
  if (!d_out) return invalid("wk_trainer_weights: null pointer");
  return wk::on_device(t->device, [&]() -> wk_status {
    const hipError_t e = hipMemcpyAsync(d_out, t->d_w, sizeof(float) * wk::kNumWeights, hipMemcpyDeviceToDevice,
                                        (hipStream_t)stream);
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_trainer_weights");
  });
}

}  // extern "C"
