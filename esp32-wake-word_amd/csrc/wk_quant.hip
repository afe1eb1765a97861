// wk_quant.hip -- calibration of the int8 network's activation exponents
// (ml_models/main.py:71-129, quantize_model_esp: esp-ppq observes the float
// network on calibration clips and picks a power-of-2 scale per tensor).
//
// wk_calib_kernel: one fp32 forward of the xiaoa CNN per clip, convolutions in
// direct form on v_mfma_f32_16x16x4f32 (the observed values are defined as the
// direct convolution's, not the inference path's Winograd), with the tile
// layout of wk_train.hip's forward pass: one workgroup of 8 waves walks clips
// wg, wg + grid, ...; a clip's activations stay in LDS ([t + 1][ci] images with
// zero guard rows), every pre-pool value of a layer is in an accumulator of
// exactly one lane.  Seven tensors are observed per clip: the input (13 x 63),
// conv1 / conv2 / conv3 after ReLU and before the pool (32 x 63, 64 x 31,
// 128 x 15), GAP (128), classifier.0 after ReLU (64), the logit (1).  The MFMA
// tiles cover 64 / 32 / 16 columns: the lanes of columns t = 63, 31, 15 hold
// padding and count nothing, and the guard rows are never read as values.
//
// A power-of-2 quantiser needs no sort for a percentile: |x| goes to the bin of
// the smallest exponent that holds it, b = min{e : |x| <= 127 * 2^e}.  127 * 2^e
// = 1.984375 * 2^(e + 6) (mantissa field 0x7E0000), so with exponent field E the
// bin is E - 6 up to that mantissa and E - 5 above it: two integer operations on
// the bits, exact.  32 bins per tensor, e in [-24, 7], clamped (zeros lowest).
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
#include "wk_cnn_dev.h"
#include "wk_kernels.h"

namespace wk {
namespace {

constexpr int kBlock = 512;
constexpr int kNT = WK_QUANT_TENSORS, kNB = WK_QUANT_BINS;

// fragment-major forward weights [tile][step][64], step = tap * CINP/4 + cb;
// lane l: co = 16 tile + (l & 15), ci = 4 cb + (l >> 4) (wk_train.hip's forward order)
constexpr int kCfW1 = 0;                       // [2][12][64]  (Cin 13 padded to 16)
constexpr int kCfW2 = kCfW1 + 2 * 12 * 64;     // [4][24][64]
constexpr int kCfW3 = kCfW2 + 4 * 24 * 64;     // [8][48][64]
static_assert(kCfW3 + 8 * 48 * 64 == kCalibPacked, "packed size");

// LDS map (floats); row pitches 4 mod 16: the 16 rows of a B fragment land in distinct banks
constexpr int kXP = 20, kP1P = 36, kP2P = 68, kP3P = 132;
constexpr int sX = 0;                   // [66][20]  input, row t + 1
constexpr int sP1 = sX + 66 * kXP;      // [34][36]  pooled conv1
constexpr int sP2 = sP1 + 34 * kP1P;    // [18][68]  pooled conv2
constexpr int sP3 = sP2 + 18 * kP2P;    // [8][132]  pooled conv3, row = pooled step
constexpr int sG = sP3 + 8 * kP3P;      // [128]
constexpr int sH = sG + 128;            // [64]
constexpr int sF2 = sH + 64;            // [64]
constexpr int kLdsFloats = sF2 + 64;

__global__ void wk_calib_pack_kernel(const float* __restrict__ w, float* __restrict__ pk) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kCalibPacked) return;
  int base, cin, inner, wbase;
  if (i < kCfW2) { base = kCfW1; cin = 13; inner = 16; wbase = kOffW1; }
  else if (i < kCfW3) { base = kCfW2; cin = 32; inner = 32; wbase = kOffW2; }
  else { base = kCfW3; cin = 64; inner = 64; wbase = kOffW3; }
  const int j = i - base, l = j & 63, ns = 3 * inner / 4;
  const int s = (j >> 6) % ns, tile = (j >> 6) / ns, tap = s / (inner / 4), cb = s % (inner / 4);
  const int co = 16 * tile + (l & 15), ci = 4 * cb + (l >> 4);
  pk[i] = ci < cin ? w[wbase + (co * cin + ci) * 3 + tap] : 0.0f;
}

// Bin index 0..31 (exponent -24..7) of |x|.
__device__ __forceinline__ int bin_of(float x) {
  const unsigned u = __float_as_uint(x) & 0x7FFFFFFFu;
  const int b = (int)(u >> 23) - 127 - ((u & 0x7FFFFFu) <= 0x7E0000u ? 6 : 5);
  return (u == 0 || b < -24) ? 0 : (b > 7 ? kNB - 1 : b + 24);
}

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
  wave_count(cnt, valid ? bin_of(v) : -1, lane);
}

// One 16 x 16 tile of a direct-form convolution.  wf: the tile's fragments +
// lane; img: the lane's B element of tap 0, step 0 (row t0 + (l & 15), column l >> 4).
template <int CINP, int PITCH>
__device__ __forceinline__ f32x4 conv_tile(const float* __restrict__ wf, const float* img) {
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int tap = 0; tap < 3; ++tap)
#pragma unroll
    for (int cb = 0; cb < CINP / 4; ++cb) acc = mfma4(wf[(tap * (CINP / 4) + cb) * 64], img[tap * PITCH + 4 * cb], acc);
  return acc;
}

// ReLU, observe the tile's pre-pool values (lane l holds y[co0 .. co0 + 3][t];
// columns t >= TV are tile padding), maxpool(2) into the next image (TN pooled
// steps, the floor pool drops the rest; the pool partner t ^ 1 is lane l ^ 1).
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

__global__ __launch_bounds__(kBlock) void wk_calib_kernel(const float* __restrict__ feats, int64_t batch,
                                                          const float* __restrict__ w, const float* __restrict__ pk,
                                                          unsigned* __restrict__ slots) {
  __shared__ __attribute__((aligned(16))) float sm[kLdsFloats];
  __shared__ unsigned cnt[kCalibSlot];   // [7][32] counts, then the 7 maxima
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 15, q = lane >> 4;

  for (int i = tid; i < kLdsFloats; i += kBlock) sm[i] = 0.0f;
  for (int i = tid; i < kCalibSlot; i += kBlock) cnt[i] = 0u;
  __syncthreads();
  if (tid < 64) sm[sF2 + tid] = w[kOffF2 + tid];
  // classifier.0: thread (o, part) owns F1[o][16 part .. +16]
  const int fo = tid >> 3, fpart = tid & 7;
  float f1[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) f1[j] = w[kOffF1 + fo * 128 + 16 * fpart + j];
  unsigned mx[kNT];
#pragma unroll
  for (int k = 0; k < kNT; ++k) mx[k] = 0u;

  for (int64_t clip = blockIdx.x; clip < batch; clip += gridDim.x) {
    // ---- input: [13][63] -> X[t + 1][ci]
    const float* x = feats + clip * (13 * 63);
#pragma unroll
    for (int base = 0; base < 13 * 63; base += kBlock) {
      const int i = base + tid;
      const bool ok = i < 13 * 63;
      const float v = ok ? x[i] : 0.0f;
      if (ok) {
        const int ci = i / 63, t = i - 63 * ci;
        sm[sX + (t + 1) * kXP + ci] = v;
      }
      observe(cnt + 0 * kNB, mx[0], v, ok, lane);
    }
    // hoisted out of the clip loop the fragment loads would take 84 VGPRs: the base is made opaque per clip
    const float* pkc = pk;
    asm volatile("" : "+s"(pkc));
    __syncthreads();
    // ---- conv1: 2 co tiles x 4 t tiles, one per wave
    {
      const int mt = wave & 1, nt = wave >> 1, t = 16 * nt + ln, c0 = 16 * mt + 4 * q;
      const f32x4 acc = conv_tile<16, kXP>(pkc + kCfW1 + mt * 12 * 64 + lane, sm + sX + t * kXP + q);
      epi_observe_pool<63, 31>(acc, cnt + 1 * kNB, mx[1], sm + sP1 + ((t >> 1) + 1) * kP1P + c0, t, lane);
    }
    __syncthreads();
    // ---- conv2: 4 co tiles x 2 t tiles
    {
      const int mt = wave & 3, nt = wave >> 2, t = 16 * nt + ln, c0 = 16 * mt + 4 * q;
      const f32x4 acc = conv_tile<32, kP1P>(pkc + kCfW2 + mt * 24 * 64 + lane, sm + sP1 + t * kP1P + q);
      epi_observe_pool<31, 15>(acc, cnt + 2 * kNB, mx[2], sm + sP2 + ((t >> 1) + 1) * kP2P + c0, t, lane);
    }
    __syncthreads();
    // ---- conv3: 8 co tiles x 1 t tile
    {
      const int t = ln, c0 = 16 * wave + 4 * q;
      const f32x4 acc = conv_tile<64, kP2P>(pkc + kCfW3 + wave * 48 * 64 + lane, sm + sP2 + t * kP2P + q);
      epi_observe_pool<15, 7>(acc, cnt + 3 * kNB, mx[3], sm + sP3 + (t >> 1) * kP3P + c0, t, lane);
    }
    __syncthreads();
    // ---- mean over the 7 pooled steps (waves 0 and 1)
    if (wave < 2) {
      float s = 0.0f;
#pragma unroll
      for (int p = 0; p < 7; ++p) s += sm[sP3 + p * kP3P + tid];
      s /= 7.0f;
      sm[sG + tid] = s;
      observe(cnt + 4 * kNB, mx[4], s, true, lane);
    }
    __syncthreads();
    // ---- classifier.0 + ReLU: 8 threads per output row
    {
      float s = 0.0f;
#pragma unroll
      for (int j = 0; j < 16; ++j) s = fmaf(f1[j], sm[sG + 16 * fpart + j], s);
      s += dpp<0xB1>(s);
      s += dpp<0x4E>(s);
      s += dpp<0x141>(s);
      if (fpart == 0) sm[sH + fo] = fmaxf(s, 0.0f);
    }
    __syncthreads();
    // ---- classifier.2 (wave 0).  The next clip's writes to sH come five barriers later.
    if (wave == 0) {
      const float hv = sm[sH + lane];
      observe(cnt + 5 * kNB, mx[5], hv, true, lane);
      const float z = wave_sum(sm[sF2 + lane] * hv);
      observe(cnt + 6 * kNB, mx[6], z, lane == 0, lane);
    }
  }

  // ---- this workgroup's slot
#pragma unroll
  for (int k = 0; k < kNT; ++k) atomicMax(&cnt[kNT * kNB + k], mx[k]);
  __syncthreads();
  for (int i = tid; i < kCalibSlot; i += kBlock) slots[(size_t)blockIdx.x * kCalibSlot + i] = cnt[i];
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

hipError_t launch_calibrate(const float* w, const float* feats, int64_t batch, void* workspace, hipStream_t stream) {
  unsigned long long* tot = (unsigned long long*)workspace;
  float* pk = (float*)((char*)workspace + kCalibTotalsBytes);
  unsigned* slots = (unsigned*)(pk + kCalibPacked);
  const int grid = (int)(batch < kCalibGridCap ? batch : kCalibGridCap);
  wk_calib_pack_kernel<<<(kCalibPacked + 255) / 256, 256, 0, stream>>>(w, pk);
  wk_calib_kernel<<<grid, kBlock, 0, stream>>>(feats, batch, w, pk, slots);
  wk_calib_sum_kernel<<<1, 256, 0, stream>>>(slots, grid, tot);
  return hipGetLastError();
}

}  // namespace wk
