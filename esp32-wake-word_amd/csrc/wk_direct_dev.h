// wk_direct_dev.h -- the fp32 forward of the xiaoa CNN in direct form, the one
// definition behind the training step (wk_train.hip) and calibration
// (wk_quant.hip).  Both are defined on the direct convolution's
// pre-activations, not on the inference path's Winograd (wk_cnn_dev.h).
//
// One workgroup of kDirectBlock threads (8 waves) holds one clip in LDS as
// [t + 1][ci] images with zero guard rows.  Each convolution is an implicit
// GEMM Y[co][t] = sum_{tap,ci} W[co][ci][tap] P[t + tap - 1][ci] on
// v_mfma_f32_16x16x4f32: conv1 32 x 64 x 48, conv2 64 x 32 x 96, conv3
// 128 x 16 x 192, eight 16 x 16 tiles each, one per wave, so every pre-pool
// value of a layer is in an accumulator of exactly one lane.  What a caller
// does with a tile (route flags, observation, the order of ReLU and pool) is
// its own epilogue.
#pragma once
#include <type_traits>

#include "wk_cnn_dev.h"
#include "wk_kernels.h"

namespace wk {

constexpr int kDirectBlock = 512;

// Fragment-major forward weights (floats): A fragments [tile][step][64], step =
// tap * CINP/4 + cb, lane l: co = 16 tile + (l & 15), ci = 4 cb + (l >> 4).
// launch_pack_direct (wk_train.hip) builds them.
constexpr int kDfW1 = 0;                        // [2][12][64]  (Cin 13 padded to 16)
constexpr int kDfW2 = kDfW1 + 2 * 12 * 64;      // [4][24][64]
constexpr int kDfW3 = kDfW2 + 4 * 24 * 64;      // [8][48][64]
constexpr int kDirectFwdPacked = kDfW3 + 8 * 48 * 64;

// LDS map of the forward (floats); a caller's own images follow at
// kDirectLdsFloats.  Row pitches are 4 mod 16 so the 16 rows of a B fragment
// land in distinct banks.
constexpr int kXP = 20, kP1P = 36, kP2P = 68, kP3P = 132;
constexpr int sX = 0;                        // [66][20]   input, row t + 1
constexpr int sP1 = sX + 66 * kXP;           // [34][36]   pooled conv1
constexpr int sP2 = sP1 + 34 * kP1P;         // [18][68]   pooled conv2
constexpr int sP3 = sP2 + 18 * kP2P;         // [8][132]   pooled conv3, row = pooled step
constexpr int sG = sP3 + 8 * kP3P;           // [128]      mean over time
constexpr int sH = sG + 128;                 // [64]       classifier.0 output after ReLU
constexpr int sF2 = sH + 64;                 // [64]       classifier.2 weights
constexpr int kDirectLdsFloats = sF2 + 64;

// Zero the workgroup's LDS floats (the guard rows and padded channels stay
// zero from here on), load classifier.2's weights and this thread's share of
// classifier.0's: thread (o, part) = (tid >> 3, tid & 7) owns F1[o][16 part .. +16].
template <int LDS_FLOATS>
__device__ __forceinline__ void direct_setup(float* sm, const float* __restrict__ w, int tid, float (&f1)[16]) {
  for (int i = tid; i < LDS_FLOATS; i += kDirectBlock) sm[i] = 0.0f;
  __syncthreads();
  if (tid < 64) sm[sF2 + tid] = w[kOffF2 + tid];
#pragma unroll
  for (int j = 0; j < 16; ++j) f1[j] = w[kOffF1 + (tid >> 3) * 128 + 16 * (tid & 7) + j];
}

// The packed weights' base for one clip.  The fragment loads are
// loop-invariant; hoisted out of the clip loop they would take 84 VGPRs in
// calibration and several hundred in training, so the base is made opaque per clip.
__device__ __forceinline__ const float* per_clip_base(const float* pk) {
  asm volatile("" : "+s"(pk));
  return pk;
}

// One 16 x 16 tile of a direct-form convolution.  wf: the tile's fragments +
// lane; img: the lane's B element of tap 0, step 0 (row t0 + (l & 15), column l >> 4).
template <int CINP, int PITCH>
__device__ __forceinline__ f32x4 conv_tile(const float* __restrict__ wf, const float* img) {
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int tap = 0; tap < 3; ++tap)
#pragma unroll
    for (int cb = 0; cb < CINP / 4; ++cb)
      acc = mfma4(wf[(tap * (CINP / 4) + cb) * 64], img[tap * PITCH + 4 * cb], acc);
  return acc;
}

// This wave's tile of conv layer L (1, 2, 3): 2 co tiles x 4 t tiles, 4 x 2,
// 8 x 1.  Lane l then holds y[c0 .. c0 + 3][t], t = 16 nt + (l & 15) (columns
// t >= kConvSteps[L - 1] are tile padding); the pool partner t ^ 1 is lane
// l ^ 1.  epi(layer, acc, t, c0, lane, prow): prow = the lane's 4 channels of
// pooled step t >> 1 in the next image, for the even lanes whose pooled step
// is below kConvSteps[L] to write (the floor pool drops the rest).
template <int L, typename Epi>
__device__ __forceinline__ void conv_layer_tile(const float* __restrict__ pk, float* sm, int wave, int lane, Epi epi) {
  constexpr int CINP = 8 << L, MT = 1 << L, STEPS = 3 * CINP / 4;
  constexpr int WOFF = L == 1 ? kDfW1 : L == 2 ? kDfW2 : kDfW3;
  constexpr int IN = L == 1 ? sX : L == 2 ? sP1 : sP2, INP = L == 1 ? kXP : L == 2 ? kP1P : kP2P;
  constexpr int OUT = L == 1 ? sP1 : L == 2 ? sP2 : sP3, OUTP = L == 1 ? kP1P : L == 2 ? kP2P : kP3P;
  const int mt = wave % MT, nt = wave / MT, t = 16 * nt + (lane & 15), c0 = 16 * mt + 4 * (lane >> 4);
  const f32x4 acc = conv_tile<CINP, INP>(pk + WOFF + mt * STEPS * 64 + lane, sm + IN + t * INP + (lane >> 4));
  epi(std::integral_constant<int, L>(), acc, t, c0, lane, sm + OUT + ((t >> 1) + (L < 3 ? 1 : 0)) * OUTP + c0);
}

// Mean of channel c over the pooled conv3 steps -> G[c]; threads 0..127.
__device__ __forceinline__ float gap_channel(float* sm, int c) {
  float s = 0.0f;
#pragma unroll
  for (int p = 0; p < kConvSteps[3]; ++p) s += sm[sP3 + p * kP3P + c];
  s /= (float)kConvSteps[3];
  sm[sG + c] = s;
  return s;
}

// classifier.0 + ReLU -> H, 8 threads per output row (direct_setup's f1); g =
// the 16 G values this thread multiplied.
__device__ __forceinline__ void classifier0(float* sm, int tid, const float (&f1)[16], float (&g)[16]) {
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    g[j] = sm[sG + 16 * (tid & 7) + j];
    s = fmaf(f1[j], g[j], s);
  }
  s += dpp<0xB1>(s);
  s += dpp<0x4E>(s);
  s += dpp<0x141>(s);
  if ((tid & 7) == 0) sm[sH + (tid >> 3)] = fmaxf(s, 0.0f);
}

// classifier.2: the logit, in every lane of a wave; hv = H[lane].
__device__ __forceinline__ float classifier2(const float* sm, int lane, float& hv) {
  hv = sm[sH + lane];
  return wave_sum(sm[sF2 + lane] * hv);
}

}  // namespace wk
