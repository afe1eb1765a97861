// wk_fused_cnn_role.h -- the CNN role of the fused kernel (waves 8-15) and its
// two clip sources.
//
// The role takes the DCT-II + CMVN from the front-end's log-mel buffer into
// the conv1 input image (one wave per clip, on the matrix cores:
// dct_cmvn_clip), then runs the CNN of wk_cnn_dev.h on batches of NBF = 4
// clips.  Moving the DCT + CMVN to the CNN waves (which wait on the front-end
// about half the time) shortened the front-end's per-clip critical path by
// ~15 %.  The role is MFMA bound.  The standalone CNN kernel (wk_fused.hip)
// runs the same role on the caller's features (FeatSrc).
#pragma once
#include "wk_fused_lds.h"
#include "wk_cnn_dev.h"
#include "wk_kernels.h"   // (the weight fragments' layout: kPk*, kPb*)

namespace {

// ---------------------------------------------------------------------------
// DCT-II + CMVN of one clip on the matrix cores (extract_mfcc.py:70-80; the
// DCT of torchaudio.transforms.MFCC, ortho, 13 of 40): the 13x40 DCT (rows
// 13-15 zero) times the [40 mel][64 frame] log-mel image is a 16x40x64 fp32
// GEMM = 10 K-steps x 4 column tiles of v_mfma_f32_16x16x4f32, run by ONE wave.
// Column li of tile nt is frame 4 li + nt, so a lane's B values of one K-step
// are 4 consecutive frames: one ds_read_b128 feeds the 4 tiles.  The lane then
// holds coefficients 4 lk .. 4 lk + 3 of frames 4 li .. 4 li + 3: CMVN's
// per-coefficient sums are 3 in-register adds + a 16-lane DPP row reduction,
// and the 4 normalised coefficients of a frame leave as one 16-byte (fp32) or
// 8-byte (bf16) store into the conv1 image [clip][t][ci].  Frame 63 (column
// 15 of tile 3) is a padding column: excluded from the statistics, not stored.
// (Replaces 13 x 40 lane-per-frame FMAs + 13 separate wave reductions spread
// over the 8 CNN waves: ~1,300 VALU instructions per clip -> 40 MFMA + ~150.)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float row_sum16(float v) {   // sum over the lane's 16-lane row, in every lane
  v += dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp<0x141>(v);  // row_half_mirror
  v += dpp<0x140>(v);  // row_mirror
  return v;
}

template <int CM>
__device__ __forceinline__ void dct_cmvn_clip(const float* __restrict__ lbuf, int slot, float* __restrict__ F0,
                                              uint16_t* __restrict__ B0, uint16_t* __restrict__ X0,
                                              float* __restrict__ fo, int lane) {
  const int li = lane & 15, lk = lane >> 4;
  // A fragments dct[li][4 s + lk], s = 0..9: this lane's row of kDctB16
  // (lane-major, wk_tables.h), three 16-byte loads, re-read (L1/L2-resident,
  // 3 KB) per clip: kept live across the batch they pushed the fp32 CNN into
  // spills.
  int aoff = 48 * lane;
  asm volatile("" : "+v"(aoff));   // not loop-invariant: keep the loads here
  const auto ra = make_rsrc(kDctB16, sizeof(kDctB16));
  float dA[12];
#pragma unroll
  for (int s = 0; s < 12; s += 4) {
    const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, aoff, 4 * s, 0));
#pragma unroll
    for (int r = 0; r < 4; ++r) dA[s + r] = v[r];
  }
  f32x4 d[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
  for (int s = 0; s < 10; ++s) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(lbuf + (4 * s + lk) * WK_LSTRIDE + 4 * li);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) d[nt] = mfma4(dA[s], b[nt], d[nt]);
  }
  const bool v3 = li != 15;   // tile 3 column 15 = frame 63 (padding)
  // cmvn_lane's rule (wk_fe_dev.h): a coefficient whose 63 frames are equal
  // (digital silence) is taken as a row of zeros and normalises to exactly 0.0;
  // sum * (1/63) of 63 equal values need not round to the value.  A row is flat
  // when each lane's frames are equal and frame 4 li equals frame 4 (li + 1):
  // row_shl:1 brings the next lane's value, lane 15 keeps its own.  The
  // select sits before all arithmetic, which rows with two different values
  // go through unchanged.
  const int row0 = lane & 48;   // the first lane of this lane's 16-lane row
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float a = d[0][r];
    const float nx = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(a), __float_as_int(a), 0x101, 0xF, 0xF, false));
    const bool ne = (a != d[1][r]) | (a != d[2][r]) | (v3 & (a != d[3][r])) | (a != nx);
    const bool flat = ((__builtin_amdgcn_ballot_w64(ne) >> row0) & 0xFFFFull) == 0;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) d[nt][r] = flat ? 0.0f : d[nt][r];
  }
  float mean[4], inv[4];
  // Reciprocal constants, v_sqrt_f32 and v_rcp_f32 (each <= 1 ulp) instead of
  // IEEE divisions and the libm square root: 12 divisions per clip had
  // compiled to ~10-instruction div_scale/div_fmas/div_fixup sequences.
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float x3 = v3 ? d[3][r] : 0.0f;
    mean[r] = row_sum16((d[0][r] + d[1][r]) + (d[2][r] + x3)) * (1.0f / kNFramesB);
    float dv[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) dv[nt] = d[nt][r] - mean[r];
    dv[3] = v3 ? dv[3] : 0.0f;
    const float q = row_sum16((dv[0] * dv[0] + dv[1] * dv[1]) + (dv[2] * dv[2] + dv[3] * dv[3]));
    float sd = __builtin_amdgcn_sqrtf(q * (1.0f / (kNFramesB - 1)));
    sd = sd == 0.0f ? 1.0f : sd;   // rows 13-15 (all zero) land here and stay 0
    inv[r] = __builtin_amdgcn_rcpf(sd + 1e-8f);
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int t = 4 * li + nt;
    if (nt == 3 && !v3) continue;
    const int row = slot * I0_TP + 1 + t;
    float y[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) y[r] = (d[nt][r] - mean[r]) * inv[r];
    if constexpr (CM == kConvBf16) {
      uint2 pk;
      pk.x = bf16_bits(y[0]) | (bf16_bits(y[1]) << 16);
      pk.y = bf16_bits(y[2]) | (bf16_bits(y[3]) << 16);
      *reinterpret_cast<uint2*>(B0 + row * I0_CIP + 4 * lk) = pk;
    } else if constexpr (CM == kConvBf16x3) {
      uint32_t h[4], l[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        h[r] = bf16_bits(y[r]);
        l[r] = bf16_bits(y[r] - __uint_as_float(h[r] << 16));
      }
      *reinterpret_cast<uint2*>(X0 + row * X0_CIP + 4 * lk) = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
      *reinterpret_cast<uint2*>(X0 + row * X0_CIP + 16 + 4 * lk) = make_uint2(l[0] | (l[1] << 16), l[2] | (l[3] << 16));
    } else {
      *reinterpret_cast<f32x4*>(F0 + row * F0_CIP + 4 * lk) = f32x4{y[0], y[1], y[2], y[3]};
    }
    if (fo) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * lk + r < 13) fo[(4 * lk + r) * kNFramesB + t] = y[r];
    }
  }
}

// ---------------------------------------------------------------------------
// CNN role (waves 8-15): batches of NBF clips from the conv1 image.
// ---------------------------------------------------------------------------
// Where the CNN role's LDS lives: the fused kernel's carve window
// [kGOff, kImgEnd) -- pooled features, classifier partials, control words, the
// conv images -- at `base + offset` (base = smem in the fused kernel; the
// standalone CNN kernel, wk_fused.hip, places two such windows per workgroup).
// SRC supplies the conv1 input image of each clip (interface below):
//   init(cw, lane)   once per wave;
//   ready(i)         whether clip i's image can be made without waiting;
//   wait(i)          block until it can;
//   load(i, slot)    write clip i's normalised [63][13] MFCC into conv1 slot `slot`.
// The fused kernel's source is the DCT + CMVN of the front-end's log-mel
// (LogmelSrc); the standalone CNN's is the caller's features in HBM (FeatSrc).
template <int CM, class SRC>   // kConvF32 / kConvBf16 / kConvBf16x3
__device__ __forceinline__ void cnn_role(float* base, const float* __restrict__ pk, const uint16_t* __restrict__ pkb,
                                         int64_t n_mine, int64_t clip_base, int64_t clip_step,
                                         float* __restrict__ logits, int cw, int lane, SRC& src) {
  float* F0 = base + kF0Off;
  float* F1 = base + kF1Off;
  float* F2 = base + kF2Off;
  uint16_t* B0 = reinterpret_cast<uint16_t*>(base + kB0Off);
  uint16_t* B1 = reinterpret_cast<uint16_t*>(base + kB1Off);
  uint16_t* B2 = reinterpret_cast<uint16_t*>(base + kB2Off);
  uint16_t* X0 = reinterpret_cast<uint16_t*>(base + kX0Off);
  uint16_t* X1 = reinterpret_cast<uint16_t*>(base + kX1Off);
  uint16_t* X2 = reinterpret_cast<uint16_t*>(base + kX2Off);
  constexpr bool BF = CM == kConvBf16, X3 = CM == kConvBf16x3;
  constexpr int kLoW = kNumPackedBf16;   // the xl fragments follow the xh ones (pack_fragments_bf16x3)
  const auto rsb = make_rsrc(pkb, 2 * kNumPackedBf16 * (X3 ? 2 : 1));
  auto frag_bf = [&](int elem_off) -> s8 {   // one lane's 8 bf16 of the fragment at elem_off (x 64 lanes x 8)
    return __builtin_bit_cast(s8, __builtin_amdgcn_raw_buffer_load_b128(rsb, 16 * lane, 2 * elem_off, 0));
  };
  float* Gp = base + kGOff;
  float* FCP = base + kFcpOff;
  unsigned* ctrl = reinterpret_cast<unsigned*>(base + kCtrlOff);
  const int li = lane & 15, lk = lane >> 4;
  unsigned gen = 0;
  const auto rs = make_rsrc(pk, 4 * kNumPacked);

  // Weights come fragment-major, four k-steps per lane contiguous (wk_kernels.h
  // pack_fragments, frag_idx): one coalesced 16-byte-per-lane load per four A
  // fragments.  conv3's (48 fragments) stay in VGPRs; the other layers' are
  // re-read from L2 per batch.
  auto load_frags = [&](auto& w, int first) {   // w[s] = this lane's value of the fragment first + 64 s
    constexpr int n = sizeof(w) / sizeof(float);
    static_assert(n % 4 == 0, "whole groups of four k-steps");
#pragma unroll
    for (int s = 0; s < n; s += 4) {
      const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * lane, 4 * (first + s * 64), 0));
#pragma unroll
      for (int r = 0; r < 4; ++r) w[s + r] = v[r];
    }
  };
  float w3[48];
  s8 w3b[6];
  if constexpr (BF || X3) {
#pragma unroll
    for (int s = 0; s < 6; ++s) w3b[s] = frag_bf(kPbW3 + (cw * 6 + s) * kBfFrag);
  }
  if constexpr (CM == kConvF32) load_frags(w3, kPkW3 + cw * 48 * 64);
  const int64_t n_batches = (n_mine + NBF - 1) / NBF;
  src.init(cw, lane);
  bool eager_done = false;
  // Between the conv phases of batch b (after its conv1 has consumed the conv1
  // image): if clip 4(b+1) + cw's input is already available, make its image
  // now (fused: its buffer goes back to the front-end a whole batch earlier;
  // the double buffer otherwise stalled the front-end ~13 % of the time in fp32).
  auto try_eager = [&](int64_t b) {
    if (cw >= NBF || eager_done) return;
    const int64_t i = (b + 1) * NBF + cw;
    if (i >= n_mine) return;
    if (src.ready(i)) {
      src.load(i, cw);
      eager_done = true;
    }
  };
  // ReLU -> classifier.2 (64 -> 1) of batch bb from the classifier.0 partials
  // (one per CNN wave's k-slice): lane = (o group q = lane>>2, clip = lane&3),
  // one 16-byte read per slice.  Run by one wave, deferred to just after the
  // next batch's first barrier (one barrier per batch fewer).
  auto fc2 = [&](int64_t bb) {
    if (cw != 0) return;
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int cl = ln & (NBF - 1), q = ln >> 2;
    // In the bf16 family the slice sums are scalar fp32 adds, never f32x4
    // arithmetic (which is v_pk_add_f32): this wave runs beside the K = 32
    // convolutions of the other CNN waves on its SIMD (the K = 32 rule,
    // DESIGN 5.1; tests/test_isa_rules.py).  The fp32 build keeps the packed
    // adds (its MFMAs are K = 4; scalar measured -1 %, profiles/r06b_ab.txt).
    float h[4];
    if constexpr (CM == kConvF32) {
      f32x4 v = *reinterpret_cast<const f32x4*>(FCP + cl * 64 + 4 * q);
#pragma unroll
      for (int w = 1; w < 8; ++w) v += *reinterpret_cast<const f32x4*>(FCP + (w * NBF + cl) * 64 + 4 * q);
#pragma unroll
      for (int r = 0; r < 4; ++r) h[r] = v[r];
    } else {
      const f32x4 v = *reinterpret_cast<const f32x4*>(FCP + cl * 64 + 4 * q);
#pragma unroll
      for (int r = 0; r < 4; ++r) h[r] = v[r];
#pragma unroll
      for (int w = 1; w < 8; ++w) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(FCP + (w * NBF + cl) * 64 + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] += u[r];
      }
    }
    float acc = 0.0f;
#pragma unroll
    for (int i2 = 0; i2 < 4; ++i2) acc = __builtin_fmaf(buf_load(rs, 16 * q, 4 * (kPkF2 + i2)), fmaxf(h[i2], 0.0f), acc);
    acc += __shfl_xor(acc, 4, 64);
    acc += __shfl_xor(acc, 8, 64);
    acc += __shfl_xor(acc, 16, 64);
    acc += __shfl_xor(acc, 32, 64);
    const int64_t i = bb * NBF + cl;
    if (q == 0 && i < n_mine) logits[clip_base + clip_step * i] = acc;
  };
  WK_STAMP_INIT
  for (int64_t b = 0; b < n_batches; ++b) {
    // DCT-II + CMVN (extract_mfcc.py:70-80): CNN wave s < NBF takes clip
    // 4b + s whole on the matrix cores (dct_cmvn_clip), unless it already did
    // so eagerly during the previous batch (try_eager below).
    if (cw < NBF && !eager_done) {
      const int64_t i = b * NBF + cw;
      if (i < n_mine) {
        src.wait(i);
        src.load(i, cw);
      }
    }
    eager_done = false;
    // conv1's A fragments: loaded after the DCT (register pressure), landing during the sync.
    float w1[12];
    s8 w1b[2], w1l[2];
    if constexpr (BF || X3) {
#pragma unroll
      for (int s = 0; s < 2; ++s) w1b[s] = frag_bf(kPbW1 + ((cw & 1) * 2 + s) * kBfFrag);
    }
    if constexpr (X3) {
#pragma unroll
      for (int s = 0; s < 2; ++s) w1l[s] = frag_bf(kLoW + kPbW1 + ((cw & 1) * 2 + s) * kBfFrag);
    }
    if constexpr (CM == kConvF32) load_frags(w1, kPkW1 + (cw & 1) * 12 * 64);
    WK_STAMP(0);
    role_sync<0>(ctrl, kCtrlCnnBar, gen, lane);   // conv1 image complete (and the previous batch's partials)
    if (b > 0) fc2(b - 1);

    // Clips of this batch that exist (wave-uniform): a short last batch -- and
    // the one-window launches of the streaming path -- skip the conv passes
    // that cover only absent clips, which shortens each wave's MFMA chain
    // (single-window latency).  Full batches run every pass.
    const int nv = n_mine - b * NBF < NBF ? (int)(n_mine - b * NBF) : NBF;

    // conv1: co tile (cw&1), clip (cw>>1), 4 t-tiles.
    if ((cw >> 1) < nv) {
      const int co0 = 16 * (cw & 1), cl = cw >> 1;
      const int bo = (cl * I0_TP + li) * I0_CIP;   // this lane's t row in the bf16 [clip][t][ci] image
#pragma unroll 1
      for (int p = 0; p < 2; ++p) {
        const int ta = 32 * p, tb = ta + 16;
        f32x4 acc_a = {0, 0, 0, 0}, acc_b = {0, 0, 0, 0};
        if constexpr (BF) {
          conv_pair_bf<2, 16, I0_CIP>(B0, w1b, bo + ta * I0_CIP, bo + tb * I0_CIP, lk, acc_a, acc_b);
          epi_pool_bf<I1_CIP, I1_TP, 31>(acc_a, B1, co0, cl, ta, lane);
          epi_pool_bf<I1_CIP, I1_TP, 31>(acc_b, B1, co0, cl, tb, lane);
        } else if constexpr (X3) {
          const int bx = (cl * I0_TP + li) * X0_CIP;
          conv_pair_bf3<2, 16, X0_CIP>(X0, w1b, w1l, bx + ta * X0_CIP, bx + tb * X0_CIP, lk, acc_a, acc_b);
          epi_pool_bf3<X1_CIP, I1_TP, 31, 32>(acc_a, X1, co0, cl, ta, lane);
          epi_pool_bf3<X1_CIP, I1_TP, 31, 32>(acc_b, X1, co0, cl, tb, lane);
        } else {
          // Winograd pairs 16 p .. 16 p + 15 (outputs 32 p .. 32 p + 31)
          f32x4 m[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
          conv_wino_v<1, F0_CIP>(F0, w1, (cl * I0_TP + 2 * (16 * p + li)) * F0_CIP + 4 * lk, m);
          epi_wino_pool<F1_CIP, I1_TP, 31>(m, F1, co0, cl, 16 * p, lane);
        }
      }
    }
    WK_STAMP(1);
    role_sync<0>(ctrl, kCtrlCnnBar, gen, lane);
    try_eager(b);
    WK_STAMP(2);

    // conv2: co tile (cw&3), clips 2*(cw>>2) + {0,1}, 2 t-tiles each.
    if constexpr (BF) {
      s8 w2b[3];
#pragma unroll
      for (int s = 0; s < 3; ++s) w2b[s] = frag_bf(kPbW2 + ((cw & 3) * 3 + s) * kBfFrag);
      const int co0 = 16 * (cw & 3);
#pragma unroll 1
      for (int p = 0; p < 2; ++p) {
        const int cl = 2 * (cw >> 2) + p;
        if (cl >= nv) break;
        const int bb = (cl * I1_TP + li) * I1_CIP;
        f32x4 acc_a = {0, 0, 0, 0}, acc_b = {0, 0, 0, 0};
        conv_pair_bf<3, 32, I1_CIP>(B1, w2b, bb, bb + 16 * I1_CIP, lk, acc_a, acc_b);
        epi_pool_bf<I2_CIP, I2_TP, 15>(acc_a, B2, co0, cl, 0, lane);
        epi_pool_bf<I2_CIP, I2_TP, 15>(acc_b, B2, co0, cl, 16, lane);
      }
    } else if constexpr (X3) {
      s8 w2b[3], w2l[3];
#pragma unroll
      for (int s = 0; s < 3; ++s) w2b[s] = frag_bf(kPbW2 + ((cw & 3) * 3 + s) * kBfFrag);
#pragma unroll
      for (int s = 0; s < 3; ++s) w2l[s] = frag_bf(kLoW + kPbW2 + ((cw & 3) * 3 + s) * kBfFrag);
      const int co0 = 16 * (cw & 3);
#pragma unroll 1
      for (int p = 0; p < 2; ++p) {
        const int cl = 2 * (cw >> 2) + p;
        if (cl >= nv) break;
        const int bb = (cl * I1_TP + li) * X1_CIP;
        f32x4 acc_a = {0, 0, 0, 0}, acc_b = {0, 0, 0, 0};
        conv_pair_bf3<3, 32, X1_CIP>(X1, w2b, w2l, bb, bb + 16 * X1_CIP, lk, acc_a, acc_b);
        epi_pool_bf3<X2_CIP, I2_TP, 15, 64>(acc_a, X2, co0, cl, 0, lane);
        epi_pool_bf3<X2_CIP, I2_TP, 15, 64>(acc_b, X2, co0, cl, 16, lane);
      }
    } else {
      float w2[24];
      load_frags(w2, kPkW2 + (cw & 3) * 24 * 64);
      const int co0 = 16 * (cw & 3);
#pragma unroll 1
      for (int p = 0; p < 2; ++p) {
        const int cl = 2 * (cw >> 2) + p;
        if (cl >= nv) break;
        f32x4 m[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        conv_wino_v<2, F1_CIP, 1>(F1, w2, (cl * I1_TP + 2 * li) * F1_CIP + 4 * lk, m);
        epi_wino_pool<F2_CIP, I2_TP, 15>(m, F2, co0, cl, 0, lane);
      }
    }
    WK_STAMP(3);
    role_sync<0>(ctrl, kCtrlCnnBar, gen, lane);
    try_eager(b);
    WK_STAMP(4);

    // conv3: co tile cw, the 4 clips; GAP -> G[128][4].
    {
      const int co0 = 16 * cw;
      const int bo = li * I2_CIP;
#pragma unroll 1
      for (int p = 0; p < 2; ++p) {
        // between conv3's two passes too: the longest phase, during which the
        // front-end otherwise waited on the log-mel buffer (fp32 +1.1 %, bf16
        // +0.6 %, profiles/r06ac_eager_ab.txt; inside conv2 as well spilled, -0.6 %)
        if (p > 0) try_eager(b);
        const int ca = 2 * p, cb = 2 * p + 1;
        if (ca >= nv) break;
        f32x4 acc_a = {0, 0, 0, 0}, acc_b = {0, 0, 0, 0};
        if constexpr (BF) {
          conv_pair_bf<6, 64, I2_CIP, 3>(B2, w3b, bo + ca * I2_TP * I2_CIP, bo + cb * I2_TP * I2_CIP, lk, acc_a,
                                         acc_b);
        } else if constexpr (X3) {
          s8 w3l[6];   // the lo parts are re-read from L2 per pass (VGPR budget)
#pragma unroll
          for (int s = 0; s < 6; ++s) w3l[s] = frag_bf(kLoW + kPbW3 + (cw * 6 + s) * kBfFrag);
          const int bx = li * X2_CIP;
          conv_pair_bf3<6, 64, X2_CIP, 2>(X2, w3b, w3l, bx + ca * I2_TP * X2_CIP, bx + cb * I2_TP * X2_CIP, lk,
                                          acc_a, acc_b);
        } else {
          // Winograd: one tile of 16 pair columns = 8 pairs of clip ca, 8 of clip cb
          f32x4 m[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
          conv_wino_v<4, F2_CIP, 1>(F2, w3, ((ca + (li >> 3)) * I2_TP + 2 * (li & 7)) * F2_CIP + 4 * lk, m);
          epi_wino_gap<NBF>(m, Gp, co0, ca, lane);
          continue;
        }
        epi_gap<NBF>(acc_a, Gp, co0, ca, lane);
        epi_gap<NBF>(acc_b, Gp, co0, cb, lane);
      }
    }
    float wf1[16];
    load_frags(wf1, kPkF1 + cw * 16 * 64);
    WK_STAMP(5);
    role_sync<0>(ctrl, kCtrlCnnBar, gen, lane);
    try_eager(b);
    WK_STAMP(6);

    // classifier.0 (128 -> 64) on v_mfma_f32_4x4x1_16b_f32: 16 blocks of 4 o x
    // 4 clips, block b = lane>>2 taking o = 4b .. 4b + 3 (A: lane = o, B: lane
    // & 3 = clip), so every column is a real clip (the 16x16x4 form used 4 of its
    // 16); wave cw takes k = 16 cw .. 16 cw + 15, and its partial
    // [o = 4(lane>>2) + r][clip lane&3] leaves as one 16-byte store.
    {
      int ln = lane;
      asm volatile("" : "+v"(ln));   // addresses recomputed here rather than kept live (and spilled)
      f32x4 acc = {0, 0, 0, 0};
      const float* g = Gp + 16 * cw * NBF + (ln & (NBF - 1));
#pragma unroll
      for (int s = 0; s < 16; ++s) acc = mfma4x4(wf1[s], g[s * NBF], acc);
      *reinterpret_cast<f32x4*>(FCP + (cw * NBF + (ln & (NBF - 1))) * 64 + 4 * (ln >> 2)) = acc;
    }
    // No barrier here: classifier.2 of this batch reads the partials after the
    // next batch's first barrier (below), which already orders them; the
    // partials are next overwritten three barriers later.
    try_eager(b);
    WK_STAMP(8);
  }
  if (n_batches > 0) {
    role_sync<0>(ctrl, kCtrlCnnBar, gen, lane);
    fc2(n_batches - 1);
  }
  WK_STAMP_FLUSH(8 + cw);
}

// The fused kernel's clip source: DCT-II + CMVN of the front-end's log-mel
// image (dct_cmvn_clip), with the front-end hand-off protocol.
// FEATS: the launch also writes the CMVN'd features (parity dumps).  A
// template flag rather than a null test, so the product kernel carries no
// feature-store code (its address registers pushed the fp32 build to spill).
template <int CM, bool FEATS>
struct LogmelSrc {
  float* smem;
  unsigned* ctrl;
  float* feats_out;
  int64_t clip_base, clip_step;
  int cw, lane, diag;
  // Log-mel buffer release (kCtrlLFree + w): wave w < NBF reads only clips
  // w, w + NBF, w + 2 NBF, ...; its word holds the next clip it will read, so
  // every clip below it is released.  Waves >= NBF read none.
  __device__ __forceinline__ void init(int cw_, int lane_) {
    cw = cw_;
    lane = lane_;
    signal_set(ctrl, kCtrlLFree + cw, cw < NBF ? (unsigned)cw : 0xFFFFFFFFu, lane);
  }
  // A true answer is an acquire, like spin_until's exit: the compiler may not
  // move the caller's reads of the log-mel buffer (load() below) above the
  // ready-count read (LDS operations of a wave then complete in order).
  __device__ __forceinline__ bool ready(int64_t i) const {
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const bool r = (diag & 2) ||
                   __builtin_amdgcn_readfirstlane(lds_load(ctrl + kCtrlLReady)) >= 8u * (unsigned)(i + 1);
    asm volatile("" ::: "memory");
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    return r;
  }
  __device__ __forceinline__ void wait(int64_t i) const {
    if (!(diag & 2)) spin_until<0>(ctrl, kCtrlLReady, 8u * (unsigned)(i + 1));
  }
  __device__ __forceinline__ void load(int64_t i, int slot) const {
    float* fo = FEATS ? feats_out + (clip_base + clip_step * i) * (13 * kNFramesB) : nullptr;
    dct_cmvn_clip<CM>(smem + (i & 1 ? kL1Off : kLOff), slot, smem + kF0Off,
                      reinterpret_cast<uint16_t*>(smem + kB0Off), reinterpret_cast<uint16_t*>(smem + kX0Off), fo,
                      lane);
    signal_set(ctrl, kCtrlLFree + cw, (unsigned)(i + NBF), lane);
  }
};

// The standalone CNN's clip source (wk_cnn: LightweightKWS.forward on caller
// features, the ONNX `run` surface; wk_cnn_fused_kernel, wk_fused.hip).
// FeatSrc copies clip i's CMVN'd features [13][63] (wakeModel.py input layout)
// into the conv1 image as [t][ci] rows: lane t reads its frame's 13
// coefficients (63 lanes of one coefficient are one coalesced 252-byte read).
template <int CM>
struct FeatSrc {
  const float* feats;
  float* base;   // the role's carve base (cnn_role's `base`)
  int64_t clip_base, clip_step;
  int lane;
  __device__ __forceinline__ void init(int, int lane_) { lane = lane_; }
  __device__ __forceinline__ bool ready(int64_t) const { return true; }
  __device__ __forceinline__ void wait(int64_t) const {}
  __device__ __forceinline__ void load(int64_t i, int slot) const {
    const float* f = feats + (clip_base + clip_step * i) * (13 * kNFramesB);
    if (lane >= kNFramesB) return;
    float y[13];
#pragma unroll
    for (int c = 0; c < 13; ++c) y[c] = __builtin_nontemporal_load(f + c * kNFramesB + lane);
    const int row = slot * I0_TP + 1 + lane;
    if constexpr (CM == kConvBf16) {
      uint16_t* B0 = reinterpret_cast<uint16_t*>(base + kB0Off) + row * I0_CIP;
#pragma unroll
      for (int c = 0; c < 12; c += 4)
        *reinterpret_cast<uint2*>(B0 + c) = make_uint2(bf16_bits(y[c]) | (bf16_bits(y[c + 1]) << 16),
                                                       bf16_bits(y[c + 2]) | (bf16_bits(y[c + 3]) << 16));
      B0[12] = (uint16_t)bf16_bits(y[12]);
    } else if constexpr (CM == kConvBf16x3) {
      uint16_t* X0 = reinterpret_cast<uint16_t*>(base + kX0Off) + row * X0_CIP;
#pragma unroll
      for (int c = 0; c < 13; ++c) {
        const uint32_t h = bf16_bits(y[c]);
        X0[c] = (uint16_t)h;
        X0[16 + c] = (uint16_t)bf16_bits(y[c] - __uint_as_float(h << 16));
      }
    } else {
      float* F0 = base + kF0Off + row * F0_CIP;
#pragma unroll
      for (int c = 0; c < 12; c += 4) *reinterpret_cast<f32x4*>(F0 + c) = f32x4{y[c], y[c + 1], y[c + 2], y[c + 3]};
      F0[12] = y[12];
    }
  }
};

}  // namespace
