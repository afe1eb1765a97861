// wk_fe_dev.h -- device code of the MFCC front-end (shared by the standalone
// front-end kernel, wk_frontend.hip, and the fused kernel's front-end role,
// wk_fused_fe_role.h).
// See wk_frontend.hip for the algorithm and the reference citations.
#pragma once
#include "wk_common.h"
#include "wk_fe_lds_layout.h"
#include "wk_tables.h"

namespace wk {

// The helpers the fused kernel shares with the standalone kernels take the
// arithmetic flavour FE (FePacked / FeScalar, wk_common.h) or its complex type
// C = FE::c2; FePacked is the default, which is what the standalone kernels run.

// Raw samples of one frame-group slot, prefetched into registers one round
// ahead (buffer loads: clip base in SGPRs, out-of-range reads return 0):
// x0[n1] = x[r(i0)], x1[n1] = x[r(i0+1)] for i0 = base + 32*n1 + 2j, with
// r() the reflection of torch.stft's centre padding (mode B) -- identity
// except on the two edge frames.  The pre-emphasis partner of each sample is
// a neighbouring lane's value (DPP row rotate), so it is not loaded twice;
// xb covers the one partner outside the slot (lane 0: x[r(base-1)], lane 15:
// x[r(i0(9,15)+2)]).  Kept in the input type so the loads stay outstanding
// until first use.  (The fused kernel loads r() = identity in every round and
// rebuilds the reflected rows in registers: load_raw_part, fe_stage0_rows.)
template <typename T>
struct Raw {
  T x0[10], x1[10];
  T xb;
};

template <typename T> __device__ __forceinline__ T raw_ld(__amdgpu_buffer_rsrc_t r, int idx);
template <> __device__ __forceinline__ float raw_ld<float>(__amdgpu_buffer_rsrc_t r, int idx) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, idx * 4, 0, 0));
}
template <> __device__ __forceinline__ int16_t raw_ld<int16_t>(__amdgpu_buffer_rsrc_t r, int idx) {
  return (int16_t)__builtin_amdgcn_raw_buffer_load_b16(r, idx * 2, 0, 0);
}

// The adjacent pair x[idx], x[idx + 1] as one 8-byte (fp32) / 4-byte (int16)
// load: half the load instructions of two raw_ld (the front-end's loads are
// issue-bound: 8 front-end waves per CU share one load path).
template <typename T> __device__ __forceinline__ void raw_ld2(__amdgpu_buffer_rsrc_t r, int idx, T& a, T& b);
template <> __device__ __forceinline__ void raw_ld2<float>(__amdgpu_buffer_rsrc_t r, int idx, float& a, float& b) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, idx * 4, 0, 0);
  a = __uint_as_float(v[0]);   // (not __builtin_bit_cast of a vector element: miscompiled to v[0] for both)
  b = __uint_as_float(v[1]);
}
template <> __device__ __forceinline__ void raw_ld2<int16_t>(__amdgpu_buffer_rsrc_t r, int idx, int16_t& a,
                                                            int16_t& b) {
  const uint32_t v = __builtin_amdgcn_raw_buffer_load_b32(r, idx * 2, 0, 0);
  a = (int16_t)(v & 0xFFFFu);
  b = (int16_t)(v >> 16);
}

// Reflect index i of the centred (padded) signal of length n into [0, n).
__device__ __forceinline__ int refl_idx(int i, int n) {
  i = i < 0 ? -i : i;
  return i > n - 1 ? 2 * (n - 1) - i : i;
}

// The loader of the standalone front-end (wk_frontend.hip: any win_len, mode
// A) and of wk_scan.hip.  GENERAL (wave-uniform) = this wave-round holds an
// edge frame: per-lane reflected indices, 21 single loads.  Otherwise the 10
// pair loads + xb share one offset VGPR.
// off (GENERAL only): the frame's clip starts `off` samples into the resource
// (wk_scan.hip: the lane groups of one wave hold edge frames of different
// windows of one recording); indices are reflected within the clip first.
template <bool MODE_B, typename T>
__device__ __forceinline__ void load_raw(__amdgpu_buffer_rsrc_t rs, int base, int j, int n, bool act, bool general,
                                         Raw<T>& r, int off = 0) {
  if (!act) return;
  if (!general) {
    const int v0 = base + 2 * j;
#pragma unroll
    for (int n1 = 0; n1 < 10; ++n1) raw_ld2<T>(rs, v0 + 32 * n1, r.x0[n1], r.x1[n1]);
    r.xb = raw_ld<T>(rs, base - 1);   // mode A frame 0: index -1 -> 0 (y[0] = x[0], mfcc.c:70)
  } else {
#pragma unroll
    for (int n1 = 0; n1 < 10; ++n1) {
      const int i0 = base + 32 * n1 + 2 * j;
      r.x0[n1] = raw_ld<T>(rs, off + (MODE_B ? refl_idx(i0, n) : i0));
      r.x1[n1] = raw_ld<T>(rs, off + (MODE_B ? refl_idx(i0 + 1, n) : i0 + 1));
    }
    const int ib = j == 15 ? base + 32 * 9 + 32 : base - 1;
    r.xb = raw_ld<T>(rs, off + (MODE_B ? refl_idx(ib, n) : ib));
  }
}

// Part k (0..3) of the fused kernel's loads: rows n1 with pf_part(n1) == k
// (and xb with part 0), so a round's prefetch can be spread over the round
// instead of issued as one burst (eight waves issuing 11 loads each at once
// filled the TA FIFOs and stalled issue).  Every round issues these same
// unreflected pair loads, the two edge frames (0 and 62) included: their
// reflected rows repeat samples that other rows of the same frame hold, and
// fe_stage0_rows takes them from there (the rows' own loads fall outside the
// clip and return 0).  The one sample no row holds, x[160] for frame 0, comes
// in xb (xb_idx; base - 1 for every other frame).
// The packed flavour front-loads the parts (rows 0-3, 4-6, 7-8, 9) and issues
// them earlier in the round (fe_rest); the scalar flavour issues rows 3k..3k+2.
template <typename FE = FePacked>
__device__ __forceinline__ constexpr int pf_part(int n1) {
  return FE::staged ? n1 / 3 : (n1 < 4 ? 0 : n1 < 7 ? 1 : n1 < 9 ? 2 : 3);
}
template <typename FE = FePacked, typename T>
__device__ __forceinline__ void load_raw_part(__amdgpu_buffer_rsrc_t rs, int base, int xb_idx, int j, Raw<T>& r,
                                              int part) {
  const int v0 = base + 2 * j;
#pragma unroll
  for (int n1 = 0; n1 < 10; ++n1)
    if (pf_part<FE>(n1) == part) raw_ld2<T>(rs, v0 + 32 * n1, r.x0[n1], r.x1[n1]);
  if (part == 0) r.xb = raw_ld<T>(rs, xb_idx);
}

struct NoPrefetch {
  __device__ __forceinline__ void operator()(int) const {}
};

__device__ __forceinline__ float row_ror1(float v) {  // lane l <- lane (l-1) mod 16 of its 16-lane row
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x121, 0xF, 0xF, false));
}
__device__ __forceinline__ float row_rol1(float v) {  // lane l <- lane (l+1) mod 16 of its 16-lane row
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x12F, 0xF, 0xF, false));
}

// Tables of the workgroup (fe_init_tables; layout: wk_fe_lds_layout.h), as
// this lane sees them.
struct FeTables {
  // Analysis window, odd rows n1 negated in lanes j >= 8 (kWinB / kWinA).
  // fe_stage0: the constant table [320] (the standalone kernels read it from
  // L1).  fe_stage0_fused: this lane's window row in LDS, fe_lds::win_row_off(j).
  const float* win;
  // This lane's twiddle row in LDS, fe_lds::row_off(j): W256^(j * (s ^ (j & 8))),
  // s = 0..15, then fe_split_tw(j, k2), k2 = 0..7.
  const float* row;
};

// Two adjacent {re, im} table entries as one 16-byte LDS read (ds_read_b128):
// p is 16-byte aligned (fe_lds: row pitches and entry offsets are multiples of
// 4 floats), and the 16 lanes j of each of the read's lane groups fall on 16
// distinct bank quads.
// Written as two 8-byte loads from an address assumed 16-byte aligned, which
// the load vectoriser joins into the one ds_read_b128 (checked in the ISA:
// no table read may be a ds_read2_b64).  Written as one float4 load, the
// entries reach the arithmetic as shuffles of the loaded vector, and the fp32
// unit's compiler then no longer contracted the window product of row 9 into
// the first DFT16 butterflies (a[1] +- y9 w9 as two v_pk_fma_f32): different
// roundings, different bits.  With this form every unit compiles to the same
// floating-point operations as with the slot-major tables
// (tests/test_gpu_fe_bits.py holds it to them).
template <typename C>
__device__ __forceinline__ void lds_pair16(const float* p, C& a, C& b) {
  const C* q = reinterpret_cast<const C*>(__builtin_assume_aligned(p, 16));
  a = q[0];
  b = q[1];
}

// The real-FFT split pairs bin k = j + 16 k2 (lane j, register k2) with bin
// 256 - k (lane (16 - j) & 15).  After the one-pass transpose of fe_rest the
// lanes j >= 8 hold (-1)^k2 Z[k]; when a lane and its partner hold their
// values with opposite signs, S and D of the split trade places, and the
// twiddle -conj(W) in place of W restores |U|^2 and |U'|^2 exactly:
//   D - i(-conj W) S = i conj(W) (S - i W D),  D + i(-conj W) S = -i conj(W) (S + i W D).
__device__ __forceinline__ bool fe_split_flip(int j, int k2) {
  return j == 8 || (j >= 1 && j <= 7 && !(k2 & 1)) || (j >= 9 && (k2 & 1));
}
template <typename C = f2>
__device__ __forceinline__ C fe_split_tw(int j, int k2) {   // W512^(j + 16 k2), or -conj of it
  float sn, cs;
  sincospif(-(float)(j + 16 * k2) / 256.0f, &sn, &cs);
  return fe_split_flip(j, k2) ? C{-cs, sn} : C{cs, sn};
}

// Stage 0: pre-emphasis + window of the 320 frame samples as 160 complex
// (even, odd) pairs: lane j holds pair index 16*n1 + j, n1 = 0..9.
//   y[i] = x[i] - 0.97 x[i-1], y[0] = x[0]   (torchaudio preemphasis / mfcc.c:66-74)
// On reflected rows (mode B edge frames) y(i0) = x[r] - 0.97 x[r-1] pairs
// each sample with the NEXT one: own x1 for y0, the next lane's x0 for y1.
// This form serves load_raw's GENERAL loads (wk_frontend.hip, wk_scan.hip:
// any clip length, edge frames of several windows in one wave); the fused
// kernel's stage 0 is fe_stage0_fused below.
template <bool MODE_B, typename T>
__device__ __forceinline__ void fe_stage0(const Raw<T>& raw, int base, int n, int j, bool general,
                                          const FeTables& tb, f2 (&a)[16], float pre = -0.97f WK_SP_PARAM) {
  // All ten window pairs are read up front: issued one per iteration they
  // each exposed a full LDS round trip (the edge-frame branch kept the
  // compiler from hoisting them).
  f2 w[10];
#pragma unroll
  for (int n1 = 0; n1 < 10; ++n1) w[n1] = *reinterpret_cast<const f2*>(tb.win + 32 * n1 + 2 * j);
  float prev_rot = 0.0f;
  float y0[10], y1[10];
#pragma unroll
  for (int n1 = 0; n1 < 10; ++n1) {
    const float x0 = to_f(raw.x0[n1]), x1 = to_f(raw.x1[n1]);
    // x[i0-1]: lane j-1's x1 of this row; lane 0 takes lane 15's x1 of the previous row.
    // DPP row rotates read other lanes: they must execute with the whole row
    // active, so they are materialised (asm barrier) before any lane select.
    float rot = row_ror1(x1);
    asm volatile("" : "+v"(rot));
    const float xm = j != 0 ? rot : (n1 == 0 ? to_f(raw.xb) : prev_rot);
    prev_rot = rot;
    y0[n1] = __builtin_fmaf(pre, xm, x0);   // pre = -0.97 (0 for mfcc.c's single-frame variant)
    y1[n1] = __builtin_fmaf(pre, x0, x1);
  }
  // The windowed pairs are formed in each branch, so the two paths merge on
  // a[] (register pairs) rather than on y0/y1 (merging the halves cost ~15
  // v_mov per round to re-pair them on the common path).
  if (MODE_B && general) {   // wave-uniform: the two reflected edge frames only
#pragma unroll
    for (int n1 = 0; n1 < 10; ++n1) {
      const float x0 = to_f(raw.x0[n1]), x1 = to_f(raw.x1[n1]);
      const int i0 = base + 32 * n1 + 2 * j;
      float nx = row_rol1(x0);
      float nx1 = row_rol1(to_f(raw.x0[n1 + 1 < 10 ? n1 + 1 : 9]));
      asm volatile("" : "+v"(nx), "+v"(nx1));
      const float xn = j != 15 ? nx : (n1 < 9 ? nx1 : to_f(raw.xb));
      const bool reflected = i0 < 0 || i0 > n - 1;
      const float r0 = __builtin_fmaf(pre, x1, x0), r1 = __builtin_fmaf(pre, xn, x1);
      const float g0 = reflected ? r0 : (i0 == 0 ? x0 : y0[n1]);
      const float g1 = reflected ? r1 : y1[n1];
      a[n1] = f2{g0, g1} * w[n1];
    }
  } else {
#pragma unroll
    for (int n1 = 0; n1 < 10; ++n1) a[n1] = f2{y0[n1], y1[n1]} * w[n1];
  }
#pragma unroll
  for (int n1 = 10; n1 < 16; ++n1) a[n1] = f2{0.0f, 0.0f};
}

// Stage 0 of the fused kernel (mode B, 16,000-sample clips, Raw filled by
// load_raw_part).  EDGE, wave-uniform: 0 = no edge frame in this wave-round,
// 1 = lane group 0 holds frame 0, 2 = lane group 3 holds frame 62.  The
// centre padding reflects whole rows (tests/test_edge_frame_rows.py):
//   frame 0  (base -160):  rows 0-4 reflected, r0 = r(i0) = 160 - 32 n1 - 2 j;
//                          rows 5-9 hold x[0..159] unreflected, i0 == 0 is row 5 lane 0
//   frame 62 (base 15712): row 9 reflected, r0 = 15998 - 2 j; row 8 holds x[15968..15999]
// and a reflected row needs y(i0) = fma(pre, x[r0-1], x[r0]), y(i0+1) =
// fma(pre, x[r0-2], x[r0-1]).  Those samples sit in the frame's own registers:
//   frame 0:  (x[r0-2], x[r0-1]) is the pair of row 9 - n1, lane 15 - j (row_mirror);
//             x[r0] is the first of row 9 - n1, lane 16 - j (row_shr:1 of the
//             mirrored firsts); lane 0 takes the first of its row 10 - n1, xb = x[160] for row 0
//   frame 62: x[r0] is the first of row 8, lane 15 - j (row_mirror); (x[r0-2],
//             x[r0-1]) is the pair of row 8, lane 14 - j (row_shl:1 of the
//             mirrored pair); lane 15 takes its own row-7 pair (x[15966], x[15967])
// The DPP moves write the edge frame's lane group only (row_mask) and leave
// the other groups' operands in place, so each row is still the common two
// FMAs and the window multiply: no second loop, no per-sample index or
// select, and the same FMA forms as the per-lane reflected loads gave
// (fe_stage0's GENERAL path, which wk_scan.hip and wk_frontend.hip keep).
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_rows(float old, float src) {   // rows outside ROWS, lanes without a source: old
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), CTRL, ROWS, 0xF, false));
}
template <int EDGE, typename T, typename C>
__device__ __forceinline__ void fe_stage0_rows(const Raw<T>& raw, int lane, const C (&w)[10], C (&a)[16], float pre) {
  const int j = lane & 15;
  float prev_rot = 0.0f;
#pragma unroll
  for (int n1 = 0; n1 < 10; ++n1) {
    const float x0 = to_f(raw.x0[n1]), x1 = to_f(raw.x1[n1]);
    // x[i0-1]: lane j-1's x1 of this row; lane 0 takes lane 15's x1 of the previous row.
    // DPP moves read other lanes: they must execute with the whole row
    // active, so they are materialised (asm barrier) before any lane select.
    float rot = row_ror1(x1);
    asm volatile("" : "+v"(rot));
    const float xm = j != 0 ? rot : (n1 == 0 ? to_f(raw.xb) : prev_rot);
    prev_rot = rot;
    // y0 = fma(pre, pm, c0), y1 = fma(pre, p1, c1)
    float c0 = x0, c1 = x1, pm = xm, p1 = x0;
    if constexpr (EDGE == 1) {
      if (n1 < 5) {
        const float m0 = to_f(raw.x0[9 - n1]), m1 = to_f(raw.x1[9 - n1]);
        p1 = dpp_rows<0x140, 0x1>(x0, m0);   // x[r0-2]
        c1 = dpp_rows<0x140, 0x1>(x1, m1);   // x[r0-1]
        pm = dpp_rows<0x140, 0x1>(xm, m1);
        asm volatile("" : "+v"(p1), "+v"(c1), "+v"(pm));
        const float l0 = n1 == 0 ? to_f(raw.xb) : to_f(raw.x0[10 - n1]);
        c0 = dpp_rows<0x111, 0x1>(lane == 0 ? l0 : x0, p1);   // x[r0]
        asm volatile("" : "+v"(c0));
      }
    } else if constexpr (EDGE == 2) {
      if (n1 == 9) {
        const float q0 = to_f(raw.x0[8]), q1 = to_f(raw.x1[8]);
        c0 = dpp_rows<0x140, 0x8>(x0, q0);          // x[r0]
        float s1 = dpp_rows<0x140, 0x8>(x1, q1);    // x[r0+1]
        asm volatile("" : "+v"(c0), "+v"(s1));
        p1 = dpp_rows<0x101, 0x8>(lane == 63 ? to_f(raw.x0[7]) : x0, c0);   // x[r0-2]
        c1 = dpp_rows<0x101, 0x8>(lane == 63 ? to_f(raw.x1[7]) : x1, s1);   // x[r0-1]
        asm volatile("" : "+v"(p1), "+v"(c1));
        pm = lane >= 48 ? c1 : xm;
      }
    }
    float y0 = __builtin_fmaf(pre, pm, c0);   // pre = -0.97
    const float y1 = __builtin_fmaf(pre, p1, c1);
    if (EDGE == 1 && n1 == 5) y0 = lane == 0 ? x0 : y0;   // y[0] = x[0]
    a[n1] = C{y0, y1} * w[n1];
  }
}
template <typename T, typename C>
__device__ __forceinline__ void fe_stage0_fused(const Raw<T>& raw, int lane, int edge, const FeTables& tb,
                                                C (&a)[16], float pre = -0.97f) {
  // All ten window pairs are read up front (see fe_stage0): this lane's
  // window row, five 16-byte reads.
  C w[10];
#pragma unroll
  for (int n1 = 0; n1 < 10; n1 += 2) lds_pair16(tb.win + fe_lds::win_off(0, n1), w[n1], w[n1 + 1]);
  // The windowed pairs are formed in each branch, so the paths merge on a[]
  // (register pairs), as in fe_stage0.
  if (edge == 0) fe_stage0_rows<0>(raw, lane, w, a, pre);
  else if (edge == 1) fe_stage0_rows<1>(raw, lane, w, a, pre);
  else fe_stage0_rows<2>(raw, lane, w, a, pre);
#pragma unroll
  for (int n1 = 10; n1 < 16; ++n1) a[n1] = C{0.0f, 0.0f};
}

// Stages 1..4 of one frame -> its power row (bins 0..256) in LDS.  All
// complex arithmetic is in FE's complex type (f2: packed fp32, f2s: scalar
// pairs; wk_common.h).
// The row (8-byte aligned, kPRow = 270 floats) is also the transpose scratch.
// tb.row: this lane's twiddle row (W256 twiddles, then fe_split_tw(j, k2), k2 = 0..7).
// pf(k), k = 0..3, is called at four points of the round (prefetch parts);
// pf(-1) just before the round's first write into the row.
//
// 256-point complex FFT of the 160 (even, odd) sample pairs, four-step 16 x 16:
//   Z[k1 + 16 k2] = sum_n2 W16^(n2 k2) W256^(n2 k1) sum_n1 W16^(n1 k1) z[16 n1 + n2]
// with lane j = n2 for the first DFT16 and lane kc = k1 for the second.
// One-pass transpose of {re, im} pairs: with h = j & 8 the lanes j >= 8 hold
// their first-pass outputs in slot order k1 ^ 8 (their window rows n1 odd are
// negated: A[k1 ^ 8] = sum_n1 (-1)^n1 W16^(n1 k1) a[n1]), so every lane's
// slots 0-7 are the 8x8 blocks on the diagonal ((n2, k1) in the same half)
// and slots 8-15 the off-diagonal blocks.  Each half is 128 complex values;
// element (n2, k1) of the diagonal half sits at f2 index 17 (n2 & 7) + k1,
// of the other at 17 (n2 & 7) + (k1 ^ 8): lane-uniform immediate offsets for
// the writes (base 17 (j & 7) + h, offset s) and the reads (base kc or kc ^ 8,
// offset 17 s), each 16 lanes on 16 distinct 8-byte bank pairs, and 135
// f2 = 270 floats, inside the frame's own row (the re / im two-pass transpose
// was 16 write2 + 32 reads).
// The second DFT16 then sees its inputs rotated by 8 in lanes kc >= 8, which
// multiplies Z[kc + 16 k2] by (-1)^k2 there; fe_split_tw absorbs the sign.
//
// LDS traffic of one wave-round, in instructions and LDS-array cycles
// (MI355X: ds_read_b128 4, ds_read_b64 2, ds_read2_b64 8 per wave-instruction):
//   window (fused kernel)   5 ds_read_b128    20     (was 5 ds_read2_b64, 40)
//   W256 twiddles           8 ds_read_b128    32     (was 8 ds_read2_b64, 64)
//   split twiddles          4 ds_read_b128    16     (was 3 ds_read2_b64 + 1 ds_read_b64, 26; w0 in 2 VGPRs)
//   transpose writes        8 ds_write2_b64
//   transpose reads         8 ds_read2_b64    64
//   power-row stores        ds_write2_b32 / ds_write_b32 (the two frame groups of a half on
//                           disjoint banks: fe_lds::frame_slot)
// and per clip, in the mel (lane = frame, wk_tables.h): 159 ds_read_b64 of
// aligned bin pairs over the 8 waves, 318 cycles (were 153 ds_read2_b32 + 6
// ds_read_b32, 624: the row pitch was odd, 271, so every second row was only
// 4-byte aligned).  The pitch is 270 = the transpose scratch, which is now the
// row itself.
// The tables are lane-major (wk_fe_lds_layout.h) so that a lane's entries are
// one row read 16 bytes at a time at immediate offsets from tb.row / tb.win:
// SQ_LDS_IDX_ACTIVE per window 7,559 -> 6,618 (16 wave-rounds x 62 cycles
// predicted 992), bank conflicts unchanged; fp32 +2.0 %, bf16 +1.3 %,
// bit-identical (profiles/lds_tables_ab.md).
// The transposes' reads stay the pairs the compiler forms.  As 16 single
// ds_read_b64 (volatile LDS loads, which it does not pair) they are served
// per 32-lane half, and a half holds two frame groups whose rows (then 16 x
// 271 floats apart) started 48 banks apart: 8 of each group's 16 bank pairs
// were the other's (2-way).  Measured so: SQ_LDS_BANK_CONFLICT per window
// 440 -> 936, array cycles up, fp32 +0.1 % over the tables alone (noise),
// bf16 -2.4 %; not kept.  (At today's 8 x 270 floats the rows again start 48
// banks apart.)
template <bool MODE_B, typename FE = FePacked, typename PF>
__device__ __forceinline__ void fe_rest(typename FE::c2 (&a)[16], int j, float* __restrict__ row, const FeTables& tb,
                                        int esp_pack, const PF& pf WK_SP_PARAM) {
  typedef typename FE::c2 C;
  pf(0);
  dft16(a);  // slot s: A[s ^ (j & 8)] at a[dft16_out(s)]
  WK_FE_HIT(2);

  // twiddle W256^(n2 k1), n2 = j, k1 = s ^ (j & 8); each half is twiddled
  // just before it is written (fewer live registers)
  C* x2 = reinterpret_cast<C*>(row);
  const int wb = fe_lds::xpose_wr(j);
  // slots s0, s0 + 1: one 16-byte read of the lane's twiddle row feeds both products
  auto tw2 = [&](int s0, C& b0, C& b1) {
    C wa, wc;
    lds_pair16(tb.row + fe_lds::tw_off(0, s0), wa, wc);
    b0 = cmul2(a[dft16_out(s0)], wa);
    b1 = cmul2(a[dft16_out(s0 + 1)], wc);
  };
  C b[8];
  if constexpr (!FE::staged) pf(1);
#pragma unroll
  for (int s = 0; s < 8; s += 2) tw2(s, b[s], b[s + 1]);
  pf(-1);   // the first write into this frame's LDS row follows (fused kernel: wait until the row is free)
#pragma unroll
  for (int s = 0; s < 8; ++s) x2[wb + s] = b[s];
  WK_FE_HIT(3);
  if constexpr (FE::staged) pf(1);
  C c[16];
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 8; ++s) c[s] = x2[fe_lds::xpose_rd(j, s)];
  // The packed flavour issues prefetch parts 1-3 one step earlier than the
  // scalar one (part 1 before the twiddles, part 2 after these reads, part 3
  // before the second DFT16 rather than after it): the loads get ~1 k more
  // cycles to land before the next round needs them; with the front-loaded
  // parts, fp32 +1.5 % (profiles/r06u..r06x); the scalar unit
  // measured -0.5 to 0 % with the earlier parts 2-3.
  if constexpr (!FE::staged) pf(2);
#pragma unroll
  for (int s = 8; s < 16; s += 2) tw2(s, b[s - 8], b[s - 7]);
  wave_lds_sync();
#pragma unroll
  for (int s = 8; s < 16; ++s) x2[wb + s - 8] = b[s - 8];
  wave_lds_sync();
#pragma unroll
  for (int s = 8; s < 16; ++s) c[s] = x2[fe_lds::xpose_rd(j ^ 8, s - 8)];
  wave_lds_sync();
  WK_FE_HIT(4);

  if constexpr (FE::staged) {
    pf(2);
    dft16(c);  // +-Z[j + 16*k2] at c[dft16_out(k2)]
    pf(3);
  } else {
    pf(3);
    dft16(c);
  }
  WK_FE_HIT(5);

  // Real-FFT split, k = j + 16*k2 (k2 = 0..7), with the partner Z[256 - k]:
  //   S = Z[k] + conj Z[256-k],  D = Z[k] - conj Z[256-k],  bb = W512^k D,
  //   U = 2 X[k] = S - i bb,  U' = conj(2 X[256-k]) = S + i bb
  // (mode B folds the 1/4 of |X|^2 = |U|^2/4 into the filterbank weights).
  // {|U|^2, |U'|^2} is one packed pair: {Ux, U'x}^2 + {Uy, U'y}^2.
  // Partner: lane (16-j)&15 of this group, register 15-k2, fetched by two DPP
  // row moves (row_mirror: j <- 15-j, then row_shr:1: j <- j-1), no LDS trip;
  // lane 0 holds its own partner in register (16-k2)&15.  The twiddle is one
  // value per (lane, k2), sign-adjusted by fe_split_tw: the second part of
  // the lane's twiddle row, read two entries at a time (wsp) by the first
  // group of chains that needs them.
  C sc0 = {1.0f, 1.0f}, sc = {1.0f, 1.0f};
  if constexpr (!MODE_B) {
    // mfcc.c:267 power = |X|^2 / n_fft + 1e-12 = |U|^2 / 2048 + 1e-12; the
    // esp-dsp dsps_cplx2reC_fc32 packing (mfcc.c:261) doubles bins 1..255
    // (x4 in power) and zeroes bin 256 (parity unpinned).
    const float e = esp_pack ? 4.0f / 2048.0f : 1.0f / 2048.0f;
    sc = C{e, e};
    sc0 = esp_pack ? (j == 0 ? C{1.0f / 2048.0f, 0.0f} : sc) : sc;  // j==0, k2==0: bins 0 and 256
  }
  {
    // bin 128 (k2 = 8, column 0): X[128] = conj Z[128], so |U|^2 = 4 |Z[128]|^2.
    const C z = c[dft16_out(8)];
    float p128 = 4.0f * __builtin_fmaf(z.x, z.x, z.y * z.y);
    if constexpr (!MODE_B) p128 = __builtin_fmaf(p128, sc.x, 1e-12f);
    if (j == 0) row[128] = p128;
  }
  // The eight k2 chains are ~20 dependent packed ops each; run them G at a
  // time, stage by stage, so independent ops fill each other's latency
  // (left to itself the scheduler emitted them back to back, one chain at a
  // time, with s_nop between dependent v_pk ops).
  // FE::staged (the bf16 family's scalar front-end, FeScalar in wk_common.h)
  // also issues the group's DPP moves and each chain stage across the group: the
  // same operations per value, bit-identical, bf16 +0.8 % (profiles/
  // r06m_staged_ab.txt); the packed fp32 unit measured -0.1 % with it, so
  // it keeps the per-chain order.
  constexpr int G = 3;
  C wsp[8];
#pragma unroll
  for (int k0 = 0; k0 < 8; k0 += G) {
    C S[G], D[G], pw[G];
#pragma unroll
    for (int q = 0; q < 8; q += 2)
      if (q / G * G == k0) lds_pair16(tb.row + fe_lds::split_off(0, q), wsp[q], wsp[q + 1]);
    if constexpr (FE::staged) {
      // the partners' row_mirror moves of the group first, then their row_shr
      // moves (a DPP read of a VGPR written by the previous VALU op waits 2 states)
      float mx[G], my[G];
#pragma unroll
      for (int t = 0; t < G; ++t)
        if (k0 + t <= 7) {
          const C sv = c[dft16_out(15 - k0 - t)];
          mx[t] = dpp<0x140>(sv.x);
          my[t] = dpp<0x140>(sv.y);
        }
#pragma unroll
      for (int t = 0; t < G; ++t) {
        const int k2 = k0 + t;
        if (k2 > 7) continue;
        const C zk = c[dft16_out(k2)];
        const C own = c[dft16_out((16 - k2) & 15)];
        C zq;
        zq.x = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(own.x), __float_as_int(mx[t]), 0x111, 0xF, 0xF, false));
        zq.y = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(own.y), __float_as_int(my[t]), 0x111, 0xF, 0xF, false));
        S[t] = fma2(zq, C{1.0f, -1.0f}, zk);
        D[t] = fma2(zq, C{-1.0f, 1.0f}, zk);
      }
      // the G chains issued stage by stage (the same operations per value)
      C wt[G], tt[G], bb[G], uvx[G], uvy[G], sq[G];
#pragma unroll
      for (int t = 0; t < G; ++t)
        if (k0 + t <= 7) {
          wt[t] = wsp[k0 + t];
          tt[t] = cmul2_a(D[t], wt[t]);
        }
#pragma unroll
      for (int t = 0; t < G; ++t)
        if (k0 + t <= 7) bb[t] = cmul2_b(D[t], wt[t], tt[t]);
#pragma unroll
      for (int t = 0; t < G; ++t)
        if (k0 + t <= 7) {
          uvx[t] = fma2(by(bb[t]), C{1.0f, -1.0f}, bx(S[t]));
          uvy[t] = fma2(bx(bb[t]), C{-1.0f, 1.0f}, by(S[t]));
        }
#pragma unroll
      for (int t = 0; t < G; ++t)
        if (k0 + t <= 7) sq[t] = uvy[t] * uvy[t];
#pragma unroll
      for (int t = 0; t < G; ++t) {
        const int k2 = k0 + t;
        if (k2 > 7) continue;
        pw[t] = fma2(uvx[t], uvx[t], sq[t]);
        if constexpr (!MODE_B) pw[t] = fma2(pw[t], k2 == 0 ? sc0 : sc, C{1e-12f, 1e-12f});
      }
    } else {
#pragma unroll
      for (int t = 0; t < G; ++t) {
        const int k2 = k0 + t;
        if (k2 > 7) continue;
        const C zk = c[dft16_out(k2)];
        const C sv = c[dft16_out(15 - k2)];
        const C own = c[dft16_out((16 - k2) & 15)];
        // row_mirror (lane j <- 15 - j), then row_shr:1 (lane j <- j - 1) with
        // bound_ctrl off: lane 0 has no source and keeps `old` = its own
        // partner register -- no lane select.
        C zq;
        zq.x = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(own.x), __float_as_int(dpp<0x140>(sv.x)),
                                                          0x111, 0xF, 0xF, false));
        zq.y = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(own.y), __float_as_int(dpp<0x140>(sv.y)),
                                                          0x111, 0xF, 0xF, false));
        S[t] = fma2(zq, C{1.0f, -1.0f}, zk);
        D[t] = fma2(zq, C{-1.0f, 1.0f}, zk);
      }
#pragma unroll
      for (int t = 0; t < G; ++t) {
        const int k2 = k0 + t;
        if (k2 > 7) continue;
        const C bb = cmul2(D[t], wsp[k2]);
        const C uvx = fma2(by(bb), C{1.0f, -1.0f}, bx(S[t]));
        const C uvy = fma2(bx(bb), C{-1.0f, 1.0f}, by(S[t]));
        pw[t] = fma2(uvx, uvx, uvy * uvy);
        if constexpr (!MODE_B) pw[t] = fma2(pw[t], k2 == 0 ? sc0 : sc, C{1e-12f, 1e-12f});
      }
    }
    // the group's low bins first, then its high bins: same-base stores 16
    // dwords apart, back to back, which the compiler pairs into ds_write2_b32
#pragma unroll
    for (int t = 0; t < G; ++t)
      if (k0 + t <= 7) row[j + 16 * (k0 + t)] = pw[t].x;
#pragma unroll
    for (int t = 0; t < G; ++t)
      if (k0 + t <= 7) row[256 - j - 16 * (k0 + t)] = pw[t].y;
  }
  WK_FE_HIT(6);
}

template <bool MODE_B, int W>
__device__ __forceinline__ void mel_wave(const float* p, float* l) {
  if constexpr (MODE_B) melB_wave<W>(p, l); else melA_wave<W>(p, l);
}

template <bool MODE_B>
__device__ __forceinline__ void mel_dispatch(int wave, const float* p, float* l) {
  switch (wave) {
    case 0: mel_wave<MODE_B, 0>(p, l); break;
    case 1: mel_wave<MODE_B, 1>(p, l); break;
    case 2: mel_wave<MODE_B, 2>(p, l); break;
    case 3: mel_wave<MODE_B, 3>(p, l); break;
    case 4: mel_wave<MODE_B, 4>(p, l); break;
    case 5: mel_wave<MODE_B, 5>(p, l); break;
    case 6: mel_wave<MODE_B, 6>(p, l); break;
    default: mel_wave<MODE_B, 7>(p, l); break;
  }
}

// CMVN over the 63 lanes of one coefficient row (extract_mfcc.py:76-80):
// mean, unbiased std, std==0 -> 1, (x - mean) / (std + 1e-8).
//
// A row of equal values (digital silence: every frame has the same bits) has
// std == 0 and normalises to 0.0 in the reference.  In fp32 the sum of 63 equal
// values divided by 63 need not round to the value: then x - mean was an ulp in
// every lane and the whole row came out +-sqrt(62/63).  Such a row is therefore
// taken as a row of zeros, whose statistics are exact; a row with any two
// values different is untouched.  dct_cmvn_clip (wk_fused_cnn_role.h) and
// wk_normalize_kernel (wk_misc.hip) follow the same rule.
// (The ballot is a statement of its own, outside any select: every lane takes part.)
__device__ __forceinline__ bool cmvn_row_is_flat(float v, bool valid) {
  const float p = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__float_as_int(v), 0));   // frame 0: always valid
  return __builtin_amdgcn_ballot_w64(valid & (v != p)) == 0;
}

__device__ __forceinline__ float cmvn_lane(float v, bool valid, int n) {
  const bool flat = cmvn_row_is_flat(v, valid);
  v = flat ? 0.0f : v;
  const float mean = wave_sum(valid ? v : 0.0f) / (float)n;
  const float d = valid ? v - mean : 0.0f;
  float sd = sqrtf(wave_sum(d * d) / (float)(n - 1));
  sd = sd == 0.0f ? 1.0f : sd;
  return d * (1.0f / (sd + 1e-8f));   // wave-uniform reciprocal
}

// Two independent coefficient rows at once (interleaved reductions).
__device__ __forceinline__ void cmvn_lane2(float& v0, float& v1, bool valid, int n) {
  const bool flat0 = cmvn_row_is_flat(v0, valid), flat1 = cmvn_row_is_flat(v1, valid);
  v0 = flat0 ? 0.0f : v0;
  v1 = flat1 ? 0.0f : v1;
  const float m0 = wave_sum(valid ? v0 : 0.0f) / (float)n;
  const float m1 = wave_sum(valid ? v1 : 0.0f) / (float)n;
  const float d0 = valid ? v0 - m0 : 0.0f;
  const float d1 = valid ? v1 - m1 : 0.0f;
  float s0 = sqrtf(wave_sum(d0 * d0) / (float)(n - 1));
  float s1 = sqrtf(wave_sum(d1 * d1) / (float)(n - 1));
  s0 = s0 == 0.0f ? 1.0f : s0;
  s1 = s1 == 0.0f ? 1.0f : s1;
  v0 = d0 * (1.0f / (s0 + 1e-8f));
  v1 = d1 * (1.0f / (s1 + 1e-8f));
}

// LDS carve (floats; fe_lds::carve): twiddle rows [16 lanes][52] | log-mel
// [40][64] | power rows [63][270] | window rows [16 lanes][20].  The standalone
// front-end stops before the window (it reads the window from the constant
// table: kFeLdsNoWin keeps two workgroups per CU); the fused kernel copies it
// to LDS.
constexpr fe_lds::Carve kFeCarve = fe_lds::carve(WK_LSTRIDE, kNFramesB, kPRow);
constexpr int kTabOff = kFeCarve.tab, kTabSize = fe_lds::kTabSize;
constexpr int kLOff = kFeCarve.logmel, kLSize = 40 * WK_LSTRIDE;
constexpr int kPOff = kFeCarve.power, kPSize = kNFramesB * kPRow;
constexpr int kFeLdsNoWin = kFeCarve.end_no_win;
constexpr int kWinOff = kFeCarve.win, kWinSize = fe_lds::kWinSize;
constexpr int kFeLds = kFeCarve.end;
static_assert(kFeLdsNoWin * 4 <= fe_lds::kStandaloneLimitBytes, "standalone front-end LDS must allow 2 workgroups per CU");
static_assert(kLOff % 4 == 0, "log-mel rows are read with ds_read_b128");
static_assert(kTabOff % 4 == 0 && fe_lds::kRowPitch % 4 == 0 && kWinOff % 4 == 0 && fe_lds::kWinPitch % 4 == 0,
              "table rows are read with ds_read_b128 (the carve's base is 16-byte aligned)");
static_assert(kPOff % 2 == 0 && kPRow % 2 == 0 && kPRow >= fe_lds::kXposeFloats && kPRow >= 258,
              "a power row is 8-byte aligned: it is its own transpose scratch and the mel reads it as pairs of bins");
static_assert(fe_lds::mel_rows_conflict_free(kPRow), "lane-per-frame ds_read_b64: 32 lanes on 32 distinct bank pairs");

// Fill the twiddle rows (and the window rows, WIN) of the LDS carve (all threads of the WG).
// FE: the split twiddles pass through the flavour's complex type, as the rest
// of the kernel's arithmetic does (built in f2 inside a scalar kernel, the
// same values came out as different device code).
template <bool MODE_B, bool WIN, typename FE = FePacked>
__device__ __forceinline__ void fe_init_tables(float* smem, int tid, int nthreads) {
  if (WIN)
    for (int i = tid; i < 320; i += nthreads) {
      const int n1 = i / 32, jj = (i % 32) / 2, c = i & 1;   // i == fe_lds::win_src(jj, n1) + c
      smem[kWinOff + fe_lds::win_off(jj, n1) + c] = MODE_B ? kWinB[i] : kWinA[i];
    }
  for (int i = tid; i < 16 * 16; i += nthreads) {
    const int s = i / 16, jj = i % 16, k1 = s ^ (jj & 8);
    float sn, cs;
    sincospif(-(float)(jj * k1) / 128.0f, &sn, &cs);
    smem[kTabOff + fe_lds::tw_off(jj, s)] = cs;
    smem[kTabOff + fe_lds::tw_off(jj, s) + 1] = sn;
  }
  for (int i = tid; i < 8 * 16; i += nthreads) {
    const int k2 = i / 16, jj = i % 16;
    const typename FE::c2 w = fe_split_tw<typename FE::c2>(jj, k2);
    smem[kTabOff + fe_lds::split_off(jj, k2)] = w.x;
    smem[kTabOff + fe_lds::split_off(jj, k2) + 1] = w.y;
  }
}

// The tables as lane j sees them.  win: the constant table (standalone
// kernels, fe_stage0) or null = the window rows in LDS (fused kernel, fe_stage0_fused).
__device__ __forceinline__ FeTables fe_tables(const float* smem, int j, const float* win_const) {
  return {win_const ? win_const : smem + kWinOff + fe_lds::win_row_off(j), smem + kTabOff + fe_lds::row_off(j)};
}

}  // namespace wk
