// wk_ctc_logmel.hip -- X1 of the GRU-CTC head (wk_ctc.hip): audio -> log-mel 80
// + global z-score (ctc.py:82-107).
//
// Kernels:
//   ctc_logmel_fft2_kernel reflect-padded frames x periodic Hann(400) -> 400-point
//                         real DFT (two frames per complex 20 x 20 four-step FFT)
//                         -> power -> HTK mel -> ln(+1e-8), fused; optionally the
//                         z-score's per-pass partial sums.
//   ctc_zstats_kernel     {mean, 1/std} per utterance from those partials.
//   ctc_zscore_kernel     one block per utterance, two-pass mean / unbiased std.
// Host:
//   mel_fbank, pick_mel_windows, ctc_logmel_tables   the kernel's window, twiddle
//                         and straight-line mel-window tables.
//   ctc_logmel_layout     grid, passes per wave and statistics slots of a launch.
#include <math.h>

#include <algorithm>
#include <functional>

#include "wk_ctc_dev.h"

using namespace wk;

namespace {

// ---------------------------------------------------------------------------
// X1: log-mel.  The 400-point DFT is 20 x 20 four-step (n = 20 n1 + n2,
// k = k1 + 20 k2), each DFT-20 4 x DFT-5 + constant twiddles + 5 x DFT-4 in
// packed fp32 (ctc_logmel_fft2_kernel below).
// ---------------------------------------------------------------------------
// W20^e = exp(-2 pi i e / 20).
__constant__ constexpr float kW20c[20] = {1.000000000e+00f, 9.510565163e-01f, 8.090169944e-01f, 5.877852523e-01f, 3.090169944e-01f, 0.000000000e+00f, -3.090169944e-01f, -5.877852523e-01f, -8.090169944e-01f, -9.510565163e-01f, -1.000000000e+00f, -9.510565163e-01f, -8.090169944e-01f, -5.877852523e-01f, -3.090169944e-01f, 0.000000000e+00f, 3.090169944e-01f, 5.877852523e-01f, 8.090169944e-01f, 9.510565163e-01f};
__constant__ constexpr float kW20s[20] = {0.000000000e+00f, -3.090169944e-01f, -5.877852523e-01f, -8.090169944e-01f, -9.510565163e-01f, -1.000000000e+00f, -9.510565163e-01f, -8.090169944e-01f, -5.877852523e-01f, -3.090169944e-01f, 0.000000000e+00f, 3.090169944e-01f, 5.877852523e-01f, 8.090169944e-01f, 9.510565163e-01f, 1.000000000e+00f, 9.510565163e-01f, 8.090169944e-01f, 5.877852523e-01f, 3.090169944e-01f};
__device__ __forceinline__ f2 w20(int e) { return f2{kW20c[e % 20], kW20s[e % 20]}; }

// In-register DFT-5 (forward), natural order in and out.
__device__ __forceinline__ void dft5(f2& x0, f2& x1, f2& x2, f2& x3, f2& x4) {
  constexpr float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;
  constexpr float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;
  const f2 t1 = x1 + x4, t2 = x2 + x3, t3 = x1 - x4, t4 = x2 - x3;
  const f2 a1 = fma2(f2{c2, c2}, t2, fma2(f2{c1, c1}, t1, x0));
  const f2 a2 = fma2(f2{c1, c1}, t2, fma2(f2{c2, c2}, t1, x0));
  const f2 b1 = fma2(f2{s2, s2}, t4, f2{s1, s1} * t3);   // Y1 = a1 - i b1, Y4 = a1 + i b1
  const f2 b2 = fma2(f2{-s1, -s1}, t4, f2{s2, s2} * t3); // Y2 = a2 - i b2, Y3 = a2 + i b2
  x0 = x0 + t1 + t2;
  x1 = sub_ib(a1, b1);
  x4 = add_ib(a1, b1);
  x2 = sub_ib(a2, b2);
  x3 = add_ib(a2, b2);
}

// In-register DFT-20 (forward): x[0..19] natural order -> X[k] in x[k].
// n = 4 m + r: DFT-5 over m per r, twiddle W20^(r ka), DFT-4 over r per ka;
// X[ka + 5 kb] comes out of the DFT-4 of column ka at position kb.
__device__ __forceinline__ void dft20(f2 (&x)[20]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) dft5(x[r], x[4 + r], x[8 + r], x[12 + r], x[16 + r]);   // B[r][ka] at x[4 ka + r]
#pragma unroll
  for (int r = 1; r < 4; ++r)
#pragma unroll
    for (int ka = 1; ka < 5; ++ka) x[4 * ka + r] = cmulc(x[4 * ka + r], w20(r * ka));
  f2 y[20];
#pragma unroll
  for (int ka = 0; ka < 5; ++ka) {
    f2 b0 = x[4 * ka], b1 = x[4 * ka + 1], b2 = x[4 * ka + 2], b3 = x[4 * ka + 3];
    dft4(b0, b1, b2, b3);
    y[ka] = b0;
    y[ka + 5] = b1;
    y[ka + 10] = b2;
    y[ka + 15] = b3;
  }
#pragma unroll
  for (int k = 0; k < 20; ++k) x[k] = y[k];
}


// ---------------------------------------------------------------------------
// X1, two frames per complex FFT (round 3).  The 400-point DFT of a real frame
// wastes half of a complex FFT, so a lane group runs one complex four-step FFT
// on z = x_a + i x_b of two frames and separates the spectra afterwards:
// X_a[k] = (Z[k] + conj Z[400-k]) / 2, X_b[k] = (Z[k] - conj Z[400-k]) / (2i).
// Lane (g = lane / 20, q = lane % 20) of a wave owns frame pair g (rows
// 6 ps + 2 g, + 1; lanes 60-63 idle):
//   stage 1: lane (g, n2 = q): DFT-20 over n1 of z[20 n1 + n2] -> A[n2][k1],
//            all 20 k1 (no conjugate symmetry for a complex input);
//   stage 2: lane (g, k1 = q): twiddle W400^(n2 k1), DFT-20 over n2 ->
//            Z[k1 + 20 k2] in v[k2];
//   exchange: the partner of bin k1 + 20 k2 is 400 - k1 - 20 k2 =
//            (20 - k1) + 20 (19 - k2) in lane 20 - k1 (k1 > 0), or
//            20 (20 - k2) in the lane itself (k1 = 0): every lane publishes
//            v[10..19] (lane 0 also v[0]) and reads its partner's, one LDS
//            round trip;
//   power:   |Z[k] + conj Z'|^2 and |Z[k] - conj Z'|^2 for k = q + 20 k2,
//            k2 = 0..9 (bin 200 by lane 0), stored as {P_a, P_b} pairs; the
//            1/4 of the separation rides in the mel weights (exact);
//   mel:     straight-line per-lane windows (weights in registers), one
//            8-byte read per pair and tap feeding two FMAs, then ln(+1e-8).
// The separation is exact only in exact arithmetic: in fp32 each frame of a
// pair receives the FFT's rounding asymmetry of the other, <= ~1e-13 of the
// partner's power per bin.  Against a frame with any signal at a supported
// level (down to 1e-3 of full scale) that is below its own rounding; against
// an all-zero frame (zero padding, digital silence) next to int16-scaled
// audio it is ~1e-4 per bin, far above the 1e-8 floor.  So a frame whose 400
// loaded samples are all exactly zero is given power exactly 0: its lane
// group votes on the raw samples, and the row's mel sums are zeroed ahead of
// the logarithm (wave-uniform branches, taken only by passes that hold such
// a frame).  Every mel value of the frame is then ln(1e-8f) bit for bit and
// its STATS terms are exactly 0.  A quiet but non-zero frame keeps the leak.
// One 12-wave workgroup per CU (3 waves per SIMD), the tables once per CU.
// LDS pitches (see the per-access notes) keep the stage-1 writes, stage-2
// reads and pair-power writes free of bank conflicts.
// ---------------------------------------------------------------------------
constexpr int kF2Waves = 12, kF2Pairs = 3;
constexpr int kTwPitch = 21;    // twiddle rows (float2): stage-2 reads, lane = k1
constexpr int kMelW1 = 8, kMelW2 = 7;   // mel windows: mels 0-63 <= 8 bins, mels 64-79 <= 14 = 2 x 7 (host-checked)
constexpr int kA2Pitch = 25;    // A[g][n2][k1] rows (float2): 25 = 1 mod 8 -> stage-2 lane groups start 40 banks apart
constexpr int kE2Pitch = 11;   // exchange rows (float2): 22 dwords -> 20 partner rows on distinct banks
                                // (pitch 12 put them on 8 bank pairs: 24 p mod 64 has period 8)
constexpr int kP2Pitch = 212;   // pair-power rows (float2): 2 x 212 = 40 mod 64 banks between lane groups
static_assert(kF2Pairs * kP2Pitch <= kF2Pairs * 20 * kA2Pitch, "power rows alias the A region");
static_assert(kF2Pairs * 20 * kE2Pitch <= kF2Pairs * 20 * kA2Pitch, "exchange rows alias the A region");
struct CtcFft2Lds {
  float win[kNfft];
  f2 tw[20][kTwPitch];
  f2 w[kF2Waves][kF2Pairs * 20 * kA2Pitch];   // per wave: A, then the exchange, then the power rows
};

// Passes (6 rows each) are dealt to the waves in contiguous ranges of R
// (wave W takes passes [W R, W R + R)), so a wave walks its rows in order: the
// (utterance, frame) of its rows advance by addition, with one division per
// range rather than per pass.
//
// STATS (wk_ctc_transcribe, fp16 mode, T >= 6): the features stay un-normalised
// and each wave also leaves, per utterance its range touches, the sums of
// (x - K) and (x - K)^2 over that utterance's log-mel values x in its rows, with
// K = ln(1e-8) the floor of x (so a silent utterance sums to exactly 0): lanes
// keep running sums while the utterance lasts and reduce them across the wave
// only when it changes (2-3 times per range instead of once per pass).  Slot
// part[W MS + j] holds the range's j-th utterance; ctc_zstats_kernel folds the
// slots into each utterance's mean and 1/std, which the encoder applies as it
// loads.
__device__ __forceinline__ float row16_sum(float v) {   // every lane: the sum over its 16-lane row (DPP)
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x124, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128, 0xF, 0xF, false));
  return v;
}
template <bool STATS>
__global__ __launch_bounds__(kF2Waves * 64, 1) void ctc_logmel_fft2_kernel(const float* __restrict__ audio, int64_t stride,
                                                                            int n_valid, int n_pad, int T, int64_t rows,
                                                                            const float* __restrict__ win_g,
                                                                            const float* __restrict__ tw_g,
                                                                            const float* __restrict__ melw,
                                                                            const int* __restrict__ melws,
                                                                            float* __restrict__ feats,
                                                                            int64_t R, int MS,
                                                                            float2* __restrict__ part) {
  __shared__ CtcFft2Lds L;
  constexpr int NT = kF2Waves * 64;
  for (int i = threadIdx.x; i < kNfft; i += NT) L.win[i] = win_g[i];
  for (int i = threadIdx.x; i < 400; i += NT) L.tw[i / 20][i % 20] = f2{tw_g[2 * i], tw_g[2 * i + 1]};
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform (buffer resources)
  const int g = lane / 20, q = lane - 20 * (lane / 20);   // pair slot (3 = idle lanes 60-63), n2 / k1
  f2* A = L.w[wv];
  typedef volatile __attribute__((address_space(3))) f2 vlf2;
#define LM_R(p, i) (*(const vlf2*)((p) + (i)))
#define LM_W(p, i, val) (*(vlf2*)((p) + (i)) = (val))
  constexpr int kRowsPerPass = 2 * kF2Pairs;
  const int64_t passes = (rows + kRowsPerPass - 1) / kRowsPerPass;
  const int64_t wid = (int64_t)blockIdx.x * kF2Waves + wv;
  const int64_t p_beg = wid * R, p_end = p_beg + R < passes ? p_beg + R : passes;
  const int nv_min = n_valid < n_pad ? n_valid : n_pad;
  // The lane's 20 samples x[20 n1 + q] of one frame (row) of pass ps_; idle
  // lanes and rows past the end read utterance 0's first samples (nothing
  // they compute is stored).  Wave-uniform paths, exactly 20 loads each.
  auto load_one = [&](bool live, int b, int t, float (&raw)[20]) {
    const float* xa = audio + (int64_t)(live ? b : 0) * stride;
    const int p0 = live ? t * kHop - kNfft / 2 : 0;
    if (__all(p0 >= 0 && p0 + kNfft <= nv_min)) {
      const float* xp = xa + p0 + q;
#pragma unroll
      for (int n1 = 0; n1 < 20; ++n1) raw[n1] = xp[20 * n1];
    } else {
#pragma unroll
      for (int n1 = 0; n1 < 20; ++n1) {
        int p = p0 + 20 * n1 + q;
        p = p < 0 ? -p : p;
        p = p > n_pad - 1 ? 2 * (n_pad - 1) - p : p;
        const bool in = p < n_valid;
        const float x = xa[in ? p : 0];
        raw[n1] = in ? x : 0.0f;
      }
    }
  };
  // The pass to load next: its first row (utterance lb, frame lt; wave-
  // uniform) advances by 6 per pass.  Frame a of the lane group's pair is row
  // 2 g after it, frame b the next row (t + 1, or frame 0 of the next utterance).
  int64_t lrow = p_beg * kRowsPerPass;
  int lb = (int)((unsigned)(lrow < rows ? lrow : 0) / (unsigned)T);   // rows < 2^31 (host check)
  int lt = (int)(lrow < rows ? lrow : 0) - lb * T;
  auto load_pair = [&](bool pass_live, float (&ra_)[20], float (&rb_)[20]) {
    const int64_t row = lrow + 2 * g;
    const bool live_a = g < kF2Pairs && pass_live && row < rows;
    const bool live_b = live_a && row + 1 < rows;
    int ba = lb, ta = lt + 2 * g;
    while (ta >= T) {   // (once at most for T >= 5)
      ta -= T;
      ++ba;
    }
    const bool wrap = ta + 1 == T;
    load_one(live_a, ba, ta, ra_);
    load_one(live_b, wrap ? ba + 1 : ba, wrap ? 0 : ta + 1, rb_);
    lrow += kRowsPerPass;
    lt += kRowsPerPass;
    while (lt >= T) {
      lt -= T;
      ++lb;
    }
  };
  // the lane's mel windows: mel `lane` (kMelW1 taps from bin ws1) and half
  // `lane & 1` of mel 64 + lane / 2 (kMelW2 taps from ws2; lanes >= 32: zero weights)
  float mw1[kMelW1], mw2[kMelW2];
#pragma unroll
  for (int j = 0; j < kMelW1; ++j) mw1[j] = melw[lane * kMelW1 + j];
#pragma unroll
  for (int j = 0; j < kMelW2; ++j) mw2[j] = melw[64 * kMelW1 + lane * kMelW2 + j];
  const int ws1 = melws[lane], ws2 = melws[64 + lane];
  float ra[20], rb[20];
  int ta_cur = lt;   // frame index of the current pass's first row in its utterance
  load_pair(p_beg < p_end, ra, rb);
  const bool lact = g < kF2Pairs;
  // STATS: the lane's running sums for the current utterance ({x, y}: its two
  // filters), and the slot of the next one to flush
  f2 s_run = {0.0f, 0.0f}, q_run = {0.0f, 0.0f};
  int seg = 0;
  auto flush = [&]() {   // (wave-uniform) reduce the running sums over the wave into the next slot
    float t0 = sum_rows4(row16_sum(s_run.x + s_run.y));
    float t1 = sum_rows4(row16_sum(q_run.x + q_run.y));
    if (lane == 0) part[wid * MS + seg] = make_float2(t0, t1);
    ++seg;
    s_run = f2{0.0f, 0.0f};
    q_run = f2{0.0f, 0.0f};
  };
  for (int64_t ps = p_beg; ps < p_end; ++ps) {
    const int ta_pass = ta_cur;
    ta_cur = lt;   // (the next pass's, before load_pair advances it)
    // stage 1: lane (g, n2 = q): DFT-20 over n1 of z[20 n1 + n2] = w (x_a + i x_b)
    f2 v[20];
    {
      // All twenty window reads first (one LDS wait), then the products; the
      // memory clobber after them keeps the next pass's loads behind the
      // products.  (A clobber per product had serialised the window reads:
      // twenty LDS round trips per pass, each waited for.)
      float wn[20];
#pragma unroll
      for (int n1 = 0; n1 < 20; ++n1) wn[n1] = L.win[20 * n1 + q];
#pragma unroll
      for (int n1 = 0; n1 < 20; ++n1) {
        v[n1] = f2{ra[n1], rb[n1]} * f2{wn[n1], wn[n1]};
        asm volatile("" ::"v"(v[n1].x), "v"(v[n1].y));
      }
      asm volatile("" ::: "memory");   // ahead of the next pass's loads
    }
    // All-zero frames (see the header): the lane groups vote on the raw
    // samples (sign bit aside: -0 is zero) before the next pass's overwrite
    // them -- first on the 20 centre samples 200 + q alone, and only a wave
    // with a frame whose centre is all zero looks at the rest.  Bit f of zmask
    // (wave-uniform): row f of the pass is all zero.
    constexpr unsigned long long kGrp = 0xFFFFFull;   // a lane group's 20 lanes
    auto zero_groups = [&](unsigned long long nz) {   // bit 2 g: group g has no lane set in nz
      return ((nz & kGrp) == 0 ? 1u : 0u) | ((nz >> 20 & kGrp) == 0 ? 4u : 0u) | ((nz >> 40 & kGrp) == 0 ? 16u : 0u);
    };
    unsigned zmask = 0;
    if (zero_groups(__ballot((__float_as_uint(ra[10]) << 1) != 0)) | zero_groups(__ballot((__float_as_uint(rb[10]) << 1) != 0))) {
      unsigned ba = 0, bb = 0;
#pragma unroll
      for (int n1 = 0; n1 < 20; n1 += 2) {
        ba |= __float_as_uint(ra[n1]) | __float_as_uint(ra[n1 + 1]);
        bb |= __float_as_uint(rb[n1]) | __float_as_uint(rb[n1 + 1]);
      }
      zmask = zero_groups(__ballot((ba << 1) != 0)) | zero_groups(__ballot((bb << 1) != 0)) << 1;
    }
    load_pair(ps + 1 < p_end, ra, rb);
    dft20(v);
    // A rows: lane (g, q) writes A[g][q][0..19]; pitch 25 float2 = 50 dwords:
    // 50 i mod 64 over 32 lanes is 2 x (25 i mod 32), all distinct
    if (lact) {
#pragma unroll
      for (int k1 = 0; k1 < 20; ++k1) LM_W(A, (g * 20 + q) * kA2Pitch + k1, v[k1]);
    }
    wave_lds_sync();
    // stage 2: lane (g, k1 = q) gathers column k1: lane groups g start at
    // 40 g x 25 = 40 g mod 64 dwords, so half-waves touch disjoint banks
    // (software-pipelined in chunks of four: the reads of chunk c + 1 issue
    // before chunk c's twiddle products, so only the first chunk's reads are
    // waited for in full)
    if (lact) {
      constexpr int CK = 4;
      f2 ab[2][CK], tb[2][CK];
      auto ldc = [&](int c, int b) {
#pragma unroll
        for (int k = 0; k < CK; ++k) {
          ab[b][k] = LM_R(A, (g * 20 + CK * c + k) * kA2Pitch + q);
          tb[b][k] = L.tw[q][CK * c + k];
        }
      };
      ldc(0, 0);
#pragma unroll
      for (int c = 0; c < 20 / CK; ++c) {
        if (c + 1 < 20 / CK) ldc(c + 1, (c + 1) & 1);
#pragma unroll
        for (int k = 0; k < CK; ++k) v[CK * c + k] = cmul2(ab[c & 1][k], tb[c & 1][k]);
      }
    }
    dft20(v);   // Z[q + 20 k2] in v[k2]
    // exchange (the A reads of this wave are done: one wave's LDS ops complete in order)
    f2* E = A;
    if (lact) {
      f2* e = E + (g * 20 + q) * kE2Pitch;
#pragma unroll
      for (int j = 0; j < 10; ++j) LM_W(e, j, v[10 + j]);
      if (q == 0) e[10] = v[0];
    }
    wave_lds_sync();
    // partner values pp[k2] = Z[400 - q - 20 k2]: lane 20 - q's v[19 - k2]
    // (= its published slot 9 - k2), or for q = 0 the lane's own v[20 - k2]
    // (slots shifted by one, slot 10 = v[0])
    f2 pp[10];
    {
      const f2* base = E + (g * 20 + (q == 0 ? 0 : 20 - q)) * kE2Pitch + (q == 0 ? 1 : 0);
#pragma unroll
      for (int k2 = 0; k2 < 10; ++k2) pp[k2] = LM_R(base, 9 - k2);
    }
    wave_lds_sync();
    // pair powers {|Z + conj Z'|^2, |Z - conj Z'|^2} = 4 {P_a, P_b}; row pitch
    // 212 float2: lane groups 40 banks apart, conflict-free 8-byte writes
    f2* PW = A;
    if (lact) {
      f2* pr = PW + g * kP2Pitch + q;
#pragma unroll
      for (int k2 = 0; k2 < 10; ++k2) {
        const f2 sa = f2{v[k2].x + pp[k2].x, v[k2].y - pp[k2].y};   // Z + conj Z'
        const f2 sb = f2{v[k2].x - pp[k2].x, v[k2].y + pp[k2].y};   // Z - conj Z'
        LM_W(pr, 20 * k2, (f2{__builtin_fmaf(sa.x, sa.x, sa.y * sa.y), __builtin_fmaf(sb.x, sb.x, sb.y * sb.y)}));
      }
      if (q == 0) {   // bin 200 is its own partner: 4 {Re^2, Im^2}
        const f2 z = v[10];
        pr[200] = f2{4.0f * z.x * z.x, 4.0f * z.y * z.y};
      }
    }
    wave_lds_sync();
    // pair powers -> HTK mel -> ln(+1e-8), straight-line: lane l takes mel l
    // over a fixed window of kMelW1 bins, and lanes 0-31 the halves of mel
    // 64 + l / 2 over kMelW2 bins each (summed by a DPP swap); weights (x 1/4,
    // zero outside the filter) and window starts are per-lane registers, so a
    // tap is three 8-byte power reads (one per pair, immediate offsets) and
    // three packed FMAs, with no per-lane trip count
    {
      const f2* p1 = PW + ws1;
      const f2* p2 = PW + ws2;
      f2 a0 = {0.0f, 0.0f}, a1 = {0.0f, 0.0f}, a2 = {0.0f, 0.0f};
      f2 c0 = {0.0f, 0.0f}, c1 = {0.0f, 0.0f}, c2 = {0.0f, 0.0f};
      typedef const volatile __attribute__((address_space(3))) f2 vf2;
#define LM_RD(p, i) (*(vf2*)((p) + (i)))
      // Software-pipelined one tap ahead: the volatile reads issue in source
      // order, so tap j + 1's six reads are written before tap j's FMAs (in two
      // separate loops the second set's reads had been issued one at a time,
      // each waited for: ~21 serial LDS round trips per pass).
      f2 x1[2][3], x2[2][3];
      auto ld = [&](int j, int b) {
        if (j < kMelW1) {
          x1[b][0] = LM_RD(p1, j);
          x1[b][1] = LM_RD(p1, kP2Pitch + j);
          x1[b][2] = LM_RD(p1, 2 * kP2Pitch + j);
        }
        if (j < kMelW2) {
          x2[b][0] = LM_RD(p2, j);
          x2[b][1] = LM_RD(p2, kP2Pitch + j);
          x2[b][2] = LM_RD(p2, 2 * kP2Pitch + j);
        }
      };
      static_assert(kMelW1 >= kMelW2, "the first window is the longer one");
      ld(0, 0);
#pragma unroll
      for (int j = 0; j < kMelW1; ++j) {
        if (j + 1 < kMelW1) ld(j + 1, (j + 1) & 1);
        const int b = j & 1;
        a0 = fma2(x1[b][0], f2{mw1[j], mw1[j]}, a0);
        a1 = fma2(x1[b][1], f2{mw1[j], mw1[j]}, a1);
        a2 = fma2(x1[b][2], f2{mw1[j], mw1[j]}, a2);
        if (j < kMelW2) {
          c0 = fma2(x2[b][0], f2{mw2[j], mw2[j]}, c0);
          c1 = fma2(x2[b][1], f2{mw2[j], mw2[j]}, c1);
          c2 = fma2(x2[b][2], f2{mw2[j], mw2[j]}, c2);
        }
      }
#undef LM_RD
      float cv[6] = {c0.x, c0.y, c1.x, c1.y, c2.x, c2.y};
#pragma unroll
      for (int f = 0; f < 6; ++f)   // + the other half (lane ^ 1)
        cv[f] += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, cv[f]), 0xB1, 0xF, 0xF, false));
      // stores through a resource over the pass's rows: rows past the end
      // fall outside num_records, and lanes 1, 3, ... of the second set (odd
      // halves) and 32-63 aim past it too -- no branch per frame
      const int64_t r0 = ps * kRowsPerPass;
      const int64_t nr = rows - r0 < kRowsPerPass ? rows - r0 : kRowsPerPass;
      const __amdgpu_buffer_rsrc_t fr = make_rsrc(feats + r0 * kMels, (uint32_t)(nr > 0 ? nr : 0) * kMels * 4);
      float av[6] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y};
      if (zmask) {   // (wave-uniform, rare) an all-zero row has power 0, not the separation's rounding of its partner's
#pragma unroll
        for (int f = 0; f < 6; ++f)
          if (zmask >> f & 1) av[f] = cv[f] = 0.0f;
      }
      const bool half0 = lane < 2 * (kMels - 64) && (lane & 1) == 0;
      const int o2 = half0 ? 4 * (64 + (lane >> 1)) : 0x40000000;
      float la[6], lc[6];
#pragma unroll
      for (int f = 0; f < 6; ++f) {
        la[f] = wk_logf(av[f] + 1e-8f);
        lc[f] = wk_logf(cv[f] + 1e-8f);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, la[f]), fr, 4 * (f * kMels + lane), 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, lc[f]), fr, o2 + 4 * f * kMels, 0, 0);
      }
      if constexpr (STATS) {
        // rows r0 .. r0 + nr - 1; those from bnd on belong to the next utterance
        const int bnd = T - ta_pass;
        const float m2 = half0 ? 1.0f : 0.0f;   // the second filter set counts once per mel (even lanes 0-30)
        const float kLogFloor = wk_logf(1e-8f);   // bit-identical to a silent bin's value
        // per frame P = {x - K, (y - K) m2} for the lane's two filters
        const f2 pm = {1.0f, m2}, pk = {-kLogFloor, -kLogFloor * m2};
        if (ta_pass == 0 && ps != p_beg) flush();   // the previous pass ended an utterance
        if (bnd >= 6 && nr == 6) {   // the common pass: one utterance, all rows live
#pragma unroll
          for (int f = 0; f < 6; ++f) {
            const f2 P = fma2(f2{la[f], lc[f]}, pm, pk);
            s_run = s_run + P;
            q_run = fma2(P, P, q_run);
          }
        } else {
#pragma unroll
          for (int f = 0; f < 6; ++f) {
            if (f == bnd && f < nr) flush();   // (wave-uniform) the utterance ends inside this pass
            const f2 P = fma2(f2{la[f], lc[f]}, pm, pk);
            if (f < nr) {   // wave-uniform
              s_run = s_run + P;
              q_run = fma2(P, P, q_run);
            }
          }
        }
        if (ps + 1 == p_end) flush();   // the range's last utterance
      }
    }
    wave_lds_sync();
  }
}

// Global z-score of one utterance per block (ctc.py:101-104: mean, unbiased
// std, applied only when std > 0).  Up to kZsCache float4 per thread stay in
// registers between the two reductions and the write-back, so the utterance
// is read from HBM once (it was read three times: 0.27 ms per 4096
// utterances); longer utterances (> 32,768 values, T > 409) re-read.
// The sums are double: a constant utterance (digital silence: every value
// ln(1e-8)) then has mean = its value and std = 0 exactly, and stays
// un-normalised.  (torch's float std of a constant tensor is rounding noise
// -- 1.9e-6 for 301 x 80 values of ln(1e-8) -- so ctc.py's `std() > 0` passes
// and its output is that noise's quotient; the build takes the exact reading,
// as ctc_zstats_kernel does on the one-call path.)
constexpr int kZsCache = 8;
__global__ __launch_bounds__(1024) void ctc_zscore_kernel(float* __restrict__ feats, int64_t n_per) {
  __shared__ double red[16];
  __shared__ double bc;
  float* f = feats + (int64_t)blockIdx.x * n_per;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  auto block_sum = [&](double v) -> double {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[w] = v;
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int i = 0; i < 16; ++i) s += red[i];
      bc = s;
    }
    __syncthreads();
    const double r = bc;
    __syncthreads();
    return r;
  };
  const int64_t n4 = n_per / 4;
  if (n_per % 4 == 0 && n4 <= 1024 * kZsCache && ((uintptr_t)f & 15) == 0) {
    float4* f4 = reinterpret_cast<float4*>(f);
    float4 v[kZsCache];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kZsCache; ++k) {
      const int64_t i = tid + 1024 * k;
      v[k] = i < n4 ? f4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      s += ((double)v[k].x + (double)v[k].y) + ((double)v[k].z + (double)v[k].w);
    }
    const double mean = block_sum(s) / (double)n_per;
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < kZsCache; ++k) {
      if (tid + 1024 * k < n4) {
        const double a = v[k].x - mean, b = v[k].y - mean, c = v[k].z - mean, d = v[k].w - mean;
        q += (a * a + b * b) + (c * c + d * d);
      }
    }
    const double sd = sqrt(block_sum(q) / (double)(n_per - 1));
    if (!(sd > 0.0)) return;   // ctc.py:101-104: only when std > 0
    const float mf = (float)mean, inv = (float)(1.0 / sd);
#pragma unroll
    for (int k = 0; k < kZsCache; ++k) {
      const int64_t i = tid + 1024 * k;
      if (i < n4) f4[i] = make_float4((v[k].x - mf) * inv, (v[k].y - mf) * inv, (v[k].z - mf) * inv, (v[k].w - mf) * inv);
    }
    return;
  }
  double s = 0.0;
  for (int64_t i = tid; i < n_per; i += 1024) s += (double)f[i];
  const double mean = block_sum(s) / (double)n_per;
  double q = 0.0;
  for (int64_t i = tid; i < n_per; i += 1024) {
    const double d = (double)f[i] - mean;
    q += d * d;
  }
  const double sd = sqrt(block_sum(q) / (double)(n_per - 1));
  if (!(sd > 0.0)) return;
  const float mf = (float)mean, inv = (float)(1.0 / sd);
  for (int64_t i = tid; i < n_per; i += 1024) f[i] = (f[i] - mf) * inv;
}

// The z-score's statistics for wk_ctc_transcribe: one wave per utterance
// folds the log-mel waves' {S, Q} slots for it (ctc_logmel_fft2_kernel<true>:
// wave w's range of R passes starts in utterance 6 w R / T, its j-th slot is
// that utterance + j) in double into zs[b] = {mean, 1/std} (unbiased std,
// ctc.py:101-104), or {0, 1} when std is 0 (no normalisation).  Needs T >= 6:
// a pass then spans at most two utterances.  The partials are float sums, so
// Q - S m carries ~1e-6 of
// Q's size in rounding: a variance at or below 1e-5 of the mean square (a
// constant utterance, silent or not, lands there) is recomputed exactly from
// the utterance's raw rows, two passes in double -- a constant utterance then
// gets std 0 exactly and stays un-normalised, as ctc.py:104's `std() > 0` test
// leaves it.
__global__ __launch_bounds__(256) void ctc_zstats_kernel(const float2* __restrict__ part, const float* __restrict__ feats,
                                                         int64_t batch, int T, int64_t R, int MS,
                                                         float2* __restrict__ zs) {
  // one wave per utterance: lane i takes the waves w0 + i, + 64, ... whose ranges hold its rows
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= batch) return;   // (wave-uniform)
  const int64_t r0 = b * T, w0 = r0 / 6 / R, w1 = (r0 + T - 1) / 6 / R;
  double S = 0.0, Q = 0.0;
  for (int64_t w = w0 + lane; w <= w1; w += 64) {
    const int64_t first = w * R * 6 / T;   // the utterance of the range's first row
    const float2 v = part[w * MS + (b - first)];
    S += v.x;
    Q += v.y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    S += __shfl_xor(S, o, 64);
    Q += __shfl_xor(Q, o, 64);
  }
  const double n = (double)T * kMels;
  double m = S / n, var = (Q - S * m) / (n - 1.0);
  m += (double)wk_logf(1e-8f);   // S, Q are sums of x - ln(1e-8)
  // (Q == 0: every value is the floor ln(1e-8), digital silence: std 0 as it stands)
  if (Q > 0.0 && var <= 1e-5 * (Q / n)) {   // (wave-uniform) within the partials' rounding: exact two-pass statistics
    const float* f = feats + r0 * kMels;
    const int64_t cnt = (int64_t)T * kMels;
    double s1 = 0.0;
    for (int64_t i = lane; i < cnt; i += 64) s1 += (double)f[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s1 += __shfl_xor(s1, o, 64);
    m = s1 / n;
    double s2 = 0.0;
    for (int64_t i = lane; i < cnt; i += 64) {
      const double d = (double)f[i] - m;
      s2 += d * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o, 64);
    var = s2 / (n - 1.0);
  }
  const float sd = var > 0.0 ? (float)sqrt(var) : 0.0f;
  if (lane == 0) zs[b] = sd > 0.0f ? make_float2((float)m, 1.0f / sd) : make_float2(0.0f, 1.0f);
}
// Window starts of ctc_logmel_fft2_kernel's straight-line filterbank.  A tap
// is a ds_read_b64 of the pair-power row at bin ws[lane] + j, served 32 lanes
// at a time: two lanes of a half-wave share banks when their starts differ by
// a nonzero multiple of 32 bins.  A filter shorter than its window can start
// up to (window - length) bins early (the extra taps weigh 0), so the starts
// are chosen with distinct residues mod 32 per half-wave where possible
// (equal starts are free: one address is a broadcast).  Set 1: mel l over
// kMelW1 bins; set 2 (lanes 0-31): mel 64 + l / 2 split at cut[l] between two
// kMelW2-bin windows.  A half-wave without a solution keeps the natural starts.
void pick_mel_windows(const std::vector<int>& st, const std::vector<int>& ln, std::vector<int>& ws, std::vector<int>& cut) {
  auto conflict_free = [](const int* w, int n) {
    for (int a = 0; a < n; ++a)
      for (int b = a + 1; b < n; ++b)
        if (w[a] != w[b] && (w[a] - w[b]) % 32 == 0) return false;
    return true;
  };
  // set 1, per half-wave: bipartite matching of lanes to residues
  for (int h = 0; h < 2; ++h) {
    int* w = &ws[32 * h];
    for (int l = 0; l < 32; ++l) w[l] = std::min(st[32 * h + l], kBins - kMelW1);
    if (conflict_free(w, 32)) continue;
    int owner[32], pick[32];
    std::fill(owner, owner + 32, -1);
    std::function<bool(int, unsigned&)> aug = [&](int l, unsigned& seen) -> bool {
      const int m = 32 * h + l, hi = std::min(st[m], kBins - kMelW1), lo = std::max(0, st[m] + ln[m] - kMelW1);
      for (int s = hi; s >= lo; --s) {
        const int r = s & 31;
        if (seen >> r & 1u) continue;
        seen |= 1u << r;
        if (owner[r] < 0 || aug(owner[r], seen)) { owner[r] = l; pick[l] = s; return true; }
      }
      return false;
    };
    bool ok = true;
    for (int l = 0; l < 32 && ok; ++l) { unsigned seen = 0; ok = aug(l, seen); }
    if (ok)
      for (int l = 0; l < 32; ++l) w[l] = pick[l];
  }
  // set 2: per mel a pair (h0, h1); the cut is h0 + kMelW2.  Depth-first,
  // most constrained mel first, with a node budget (then natural starts)
  int sol[16][2], order[16], nopt[16];
  std::vector<std::pair<int, int>> opts[16];
  for (int p = 0; p < 16; ++p) {
    const int m = 64 + p;
    for (int h0 = std::max(0, st[m] + ln[m] - 2 * kMelW2); h0 <= st[m]; ++h0)
      for (int h1 = std::max(h0, st[m] + ln[m] - kMelW2); h1 <= std::min(h0 + kMelW2, kBins - kMelW2); ++h1)
        if ((h0 & 31) != (h1 & 31)) opts[p].push_back({h0, h1});
    nopt[p] = (int)opts[p].size();
    order[p] = p;
  }
  std::stable_sort(order, order + 16, [&](int a, int b) { return nopt[a] < nopt[b]; });
  unsigned used = 0;
  long budget = 1 << 20;
  std::function<bool(int)> bt = [&](int d) -> bool {
    if (d == 16) return true;
    const int p = order[d];
    for (const auto& o : opts[p]) {
      if (--budget < 0) return false;
      const unsigned bits = (1u << (o.first & 31)) | (1u << (o.second & 31));
      if (used & bits) continue;
      used |= bits;
      sol[p][0] = o.first;
      sol[p][1] = o.second;
      if (bt(d + 1)) return true;
      used &= ~bits;
    }
    return false;
  };
  const bool ok2 = bt(0);
  for (int l = 0; l < 32; ++l) {
    const int m = 64 + l / 2;
    const int h0 = ok2 ? sol[l / 2][0] : std::min(st[m], kBins - kMelW2);
    const int h1 = ok2 ? sol[l / 2][1] : std::min(st[m] + kMelW2, kBins - kMelW2);
    ws[64 + l] = (l & 1) ? h1 : h0;
    cut[64 + l] = (l & 1) ? kBins : std::min(h0 + kMelW2, h1 + kMelW2);
  }
  // (lanes 32-63 of set 2 carry zero weights and all read bin 0: a broadcast)
}

// HTK mel filterbank of torchaudio.functional.melscale_fbanks(201, 0, 8000, 80, 16000), in fp32 like torch.
void mel_fbank(std::vector<float>& fb) {
  fb.assign((size_t)kBins * kMels, 0.0f);
  const double m_min = 0.0, m_max = 2595.0 * log10(1.0 + 8000.0 / 700.0);
  std::vector<float> f_pts(kMels + 2), freqs(kBins);
  for (int i = 0; i < kMels + 2; ++i) {
    const float m = (float)(m_min + (m_max - m_min) * i / (kMels + 1));
    f_pts[i] = 700.0f * (powf(10.0f, m / 2595.0f) - 1.0f);
  }
  for (int k = 0; k < kBins; ++k) freqs[k] = (float)(8000.0 * k / (kBins - 1));
  for (int k = 0; k < kBins; ++k)
    for (int m = 0; m < kMels; ++m) {
      const float down = -(f_pts[m] - freqs[k]) / (f_pts[m + 1] - f_pts[m]);
      const float up = (f_pts[m + 2] - freqs[k]) / (f_pts[m + 2] - f_pts[m + 1]);
      const float v = fminf(down, up);
      fb[(size_t)k * kMels + m] = v > 0.0f ? v : 0.0f;
    }
}

}  // namespace

namespace wk {

bool ctc_logmel_tables(CtcLogmelTables* t) {
  // FFT tables: periodic Hann(400) and the four-step twiddles W400^(n2 k1), in double -> fp32
  t->win.resize(kNfft);
  t->tw.resize(2 * 400);
  for (int n = 0; n < kNfft; ++n) t->win[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * n / kNfft));
  for (int k1 = 0; k1 < 20; ++k1)
    for (int n2 = 0; n2 < 20; ++n2) {
      const double ang = -2.0 * M_PI * (double)(n2 * k1) / kNfft;
      t->tw[2 * (k1 * 20 + n2)] = (float)cos(ang);
      t->tw[2 * (k1 * 20 + n2) + 1] = (float)sin(ang);
    }
  // mel filterbank: per filter its first bin and length
  std::vector<float> fb;
  mel_fbank(fb);
  std::vector<int> st(kMels), ln(kMels);
  for (int m = 0; m < kMels; ++m) {
    int a0 = -1, z = -1;
    for (int k = 0; k < kBins; ++k)
      if (fb[(size_t)k * kMels + m] != 0.0f) { if (a0 < 0) a0 = k; z = k; }
    if (a0 < 0) a0 = z = 0;
    st[m] = a0;
    ln[m] = z - a0 + 1;
  }
  // straight-line windows of ctc_logmel_fft2_kernel (see there)
  std::vector<float>& mw = t->melw;
  std::vector<int>& ws = t->melws;
  mw.assign((size_t)64 * (kMelW1 + kMelW2), 0.0f);
  ws.assign(128, 0);
  std::vector<int> cut(128, kBins);   // (second set) a lane takes filter bins in [ws, cut)
  bool fits = kMels == 80;
  for (int m = 0; m < 64 && fits; ++m) fits = ln[m] <= kMelW1;
  for (int m = 64; m < kMels && fits; ++m) fits = ln[m] <= 2 * kMelW2;
  if (!fits) return false;
  pick_mel_windows(st, ln, ws, cut);
  for (int m = 0; m < 64; ++m)
    for (int j = 0; j < kMelW1; ++j) {
      const int k = ws[m] + j;
      const bool mine = k >= st[m] && k < st[m] + ln[m];
      mw[(size_t)m * kMelW1 + j] = mine ? 0.25f * fb[(size_t)k * kMels + m] : 0.0f;
    }
  for (int l = 0; l < 32; ++l) {
    const int m = 64 + l / 2;
    for (int j = 0; j < kMelW2; ++j) {
      const int k = ws[64 + l] + j;
      const bool mine = k >= st[m] && k < st[m] + ln[m] && k < cut[64 + l] && ((l & 1) == 0 || k >= cut[64 + l - 1]);
      mw[(size_t)64 * kMelW1 + (size_t)l * kMelW2 + j] = mine ? 0.25f * fb[(size_t)k * kMels + m] : 0.0f;
    }
  }
  // every filter tap lands in exactly one window
  for (int m = 0; m < kMels && fits; ++m) {
    int taps = 0;
    if (m < 64) {
      for (int j = 0; j < kMelW1; ++j) taps += mw[(size_t)m * kMelW1 + j] != 0.0f;
    } else {
      for (int h = 0; h < 2; ++h)
        for (int j = 0; j < kMelW2; ++j) taps += mw[(size_t)64 * kMelW1 + (size_t)(2 * (m - 64) + h) * kMelW2 + j] != 0.0f;
    }
    int nz = 0;
    for (int k = st[m]; k < st[m] + ln[m]; ++k) nz += fb[(size_t)k * kMels + m] != 0.0f;
    fits = taps == nz;
  }
  return fits;
}

CtcLogmelLayout ctc_logmel_layout(int n_cu, int64_t rows, int T) {
  CtcLogmelLayout L;
  const int64_t passes = (rows + 2 * kF2Pairs - 1) / (2 * kF2Pairs);
  const int64_t blocks = (passes + kF2Waves - 1) / kF2Waves;
  L.grid = (unsigned)(blocks < n_cu ? blocks : n_cu);
  const int64_t nw = (int64_t)L.grid * kF2Waves;
  L.R = (passes + nw - 1) / nw;
  L.MS = (int)((2 * kF2Pairs * L.R - 1) / T + 2);
  L.slots = nw * L.MS;
  return L;
}

void launch_ctc_logmel(const float* audio, int64_t stride, int n_valid, int n_pad, int T, int64_t rows, const float* win,
                       const float* tw, const float* melw, const int* melws, float* feats, const CtcLogmelLayout& lay,
                       float2* part, hipStream_t st) {
  const auto kernel = part ? ctc_logmel_fft2_kernel<true> : ctc_logmel_fft2_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(lay.grid), dim3(kF2Waves * 64), 0, st, audio, stride, n_valid, n_pad, T, rows, win, tw, melw,
                     melws, feats, lay.R, lay.MS, part);
}

void launch_ctc_zscore(float* feats, int64_t batch, int T, const CtcLogmelLayout& lay, const float2* part, float2* zs,
                       hipStream_t st) {
  if (part)
    hipLaunchKernelGGL(ctc_zstats_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, part, feats, batch, T, lay.R,
                       lay.MS, zs);
  else
    hipLaunchKernelGGL(ctc_zscore_kernel, dim3((unsigned)batch), dim3(1024), 0, st, feats, (int64_t)T * kMels);
}

}  // namespace wk
