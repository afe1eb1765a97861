// wk_fe_lds_layout.h -- where the front-end's LDS tables live (plain C++:
// included by the device code, wk_fe_dev.h, and by the host-side layout test,
// tests/test_fe_lds_layout.py).  Every function maps (table, lane j, slot) to
// a float offset; fe_init_tables fills the tables through them and the device
// reads go through them.
//
// The tables depend only on the lane j = lane & 15 and are re-read in full by
// every wave-round, so they are lane-major: one lane's values are contiguous
// and 16-byte aligned, read with ds_read_b128 at immediate offsets from one
// per-lane base (slot-major, a lane's consecutive values sat 128 bytes apart
// and the compiler paired them into ds_read2_b64: 8 LDS-array cycles per 16
// bytes per lane against ds_read_b128's 4).
//
// Banking of ds_read_b128: bank = (byte address / 4) mod 64, served in four
// groups of 16 lanes, each holding the 16 distinct j once (the four frame
// groups of a wave read the same address for the same j and broadcast).  A
// row pitch of 4 * odd floats puts the 16 j of one read on the 16 distinct
// bank quads: row base quad = j * (pitch / 4) mod 16, a bijection for odd
// pitch / 4.
#pragma once

namespace wk {
namespace fe_lds {

constexpr int kLanes = 16;

// Twiddle rows, one per lane j:
//   [ W256^(j * (s ^ (j & 8))), s = 0..15 : 32 floats
//   | fe_split_tw(j, k2), k2 = 0..7      : 16 floats   (k2 = 0 is the former register pair w0)
//   | 4 floats of padding ]
constexpr int kRowPitch = 52;                 // 4 * 13
constexpr int kRowUsed = 48;
constexpr int kTabSize = kLanes * kRowPitch;   // 832 floats
constexpr int kTwSlots = 16, kSplitSlots = 8;

constexpr int row_off(int j) { return j * kRowPitch; }
constexpr int tw_off(int j, int s) { return row_off(j) + 2 * s; }             // {re, im}
constexpr int split_off(int j, int k2) { return row_off(j) + 32 + 2 * k2; }   // {re, im}

// Analysis window (in LDS in the fused kernel only), one row per lane j: the
// ten pairs win[32 n1 + 2 j], win[32 n1 + 2 j + 1], n1 = 0..9, of the constant
// table (kWinB / kWinA: sign-adjusted, wk_tables.h).
constexpr int kWinPitch = 20;                 // 4 * 5
constexpr int kWinRows = 10;
constexpr int kWinSize = kLanes * kWinPitch;   // 320 floats, as the flat table
constexpr int win_row_off(int j) { return j * kWinPitch; }
constexpr int win_off(int j, int n1) { return win_row_off(j) + 2 * n1; }      // first of the pair
constexpr int win_src(int j, int n1) { return 32 * n1 + 2 * j; }              // its index in the constant table

// Transpose scratch = the frame's power row (fe_rest), in f2 (8-byte) units
// from the 8-byte aligned row base: writes at xpose_wr(j) + s,
// reads of the diagonal half at xpose_rd(j, s), of the other at xpose_rd(j ^ 8, s).
constexpr int kXposePitch = 17;
constexpr int xpose_wr(int j) { return kXposePitch * (j & 7) + (j & 8); }
constexpr int xpose_rd(int kc, int s) { return kc + kXposePitch * s; }
constexpr int kXposeFloats = 2 * (kXposePitch * 7 + 15 + 1);   // 270 = the power row's pitch (wk_common.h kPRow)

// Frame slots of the FFT phase (16 lanes per frame): lane group g of wave w
// takes slot w + 8 (g & 1) + 16 r + 32 (g >> 1) in round r.  The two groups of
// a 32-lane half are 8 rows apart, 8 x 270 = 16 mod 32 floats: their power-row
// stores (ds_write_b32 / ds_write2_b32: bank = dword address mod 32, 16
// consecutive banks per group) land on disjoint banks.  (16 rows apart, as
// with the odd pitch 271, 16 x 270 = 0 mod 32: every store 2-way, which a
// ds_write2_b32 pays for.)  Slot 0 is wave 0 / round 0 / group 0, slot 62
// wave 6 / round 1 / group 3, the padding slot 63 wave 7 / round 1 / group 3:
// the lanes the edge-frame paths of fe_stage0 assume.
constexpr int kRoundSlots = 16;
constexpr int slot_base(int g) { return 8 * (g & 1) + 32 * (g >> 1); }
constexpr int frame_slot(int w, int r, int g) { return w + kRoundSlots * r + slot_base(g); }

// The mel's lane-per-frame reads of the power rows, {p[2m], p[2m+1]} as one
// ds_read_b64: served per 32-lane half, lane l at float address p_row * l + 2m.
// Conflict-free when the 32 row bases of a half sit on 32 distinct bank pairs
// (p_row even; 270 = 14 mod 64, and 7 l mod 32 is a bijection).
constexpr bool mel_rows_conflict_free(int p_row) {
  if (p_row % 2) return false;
  for (int half = 0; half < 2; ++half) {
    unsigned seen = 0;
    for (int l = 32 * half; l < 32 * half + 32; ++l) seen |= 1u << ((p_row * l % 64) / 2);
    if (seen != 0xffffffffu) return false;
  }
  return true;
}

static_assert(kRowPitch % 4 == 0 && (kRowPitch / 4) % 2 == 1 && kRowUsed <= kRowPitch,
              "twiddle rows: 16-byte aligned, 16 lanes on 16 distinct bank quads");
static_assert(kWinPitch % 4 == 0 && (kWinPitch / 4) % 2 == 1 && 2 * kWinRows <= kWinPitch,
              "window rows: 16-byte aligned, 16 lanes on 16 distinct bank quads");
static_assert(2 * kTwSlots + 2 * kSplitSlots == kRowUsed && (2 * kTwSlots) % 4 == 0, "row contents");

// The carve (floats): twiddle rows | log-mel [40][lstride] | power rows
// [n_frames][p_row] | window (fused kernel only).
struct Carve {
  int tab, logmel, power, end_no_win, win, end;
};
constexpr Carve carve(int lstride, int n_frames, int p_row) {
  Carve c = {};
  c.tab = 0;
  c.logmel = c.tab + kTabSize;
  c.power = c.logmel + 40 * lstride;
  c.end_no_win = c.power + n_frames * p_row;
  c.win = (c.end_no_win + 3) & ~3;
  c.end = c.win + kWinSize;
  return c;
}
constexpr int kStandaloneLimitBytes = 81920;   // two standalone front-end workgroups per CU
constexpr int kFusedLimitBytes = 163840;

}  // namespace fe_lds
}  // namespace wk
