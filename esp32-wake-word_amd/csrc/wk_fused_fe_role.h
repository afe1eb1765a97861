// wk_fused_fe_role.h -- the front-end role of the fused kernel (waves 0-7).
//
// The eight waves run the FFT and the lane-per-frame mel filterbank of
// wk_fe_dev.h clip after clip and write each clip's log-mel image [40][63]
// into one of two LDS buffers, which the CNN role (wk_fused_cnn_role.h) takes
// from there.  The role is VALU + LDS bound and the kernel's critical path.
// The complex arithmetic is packed fp32 beside the fp32 convolutions and
// scalar fp32 pairs beside the bf16 family (the flavour FE: FePacked /
// FeScalar, wk_common.h): the role's text is the same.
#pragma once
#include "wk_fused_lds.h"

namespace {

// ---------------------------------------------------------------------------
// Front-end role (waves 0-7): mode B (torchaudio + CMVN), one clip at a time.
// ---------------------------------------------------------------------------
template <typename T, typename FE>
__device__ __forceinline__ void fe_role(float* smem, const T* __restrict__ audio, int64_t n_mine,
                                        int64_t clip_stride, int wave, int lane, int diag) {
  float* P = smem + kPOff;
  float* L = smem + kLOff;
  float* L1 = smem + kL1Off;
  unsigned* ctrl = reinterpret_cast<unsigned*>(smem + kCtrlOff);
  const int g = lane >> 4, j = lane & 15;
  const FeTables tb = fe_tables(smem, j, nullptr);   // window and twiddle rows of lane j, both in LDS
  const int slot_base = fe_lds::slot_base(g);
  const int64_t G = gridDim.x;
  unsigned gen = 0, p_wait = 0;

  // Static frame assignment: wave w, round r, lane group g takes frame
  // w + 8(g&1) + 16r + 32(g>>1) (fe_lds::frame_slot; groups 0/1 8 frames
  // apart: 8 x 270 = 16 mod 32 floats, disjoint LDS banks for the stores).
  // A dynamic hand-out through an LDS counter was measured slower: the
  // atomic's return latency lands on the prefetch path.  Both edge
  // frames in wave 0's round 0 (when an edge round still issued 21 per-lane
  // reflected loads: one such round per clip instead of two) measured -1 %:
  // that wave then finishes last at the clip barrier.
  //
  // Prefetch context of a round, built once per round: the clip's buffer
  // resource and the lane group's sample offsets.  Every round issues the
  // same pair loads; the two rounds that hold a reflected edge frame (frame 0
  // in wave 0 round 0, frame 62 in round 1 of the wave with slot 6;
  // wave-uniform) differ only in stage 0, which takes the reflected rows from
  // the frame's other rows by DPP (fe_stage0_rows: +36 / +9 instructions on
  // the common round; the reflected-index rounds were +280 and held every
  // wave at the power-row barrier, fp32 +2.2-2.7 %, profiles/edge_rows_ab.md),
  // and in frame 0's xb.  Past the workgroup's last clip the resource has
  // num_records 0, so those loads return 0 without a branch; the padding
  // slot (frame 63) needs no lane mask either, since its samples past the clip's end come back 0 from the same
  // bounds check.  (Rebuilt inside each of the four prefetch parts, the 64-bit
  // clip address, the `i < n_mine` test and the per-lane `frame < 63` exec mask
  // cost ~28 scalar/branch instructions per part, ~13 % of a round's issue.)
  const int64_t step = G * clip_stride;
  const T* cptr = audio + (int64_t)blockIdx.x * clip_stride;   // clip i of this workgroup
  constexpr uint32_t kClipBytes = kWinSamples * sizeof(T);
  struct PfCtx {
    __amdgpu_buffer_rsrc_t rs;
    int base;   // first sample of the lane group's frame (before reflection)
    int xb;     // the sample before it; frame 0: x[160], the one reflected sample no row holds
  };
  // Frame slot of round r (the wave's own, moving the edge frames to other
  // waves measured neutral).  The scalar flavour (FE::round1_swap) swaps
  // round 1's slots between waves w and w ^ 4, so its second edge frame (62)
  // runs on wave 2 rather than wave 6: waves 4-7 issue after 0-3 on each SIMD
  // and reach the power-row barrier last.  Tuned when wave 6's edge round
  // was the slow one (bf16 +0.8 %, packed fp32 unit -0.8 %,
  // profiles/r06ae_round1_swap_ab.txt) and re-measured with the short edge
  // rounds: bf16 still +1.5 % with the swap, fp32 +0.1 % (noise) and keeps the
  // plain mapping (profiles/edge_rows_ab.md).  Bit-identical either way.
  auto fwr = [&](int r) { return FE::round1_swap && r == 1 ? wave ^ 4 : wave; };
  auto pf_ctx = [&](const T* p, bool ok, int r) -> PfCtx {
    const int fl = fwr(r) + fe_lds::kRoundSlots * r + slot_base;
    return {make_rsrc(p, ok ? kClipBytes : 0u), 256 * fl - 160, fl == 0 ? 160 : 256 * fl - 161};
  };

  Raw<T> pf;
  {
    const PfCtx c0 = pf_ctx(cptr, n_mine > 0, 0);
#pragma unroll
    for (int k = 0; k < 4; ++k) load_raw_part<FE>(c0.rs, c0.base, c0.xb, j, pf, k);
  }
  WK_STAMP_INIT
  for (int64_t i = 0; i < n_mine; ++i) {
#pragma unroll 1
    for (int r = 0; r <= 1; ++r) {
      const int fl = fwr(r) + fe_lds::kRoundSlots * r + slot_base;   // == frame index t (one chunk per clip)
      const int edge = r == 0 && fwr(r) == 0 ? 1 : r == 1 && fwr(r) == 6 ? 2 : 0;   // frame 0 / 62 in this wave-round
      typename FE::c2 a[16];
#ifdef WK_DIAG
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // diagnostic: time the wait for the prefetched audio apart
      WK_STAMP(11);
#endif
      // Every lane runs the round (the frame-63 slot into a scratch row) so
      // the prefetch parts issued from inside fe_rest load for all lanes.
      fe_stage0_fused(pf, lane, edge, tb, a);
      WK_STAMP(0);
      // next round: (i, 1) after round 0, (i + 1, 0) after round 1
      const PfCtx nx = r < 1 ? pf_ctx(cptr, true, r + 1) : pf_ctx(cptr + step, i + 1 < n_mine, 0);
      // k = -1: the round is about to write its first power-row element.  In
      // round 0 that needs every wave done reading clip i-1's rows (its mel);
      // waiting there rather than before the round lets stage 0, the loads and
      // the first DFT16 overlap the slower waves' mel.
      auto pf_part = [&](int k) {
        if (k >= 0) {
          load_raw_part<FE>(nx.rs, nx.base, nx.xb, j, pf, k);
        } else if (r == 0) {
          spin_until<kPrioFe>(ctrl, kCtrlFeBar, p_wait);
          WK_STAMP(9);
        }
      };
      WK_STAMP(1);
      float* row = fl < kNFramesB ? P + fl * kPRow : smem + kDummyRowOff;
      fe_rest<true, FE>(a, j, row, tb, 0, pf_part WK_SP_ARG);
    }
    role_sync<kPrioFe>(ctrl, kCtrlFeBar, gen, lane);               // all power rows of clip i written
    WK_STAMP(7);
    if (i >= 2 && !(diag & 1)) spin_until_all8<kPrioFe>(ctrl, kCtrlLFree, (unsigned)(i - 1));   // clip i-2's DCT done
    WK_STAMP(10);
    {
      // The row base stays opaque (one VGPR with kPOff in it, 8-byte aligned:
      // kPOff and kPRow are even), so the mel's ds_read_b64 of bin pairs take
      // their offsets as immediates from one address register.
      int prow = kPOff + min(lane, kNFramesB - 1) * kPRow;
      asm volatile("" : "+v"(prow));
      mel_dispatch<true>(wave, smem + prow, (i & 1 ? L1 : L) + lane);
      WK_STAMP(8);
      signal_add(ctrl, kCtrlLReady, lane);
    }
    // Split barrier: arrive now, wait before this wave next writes a power
    // row (its first round of clip i+1), after its stage 0 and prefetch.
    gen += 8;
    signal_add(ctrl, kCtrlFeBar, lane);
    p_wait = gen;
    cptr += step;
  }
  WK_STAMP_FLUSH(wave);
}

}  // namespace
