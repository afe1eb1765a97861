// wk_fused_dev.h -- the whole hot path in one persistent, warp-specialised
// kernel: wk_fused_kernel and the helper that launches it.
//
//   audio (HBM) -> MFCC front-end (VALU/LDS) -> features (LDS) -> xiaoa CNN
//   (fp32 MFMA) -> logit (HBM)
//
// One 16-wave workgroup per CU.  Waves 0-7 (front-end role,
// wk_fused_fe_role.h) run the FFT and the lane-per-frame mel filterbank of
// wk_fe_dev.h clip after clip and write each clip's log-mel image [40][63]
// into one of two LDS buffers.  Waves 8-15 (CNN role, wk_fused_cnn_role.h)
// take the DCT-II + CMVN from that buffer into the conv1 input image, then run
// the CNN of wk_cnn_dev.h on batches of NBF = 4 clips.  What the roles share
// -- the LDS carve and the counter protocol that stands in for s_barrier -- is
// wk_fused_lds.h.  The front-end is VALU + LDS bound and the CNN is
// MFMA bound; on CDNA4 the matrix and vector pipes issue concurrently from
// different waves, so the roles overlap on every SIMD (2 front-end + 2 CNN
// waves per SIMD), and features never touch HBM: per clip the kernel reads
// its 64,000 audio bytes and writes one 4-byte logit.
//
// The conv mode picks the front-end's arithmetic flavour (FE in the kernel;
// FePacked / FeScalar, wk_common.h).  fp32 convolutions: complex arithmetic as
// packed fp32 (v_pk_*_f32).  bf16 / bf16x3: the same front-end as scalar fp32 pairs.
// Beside the bf16 MFMAs, which run on the matrix pipe, packed fp32 issues
// slower than scalar: +4.8 % bf16.  Beside the fp32 MFMAs, which share the
// fp32 datapath, scalar is 2.8 % slower (profiles/r05au_*).
// Product builds include this header in two units that compile in parallel,
// wk_fused.hip (fp32) and wk_fused_xdl.hip (the bf16 family); diagnostic
// builds (-DWK_DIAG) keep every precision in wk_fused.hip, each with the
// flavour it ships with.
#pragma once
#include "wk_fused_lds.h"
#include "wk_fused_fe_role.h"
#include "wk_fused_cnn_role.h"
#include "wk_kernels.h"
#include <type_traits>

namespace {

template <typename T, int CM, bool FEATS>
__global__ __launch_bounds__(kFusedBlock, 4) void wk_fused_kernel(const T* __restrict__ audio, int64_t batch,
                                                                 int64_t clip_stride, const float* __restrict__ wts,
                                                                 const uint16_t* __restrict__ wbf,
                                                                 float* __restrict__ logits,
                                                                 float* __restrict__ feats_out, unsigned* err,
                                                                 int diag) {
  __shared__ __attribute__((aligned(16))) float smem[kFusedLds];
#ifndef WK_DIAG
  diag = 0;   // role isolation (1 = front-end role only, 2 = CNN role only) in -DWK_DIAG builds; folded away here
#endif
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  typedef std::conditional_t<CM == kConvF32, FePacked, FeScalar> FE;   // the precision's front-end flavour
  fe_init_tables<true, true, FE>(smem, tid, kFusedBlock);
  for (int i = tid; i < kFusedLds - kGOff; i += kFusedBlock) smem[kGOff + i] = 0.0f;  // ctrl, guards, pads
  __syncthreads();
  const int64_t n_mine = batch > (int64_t)blockIdx.x ? (batch - 1 - blockIdx.x) / gridDim.x + 1 : 0;
  // The front-end role is the critical path: static issue priority over the
  // CNN role measured +0.5-0.9 % (priority 1-3); the reverse (CNN over
  // front-end) measured -13 %.
  if (wave < kFeWaves) __builtin_amdgcn_s_setprio(kPrioFe);
  if (wave < kFeWaves) {
    if (!(diag & 2)) fe_role<T, FE>(smem, audio, n_mine, clip_stride, wave, lane, diag);
  } else {
    if (!(diag & 1)) {
      LogmelSrc<CM, FEATS> src = {smem, reinterpret_cast<unsigned*>(smem + kCtrlOff), feats_out, (int64_t)blockIdx.x,
                                  (int64_t)gridDim.x, 0, 0, diag};
      cnn_role<CM>(smem, wts, wbf, n_mine, (int64_t)blockIdx.x, (int64_t)gridDim.x, logits, wave - kFeWaves, lane,
                   src);
    }
  }
  report_abort(reinterpret_cast<unsigned*>(smem + kCtrlOff), err, lane);
}

// Launch wk_fused_kernel<T, CM, FEATS>, FEATS = whether the caller wants the
// features: one workgroup per clip up to grid_cap.
template <typename T, int CM>
hipError_t launch_fused_as(const void* audio, int64_t batch, int64_t clip_stride, const float* w, const uint16_t* wbf,
                           float* logits, float* feats_or_null, int grid_cap, hipStream_t stream, unsigned* err,
                           int diag) {
  const dim3 g((int)(batch < grid_cap ? batch : grid_cap)), blk(kFusedBlock);
  if (feats_or_null)
    hipLaunchKernelGGL((wk_fused_kernel<T, CM, true>), g, blk, 0, stream, (const T*)audio, batch, clip_stride, w, wbf,
                       logits, feats_or_null, err, diag);
  else
    hipLaunchKernelGGL((wk_fused_kernel<T, CM, false>), g, blk, 0, stream, (const T*)audio, batch, clip_stride, w, wbf,
                       logits, nullptr, err, diag);
  return hipGetLastError();
}

// launch_fused_as for the conv mode among CM, REST... (the conv modes a unit
// compiles, which it states in one line); the last of them takes every other
// value.  `a` = launch_fused_as's arguments.  The unit's kernels are emitted in
// the order they are named here: audio type, then the list's order, then FEATS
// (device-code comparisons between builds count on it, profiles/fused_split_ab.md).
template <typename T, int CM, int... REST, typename... A>
hipError_t launch_fused_mode(int conv_mode, A... a) {
  if constexpr (sizeof...(REST) > 0)
    return conv_mode == CM ? launch_fused_as<T, CM>(a...) : launch_fused_mode<T, REST...>(conv_mode, a...);
  else
    return launch_fused_as<T, CM>(a...);
}
template <int... CMS, typename... A>
hipError_t launch_fused_modes(bool i16, int conv_mode, A... a) {
  return i16 ? launch_fused_mode<int16_t, CMS...>(conv_mode, a...) : launch_fused_mode<float, CMS...>(conv_mode, a...);
}

}  // namespace
