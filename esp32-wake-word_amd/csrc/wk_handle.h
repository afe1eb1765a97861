// wk_handle.h -- the wk_handle struct and what the C-ABI units that take one
// share (internal): wk_api.hip (create / destroy, wk_mfcc, wk_cnn, wk_forward),
// wk_scan.hip, wk_quant.hip, wk_stream.hip, wk_compat.hip.
#pragma once
#include <mutex>
#include <vector>

#include "wk_devmem.h"
#include "wk_kernels.h"

struct wk_handle {
  wk_config cfg;
  int n_cu;
  // protocol error word of the fused kernel: pinned, mapped host memory and its
  // device alias (the kernel writes it, the host reads it after a sync)
  wk::PinnedBuf<unsigned> err;
  // The unfused / int8 path stages features in d_feats_ws.  Calls may come on
  // different streams (and host threads), so each use of the workspace waits
  // on the event recorded after the previous one (stream order across streams).
  std::mutex ws_mu;
  hipEvent_t ws_free;
  bool ws_used;
  bool ws_poisoned;      // the workspace's last use could neither be recorded nor drained: later
                         // staged forwards refuse to run (WK_ERR_HIP) rather than race it
  wk::DevBuf<float> d_weights;    // packed WK_NUM_WEIGHTS floats, or null (front-end only handle)
  wk::DevBuf<float> d_packed;     // fragment-major weights (wk::pack_fragments) for the fused kernel
  wk::DevBuf<float> d_feats_ws;   // feature workspace for the unfused path
  wk::DevBuf<int8_t> d_int8;      // int8 weights (WK_PREC_INT8, wk::quantize_int8_weights at quant.e_w)
  std::vector<float> h_w;    // host copy of the fp32 weights (wk_set_quant re-quantises them, wk_calibrate ranges them)
  wk_quant_spec quant;       // WK_PREC_INT8: the spec in force (wk_set_quant; default xiaoa.info's) ...
  wk::Int8Params qp;         // ... and what the int8 kernels take from it
  wk::DevBuf<uint16_t> d_bf16;    // bf16 conv fragments (WK_PREC_BF16; BF16X3: hi then lo, wk::pack_fragments_bf16)
  int64_t ws_clips;
  int unfused;           // WAKEWORD_UNFUSED=1: front-end + CNN as two kernels (A/B testing)
  int fused_exp;         // WAKEWORD_FUSED_EXP, -DWK_DIAG builds only: role-isolation timing
                         // experiments (wrong logits); always 0 in the shipped library
  int fe_wg_per_cu = 2;  // standalone front-end workgroups per CU (WAKEWORD_FE_WG_PER_CU, -DWK_DIAG builds
                         // only: the occupancy experiment of DESIGN 5.1); 2 in the shipped library
};

namespace wk {

// Convolution arithmetic of the fused kernels (wk_fused_lds.h kConvF32 / kConvBf16 / kConvBf16x3).
inline int conv_mode_of(const wk_handle* h) {
  return h->cfg.precision == WK_PREC_BF16 ? 1 : (h->cfg.precision == WK_PREC_BF16X3 ? 2 : 0);
}

// The handle's CNN on n clips of features: the int8 network or the fused kernel's CNN role.
inline hipError_t launch_cnn(const wk_handle* h, const float* feats, int64_t n, float* logits, hipStream_t stream,
                             unsigned* d_err) {
  return h->cfg.precision == WK_PREC_INT8
             ? launch_int8_cnn(feats, n, h->d_int8, h->qp, logits, 4 * h->n_cu, stream)
             : launch_cnn_fused(feats, n, h->d_packed, h->d_bf16, conv_mode_of(h), logits, h->n_cu, stream, d_err);
}

wk_status check_audio(const void* d_audio, int32_t dtype, int64_t batch, int32_t win_len, int64_t clip_stride,
                      bool mode_b);

// wk_forward with the error word the launches report to: the handle's
// (wk_forward, wk_scan) or a stream object's own (wk_stream_push).
wk_status forward_impl(wk_handle* h, const void* d_audio, int32_t dtype, int64_t batch, int32_t win_len,
                       int64_t clip_stride, float* d_logits, float* d_feats_or_null, void* stream, unsigned* d_err);

}  // namespace wk
