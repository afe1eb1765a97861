// wk_fused_xdl.hip -- the bf16-family unit of the fused kernel
// (wk_fused_dev.h; conv_mode 1 = bf16, config 4; 2 = split bf16), with the
// front-end's complex arithmetic as scalar fp32 pairs (FeScalar, wk_common.h;
// the kernel picks it from the conv mode).  It defines wk::launch_fused_xdl
// only; wk::launch_fused (wk_fused.hip) calls it for those modes.  Empty in
// diagnostic builds (-DWK_DIAG), which keep every precision in wk_fused.hip:
// the stamps' global is one device symbol.
#include "wk_fused_dev.h"

#ifndef WK_DIAG
namespace wk {

hipError_t launch_fused_xdl(bool i16, const void* audio, int64_t batch, int64_t clip_stride, const float* w,
                            const uint16_t* wbf, int conv_mode, float* logits, float* feats_or_null, int grid_cap,
                            hipStream_t stream, unsigned* err, int diag) {
  if (batch == 0) return hipSuccess;
  if (conv_mode != kConvF32 && !wbf) return hipErrorInvalidValue;
  return launch_fused_modes<kConvBf16x3, kConvBf16>(i16, conv_mode, audio, batch, clip_stride, w, wbf, logits,
                                                    feats_or_null, grid_cap, stream, err, diag);
}

}  // namespace wk
#endif
