// wk_fused.hip -- the fp32 unit of the fused kernel (wk_fused_dev.h), with the
// front-end's complex arithmetic as packed fp32: wk::launch_fused, which hands
// the bf16 family to wk_fused_xdl.hip, and the standalone CNN
// (wk_cnn_fused_kernel, wk::launch_cnn_fused) in every precision.  Diagnostic
// builds (-DWK_DIAG) keep every precision of the fused kernel here, each with
// its product front-end, and add the phase stamps' global and its reader.
#include "wk_fused_dev.h"

namespace {

#ifdef WK_DIAG
// Diagnostic builds only (-DWK_DIAG, tools/debug): per-wave cycle sums per phase.
__device__ unsigned long long g_wk_stamps[16][16];
#endif

// ---------------------------------------------------------------------------
// Standalone CNN (wk_cnn: LightweightKWS.forward on caller features, the ONNX
// `run` surface).  The same CNN role as the fused kernel, fed from HBM
// (FeatSrc, wk_fused_cnn_role.h): each 1024-thread workgroup runs TWO
// independent CNN roles of 8 waves, each with its own carve of images / pooled
// features / control words, on interleaved clips.
// ---------------------------------------------------------------------------
constexpr int kCnnCarve = kImgEnd - kGOff;   // floats per CNN role: the fused carve window [kGOff, kImgEnd)
constexpr int kCnnLds = 2 * kCnnCarve;
static_assert(kCnnLds * 4 <= 163840, "standalone CNN LDS budget");
static_assert(kCnnCarve % 4 == 0 && kGOff % 4 == 0, "16-byte aligned carves");

template <int CM>
__global__ __launch_bounds__(kFusedBlock, 4) void wk_cnn_fused_kernel(const float* __restrict__ feats, int64_t batch,
                                                                     const float* __restrict__ wts,
                                                                     const uint16_t* __restrict__ wbf,
                                                                     float* __restrict__ logits, unsigned* err) {
  __shared__ __attribute__((aligned(16))) float smem[kCnnLds];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < kCnnLds; i += kFusedBlock) smem[i] = 0.0f;   // guards, padding ci, control words
  __syncthreads();
  const int role = wave >> 3;
  float* base = smem + role * kCnnCarve - kGOff;   // base + kGOff = this role's window
  const int64_t cb = 2 * (int64_t)blockIdx.x + role, cs = 2 * (int64_t)gridDim.x;
  const int64_t n_mine = batch > cb ? (batch - 1 - cb) / cs + 1 : 0;
  FeatSrc<CM> src = {feats, base, cb, cs, 0};
  cnn_role<CM>(base, wts, wbf, n_mine, cb, cs, logits, wave & 7, lane, src);
  report_abort(reinterpret_cast<const unsigned*>(base + kCtrlOff), err, lane);   // this wave's role
}

}  // namespace

#ifdef WK_DIAG
extern "C" int wk_debug_stamps(unsigned long long* host_out, int reset) {
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_wk_stamps), sizeof(g_wk_stamps)) != hipSuccess) return 1;
  if (reset) {
    static unsigned long long zero[16][16];
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_wk_stamps), zero, sizeof(zero)) != hipSuccess) return 1;
  }
  return 0;
}
#endif

namespace wk {

hipError_t launch_fused(bool i16, const void* audio, int64_t batch, int64_t clip_stride, const float* w,
                        const uint16_t* wbf, int conv_mode, float* logits, float* feats_or_null, int grid_cap,
                        hipStream_t stream, unsigned* err, int diag) {
  if (batch == 0) return hipSuccess;
  if (conv_mode != kConvF32 && !wbf) return hipErrorInvalidValue;
#ifdef WK_DIAG   // every precision here: the stamps' global is one device symbol
  return launch_fused_modes<kConvBf16, kConvBf16x3, kConvF32>(i16, conv_mode, audio, batch, clip_stride, w, wbf, logits,
                                                              feats_or_null, grid_cap, stream, err, diag);
#else
  if (conv_mode != kConvF32)   // the bf16 family: wk_fused_xdl.hip (scalar-fp32 front-end)
    return launch_fused_xdl(i16, audio, batch, clip_stride, w, wbf, conv_mode, logits, feats_or_null, grid_cap, stream,
                            err, diag);
  return launch_fused_modes<kConvF32>(i16, conv_mode, audio, batch, clip_stride, w, wbf, logits, feats_or_null,
                                      grid_cap, stream, err, diag);
#endif
}

hipError_t launch_cnn_fused(const float* feats, int64_t batch, const float* w, const uint16_t* wbf, int conv_mode,
                            float* logits, int grid_cap, hipStream_t stream, unsigned* err) {
  if (batch == 0) return hipSuccess;
  if (conv_mode != kConvF32 && !wbf) return hipErrorInvalidValue;
  const int64_t roles = (batch + NBF - 1) / NBF;   // at least one batch of clips per CNN role
  const int grid = (int)((roles + 1) / 2 < grid_cap ? (roles + 1) / 2 : grid_cap);
  if (conv_mode == kConvBf16)
    hipLaunchKernelGGL(wk_cnn_fused_kernel<kConvBf16>, dim3(grid), dim3(kFusedBlock), 0, stream, feats, batch, w, wbf,
                       logits, err);
  else if (conv_mode == kConvBf16x3)
    hipLaunchKernelGGL(wk_cnn_fused_kernel<kConvBf16x3>, dim3(grid), dim3(kFusedBlock), 0, stream, feats, batch, w,
                       wbf, logits, err);
  else
    hipLaunchKernelGGL(wk_cnn_fused_kernel<kConvF32>, dim3(grid), dim3(kFusedBlock), 0, stream, feats, batch, w, wbf,
                       logits, err);
  return hipGetLastError();
}

}  // namespace wk
