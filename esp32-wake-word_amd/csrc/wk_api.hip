// wk_api.hip -- the core of the C ABI of include/wakeword.h: status strings and
// the error helpers, the handle (wk_create / wk_destroy / wk_check_device_errors),
// wk_mfcc, wk_cnn, wk_forward, and the one-line wrappers of the wk_misc.hip
// kernels.  The other surfaces sit beside their kernels: wk_scan.hip,
// wk_quant.hip, wk_stream.hip, wk_esp_mfcc.hip, wk_train.hip, wk_ctc*.hip, and
// the mfcc.h shims in wk_compat.hip.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "wk_handle.h"

namespace wk {

thread_local std::string g_last_error;

wk_status hip_fail(hipError_t e, const char* what) {
  g_last_error = std::string(what) + ": " + hipGetErrorString(e);
  return WK_ERR_HIP;
}

wk_status invalid(const char* what) {
  g_last_error = what;
  return WK_ERR_INVALID_ARG;
}

wk_status fail(wk_status s, const char* what) {
  g_last_error = what;
  return s;
}

// ---- shared with the other units that take a wk_handle (declared in wk_handle.h)

wk_status check_audio(const void* d_audio, int32_t dtype, int64_t batch, int32_t win_len, int64_t clip_stride,
                      bool mode_b) {
  if (batch < 0) return invalid("batch < 0");
  if (batch > 0 && !d_audio) return invalid("null audio pointer");
  if (dtype != WK_DTYPE_F32 && dtype != WK_DTYPE_I16) return invalid("bad dtype");
  if (mode_b && win_len != WK_WIN_SAMPLES) return invalid("mode B (torchaudio+CMVN) requires win_len == 16000");
  if (!mode_b && win_len < 320) return invalid("mode A requires win_len >= 320");
  if (batch > 1 && clip_stride < 1) return invalid("clip_stride < 1");   // < win_len = overlapping (sliding) windows
  return WK_OK;
}

wk_status forward_impl(wk_handle* h, const void* d_audio, int32_t dtype, int64_t batch, int32_t win_len,
                       int64_t clip_stride, float* d_logits, float* d_feats_or_null, void* stream, unsigned* d_err) {
  if (!h) return invalid("wk_forward: null handle");
  if (h->cfg.mode != WK_MODE_TORCHAUDIO_CMVN) {
    g_last_error = "wk_forward: the xiaoa CNN consumes mode-B (torchaudio+CMVN) features";
    return WK_ERR_UNSUPPORTED;
  }
  if (!h->d_weights) return invalid("wk_forward: handle created without weights");
  wk_status s = check_audio(d_audio, dtype, batch, win_len, clip_stride, true);
  if (s != WK_OK) return s;
  if (batch > 0 && !d_logits) return invalid("wk_forward: null logits");
  const bool int8 = h->cfg.precision == WK_PREC_INT8;
  return on_device(h->cfg.device, [&]() -> wk_status {
    if (!h->unfused && !int8) {
      hipError_t e = wk::launch_fused(dtype == WK_DTYPE_I16, d_audio, batch, clip_stride, h->d_packed, h->d_bf16,
                                      conv_mode_of(h), d_logits, d_feats_or_null, h->n_cu, (hipStream_t)stream, d_err,
                                      h->fused_exp);
      return e == hipSuccess ? WK_OK : hip_fail(e, "fused launch");
    }
    const size_t esz = dtype == WK_DTYPE_I16 ? 2 : 4;
    // Features staged in the shared workspace: order this use after the last
    // one, whatever stream it ran on (a caller-provided feature buffer needs no ordering).
    std::unique_lock<std::mutex> ws_lock(h->ws_mu, std::defer_lock);
    if (!d_feats_or_null && batch > 0) {
      ws_lock.lock();
      if (h->ws_poisoned)
        return wk::fail(WK_ERR_HIP, "wk_forward: the feature workspace's previous use could not be ordered or drained");
      hipError_t e = h->ws_used ? hipStreamWaitEvent((hipStream_t)stream, h->ws_free, 0) : hipSuccess;
      if (e != hipSuccess) return hip_fail(e, "hipStreamWaitEvent(workspace)");
    }
    // Every exit after the first launch (a failed later launch included) marks
    // the workspace busy until this stream's queued chunks are done, so the next
    // call on another stream still waits for them.  If the event cannot be
    // recorded, this stream is drained instead (the workspace is then idle)
    // and the failure is reported.
    bool launched = false;
    struct WsRelease {
      wk_handle* h;
      std::unique_lock<std::mutex>& lk;
      bool& launched;
      hipStream_t st;
      hipError_t release() {
        if (!lk.owns_lock() || !launched) return hipSuccess;
        launched = false;
        hipError_t e = hipEventRecord(h->ws_free, st);
        if (e == hipSuccess) {
          h->ws_used = true;
          return e;
        }
        if (hipStreamSynchronize(st) == hipSuccess || hipDeviceSynchronize() == hipSuccess) {
          h->ws_used = false;   // drained: nothing left to wait for
        } else {
          h->ws_poisoned = true;   // this call's chunks may still be queued: no later call may reuse the workspace
        }
        return e;
      }
      ~WsRelease() { (void)release(); }
    } ws_release{h, ws_lock, launched, (hipStream_t)stream};
    for (int64_t c0 = 0; c0 < batch; c0 += h->ws_clips) {
      const int64_t n = batch - c0 < h->ws_clips ? batch - c0 : h->ws_clips;
      float* feats = d_feats_or_null ? d_feats_or_null + c0 * 13 * 63 : h->d_feats_ws;
      const void* a = (const char*)d_audio + (size_t)(c0 * clip_stride) * esz;
      launched = true;   // (a failed launch may still have queued work)
      hipError_t e = wk::launch_frontend(true, dtype == WK_DTYPE_I16, a, n, win_len, clip_stride, feats, 0, 1,
                                         2 * h->n_cu, 0.97f, (hipStream_t)stream);
      if (e != hipSuccess) return hip_fail(e, "frontend launch");
      if ((e = launch_cnn(h, feats, n, d_logits + c0, (hipStream_t)stream, d_err)) != hipSuccess)
        return hip_fail(e, "cnn launch");
    }
    const hipError_t er = ws_release.release();
    if (er != hipSuccess) return hip_fail(er, "hipEventRecord(workspace)");
    return WK_OK;
  });
}

}  // namespace wk

using wk::check_audio;
using wk::g_last_error;
using wk::hip_fail;
using wk::invalid;
using wk::on_device;

namespace {

constexpr int64_t kWorkspaceClips = 16384;

}  // namespace

extern "C" {

int32_t wk_abi_version(void) { return WK_ABI_VERSION; }

const char* wk_status_string(wk_status s) {
  switch (s) {
    case WK_OK: return "WK_OK";
    case WK_ERR_INVALID_ARG: return "WK_ERR_INVALID_ARG";
    case WK_ERR_HIP: return "WK_ERR_HIP";
    case WK_ERR_NO_MEMORY: return "WK_ERR_NO_MEMORY";
    case WK_ERR_UNSUPPORTED: return "WK_ERR_UNSUPPORTED";
    case WK_ERR_DEVICE: return "WK_ERR_DEVICE";
  }
  return "WK_ERR_UNKNOWN";
}

const char* wk_last_error(void) { return g_last_error.c_str(); }

wk_status wk_create(const wk_config* cfg, const float* host_weights, wk_handle** out) {
  if (!cfg || !out) return invalid("wk_create: null cfg/out");
  *out = nullptr;
  if (cfg->mode != WK_MODE_TORCHAUDIO_CMVN && cfg->mode != WK_MODE_ESP_MFCC) return invalid("wk_create: bad mode");
  if (cfg->precision != WK_PREC_FP32 && cfg->precision != WK_PREC_BF16 && cfg->precision != WK_PREC_INT8 &&
      cfg->precision != WK_PREC_BF16X3)
    return invalid("wk_create: bad precision");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
  if (cfg->device < 0 || cfg->device >= ndev) return invalid("wk_create: device ordinal out of range");
  wk_handle* h = new (std::nothrow) wk_handle();
  if (!h) return WK_ERR_NO_MEMORY;
  h->cfg = *cfg;
  wk_quant_spec_default(&h->quant);
  (void)wk::int8_params(h->quant, &h->qp);
  {
    const char* u = getenv("WAKEWORD_UNFUSED");
    h->unfused = u && u[0] == '1';
#ifdef WK_DIAG
    const char* fx = getenv("WAKEWORD_FUSED_EXP");
    h->fused_exp = fx ? atoi(fx) : 0;
    const char* fw = getenv("WAKEWORD_FE_WG_PER_CU");
    if (fw && (atoi(fw) == 1 || atoi(fw) == 2)) h->fe_wg_per_cu = atoi(fw);
#endif
  }
  wk_status st = on_device(cfg->device, [&]() -> wk_status {
    hipDeviceProp_t prop;
    hipError_t e2 = hipGetDeviceProperties(&prop, cfg->device);
    if (e2 != hipSuccess) return hip_fail(e2, "hipGetDeviceProperties");
    h->n_cu = prop.multiProcessorCount;
    const char* call = nullptr;
    if ((e2 = h->err.alloc(1, &call)) != hipSuccess) return hip_fail(e2, (std::string(call) + "(error word)").c_str());
    *h->err.host() = 0;
    if ((e2 = hipEventCreateWithFlags(&h->ws_free, hipEventDisableTiming)) != hipSuccess)
      return hip_fail(e2, "hipEventCreate");
    if (host_weights) {
      h->h_w.assign(host_weights, host_weights + WK_NUM_WEIGHTS);
      if ((e2 = h->d_weights.alloc(WK_NUM_WEIGHTS)) != hipSuccess) return hip_fail(e2, "hipMalloc(weights)");
      if ((e2 = hipMemcpy(h->d_weights, host_weights, sizeof(float) * WK_NUM_WEIGHTS, hipMemcpyHostToDevice)) !=
          hipSuccess)
        return hip_fail(e2, "hipMemcpy(weights)");
      std::vector<float> pk(wk::kNumPacked);
      wk::pack_fragments(host_weights, pk.data());
      if ((e2 = h->d_packed.alloc(wk::kNumPacked)) != hipSuccess) return hip_fail(e2, "hipMalloc(packed weights)");
      if ((e2 = hipMemcpy(h->d_packed, pk.data(), sizeof(float) * wk::kNumPacked, hipMemcpyHostToDevice)) !=
          hipSuccess)
        return hip_fail(e2, "hipMemcpy(packed weights)");
      if (cfg->precision == WK_PREC_BF16 || cfg->precision == WK_PREC_BF16X3) {
        const bool split = cfg->precision == WK_PREC_BF16X3;   // hi fragments, then lo fragments
        std::vector<uint16_t> pb(wk::kNumPackedBf16 * (split ? 2 : 1));
        wk::pack_fragments_bf16(host_weights, pb.data());
        if (split) wk::pack_fragments_bf16(host_weights, pb.data() + wk::kNumPackedBf16, true);
        if ((e2 = h->d_bf16.alloc(pb.size())) != hipSuccess) return hip_fail(e2, "hipMalloc(bf16 weights)");
        if ((e2 = hipMemcpy(h->d_bf16, pb.data(), pb.size() * 2, hipMemcpyHostToDevice)) != hipSuccess)
          return hip_fail(e2, "hipMemcpy(bf16 weights)");
      }
      if (cfg->precision == WK_PREC_INT8) {
        std::vector<int8_t> q(wk::kNumInt8Weights);
        wk::quantize_int8_weights(host_weights, h->quant.e_w, q.data());
        if ((e2 = h->d_int8.alloc(q.size())) != hipSuccess) return hip_fail(e2, "hipMalloc(int8 weights)");
        if ((e2 = hipMemcpy(h->d_int8, q.data(), q.size(), hipMemcpyHostToDevice)) != hipSuccess)
          return hip_fail(e2, "hipMemcpy(int8 weights)");
      }
      h->ws_clips = kWorkspaceClips;
      if ((e2 = h->d_feats_ws.alloc((size_t)13 * 63 * h->ws_clips)) != hipSuccess)
        return hip_fail(e2, "hipMalloc(workspace)");
    }
    return WK_OK;
  });
  if (st != WK_OK) {
    wk_destroy(h);
    return st;
  }
  *out = h;
  return WK_OK;
}

wk_status wk_destroy(wk_handle* h) {
  if (!h) return WK_OK;
  const wk_status s = on_device(h->cfg.device, [&]() -> wk_status {
    if (h->ws_free) {   // the workspace's last use is over before it is freed
      (void)hipEventSynchronize(h->ws_free);
      (void)hipEventDestroy(h->ws_free);
    }
    delete h;   // frees the handle's device and pinned memory, with its device current
    return WK_OK;
  });
  if (s != WK_OK) delete h;   // the device could not be made current: the handle goes all the same
  return WK_OK;
}

wk_status wk_check_device_errors(wk_handle* h, uint32_t* flags_out) {
  if (!h) return invalid("wk_check_device_errors: null handle");
  return on_device(h->cfg.device, [&]() -> wk_status {
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "wk_check_device_errors: sync");
    const uint32_t f = __atomic_exchange_n(h->err.host(), 0u, __ATOMIC_SEQ_CST);
    if (flags_out) *flags_out = f;
    if (f) {
      g_last_error = "fused kernel protocol error (flags " + std::to_string(f) + "): logits since the last check are invalid";
      return WK_ERR_DEVICE;
    }
    return WK_OK;
  });
}

wk_status wk_mfcc(wk_handle* h, const void* d_audio, int32_t dtype, int64_t batch, int32_t win_len,
                  int64_t clip_stride, float* d_feats, void* stream) {
  if (!h) return invalid("wk_mfcc: null handle");
  const bool mode_b = h->cfg.mode == WK_MODE_TORCHAUDIO_CMVN;
  wk_status s = check_audio(d_audio, dtype, batch, win_len, clip_stride, mode_b);
  if (s != WK_OK) return s;
  if (batch > 0 && !d_feats) return invalid("wk_mfcc: null feats");
  return on_device(h->cfg.device, [&]() -> wk_status {
    hipError_t e = wk::launch_frontend(mode_b, dtype == WK_DTYPE_I16, d_audio, batch, win_len, clip_stride, d_feats,
                                       h->cfg.esp_dsp_packing, h->cfg.cmvn, h->fe_wg_per_cu * h->n_cu, 0.97f,
                                       (hipStream_t)stream);
    return e == hipSuccess ? WK_OK : hip_fail(e, "frontend launch");
  });
}

wk_status wk_cnn(wk_handle* h, const float* d_feats, int64_t batch, float* d_logits, void* stream) {
  if (!h) return invalid("wk_cnn: null handle");
  if (!h->d_weights) return invalid("wk_cnn: handle created without weights");
  if (batch < 0 || (batch > 0 && (!d_feats || !d_logits))) return invalid("wk_cnn: bad arguments");
  return on_device(h->cfg.device, [&]() -> wk_status {
    const hipError_t e = wk::launch_cnn(h, d_feats, batch, d_logits, (hipStream_t)stream, h->err.dev());
    return e == hipSuccess ? WK_OK : hip_fail(e, "cnn launch");
  });
}

wk_status wk_forward(wk_handle* h, const void* d_audio, int32_t dtype, int64_t batch, int32_t win_len,
                     int64_t clip_stride, float* d_logits, float* d_feats_or_null, void* stream) {
  return wk::forward_impl(h, d_audio, dtype, batch, win_len, clip_stride, d_logits, d_feats_or_null, stream,
                          h ? h->err.dev() : nullptr);
}

wk_status wk_synth_clips(uint32_t seed, int64_t first, int64_t count, int32_t n, float* d_out, void* stream) {
  if (count < 0 || n <= 0 || (count > 0 && !d_out)) return invalid("wk_synth_clips: bad arguments");
  hipError_t e = wk::launch_synth(seed, first, count, n, d_out, (hipStream_t)stream);
  return e == hipSuccess ? WK_OK : hip_fail(e, "synth launch");
}

wk_status wk_normalize(const float* d_in, float* d_out, int64_t batch, int32_t n_coef, int32_t n_time,
                       int32_t method, void* stream) {
  if (batch < 0 || n_coef <= 0 || n_time <= 1 || method < 0 || method > 3) return invalid("wk_normalize: bad args");
  if (batch > 0 && (!d_in || !d_out)) return invalid("wk_normalize: null pointer");
  hipError_t e = wk::launch_normalize(d_in, d_out, batch, n_coef, n_time, method, (hipStream_t)stream);
  return e == hipSuccess ? WK_OK : hip_fail(e, "normalize launch");
}

wk_status wk_record_front(const int16_t* d_tdm, int64_t n_out, int16_t* d_out16, float* d_out_f32_or_null,
                          void* stream) {
  if (n_out < 0 || (n_out > 0 && (!d_tdm || !d_out16))) return invalid("wk_record_front: bad arguments");
  if (n_out > 1 && ((uintptr_t)d_tdm & 15)) return invalid("wk_record_front: d_tdm must be 16-byte aligned");
  if (((uintptr_t)d_out16 & 3) || ((uintptr_t)d_out_f32_or_null & 7))
    return invalid("wk_record_front: d_out16 must be 4-byte and d_out_f32 8-byte aligned");
  hipError_t e = wk::launch_record_front(d_tdm, n_out, d_out16, d_out_f32_or_null, (hipStream_t)stream);
  return e == hipSuccess ? WK_OK : hip_fail(e, "record_front launch");
}

wk_status wk_quantize_frames(const float* d_mfcc, int64_t n_values, int8_t* d_out_i8, void* stream) {
  if (n_values < 0 || (n_values > 0 && (!d_mfcc || !d_out_i8))) return invalid("wk_quantize_frames: bad arguments");
  hipError_t e = wk::launch_quantize_frames(d_mfcc, n_values, d_out_i8, (hipStream_t)stream);
  return e == hipSuccess ? WK_OK : hip_fail(e, "quantize_frames launch");
}

wk_status wk_device_cmvn(const void* d_frames, int32_t dtype, int64_t n_frames, int8_t* d_out_i8,
                         float* d_feats_or_null, void* stream) {
  if (n_frames < 0 || (dtype != WK_DTYPE_I8 && dtype != WK_DTYPE_F32)) return invalid("wk_device_cmvn: bad args");
  if (!d_out_i8 && !d_feats_or_null) return invalid("wk_device_cmvn: no output");
  const int64_t n_windows = n_frames >= 63 ? n_frames - 62 : 0;
  if (n_windows > 0 && !d_frames) return invalid("wk_device_cmvn: null frames");
  hipError_t e = wk::launch_device_cmvn(d_frames, dtype == WK_DTYPE_I8, n_windows, d_out_i8, d_feats_or_null,
                                        (hipStream_t)stream);
  return e == hipSuccess ? WK_OK : hip_fail(e, "device_cmvn launch");
}

}  // extern "C"
