// wk_compat.hip -- mfcc.h compatibility shims (main/esp_mfcc/mfcc.h:10-17,
// mfcc.c:431-563) of libwakeword.so: host signal in, malloc'd host block out,
// computed on device 0.  No kernel of its own.
#include <stdio.h>
#include <stdlib.h>

#include <mutex>
#include <utility>
#include <vector>

#include "wk_devmem.h"
#include "wk_kernels.h"
#include "wk_mfcc_shim.h"

using wk::hip_fail;
using wk::on_device;

static std::mutex g_compat_mu;
static wk_handle* g_compat = nullptr;

// The fixed-geometry mode-A handle of the shims (reference configuration).
static bool compat_handle() {
  if (g_compat) return true;
  wk_config cfg = {WK_MODE_ESP_MFCC, WK_PREC_FP32, 1, 0, 0};
  if (wk_create(&cfg, nullptr, &g_compat) != WK_OK) {
    fprintf(stderr, "E (MFCC) device init failed: %s\n", wk_last_error());
    return false;
  }
  return true;
}

// Every other parameter set: wk_esp_mfcc objects, cached per parameter set
// (mfcc.c rebuilds its tables per call; the single-frame variant caches its
// filterbank per (sr, n_filters, n_fft), mfcc.c:362-377).  Caller holds g_compat_mu.
struct EspKey {
  int sr, frame, n_fft, n_filters, n_mfcc;
  bool operator==(const EspKey& o) const {
    return sr == o.sr && frame == o.frame && n_fft == o.n_fft && n_filters == o.n_filters && n_mfcc == o.n_mfcc;
  }
};
static std::vector<std::pair<EspKey, wk_esp_mfcc*>> g_esp_cache;
static wk_esp_mfcc* esp_object(const EspKey& k) {
  for (auto& e : g_esp_cache)
    if (e.first == k) return e.second;
  wk_esp_mfcc* m = nullptr;
  if (wk_esp_mfcc_create(k.sr, k.frame, k.n_fft, k.n_filters, k.n_mfcc, 1, 0, &m) != WK_OK) return nullptr;
  if (g_esp_cache.size() >= 8) {   // oldest out
    (void)wk_esp_mfcc_destroy(g_esp_cache.front().second);
    g_esp_cache.erase(g_esp_cache.begin());
  }
  g_esp_cache.emplace_back(k, m);
  return m;
}

// Host signal -> malloc'd host [nf][n_mfcc] through the device: `run` fills
// d_out from d_sig.  Caller holds g_compat_mu.
template <class F>
static float* shim_run(const float* signal, int n_in, size_t n_out, const char* what, F run) {
  float* host_out = (float*)malloc(sizeof(float) * (n_out ? n_out : 1));
  if (!host_out) return nullptr;
  const wk_status st = on_device(0, [&]() -> wk_status {
    wk::DevBuf<float> d_sig, d_out;   // (freed on every way out of this block, device 0 current)
    hipError_t e;
    if ((e = d_sig.alloc(n_in)) != hipSuccess) return hip_fail(e, "hipMalloc");
    if ((e = d_out.alloc(n_out ? n_out : 1)) != hipSuccess) return hip_fail(e, "hipMalloc");
    if ((e = hipMemcpy(d_sig, signal, sizeof(float) * n_in, hipMemcpyHostToDevice)) != hipSuccess)
      return hip_fail(e, "H2D");
    const wk_status s = run(d_sig.get(), d_out.get());
    if (s != WK_OK) return s;
    if ((e = hipMemcpy(host_out, d_out, sizeof(float) * n_out, hipMemcpyDeviceToHost)) != hipSuccess)
      return hip_fail(e, "D2H");
    return WK_OK;
  });
  if (st != WK_OK) {
    fprintf(stderr, "E (MFCC) %s failed: %s\n", what, wk_last_error());
    free(host_out);
    return nullptr;
  }
  return host_out;
}

extern "C" {

float* extract_mfcc(const float* signal, int signal_len, int sampling_rate, int frame_size, int hop_size, int n_fft,
                    int n_filters, int n_mfcc) {
  if (!wk::shim::check_signal(signal, signal_len, frame_size, hop_size)) return nullptr;
  std::lock_guard<std::mutex> lock(g_compat_mu);
  const size_t n_out = (size_t)wk::shim::frame_count(signal_len, frame_size, hop_size) * n_mfcc;
  if (sampling_rate == 16000 && frame_size == 320 && hop_size == 256 && n_fft == 512 && n_filters == 40 &&
      n_mfcc == 13) {
    if (!compat_handle()) return nullptr;
    return shim_run(signal, signal_len, n_out, "extract_mfcc", [&](float* d_sig, float* d_out) {
      return wk_mfcc(g_compat, d_sig, WK_DTYPE_F32, 1, signal_len, signal_len, d_out, nullptr);
    });
  }
  wk_esp_mfcc* m = esp_object({sampling_rate, frame_size, n_fft, n_filters, n_mfcc});
  if (!m) {
    fprintf(stderr, "E (MFCC) unsupported configuration: %s\n", wk_last_error());
    return nullptr;
  }
  return shim_run(signal, signal_len, n_out, "extract_mfcc", [&](float* d_sig, float* d_out) {
    return wk_esp_mfcc_run(m, d_sig, 1, signal_len, signal_len, hop_size, 0.97f, d_out, nullptr);
  });
}

void free_mfcc(float* mfcc) { free(mfcc); }

// mfcc.c:297-427 flow_extract_mfcc_single_frame: one frame, NO pre-emphasis,
// symmetric Hamming over frame_size, |FFT|^2/n_fft + 1e-12 (esp-dsp packing),
// mel, ln, DCT-II -> malloc'd n_mfcc floats (free with free_mfcc), NULL on bad
// arguments (mfcc.c:300-303).  The reference configuration (320-sample frame,
// 16 kHz, 512, 40 filters, n_mfcc <= 13) runs on the fixed-geometry kernel,
// any other on wk_esp_mfcc.
float* flow_extract_mfcc_single_frame(const float* frame, int frame_size, int sampling_rate, int n_fft, int n_filters,
                                      int n_mfcc) {
  if (!wk::shim::check_frame(frame, frame_size, n_fft)) return nullptr;
  if (n_mfcc < 1) {
    fprintf(stderr, "E (MFCC) Invalid n_mfcc\n");
    return nullptr;
  }
  std::lock_guard<std::mutex> lock(g_compat_mu);
  if (sampling_rate == 16000 && frame_size == 320 && n_fft == 512 && n_filters == 40 && n_mfcc <= 13) {
    if (!compat_handle()) return nullptr;
    // (the first n_mfcc of the 13 are the caller's; the block is larger than it needs)
    return shim_run(frame, frame_size, 13, "flow_extract_mfcc_single_frame", [&](float* d_sig, float* d_out) {
      const hipError_t e = wk::launch_frontend(false, false, d_sig, 1, frame_size, frame_size, d_out, 1, 0, 1, 0.0f,
                                               nullptr);
      return e == hipSuccess ? WK_OK : hip_fail(e, "frontend launch");
    });
  }
  wk_esp_mfcc* m = esp_object({sampling_rate, frame_size, n_fft, n_filters, n_mfcc});
  if (!m) {
    fprintf(stderr, "E (MFCC) unsupported configuration: %s\n", wk_last_error());
    return nullptr;
  }
  return shim_run(frame, frame_size, (size_t)n_mfcc, "flow_extract_mfcc_single_frame", [&](float* d_sig, float* d_out) {
    return wk_esp_mfcc_run(m, d_sig, 1, frame_size, frame_size, frame_size, 0.0f, d_out, nullptr);
  });
}

void analyze_mfcc_range(float* mfcc, int size, const char* label) { wk::shim::analyze_range(mfcc, size, label); }

}  // extern "C"
