// wk_stream.hip -- the streaming ring:
// the wk_stream_* C ABI and its ingest kernel.
//
// A ring of `cap` float samples, stored mirrored (sample p at p % cap and
// p % cap + cap), so every window of <= cap samples is contiguous and a run of
// consecutive windows is one strided wk_forward launch.  Writes follow
// ring_buffer.c:57-117 (write_rinbuffer): a push longer than the ring keeps
// only its newest `cap` samples, older data is overwritten.  Window k covers
// stream samples [k*hop, k*hop + 16000); a push completes every window whose
// end it reaches; windows whose start was already overwritten are dropped.
//
// The mirrored ring is in device memory.  A push writes its samples once into
// a pinned, mapped host staging ring of `cap` (same positions); a push that
// completes windows first launches wk_ring_ingest_kernel, which reads the
// samples pushed since the last launch (only the newest `cap`: older ones are
// overwritten, and no window left to score starts there) across PCIe into both
// copies of the device ring, then the fused kernel reads its windows from HBM
// and writes the logits straight into pinned host memory -- two launches and
// one wait per push, no copy commands.  (Reading each window across PCIe
// instead, zero-copy from a mirrored host ring, cost ~9 us per window: one
// workgroup's loads over PCIe latency; a hop of new samples is one round trip.)
#include <string.h>

#include <memory>
#include <new>
#include <string>

#include "wk_handle.h"

using wk::g_last_error;
using wk::hip_fail;
using wk::invalid;
using wk::on_device;

namespace {

// Streaming ring ingest (wk_stream_push): ring samples [pos, pos + m) (mod
// cap, m <= cap) from the pinned host staging ring, read across PCIe, into
// both copies of the mirrored device ring.
__global__ __launch_bounds__(256) void wk_ring_ingest_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                             int64_t cap, int64_t pos, int64_t m) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = pos + i < cap ? pos + i : pos + i - cap;
    const float v = src[p];
    dst[p] = v;
    dst[p + cap] = v;
  }
}

hipError_t launch_ring_ingest(const float* src, float* dst, int64_t cap, int64_t pos, int64_t m, hipStream_t stream) {
  if (m <= 0) return hipSuccess;
  if (pos < 0 || pos >= cap || m > cap) return hipErrorInvalidValue;
  int64_t blocks = (m + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(wk_ring_ingest_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, dst, cap, pos, m);
  return hipGetLastError();
}

}  // namespace

struct wk_stream {
  wk_handle* h;
  hipStream_t st;
  int32_t hop, cap;
  int64_t total;        // samples pushed since create / reset
  int64_t next_win;     // index of the next window to score
  int64_t ingested;     // stream samples [0, ingested) are in d_ring (as far as it holds them)
  wk::PinnedBuf<float> ring;      // [cap] staging ring (written by the host, read by the ingest kernel)
  wk::DevBuf<float> d_ring;       // device [2*cap], mirrored: sample p at p % cap and p % cap + cap
  wk::PinnedBuf<float> logits;    // [max_win] (written by the kernel)
  wk::PinnedBuf<unsigned> err;    // this stream object's own error word (its pushes' launches only)
  int32_t max_win;
};

extern "C" {

wk_status wk_stream_create(wk_handle* h, int32_t hop, int32_t capacity, void* stream, wk_stream** out) {
  if (!h || !out) return invalid("wk_stream_create: null argument");
  if (hop < 1 || capacity < WK_WIN_SAMPLES + hop) return invalid("wk_stream_create: need hop >= 1, capacity >= 16000 + hop");
  if (h->cfg.mode != WK_MODE_TORCHAUDIO_CMVN || !h->d_weights)
    return invalid("wk_stream_create: needs a mode-B handle with weights");
  *out = nullptr;
  return on_device(h->cfg.device, [&]() -> wk_status {
    // (the scalar members start at zero; a failed create frees it here, device current)
    std::unique_ptr<wk_stream> s(new (std::nothrow) wk_stream());
    if (!s) return WK_ERR_NO_MEMORY;
    s->h = h;
    s->st = (hipStream_t)stream;
    s->hop = hop;
    s->cap = capacity;
    s->max_win = (capacity - WK_WIN_SAMPLES) / hop + 1;
    hipError_t e;
    if ((e = s->ring.alloc((size_t)capacity)) != hipSuccess || (e = s->d_ring.alloc(2 * (size_t)capacity)) != hipSuccess ||
        (e = s->logits.alloc((size_t)s->max_win)) != hipSuccess || (e = s->err.alloc(1)) != hipSuccess)
      return e == hipErrorOutOfMemory ? WK_ERR_NO_MEMORY : hip_fail(e, "wk_stream_create");
    memset(s->ring.host(), 0, sizeof(float) * (size_t)capacity);
    *s->err.host() = 0;
    *out = s.release();
    return WK_OK;
  });
}

wk_status wk_stream_destroy(wk_stream* s) {
  if (!s) return WK_OK;
  return on_device(s->h->cfg.device, [&]() -> wk_status {
    (void)hipStreamSynchronize(s->st);
    delete s;
    return WK_OK;
  });
}

wk_status wk_stream_reset(wk_stream* s) {
  if (!s) return invalid("wk_stream_reset: null stream");
  s->total = 0;
  s->next_win = 0;
  s->ingested = 0;
  return WK_OK;
}

wk_status wk_stream_push(wk_stream* s, const float* samples, int64_t n, float* out_logits, int64_t* out_end,
                         int32_t max_out, int32_t* n_out) {
  if (!s || !n_out || n < 0 || (n > 0 && !samples) || max_out < 0 || (max_out > 0 && !out_logits))
    return invalid("wk_stream_push: bad arguments");
  *n_out = 0;
  // Every push that launches work waits for it before returning, so no kernel
  // is reading the host staging ring while it is rewritten here.
  const int64_t cap = s->cap;
  // 1. ring write (overwrite-oldest): only the newest `cap` samples of a long push survive.
  const int64_t skip = n > cap ? n - cap : 0;
  const int64_t m = n - skip;
  const int64_t p0 = s->total + skip;
  for (int64_t done = 0; done < m;) {   // at most two segments (wrap)
    const int64_t pos = (p0 + done) % cap;
    const int64_t len = m - done < cap - pos ? m - done : cap - pos;
    memcpy(s->ring.host() + pos, samples + skip + done, sizeof(float) * (size_t)len);
    done += len;
  }
  s->total += n;
  // 2. windows completed by this push whose start is still in the ring.
  const int64_t last = s->total >= WK_WIN_SAMPLES ? (s->total - WK_WIN_SAMPLES) / s->hop : -1;
  int64_t first = s->next_win;
  const int64_t oldest = s->total > cap ? (s->total - cap + s->hop - 1) / s->hop : 0;
  if (first < oldest) first = oldest;
  if (last - first + 1 > max_out) first = last - max_out + 1;   // report the newest max_out
  s->next_win = last + 1 > s->next_win ? last + 1 : s->next_win;
  const int64_t k = last - first + 1;
  if (k <= 0) return WK_OK;
  return on_device(s->h->cfg.device, [&]() -> wk_status {
    // 3. score them: contiguous strided runs in the mirrored ring.  On any
    // failure after the first launch the stream is drained before returning,
    // so no kernel is still reading the host ring when the next push rewrites it.
    struct Drain {
      hipStream_t st;
      bool armed = false;
      ~Drain() {
        if (armed) (void)hipStreamSynchronize(st);
      }
    } drain{s->st};
    hipError_t e;
    // the samples pushed since the last launch that the staging ring still holds
    const int64_t from = s->ingested > s->total - cap ? s->ingested : s->total - cap;
    drain.armed = true;
    if ((e = launch_ring_ingest(s->ring.dev(), s->d_ring, cap, from % cap, s->total - from, s->st)) != hipSuccess)
      return hip_fail(e, "wk_stream_push: ingest");
    s->ingested = s->total;
    int64_t w = first;
    while (w <= last) {
      const int64_t off = (w * s->hop) % cap;
      int64_t run = (2 * cap - WK_WIN_SAMPLES - off) / s->hop + 1;   // windows that fit before the mirror end
      if (run > last - w + 1) run = last - w + 1;
      wk_status st = wk::forward_impl(s->h, s->d_ring + off, WK_DTYPE_F32, run, WK_WIN_SAMPLES, s->hop,
                                      s->logits.dev() + (w - first), nullptr, s->st, s->err.dev());
      if (st != WK_OK) return st;
      w += run;
    }
    if ((e = hipStreamSynchronize(s->st)) != hipSuccess) return hip_fail(e, "wk_stream_push: sync");
    drain.armed = false;
    // synced, and only this stream object's launches report to its word: final
    if (const uint32_t f = __atomic_exchange_n(s->err.host(), 0u, __ATOMIC_SEQ_CST)) {
      g_last_error = "fused kernel protocol error (flags " + std::to_string(f) + "): these logits are invalid";
      return WK_ERR_DEVICE;
    }
    memcpy(out_logits, s->logits.host(), sizeof(float) * (size_t)k);
    if (out_end)
      for (int64_t i = 0; i < k; ++i) out_end[i] = (first + i) * s->hop + WK_WIN_SAMPLES;
    *n_out = (int32_t)k;
    return WK_OK;
  });
}

}  // extern "C"
