// wk_ctc.hip -- the GRU-CTC head (ml_models/ctc.py) on gfx950:
// the inference half of the wk_ctc_* C ABI.
//
//   audio -> log-mel 80 + global z-score (ctc.py:82-107)          wk_ctc_logmel.hip
//         -> Linear 80->128 + LayerNorm + ReLU (ctc.py:125-130)   wk_ctc_dense.hip
//         -> 2-layer bidirectional GRU, H = 128 (ctc.py:133-140)  wk_ctc_gru.hip
//         -> Linear 256->V, log_softmax (ctc.py:143-152)          wk_ctc_out.hip (fp16), wk_ctc_dense.hip (fp32 GEMM)
//         -> greedy CTC decode (ctc.py:453-471)                   wk_ctc_out.hip
//
// This unit holds no kernel: creating and destroying the handle of
// wk_ctc_handle.h (weights uploaded in each kernel's layout by its unit's
// packer), growing its workspaces, stage timing, and the stage sequence of
// wk_ctc_features / wk_ctc_forward / wk_ctc_transcribe over the launchers
// declared in wk_ctc_dev.h.  The entry points that need an fp32 handle
// (training forward, backward, dropout masks, weights, optimiser) are in
// wk_ctc_train.hip, which runs the forward through the stage functions here.
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <new>
#include <string>
#include <type_traits>

#include "wk_ctc_handle.h"

using namespace wk;

namespace {

// wk_ctc_forward's workspace: the buffers this handle's path uses (fp32: x0,
// gi, y0, y1, logits; fp16: the half tensors, gi only for the GEMM projections;
// the attribution mixes add the other precision's y1 / logits), at `rows` rows.
std::vector<WsEntry> ws_table(wk_ctc* c, size_t rows) {
  const bool f16 = c->f16, m1 = c->mix == 1, m2 = c->mix == 2;
  const size_t F = sizeof(float) * rows, Hf = sizeof(__half) * rows, H = kH, V = (size_t)c->cfg.vocab;
  CtcInferWs& w = c->ws;
  return {{&w.x0, !f16 * F * H},
          {&w.gi, (!f16 || c->gru_gemm) * F * 6 * H},
          {&w.y0, !f16 * F * 2 * H},
          {&w.y1, (!f16 || m1) * F * 2 * H},
          {&w.logits, (!f16 || m1) * F * V},
          {&w.best, sizeof(int) * rows},
          {&w.best2, sizeof(int) * rows},
          {&w.x0h, f16 * Hf * H},
          {&w.y0h, f16 * Hf * 2 * H},
          {&w.y1h, (f16 || m2) * Hf * 2 * H},
          {&w.logits16, f16 * Hf * V}};
}

// Fold the recorded stage events into the per-stage sums (synchronises on them).
hipError_t fold_events(wk_ctc* c) {
  CtcStageTimes& p = c->prof;
  hipError_t err = hipSuccess;
  for (int i = 0; i < p.n_ev; ++i) {
    float ms = 0.0f;
    hipError_t e = hipEventSynchronize(p.ev[i].b);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, p.ev[i].a, p.ev[i].b);
    if (e == hipSuccess) {
      p.ms[p.ev[i].stage] += ms;
      p.n[p.ev[i].stage] += 1;
    } else if (err == hipSuccess) {
      err = e;
    }
    (void)hipEventDestroy(p.ev[i].a);
    (void)hipEventDestroy(p.ev[i].b);
  }
  p.n_ev = 0;
  return err;
}

// Stage bracket: records an event pair around `body` when profiling is on (and
// the caller's stages are bracketed at all).  body returns a wk_status, or
// nothing when it only enqueues kernels.
template <typename F>
wk_status timed(wk_ctc* c, int stage, hipStream_t st, F body, bool bracket = true) {
  auto launch = [&]() -> wk_status {
    if constexpr (std::is_void<decltype(body())>::value) {
      body();
      return WK_OK;
    } else {
      return body();
    }
  };
  CtcStageTimes& p = c->prof;
  if (!p.on || !bracket) return launch();
  if (p.n_ev == 64 && fold_events(c) != hipSuccess) return fail(WK_ERR_HIP, "wk_ctc stage timing");
  auto& e = p.ev[p.n_ev];
  if (hipEventCreate(&e.a) != hipSuccess) return fail(WK_ERR_HIP, "hipEventCreate");
  if (hipEventCreate(&e.b) != hipSuccess) {
    (void)hipEventDestroy(e.a);
    return fail(WK_ERR_HIP, "hipEventCreate");
  }
  e.stage = stage;
  ++p.n_ev;
  (void)hipEventRecord(e.a, st);
  const wk_status s = launch();
  (void)hipEventRecord(e.b, st);
  return s;
}

hipError_t upload_f16(DevBuf<__half>& d, const float* h, size_t n) {
  std::vector<__half> t(n);
  for (size_t i = 0; i < n; ++i) t[i] = __float2half(h[i]);
  return d.upload(t);
}
hipError_t upload_f16(DevBuf<__half>& d, const std::vector<float>& h) { return upload_f16(d, h.data(), h.size()); }

}  // namespace

namespace wk {

wk_status ctc_grow(hipStream_t st, const std::vector<WsEntry>& bufs, std::initializer_list<WsCap> caps, const char* what) {
  hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail(e, "sync");
  for (const WsCap& k : caps) *k.cap = 0;
  for (const WsEntry& b : bufs) b.buf->reset();
  for (const WsEntry& b : bufs)
    if (b.bytes && e == hipSuccess) e = b.buf->alloc_bytes(b.bytes);
  if (e != hipSuccess) {
    for (const WsEntry& b : bufs) b.buf->reset();
    return ctc_alloc_failed(e, what);
  }
  for (const WsCap& k : caps) *k.cap = k.value;
  return WK_OK;
}

wk_status stage_encoder(const Fwd& f, const float* d_feats, const float2* zs, void* x0) {
  const wk_ctc* c = f.c;
  return timed(f.c, WK_CTC_STAGE_ENCODER, f.st, [&] {
    launch_ctc_encoder(c->f16, d_feats, (int)f.batch, f.T, c->w.enc_w, c->w.enc_b, c->w.ln_g, c->w.ln_b, zs, x0, c->n_cu, f.st);
  }, f.timed);
}

wk_status stage_gru(const Fwd& f, int l, const void* in, float* gi, void* y) {
  wk_ctc* c = f.c;
  const CtcWeights& w = c->w;
  const int H = kH, din = l == 0 ? H : 2 * H;
  if (c->f16 && !c->gru_gemm)   // projection fused into the recurrence: no GEMM, no gate-input tensor
    return timed(c, WK_CTC_STAGE_GRU0 + 2 * l, f.st, [&] {
      launch_ctc_gru16x(din, (const __half*)in, w.wih16x_pk[l], w.whh16x_pk[l], w.bih[l], w.bhh[l], f.batch, f.T, (__half*)y, f.st);
    }, f.timed);
  wk_status s = timed(c, WK_CTC_STAGE_PROJ0 + 2 * l, f.st, [&]() -> wk_status {
    return c->f16 ? ctc_gemm_nt(f.st, f.rows, 6 * H, din, in, w.wih16[l], gi, true, true)   // fp16 gates
                  : ctc_gemm_nt(f.st, f.rows, 6 * H, din, in, w.wih[l], gi, false);
  }, f.timed);
  if (s != WK_OK) return s;
  return timed(c, WK_CTC_STAGE_GRU0 + 2 * l, f.st, [&] {
    launch_ctc_gru(c->f16, gi, c->f16 ? (void*)w.whh16_pk[l] : (void*)w.whh_pk[l], w.bih[l], w.bhh[l], f.batch, f.T, y, f.st);
  }, f.timed);
}

wk_status stage_out32(const Fwd& f, const float* y, float* logits, float* d_log_probs, int* best) {
  const CtcWeights& w = f.c->w;
  const int V = f.c->cfg.vocab;
  return timed(f.c, WK_CTC_STAGE_OUTPUT, f.st, [&]() -> wk_status {
    if (!d_log_probs)   // decode only: the argmax inside the GEMM, no [rows][V] logits
      return ctc_gemm_argmax(f.st, f.rows, V, 2 * kH, y, w.out_w, w.out_b, reinterpret_cast<unsigned long long*>(logits), best);
    const wk_status g = ctc_gemm_nt(f.st, f.rows, V, 2 * kH, y, w.out_w, logits, false);
    if (g != WK_OK) return g;
    launch_ctc_argmax(false, logits, w.out_b, f.rows, V, d_log_probs, best, 0, 0, f.st);
    return WK_OK;
  }, f.timed);
}

}  // namespace wk

extern "C" {

int64_t wk_ctc_num_weights(const wk_ctc_config* cfg) { return cfg ? ctc_blob(cfg->vocab, cfg->hidden).off[kCtcSegs] : -1; }

wk_status wk_ctc_create(const wk_ctc_config* cfg, const float* w, wk_ctc** out) {
  if (!cfg || !w || !out) return invalid("wk_ctc_create: null argument");
  if (cfg->hidden != kH || cfg->layers != 2 || cfg->n_mels != kMels || cfg->vocab < 2)
    return fail(WK_ERR_UNSUPPORTED, "wk_ctc_create: this build implements hidden=128, layers=2, n_mels=80, vocab>=2");
  if (cfg->precision != 0 && cfg->precision != 1) return invalid("wk_ctc_create: precision must be 0 (fp32) or 1 (fp16)");
  *out = nullptr;
  return on_device(cfg->device, [&]() -> wk_status {
    // (the scalar members start at zero; a failed create frees it here, device current)
    std::unique_ptr<wk_ctc> c(new (std::nothrow) wk_ctc());
    if (!c) return WK_ERR_NO_MEMORY;
    c->cfg = *cfg;
    c->f16 = cfg->precision == 1;
    const char* gg = getenv("WAKEWORD_CTC_GEMM");
    c->gru_gemm = gg && gg[0] == '1';
    const char* mx = getenv("WAKEWORD_CTC_MIX");
    c->mix = mx ? (strcmp(mx, "out32") == 0 ? 1 : strcmp(mx, "out16") == 0 ? 2 : 0) : 0;
    const char* rs = getenv("WAKEWORD_CTC_RESCORE");
    c->rescore = !(rs && rs[0] == '0');
    hipDeviceProp_t prop;
    c->n_cu = hipGetDeviceProperties(&prop, cfg->device) == hipSuccess ? prop.multiProcessorCount : 256;
    const int H = kH, V = cfg->vocab;
    const CtcBlob blob = ctc_blob(V);
    const bool f16 = c->f16;
    CtcWeights& cw = c->w;
    // segment k of the blob to a buffer of its own
    auto up = [&](DevBuf<float>& buf, int k) { return buf.upload(w + blob.off[k], (size_t)(blob.off[k + 1] - blob.off[k])); };
    hipError_t e = up(cw.enc_w, kSegEncW);
    if (e == hipSuccess) e = up(cw.enc_b, kSegEncB);
    if (e == hipSuccess) e = up(cw.ln_g, kSegLnG);
    if (e == hipSuccess) e = up(cw.ln_b, kSegLnB);
    for (int l = 0; l < 2 && e == hipSuccess; ++l) {
      // the blob holds, per direction, W_ih, W_hh, b_ih, b_hh; the kernels take each tensor with both directions adjacent
      const int din = l == 0 ? H : 2 * H;
      std::vector<float> t[4];   // W_ih, W_hh, b_ih, b_hh
      for (int d = 0; d < 2; ++d)
        for (int k = 0; k < 4; ++k) t[k].insert(t[k].end(), w + blob.off[ctc_gru_seg(l, d, k)], w + blob.off[ctc_gru_seg(l, d, k) + 1]);
      const std::vector<float>&wih = t[kGruWih], &whh = t[kGruWhh];
      e = cw.wih[l].upload(wih);
      if (e == hipSuccess && f16) e = upload_f16(cw.wih16[l], wih);
      if (e == hipSuccess && f16) e = upload_f16(cw.wih16x_pk[l], ctc_pack_frag32(wih.data(), din, kCtcGateScale));
      if (e == hipSuccess && f16) e = upload_f16(cw.whh16x_pk[l], ctc_pack_frag32(whh.data(), H, kCtcGateScale));
      if (e == hipSuccess) e = cw.bih[l].upload(t[kGruBih]);
      if (e == hipSuccess) e = cw.bhh[l].upload(t[kGruBhh]);
      if (e == hipSuccess) e = cw.whh_pk[l].upload(ctc_pack_whh(whh.data()));
      if (e == hipSuccess && !f16) e = cw.whh[l].upload(whh);
      if (e == hipSuccess && !f16) e = cw.whht_pk[l].upload(ctc_pack_whht(whh.data()));
      if (e == hipSuccess && f16) e = upload_f16(cw.whh16_pk[l], ctc_pack_whh16(whh.data()));
    }
    if (e == hipSuccess) e = up(cw.out_w, kSegOutW);
    if (e == hipSuccess && (f16 || c->mix == 2)) e = upload_f16(cw.out_w16, w + blob.off[kSegOutW], (size_t)V * 2 * H);
    if (e == hipSuccess) e = up(cw.out_b, kSegOutB);
    if (e == hipSuccess) e = cw.zero_b.upload(std::vector<float>((size_t)V, 0.0f));
    CtcLogmelTables lm;
    if (e == hipSuccess && !ctc_logmel_tables(&lm)) e = hipErrorInvalidValue;
    if (e == hipSuccess) e = cw.fft_win.upload(lm.win);
    if (e == hipSuccess) e = cw.fft_tw.upload(lm.tw);
    if (e == hipSuccess) e = cw.melw.upload(lm.melw);
    if (e == hipSuccess) e = cw.melws.upload(lm.melws);
    if (e != hipSuccess) return ctc_alloc_failed(e, "wk_ctc_create");
    *out = c.release();
    return WK_OK;
  });
}

wk_status wk_ctc_destroy(wk_ctc* c) {
  if (!c) return WK_OK;
  return on_device(c->cfg.device, [&]() -> wk_status {
    (void)hipDeviceSynchronize();
    (void)fold_events(c);   // (destroys the stage events still recorded)
    delete c;
    return WK_OK;
  });
}

namespace {
// wk_ctc_features; with `part` (wk_ctc_transcribe, T >= 6) the features stay
// raw and the z-score's statistics go to zs instead of being applied in place.
wk_status ctc_features(wk_ctc* c, const float* d_audio, int64_t batch, int32_t n_valid, int32_t n_samples,
                       int64_t stride, float* d_feats, void* stream, float2* part, float2* zs) {
  if (!c || batch < 0 || (batch > 0 && (!d_audio || !d_feats)) || n_samples < kNfft / 2 + 1 || n_valid < 0 ||
      (batch > 1 && stride < (n_valid < n_samples ? n_valid : n_samples)))
    return invalid("wk_ctc_features: bad arguments (n_samples must exceed 200 for the reflect pad)");
  if (batch == 0) return WK_OK;
  const int T = 1 + n_samples / kHop;
  const int64_t rows = batch * (int64_t)T;
  if (rows > INT32_MAX) return invalid("wk_ctc_features: batch x frames exceeds 2^31 rows");
  return on_device(c->cfg.device, [&]() -> wk_status {
    hipStream_t st = (hipStream_t)stream;
    const CtcWeights& w = c->w;
    const int nv = n_valid < n_samples ? n_valid : n_samples;
    // n_valid == 0: every sample is padding; the kernel's (masked) loads then
    // read a device table instead of a possibly empty audio buffer
    const float* au = nv > 0 ? d_audio : w.fft_win;
    const CtcLogmelLayout lay = ctc_logmel_layout(c->n_cu, rows, T);
    if (part && (size_t)lay.slots > c->tr.slots) return invalid("wk_ctc_transcribe: statistics workspace too small");
    wk_status s = timed(c, WK_CTC_STAGE_LOGMEL, st, [&] {
      launch_ctc_logmel(au, nv > 0 ? stride : (int64_t)0, nv, n_samples, T, rows, w.fft_win, w.fft_tw, w.melw, w.melws, d_feats, lay,
                        part, st);
    });
    if (s == WK_OK) s = timed(c, WK_CTC_STAGE_ZSCORE, st, [&] { launch_ctc_zscore(d_feats, batch, T, lay, part, zs, st); });
    return s == WK_OK ? ctc_launched("wk_ctc_features") : s;
  });
}

// fp16 output layer + argmax fused on y [rows][256] fp16 (fp16 logits are
// written only for log_softmax), then the near-tie rows decided again in fp32
// (tokens independent of log-probs: both variants).  time_major: y's rows are
// t B + b (the fp16 path); batch-major is the out16 attribution path on an
// fp32 handle, which keeps the unfolded kernel its parity numbers were taken with.
wk_status stage_out16(const Fwd& f, const __half* y, float* d_log_probs, bool time_major) {
  wk_ctc* c = f.c;
  const CtcWeights& w = c->w;
  CtcInferWs& ws = c->ws;
  const int V = c->cfg.vocab;
  return timed(c, WK_CTC_STAGE_OUTPUT, f.st, [&] {
    launch_ctc_out16(y, w.out_w16, w.out_b, f.rows, V, d_log_probs ? ws.logits16 : nullptr, ws.best, ws.best2, c->f16, f.st);
    if (d_log_probs)   // bias already in
      launch_ctc_argmax(true, ws.logits16, w.zero_b, f.rows, V, d_log_probs, nullptr, time_major ? (int)f.batch : 0, f.T, f.st);
    if (ctc_out_keyed(V) && c->rescore) launch_ctc_rescore(y, w.out_w, w.out_b, f.rows, ws.best, ws.best2, f.st);
  });
}

wk_status stage_decode(const Fwd& f, int32_t* d_tokens, int32_t* d_lengths, bool time_major) {
  return timed(f.c, WK_CTC_STAGE_DECODE, f.st,
               [&] { launch_ctc_greedy(f.c->ws.best, f.batch, f.T, d_tokens, d_lengths, time_major ? 1 : 0, f.st); });
}

// wk_ctc_forward; with zs (wk_ctc_transcribe, fp16 mode) the encoder z-scores
// the raw feature rows as it loads them.
wk_status ctc_forward(wk_ctc* c, const float* d_feats, int64_t batch, int32_t T, float* d_log_probs, int32_t* d_tokens,
                      int32_t* d_lengths, void* stream, const float2* zs) {
  if (!c || batch < 0 || T < 1 || (batch > 0 && (!d_feats || !d_tokens || !d_lengths)))
    return invalid("wk_ctc_forward: bad arguments");
  if (batch == 0) return WK_OK;
  const int64_t rows = batch * (int64_t)T;
  if (rows > INT32_MAX) return invalid("wk_ctc_forward: batch x frames exceeds 2^31 rows");
  const bool f16 = c->f16;
  // fp16 encoder: 32-bit buffer offsets over the [rows][80] fp32 features
  if (f16 && rows * kMels * 4 >= (int64_t)0x7FFFFF00) return invalid("wk_ctc_forward: fp16 mode takes < 6.7 M rows per call");
  return on_device(c->cfg.device, [&]() -> wk_status {
    hipStream_t st = (hipStream_t)stream;
    CtcInferWs& ws = c->ws;
    if ((size_t)rows > ws.rows)   // grows on first use of a larger batch x T (then reused)
      if (const wk_status s = ctc_grow(st, ws_table(c, (size_t)rows), {{&ws.rows, (size_t)rows}}, "wk_ctc_forward workspace")) return s;
    ws.last_batch = batch;
    ws.last_T = T;
    const Fwd f{c, st, batch, rows, T, true};
    // the handle's precision picks the activation tensors (fp16: time-major rows)
    auto act = [&](const DevBuf<__half>& h, const DevBuf<float>& s) { return f16 ? (void*)h.get() : (void*)s.get(); };
    wk_status s = stage_encoder(f, d_feats, zs, act(ws.x0h, ws.x0));
    if (s == WK_OK) s = stage_gru(f, 0, act(ws.x0h, ws.x0), ws.gi, act(ws.y0h, ws.y0));
    if (s == WK_OK) s = stage_gru(f, 1, act(ws.y0h, ws.y0), ws.gi, act(ws.y1h, ws.y1));
    if (s != WK_OK) return s;
    if (f16 && c->mix == 1) {   // attribution: the fp16 path's y1, widened, through the fp32 output layer
      if (d_log_probs) return fail(WK_ERR_UNSUPPORTED, "WAKEWORD_CTC_MIX=out32 decodes only (no log-probs)");
      launch_ctc_convert(ws.y1h, ws.y1, rows * 2 * kH, c->n_cu, st);
      s = stage_out32(f, ws.y1, ws.logits, nullptr, ws.best);
    } else if (!f16 && c->mix == 2) {   // attribution: the fp32 path's y1, rounded, through the fp16 output kernel
      if (d_log_probs) return fail(WK_ERR_UNSUPPORTED, "WAKEWORD_CTC_MIX=out16 decodes only (no log-probs)");
      launch_ctc_convert(ws.y1, ws.y1h, rows * 2 * kH, c->n_cu, st);
      s = stage_out16(f, ws.y1h, nullptr, false);
    } else {
      s = f16 ? stage_out16(f, ws.y1h, d_log_probs, true) : stage_out32(f, ws.y1, ws.logits, d_log_probs, ws.best);
    }
    if (s == WK_OK) s = stage_decode(f, d_tokens, d_lengths, f16);   // (best[] follows the rows: time-major in fp16 mode)
    return s == WK_OK ? ctc_launched("wk_ctc_forward") : s;
  });
}
}  // namespace

wk_status wk_ctc_features(wk_ctc* c, const float* d_audio, int64_t batch, int32_t n_valid, int32_t n_samples,
                          int64_t stride, float* d_feats, void* stream) {
  return ctc_features(c, d_audio, batch, n_valid, n_samples, stride, d_feats, stream, nullptr, nullptr);
}

wk_status wk_ctc_forward(wk_ctc* c, const float* d_feats, int64_t batch, int32_t T, float* d_log_probs,
                         int32_t* d_tokens, int32_t* d_lengths, void* stream) {
  return ctc_forward(c, d_feats, batch, T, d_log_probs, d_tokens, d_lengths, stream, nullptr);
}

wk_status wk_ctc_transcribe(wk_ctc* c, const float* d_audio, int64_t batch, int32_t n_valid, int32_t n_samples,
                            int64_t stride, int32_t* d_tokens, int32_t* d_lengths, void* stream) {
  if (!c || batch < 0 || n_samples < kNfft / 2 + 1 || (batch > 0 && (!d_tokens || !d_lengths)))
    return invalid("wk_ctc_transcribe: bad arguments");
  if (batch == 0) return WK_OK;
  const int T = 1 + n_samples / kHop;
  const int64_t rows = batch * (int64_t)T;
  if (rows > INT32_MAX) return invalid("wk_ctc_transcribe: batch x frames exceeds 2^31 rows");
  const bool fused = c->f16 && T >= 6;   // (a log-mel pass of 6 rows then spans at most two utterances)
  return on_device(c->cfg.device, [&]() -> wk_status {
    CtcTranscribeWs& tr = c->tr;
    const size_t slots = (size_t)ctc_logmel_layout(c->n_cu, rows, T).slots;
    tr.last_T = 0;   // (set once every stage is enqueued)
    if ((size_t)rows > tr.rows || (size_t)batch > tr.batch || slots > tr.slots)   // grows, then reused
      if (const wk_status s = ctc_grow((hipStream_t)stream,
                                       {{&tr.feats, sizeof(float) * kMels * (size_t)rows},
                                        {&tr.part, sizeof(float2) * slots},
                                        {&tr.zs, sizeof(float2) * (size_t)batch}},
                                       {{&tr.rows, (size_t)rows}, {&tr.batch, (size_t)batch}, {&tr.slots, slots}},
                                       "wk_ctc_transcribe workspace"))
        return s;
    wk_status s = ctc_features(c, d_audio, batch, n_valid, n_samples, stride, tr.feats, stream, fused ? tr.part.get() : nullptr,
                               fused ? tr.zs.get() : nullptr);
    if (s != WK_OK) return s;
    s = ctc_forward(c, tr.feats, batch, T, nullptr, d_tokens, d_lengths, stream, fused ? tr.zs.get() : nullptr);
    if (s != WK_OK) return s;
    tr.last_batch = batch;
    tr.last_T = T;
    tr.last_fused = fused;
    return WK_OK;
  });
}

wk_status wk_ctc_transcribe_stats(wk_ctc* c, int64_t batch, int32_t T, float* d_raw, float* d_zs, void* stream) {
  if (!c || batch < 0 || T < 1) return invalid("wk_ctc_transcribe_stats: bad arguments");
  const CtcTranscribeWs& tr = c->tr;
  if (tr.last_T == 0) return invalid("wk_ctc_transcribe_stats: no wk_ctc_transcribe on this handle yet");
  if (!tr.last_fused || batch != tr.last_batch || T != tr.last_T)
    return invalid(("wk_ctc_transcribe_stats: the handle's last wk_ctc_transcribe had batch " + std::to_string(tr.last_batch) +
                    ", T " + std::to_string(tr.last_T) +
                    (tr.last_fused ? " (fused)" : c->f16 ? ", not fused (T < 6)" : ", not fused (fp32 handle)") +
                    "; asked for batch " + std::to_string(batch) + ", T " + std::to_string(T))
                       .c_str());
  return on_device(c->cfg.device, [&]() -> wk_status {
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)batch * (size_t)T;
    hipError_t e = hipSuccess;
    if (d_raw) e = hipMemcpyAsync(d_raw, tr.feats.get(), sizeof(float) * rows * kMels, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && d_zs) e = hipMemcpyAsync(d_zs, tr.zs.get(), sizeof(float2) * (size_t)batch, hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_transcribe_stats");
  });
}

wk_status wk_ctc_profile(wk_ctc* c, int32_t enable) {
  if (!c) return invalid("wk_ctc_profile: null handle");
  return on_device(c->cfg.device, [&]() -> wk_status {
    const hipError_t e = fold_events(c);
    for (int i = 0; i < WK_CTC_N_STAGES; ++i) {
      c->prof.ms[i] = 0.0;
      c->prof.n[i] = 0;
    }
    c->prof.on = enable ? 1 : 0;
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_profile");
  });
}

wk_status wk_ctc_stage_times(wk_ctc* c, double* ms_sum, int64_t* counts) {
  if (!c || !ms_sum || !counts) return invalid("wk_ctc_stage_times: null argument");
  return on_device(c->cfg.device, [&]() -> wk_status {
    const hipError_t e = fold_events(c);
    for (int i = 0; i < WK_CTC_N_STAGES; ++i) {
      ms_sum[i] = c->prof.ms[i];
      counts[i] = c->prof.n[i];
    }
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_stage_times");
  });
}

wk_status wk_ctc_frame_argmax(wk_ctc* c, int64_t batch, int32_t T, int32_t* d_pred, void* stream) {
  if (!c || batch < 0 || T < 1 || (batch > 0 && !d_pred)) return invalid("wk_ctc_frame_argmax: bad arguments");
  if (batch == 0) return WK_OK;
  if (batch != c->ws.last_batch || T != c->ws.last_T || !c->ws.best)
    return invalid("wk_ctc_frame_argmax: batch and T must be those of the handle's last wk_ctc_forward");
  return on_device(c->cfg.device, [&]() -> wk_status {
    launch_ctc_pred(c->ws.best, batch, T, c->f16 ? 1 : 0, d_pred, (hipStream_t)stream);
    return ctc_launched("wk_ctc_frame_argmax");
  });
}

}  // extern "C"
