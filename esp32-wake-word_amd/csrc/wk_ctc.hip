// wk_ctc.hip -- the GRU-CTC head (ml_models/ctc.py) on gfx950:
// the wk_ctc_* C ABI.
//
//   audio -> log-mel 80 + global z-score (ctc.py:82-107)          wk_ctc_logmel.hip
//         -> Linear 80->128 + LayerNorm + ReLU (ctc.py:125-130)   wk_ctc_dense.hip
//         -> 2-layer bidirectional GRU, H = 128 (ctc.py:133-140)  wk_ctc_gru.hip
//         -> Linear 256->V, log_softmax (ctc.py:143-152)          wk_ctc_out.hip (fp16), wk_ctc_dense.hip (fp32 GEMM)
//         -> greedy CTC decode (ctc.py:453-471)                   wk_ctc_out.hip
//
// This unit holds no kernel: the handle (weights uploaded in each kernel's
// layout by its unit's packer), the workspaces, stage timing, and the stage
// sequence of wk_ctc_features / wk_ctc_forward / wk_ctc_transcribe, which
// call the launchers declared in wk_ctc_dev.h; and, for training, the fp32
// forward that keeps its activations (wk_ctc_forward_train), the entry to
// the backward pass of wk_ctc_bwd.hip (wk_ctc_backward), train-mode dropout over
// wk_ctc_dropout.hip (wk_ctc_forward_train_dropout, wk_ctc_dropout_masks), and the optimiser's
// entry points over wk_ctc_optim.hip (wk_ctc_adam_step, wk_ctc_weights,
// wk_ctc_set_weights, wk_ctc_optim_state, wk_ctc_set_optim_state).
#include <stdlib.h>
#include <string.h>

#include <array>
#include <cmath>
#include <memory>
#include <new>
#include <string>
#include <type_traits>

#include "wk_ctc_dev.h"
#include "wk_devmem.h"

using namespace wk;

struct wk_ctc {
  wk_ctc_config cfg;
  int n_cu;
  bool f16;             // precision 1: GEMM operands in fp16 (fp32 accumulate); recurrence fp32
  // weights (device)
  DevBuf<float> enc_w, enc_b, ln_g, ln_b;
  DevBuf<float> wih[2];        // per layer: [768][Din] (fwd rows then reverse rows)
  DevBuf<float> bih[2];        // per layer: [768]
  DevBuf<float> bhh[2];        // per layer: [768]
  DevBuf<float> whh_pk[2];     // per layer: [2 dir][24 tiles][32 k-steps][64 lanes]
  DevBuf<float> out_w, out_b;  // [V][256], [V]
  DevBuf<float> zero_b;        // [V] zeros: the log_softmax kernel's bias in fp16 mode (the logits carry theirs)
  DevBuf<__half> wih16[2];     // fp16 copies (precision 1)
  DevBuf<__half> whh16_pk[2];  // per layer: [2 dir][24 tiles][8 k-steps][64 lanes][4]
  DevBuf<__half> whh16x_pk[2]; // per layer: [2 dir][3 gates][8 waves][4 k-steps][64 lanes][8] (W_hh as 16x16x32 fragments, gate-scaled)
  DevBuf<__half> wih16x_pk[2]; // per layer: [2 dir][3 gates][8 waves][din/32 k-steps][64 lanes][8] (fused-projection GRU, gate-scaled)
  bool gru_gemm;        // fp16 mode: input projections as a separate GEMM (WAKEWORD_CTC_GEMM=1; A/B and checks)
  // Decision-parity attribution (WAKEWORD_CTC_MIX): 1 = "out32", the fp16
  // path up to the last GRU layer, then the output layer in fp32 (y1 widened,
  // fp32 W); 2 = "out16", the fp32 path with the fp16 output kernel (y1 and W
  // rounded to fp16).  0 (default) = the precision's own output layer.
  int mix;
  int rescore;          // fp16 output layer: near-tie rows re-decided in fp32 (default; WAKEWORD_CTC_RESCORE=0 off, A/B)
  DevBuf<__half> out_w16;
  DevBuf<float> fft_win;       // [400] periodic Hann
  DevBuf<float> fft_tw;        // [20 k1][20 n2] W400^(n2 k1), complex
  DevBuf<float> melw;          // ctc_logmel_fft2_kernel: per-lane padded mel weights x 1/4, [64][kMelW1] then [64][kMelW2]
  DevBuf<int> melws;           // their window start bins, [64] then [64]
  // workspaces (grown on demand)
  size_t ws_rows;
  DevBuf<float> x0, gi, y0, y1, logits;
  DevBuf<__half> x0h, y0h, y1h, logits16;
  DevBuf<int> best;
  DevBuf<int> best2;           // fp16 mode: the runner-up column of near-tie rows (else -1), for ctc_rescore_kernel
  DevBuf<float> tr_feats;      // wk_ctc_transcribe: [rows][80] features (raw in fp16 mode), pass partials, per-utterance z-score
  DevBuf<float2> tr_part;      // [tr_slots] per-wave log-mel statistics (ctc_logmel_fft2_kernel<true>)
  DevBuf<float2> tr_zs;
  size_t tr_rows, tr_batch, tr_slots;
  int64_t tr_last_batch;   // geometry and path of the last wk_ctc_transcribe (wk_ctc_transcribe_stats); T 0: none yet
  int32_t tr_last_T;
  bool tr_last_fused;
  int64_t last_batch;   // geometry of the last wk_ctc_forward (wk_ctc_frame_argmax)
  int32_t last_T;
  // training (fp32 handles; wk_ctc_forward_train / wk_ctc_backward): W_hh as the backward's GEMM operand
  // ([2 dir][384][128]) and as ctc_gru_bptt_kernel's W_hh^T fragments, and a workspace apart from the
  // inference one (grown on demand): what the forward saves, then the backward's scratch
  DevBuf<float> whh[2], whht_pk[2];
  size_t tn_rows;
  DevBuf<float> tn_feats, tn_x0, tn_gi[2], tn_y[2], tn_logits;
  DevBuf<float> tn_hprev, tn_dya, tn_dyb, tn_gh, tn_dai, tn_dah, tn_coef, tn_pre, tn_t0, tn_t1, tn_part;
  int64_t tn_batch;     // geometry of the last wk_ctc_forward_train (wk_ctc_backward)
  int32_t tn_T;
  // dropout of the last training forward (all off after a plain wk_ctc_forward_train), and site 1's output: the dropped
  // copy of tn_y[0], tn_rows rows, allocated by the first forward with p_gru > 0
  CtcDrop tn_drop;
  DevBuf<float> tn_y0d;
  // optimiser (fp32 handles; wk_ctc_adam_step): Adam's moments in blob order and the norm computed when the caller
  // passes none, allocated and zeroed on first use; the step count is host state
  DevBuf<float> opt_m, opt_v, opt_norm;
  bool opt_ready;
  int64_t opt_step;
  // stage timing (wk_ctc_profile): events recorded around each stage on the
  // call's stream, folded into per-stage sums when read or when the ring fills
  int prof;
  struct { int stage; hipEvent_t a, b; } ev[64];
  int n_ev;
  double stage_ms[WK_CTC_N_STAGES];
  int64_t stage_n[WK_CTC_N_STAGES];
};

namespace {

// wk_ctc_forward's workspace: which buffers this handle's path uses (fp32:
// x0, gi, y0, y1, logits; fp16: the half tensors, gi only for the GEMM
// projections; the attribution mixes add the other precision's y1 / logits).
// It sizes and regrows them; the owners in the handle are what frees them.
struct WsBuf {
  DevMem* buf;
  size_t row_bytes;
  bool needed;
};
std::array<WsBuf, 11> ws_table(wk_ctc* c) {
  const bool f16 = c->f16;
  const size_t H = kH, V = (size_t)c->cfg.vocab;
  return {{
      {&c->x0, sizeof(float) * H, !f16},
      {&c->gi, sizeof(float) * 6 * H, !f16 || c->gru_gemm},
      {&c->y0, sizeof(float) * 2 * H, !f16},
      {&c->y1, sizeof(float) * 2 * H, !f16 || c->mix == 1},
      {&c->logits, sizeof(float) * V, !f16 || c->mix == 1},
      {&c->best, sizeof(int), true},
      {&c->best2, sizeof(int), true},
      {&c->x0h, sizeof(__half) * H, f16},
      {&c->y0h, sizeof(__half) * 2 * H, f16},
      {&c->y1h, sizeof(__half) * 2 * H, f16 || c->mix == 2},
      {&c->logits16, sizeof(__half) * V, f16},
  }};
}

// Drops the old buffers first (two passes: the peak is the larger set alone);
// nothing stays allocated after a failure.
hipError_t alloc_ws(wk_ctc* c, size_t rows) {
  c->ws_rows = 0;
  for (const WsBuf& b : ws_table(c)) b.buf->reset();
  hipError_t e = hipSuccess;
  for (const WsBuf& b : ws_table(c))
    if (b.needed && e == hipSuccess) e = b.buf->alloc_bytes(b.row_bytes * rows);
  if (e == hipSuccess) {
    c->ws_rows = rows;
  } else {
    for (const WsBuf& b : ws_table(c)) b.buf->reset();
  }
  return e;
}

// The training workspace, sized like alloc_ws: rows = batch x T, floats per row.
std::array<WsBuf, 18> tn_table(wk_ctc* c) {
  const size_t F = sizeof(float), H = kH;
  return {{
      {&c->tn_feats, F * kMels, true},   {&c->tn_x0, F * H, true},        {&c->tn_gi[0], F * 6 * H, true},
      {&c->tn_gi[1], F * 6 * H, true},   {&c->tn_y[0], F * 2 * H, true},  {&c->tn_y[1], F * 2 * H, true},
      {&c->tn_logits, F * (size_t)c->cfg.vocab, true},                    {&c->tn_hprev, F * 2 * H, true},
      {&c->tn_dya, F * 2 * H, true},     {&c->tn_dyb, F * 2 * H, true},   {&c->tn_gh, F * 6 * H, true},
      {&c->tn_dai, F * 6 * H, true},     {&c->tn_dah, F * 6 * H, true},   {&c->tn_coef, F * 10 * H, true},
      {&c->tn_pre, F * H, true},         {&c->tn_t0, F * H, true},        {&c->tn_t1, F * H, true},
      {&c->tn_part, 0, true},            // (the split-K partials: sized by ctc_bwd_part_floats)
  }};
}

hipError_t alloc_tn(wk_ctc* c, size_t rows) {
  c->tn_rows = 0;
  c->tn_batch = 0;
  c->tn_y0d.reset();   // (sized with the rest: the next forward that needs it allocates it again)
  for (const WsBuf& b : tn_table(c)) b.buf->reset();
  hipError_t e = hipSuccess;
  for (const WsBuf& b : tn_table(c))
    if (e == hipSuccess)
      e = b.buf->alloc_bytes(b.row_bytes ? b.row_bytes * rows : sizeof(float) * ctc_bwd_part_floats(c->cfg.vocab, (int64_t)rows));
  if (e == hipSuccess) {
    c->tn_rows = rows;
  } else {
    for (const WsBuf& b : tn_table(c)) b.buf->reset();
  }
  return e;
}

// Fold the recorded stage events into the per-stage sums (synchronises on them).
hipError_t fold_events(wk_ctc* c) {
  hipError_t err = hipSuccess;
  for (int i = 0; i < c->n_ev; ++i) {
    float ms = 0.0f;
    hipError_t e = hipEventSynchronize(c->ev[i].b);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev[i].a, c->ev[i].b);
    if (e == hipSuccess) {
      c->stage_ms[c->ev[i].stage] += ms;
      c->stage_n[c->ev[i].stage] += 1;
    } else if (err == hipSuccess) {
      err = e;
    }
    (void)hipEventDestroy(c->ev[i].a);
    (void)hipEventDestroy(c->ev[i].b);
  }
  c->n_ev = 0;
  return err;
}

// Stage bracket: records an event pair around `body` when profiling is on.
// body returns a wk_status, or nothing when it only enqueues kernels.
template <typename F>
wk_status timed(wk_ctc* c, int stage, hipStream_t st, F body) {
  auto launch = [&]() -> wk_status {
    if constexpr (std::is_void<decltype(body())>::value) {
      body();
      return WK_OK;
    } else {
      return body();
    }
  };
  if (!c->prof) return launch();
  if (c->n_ev == 64 && fold_events(c) != hipSuccess) return fail(WK_ERR_HIP, "wk_ctc stage timing");
  auto& e = c->ev[c->n_ev];
  if (hipEventCreate(&e.a) != hipSuccess) return fail(WK_ERR_HIP, "hipEventCreate");
  if (hipEventCreate(&e.b) != hipSuccess) {
    (void)hipEventDestroy(e.a);
    return fail(WK_ERR_HIP, "hipEventCreate");
  }
  e.stage = stage;
  ++c->n_ev;
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

extern "C" {

int64_t wk_ctc_num_weights(const wk_ctc_config* cfg) {
  if (!cfg) return -1;
  const int64_t H = cfg->hidden, V = cfg->vocab;
  int64_t n = H * kMels + 3 * H;
  for (int l = 0; l < 2; ++l) n += 2 * (3 * H * (l == 0 ? H : 2 * H) + 3 * H * H + 6 * H);
  return n + V * 2 * H + V;
}

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
    const float* p = w;
    auto take = [&](size_t n) { const float* q = p; p += n; return q; };
    hipError_t e = c->enc_w.upload(take((size_t)H * kMels), (size_t)H * kMels);
    if (e == hipSuccess) e = c->enc_b.upload(take(H), H);
    if (e == hipSuccess) e = c->ln_g.upload(take(H), H);
    if (e == hipSuccess) e = c->ln_b.upload(take(H), H);
    for (int l = 0; l < 2 && e == hipSuccess; ++l) {
      // the blob holds, per direction, W_ih, W_hh, b_ih, b_hh; the kernels take each tensor with both directions adjacent
      const int din = l == 0 ? H : 2 * H;
      std::vector<float> wih(6 * (size_t)H * din), whh(6 * (size_t)H * H), bih(6 * H), bhh(6 * H);
      for (int d = 0; d < 2; ++d) {
        memcpy(&wih[(size_t)d * 3 * H * din], take(3 * (size_t)H * din), sizeof(float) * 3 * H * din);
        memcpy(&whh[(size_t)d * 3 * H * H], take(3 * (size_t)H * H), sizeof(float) * 3 * H * H);
        memcpy(&bih[d * 3 * H], take(3 * H), sizeof(float) * 3 * H);
        memcpy(&bhh[d * 3 * H], take(3 * H), sizeof(float) * 3 * H);
      }
      e = c->wih[l].upload(wih);
      if (e == hipSuccess && c->f16) e = upload_f16(c->wih16[l], wih);
      if (e == hipSuccess && c->f16) e = upload_f16(c->wih16x_pk[l], ctc_pack_frag32(wih.data(), din, kCtcGateScale));
      if (e == hipSuccess && c->f16) e = upload_f16(c->whh16x_pk[l], ctc_pack_frag32(whh.data(), H, kCtcGateScale));
      if (e == hipSuccess) e = c->bih[l].upload(bih);
      if (e == hipSuccess) e = c->bhh[l].upload(bhh);
      if (e == hipSuccess) e = c->whh_pk[l].upload(ctc_pack_whh(whh.data()));
      if (e == hipSuccess && !c->f16) e = c->whh[l].upload(whh);
      if (e == hipSuccess && !c->f16) e = c->whht_pk[l].upload(ctc_pack_whht(whh.data()));
      if (e == hipSuccess && c->f16) e = upload_f16(c->whh16_pk[l], ctc_pack_whh16(whh.data()));
    }
    const float* ow = take((size_t)V * 2 * H);
    if (e == hipSuccess) e = c->out_w.upload(ow, (size_t)V * 2 * H);
    if (e == hipSuccess && (c->f16 || c->mix == 2)) e = upload_f16(c->out_w16, ow, (size_t)V * 2 * H);
    if (e == hipSuccess) e = c->out_b.upload(take(V), V);
    if (e == hipSuccess) e = c->zero_b.upload(std::vector<float>((size_t)V, 0.0f));
    CtcLogmelTables lm;
    if (e == hipSuccess && !ctc_logmel_tables(&lm)) e = hipErrorInvalidValue;
    if (e == hipSuccess) e = c->fft_win.upload(lm.win);
    if (e == hipSuccess) e = c->fft_tw.upload(lm.tw);
    if (e == hipSuccess) e = c->melw.upload(lm.melw);
    if (e == hipSuccess) e = c->melws.upload(lm.melws);
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? WK_ERR_NO_MEMORY : hip_fail(e, "wk_ctc_create");
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
    const int nv = n_valid < n_samples ? n_valid : n_samples;
    // n_valid == 0: every sample is padding; the kernel's (masked) loads then
    // read a device table instead of a possibly empty audio buffer
    const float* au = nv > 0 ? d_audio : c->fft_win;
    const CtcLogmelLayout lay = ctc_logmel_layout(c->n_cu, rows, T);
    if (part && (size_t)lay.slots > c->tr_slots) return invalid("wk_ctc_transcribe: statistics workspace too small");
    wk_status s = timed(c, WK_CTC_STAGE_LOGMEL, st, [&] {
      launch_ctc_logmel(au, nv > 0 ? stride : (int64_t)0, nv, n_samples, T, rows, c->fft_win, c->fft_tw, c->melw, c->melws,
                        d_feats, lay, part, st);
    });
    if (s == WK_OK) s = timed(c, WK_CTC_STAGE_ZSCORE, st, [&] { launch_ctc_zscore(d_feats, batch, T, lay, part, zs, st); });
    if (s != WK_OK) return s;
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_features launch");
  });
}

// One wk_ctc_forward call, as its stages see it.  Each stage is bracketed once
// for wk_ctc_profile; launch errors surface in ctc_forward's closing check.
struct Fwd {
  wk_ctc* c;
  hipStream_t st;
  int64_t batch, rows;
  int T;
};

// features [rows][80] -> x0 (fp32, batch-major rows) or x0h (fp16: time-major rows from here on)
wk_status stage_encoder(const Fwd& f, const float* d_feats, const float2* zs) {
  wk_ctc* c = f.c;
  return timed(c, WK_CTC_STAGE_ENCODER, f.st, [&] {
    launch_ctc_encoder(c->f16, d_feats, (int)f.batch, f.T, c->enc_w, c->enc_b, c->ln_g, c->ln_b, zs,
                       c->f16 ? (void*)c->x0h : (void*)c->x0, c->n_cu, f.st);
  });
}

// GRU layer l: x0 -> y0 -> y1 (the fp16 tensors in fp16 mode)
wk_status stage_gru(const Fwd& f, int l) {
  wk_ctc* c = f.c;
  const int H = kH, din = l == 0 ? H : 2 * H;
  const float* in = l == 0 ? c->x0 : c->y0;
  const __half* in16 = l == 0 ? c->x0h : c->y0h;
  float* y = l == 0 ? c->y0 : c->y1;
  __half* y16 = l == 0 ? c->y0h : c->y1h;
  if (c->f16 && !c->gru_gemm)   // projection fused into the recurrence: no GEMM, no gate-input tensor
    return timed(c, WK_CTC_STAGE_GRU0 + 2 * l, f.st, [&] {
      launch_ctc_gru16x(din, in16, c->wih16x_pk[l], c->whh16x_pk[l], c->bih[l], c->bhh[l], f.batch, f.T, y16, f.st);
    });
  wk_status s = timed(c, WK_CTC_STAGE_PROJ0 + 2 * l, f.st, [&]() -> wk_status {
    return c->f16 ? ctc_gemm_nt(f.st, f.rows, 6 * H, din, in16, c->wih16[l], c->gi, true, true)   // fp16 gates
                  : ctc_gemm_nt(f.st, f.rows, 6 * H, din, in, c->wih[l], c->gi, false);
  });
  if (s != WK_OK) return s;
  return timed(c, WK_CTC_STAGE_GRU0 + 2 * l, f.st, [&] {
    launch_ctc_gru(c->f16, c->gi, c->f16 ? (void*)c->whh16_pk[l] : (void*)c->whh_pk[l], c->bih[l], c->bhh[l], f.batch, f.T,
                   c->f16 ? (void*)y16 : (void*)y, f.st);
  });
}

// fp16 output layer + argmax fused on y [rows][256] fp16 (fp16 logits are
// written only for log_softmax), then the near-tie rows decided again in fp32
// (tokens independent of log-probs: both variants).  time_major: y's rows are
// t B + b (the fp16 path); batch-major is the out16 attribution path on an
// fp32 handle, which keeps the unfolded kernel its parity numbers were taken with.
wk_status stage_out16(const Fwd& f, const __half* y, float* d_log_probs, bool time_major) {
  wk_ctc* c = f.c;
  const int V = c->cfg.vocab;
  return timed(c, WK_CTC_STAGE_OUTPUT, f.st, [&] {
    launch_ctc_out16(y, c->out_w16, c->out_b, f.rows, V, d_log_probs ? c->logits16 : nullptr, c->best, c->best2, c->f16, f.st);
    if (d_log_probs)   // bias already in
      launch_ctc_argmax(true, c->logits16, c->zero_b, f.rows, V, d_log_probs, nullptr, time_major ? (int)f.batch : 0, f.T, f.st);
    if (ctc_out_keyed(V) && c->rescore) launch_ctc_rescore(y, c->out_w, c->out_b, f.rows, c->best, c->best2, f.st);
  });
}

// fp32 output layer on y [rows][256] fp32
wk_status stage_out32(const Fwd& f, const float* y, float* d_log_probs) {
  wk_ctc* c = f.c;
  const int V = c->cfg.vocab;
  return timed(c, WK_CTC_STAGE_OUTPUT, f.st, [&]() -> wk_status {
    if (!d_log_probs)   // decode only: the argmax inside the GEMM, no [rows][V] logits (c->logits: the keys)
      return ctc_gemm_argmax(f.st, f.rows, V, 2 * kH, y, c->out_w, c->out_b, reinterpret_cast<unsigned long long*>(c->logits.get()),
                             c->best);
    const wk_status g = ctc_gemm_nt(f.st, f.rows, V, 2 * kH, y, c->out_w, c->logits, false);
    if (g != WK_OK) return g;
    launch_ctc_argmax(false, c->logits, c->out_b, f.rows, V, d_log_probs, c->best, 0, 0, f.st);
    return WK_OK;
  });
}

wk_status stage_decode(const Fwd& f, int32_t* d_tokens, int32_t* d_lengths, bool time_major) {
  return timed(f.c, WK_CTC_STAGE_DECODE, f.st,
               [&] { launch_ctc_greedy(f.c->best, f.batch, f.T, d_tokens, d_lengths, time_major ? 1 : 0, f.st); });
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
    hipError_t e;
    if ((size_t)rows > c->ws_rows) {   // workspace grows on first use of a larger batch (then reused)
      if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "sync");
      if ((e = alloc_ws(c, (size_t)rows)) != hipSuccess)
        return e == hipErrorOutOfMemory ? WK_ERR_NO_MEMORY : hip_fail(e, "wk_ctc_forward workspace");
    }
    c->last_batch = batch;
    c->last_T = T;
    const Fwd f{c, st, batch, rows, T};
    wk_status s = stage_encoder(f, d_feats, zs);
    for (int l = 0; l < 2 && s == WK_OK; ++l) s = stage_gru(f, l);
    if (s != WK_OK) return s;
    if (f16 && c->mix == 1) {   // attribution: the fp16 path's y1, widened, through the fp32 output layer
      if (d_log_probs) return fail(WK_ERR_UNSUPPORTED, "WAKEWORD_CTC_MIX=out32 decodes only (no log-probs)");
      launch_ctc_convert(c->y1h, c->y1, rows * 2 * kH, c->n_cu, st);
      s = stage_out32(f, c->y1, nullptr);
    } else if (!f16 && c->mix == 2) {   // attribution: the fp32 path's y1, rounded, through the fp16 output kernel
      if (d_log_probs) return fail(WK_ERR_UNSUPPORTED, "WAKEWORD_CTC_MIX=out16 decodes only (no log-probs)");
      launch_ctc_convert(c->y1, c->y1h, rows * 2 * kH, c->n_cu, st);
      s = stage_out16(f, c->y1h, nullptr, false);
    } else {
      s = f16 ? stage_out16(f, c->y1h, d_log_probs, true) : stage_out32(f, c->y1, d_log_probs);
    }
    if (s == WK_OK) s = stage_decode(f, d_tokens, d_lengths, f16);   // (best[] follows the rows: time-major in fp16 mode)
    if (s != WK_OK) return s;
    e = hipGetLastError();
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_forward launch");
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
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    const int64_t slots = ctc_logmel_layout(c->n_cu, rows, T).slots;
    c->tr_last_T = 0;   // (set once every stage is enqueued)
    if ((size_t)rows > c->tr_rows || (size_t)batch > c->tr_batch || (size_t)slots > c->tr_slots) {   // grows, then reused
      if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "sync");
      c->tr_rows = c->tr_batch = c->tr_slots = 0;
      c->tr_feats.reset();   // (all three go before any grows: the peak is the larger set alone)
      c->tr_part.reset();
      c->tr_zs.reset();
      if ((e = c->tr_feats.alloc((size_t)rows * kMels)) != hipSuccess || (e = c->tr_part.alloc((size_t)slots)) != hipSuccess ||
          (e = c->tr_zs.alloc((size_t)batch)) != hipSuccess)
        return e == hipErrorOutOfMemory ? WK_ERR_NO_MEMORY : hip_fail(e, "wk_ctc_transcribe workspace");
      c->tr_rows = (size_t)rows;
      c->tr_batch = (size_t)batch;
      c->tr_slots = (size_t)slots;
    }
    wk_status s = ctc_features(c, d_audio, batch, n_valid, n_samples, stride, c->tr_feats, stream,
                               fused ? c->tr_part : nullptr, fused ? c->tr_zs : nullptr);
    if (s != WK_OK) return s;
    s = ctc_forward(c, c->tr_feats, batch, T, nullptr, d_tokens, d_lengths, stream, fused ? c->tr_zs : nullptr);
    if (s != WK_OK) return s;
    c->tr_last_batch = batch;
    c->tr_last_T = T;
    c->tr_last_fused = fused;
    return WK_OK;
  });
}

wk_status wk_ctc_transcribe_stats(wk_ctc* c, int64_t batch, int32_t T, float* d_raw, float* d_zs, void* stream) {
  if (!c || batch < 0 || T < 1) return invalid("wk_ctc_transcribe_stats: bad arguments");
  if (c->tr_last_T == 0) return invalid("wk_ctc_transcribe_stats: no wk_ctc_transcribe on this handle yet");
  if (!c->tr_last_fused || batch != c->tr_last_batch || T != c->tr_last_T)
    return invalid(("wk_ctc_transcribe_stats: the handle's last wk_ctc_transcribe had batch " + std::to_string(c->tr_last_batch) +
                    ", T " + std::to_string(c->tr_last_T) +
                    (c->tr_last_fused ? " (fused)" : c->f16 ? ", not fused (T < 6)" : ", not fused (fp32 handle)") +
                    "; asked for batch " + std::to_string(batch) + ", T " + std::to_string(T))
                       .c_str());
  return on_device(c->cfg.device, [&]() -> wk_status {
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)batch * (size_t)T;
    hipError_t e = hipSuccess;
    if (d_raw) e = hipMemcpyAsync(d_raw, c->tr_feats.get(), sizeof(float) * rows * kMels, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && d_zs) e = hipMemcpyAsync(d_zs, c->tr_zs.get(), sizeof(float2) * (size_t)batch, hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_transcribe_stats");
  });
}

wk_status wk_ctc_profile(wk_ctc* c, int32_t enable) {
  if (!c) return invalid("wk_ctc_profile: null handle");
  return on_device(c->cfg.device, [&]() -> wk_status {
    const hipError_t e = fold_events(c);
    for (int i = 0; i < WK_CTC_N_STAGES; ++i) {
      c->stage_ms[i] = 0.0;
      c->stage_n[i] = 0;
    }
    c->prof = enable ? 1 : 0;
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_profile");
  });
}

wk_status wk_ctc_stage_times(wk_ctc* c, double* ms_sum, int64_t* counts) {
  if (!c || !ms_sum || !counts) return invalid("wk_ctc_stage_times: null argument");
  return on_device(c->cfg.device, [&]() -> wk_status {
    const hipError_t e = fold_events(c);
    for (int i = 0; i < WK_CTC_N_STAGES; ++i) {
      ms_sum[i] = c->stage_ms[i];
      counts[i] = c->stage_n[i];
    }
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_stage_times");
  });
}

wk_status wk_ctc_frame_argmax(wk_ctc* c, int64_t batch, int32_t T, int32_t* d_pred, void* stream) {
  if (!c || batch < 0 || T < 1 || (batch > 0 && !d_pred)) return invalid("wk_ctc_frame_argmax: bad arguments");
  if (batch == 0) return WK_OK;
  if (batch != c->last_batch || T != c->last_T || !c->best)
    return invalid("wk_ctc_frame_argmax: batch and T must be those of the handle's last wk_ctc_forward");
  return on_device(c->cfg.device, [&]() -> wk_status {
    launch_ctc_pred(c->best, batch, T, c->f16 ? 1 : 0, d_pred, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_frame_argmax launch");
  });
}

namespace {
// wk_ctc_forward_train, and with drop (validated) wk_ctc_forward_train_dropout: a site that is on adds one launch.
wk_status ctc_forward_train(wk_ctc* c, const float* d_feats, int64_t batch, int32_t T, const wk_ctc_dropout* drop_or_null,
                            float* d_log_probs, void* stream) {
  if (!c || !d_feats || !d_log_probs || batch <= 0 || T <= 0) return invalid("wk_ctc_forward_train: bad arguments");
  const int64_t rows = batch <= INT32_MAX ? batch * (int64_t)T : INT64_MAX;
  if (rows > INT32_MAX) return invalid("wk_ctc_forward_train: batch x frames exceeds 2^31 rows");
  if (c->f16) return fail(WK_ERR_UNSUPPORTED, "wk_ctc_forward_train: fp32 handles only (precision 0)");
  const CtcDrop drop = drop_or_null ? ctc_drop(*drop_or_null) : CtcDrop{};
  return on_device(c->cfg.device, [&]() -> wk_status {
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if ((size_t)rows > c->tn_rows) {   // grows on first use of a larger batch x T, as the inference workspace does
      if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "sync");
      if ((e = alloc_tn(c, (size_t)rows)) != hipSuccess)
        return e == hipErrorOutOfMemory ? WK_ERR_NO_MEMORY : hip_fail(e, "wk_ctc_forward_train workspace");
    }
    c->tn_batch = 0;   // (set once every stage is enqueued)
    if (drop.on[1] && !c->tn_y0d) {
      if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "sync");
      if ((e = c->tn_y0d.alloc(c->tn_rows * 2 * kH)) != hipSuccess)
        return e == hipErrorOutOfMemory ? WK_ERR_NO_MEMORY : hip_fail(e, "wk_ctc_forward_train_dropout workspace");
    }
    const int H = kH, V = c->cfg.vocab;
    if ((e = hipMemcpyAsync(c->tn_feats, d_feats, sizeof(float) * rows * kMels, hipMemcpyDeviceToDevice, st)) != hipSuccess)
      return hip_fail(e, "hipMemcpyAsync");
    // wk_ctc_forward's fp32 stages, kernel for kernel, on the training buffers
    launch_ctc_encoder(false, d_feats, (int)batch, T, c->enc_w, c->enc_b, c->ln_g, c->ln_b, nullptr, c->tn_x0.get(), c->n_cu, st);
    // site 0 in place: the backward's ReLU mask x0 > 0 holds for the dropped x0 (a kept positive stays positive)
    if (drop.on[0]) launch_ctc_dropout_fwd(drop, 0, c->tn_x0.get(), c->tn_x0.get(), rows, c->n_cu, st);
    for (int l = 0; l < 2; ++l) {
      // layer 1 reads the dropped copy of y0; tn_y[0] stays undropped, layer 0's h_prev in the backward
      const float* x = l == 0 ? c->tn_x0.get() : drop.on[1] ? c->tn_y0d.get() : c->tn_y[0].get();
      const wk_status s = ctc_gemm_nt(st, rows, 6 * H, l == 0 ? H : 2 * H, x, c->wih[l], c->tn_gi[l].get(), false);
      if (s != WK_OK) return s;
      launch_ctc_gru(false, c->tn_gi[l].get(), c->whh_pk[l].get(), c->bih[l], c->bhh[l], batch, T, c->tn_y[l].get(), st);
      if (l == 0 && drop.on[1]) launch_ctc_dropout_fwd(drop, 1, c->tn_y[0].get(), c->tn_y0d.get(), rows, c->n_cu, st);
    }
    const wk_status s = ctc_gemm_nt(st, rows, V, 2 * H, c->tn_y[1].get(), c->out_w, c->tn_logits.get(), false);
    if (s != WK_OK) return s;
    launch_ctc_argmax(false, c->tn_logits.get(), c->out_b, rows, V, d_log_probs, nullptr, 0, 0, st);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "wk_ctc_forward_train launch");
    c->tn_batch = batch;
    c->tn_T = T;
    c->tn_drop = drop;
    return WK_OK;
  });
}
}  // namespace

wk_status wk_ctc_forward_train(wk_ctc* c, const float* d_feats, int64_t batch, int32_t T, float* d_log_probs,
                               void* stream) {
  return ctc_forward_train(c, d_feats, batch, T, nullptr, d_log_probs, stream);
}

wk_status wk_ctc_forward_train_dropout(wk_ctc* c, const float* d_feats, int64_t batch, int32_t T,
                                       const wk_ctc_dropout* drop, float* d_log_probs, void* stream) {
  if (!drop) return invalid("wk_ctc_forward_train_dropout: null drop");
  for (const float p : {drop->p_enc, drop->p_gru})
    if (!(p >= 0.0f && p < 1.0f)) return invalid("wk_ctc_forward_train_dropout: p_enc and p_gru must lie in [0, 1)");
  if (drop->offset >> 63) return invalid("wk_ctc_forward_train_dropout: offset must be < 2^63");
  return ctc_forward_train(c, d_feats, batch, T, drop, d_log_probs, stream);
}

wk_status wk_ctc_dropout_masks(wk_ctc* c, uint8_t* d_mask_enc_or_null, uint8_t* d_mask_gru_or_null, void* stream) {
  if (!c) return invalid("wk_ctc_dropout_masks: null handle");
  if (c->f16) return fail(WK_ERR_UNSUPPORTED, "wk_ctc_dropout_masks: fp32 handles only (precision 0)");
  if (c->tn_batch <= 0) return invalid("wk_ctc_dropout_masks: no training forward on this handle yet");
  return on_device(c->cfg.device, [&]() -> wk_status {
    uint8_t* const out[2] = {d_mask_enc_or_null, d_mask_gru_or_null};
    for (int s = 0; s < 2; ++s)
      if (out[s]) launch_ctc_dropout_mask(c->tn_drop, s, out[s], c->tn_batch * (int64_t)c->tn_T, c->n_cu, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_dropout_masks launch");
  });
}

wk_status wk_ctc_backward(wk_ctc* c, int64_t batch, int32_t T, const float* d_dlogits, float* d_grads, float* d_grad_norm,
                          void* stream) {
  if (!c || !d_dlogits || !d_grads || batch <= 0 || T <= 0) return invalid("wk_ctc_backward: bad arguments");
  if (batch > INT32_MAX || batch * (int64_t)T > INT32_MAX) return invalid("wk_ctc_backward: batch x frames exceeds 2^31 rows");
  if (c->f16) return fail(WK_ERR_UNSUPPORTED, "wk_ctc_backward: fp32 handles only (precision 0)");
  if (batch != c->tn_batch || T != c->tn_T || (size_t)(batch * (int64_t)T) > c->tn_rows)
    return invalid("wk_ctc_backward: batch and T must be those of the handle's last wk_ctc_forward_train");
  return on_device(c->cfg.device, [&]() -> wk_status {
    CtcBwd a{};
    a.B = batch;
    a.T = T;
    a.V = c->cfg.vocab;
    a.n_cu = c->n_cu;
    a.feats = c->tn_feats;
    a.x0 = c->tn_x0;
    a.x1 = c->tn_drop.on[1] ? c->tn_y0d : c->tn_y[0];
    a.drop = c->tn_drop;
    a.enc_w = c->enc_w;
    a.enc_b = c->enc_b;
    a.ln_g = c->ln_g;
    a.out_w = c->out_w;
    for (int l = 0; l < 2; ++l) {
      a.gi[l] = c->tn_gi[l];
      a.y[l] = c->tn_y[l];
      a.wih[l] = c->wih[l];
      a.whh[l] = c->whh[l];
      a.whht_pk[l] = c->whht_pk[l];
      a.bih[l] = c->bih[l];
      a.bhh[l] = c->bhh[l];
    }
    a.hprev = c->tn_hprev;
    a.dya = c->tn_dya;
    a.dyb = c->tn_dyb;
    a.gh = c->tn_gh;
    a.da_i = c->tn_dai;
    a.da_h = c->tn_dah;
    a.coef = c->tn_coef;
    a.pre = c->tn_pre;
    a.t0 = c->tn_t0;
    a.t1 = c->tn_t1;
    a.part = c->tn_part;
    a.part_floats = ctc_bwd_part_floats(c->cfg.vocab, (int64_t)c->tn_rows);
    a.dlogits = d_dlogits;
    a.grads = d_grads;
    a.norm = d_grad_norm;
    launch_ctc_backward(a, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_backward launch");
  });
}

namespace {

// The handle's weight buffers in blob order (wk_ctc_create's `take` sequence).
CtcSegTable seg_table(const wk_ctc* c) {
  const int64_t H = kH, V = c->cfg.vocab;
  CtcSegTable t;
  int k = 0;
  int64_t off = 0;
  auto add = [&](float* p, int64_t len) {
    t.s[k++] = {off, len, p};
    off += len;
  };
  add(c->enc_w, H * kMels);
  add(c->enc_b, H);
  add(c->ln_g, H);
  add(c->ln_b, H);
  for (int l = 0; l < 2; ++l)
    for (int d = 0; d < 2; ++d) {
      const int64_t din = l == 0 ? H : 2 * H;
      add(c->wih[l] + d * 3 * H * din, 3 * H * din);
      add(c->whh[l] + d * 3 * H * H, 3 * H * H);
      add(c->bih[l] + d * 3 * H, 3 * H);
      add(c->bhh[l] + d * 3 * H, 3 * H);
    }
  add(c->out_w, V * 2 * H);
  add(c->out_b, V);
  return t;
}

// Every W_hh layout an fp32 entry point reads, from whh[l].
void refresh_whh(const wk_ctc* c, hipStream_t st) {
  launch_ctc_refresh({{c->whh[0], c->whh[1]}, {c->whh_pk[0], c->whh_pk[1]}, {c->whht_pk[0], c->whht_pk[1]}}, st);
}

// The weight-changing calls: fp32 handles, and not the attribution mode (its fp16 out_w16 would go stale).
wk_status mutable_handle(const wk_ctc* c, const char* fn) {
  if (c->f16) return fail(WK_ERR_UNSUPPORTED, (std::string(fn) + ": fp32 handles only (precision 0)").c_str());
  if (c->mix) return fail(WK_ERR_UNSUPPORTED, (std::string(fn) + ": not on a handle created under WAKEWORD_CTC_MIX").c_str());
  return WK_OK;
}

// Adam's state, zeroed, on first use (stream-ordered; the allocation is what may block).
wk_status ensure_optim(wk_ctc* c, hipStream_t st, const char* fn) {
  if (c->opt_ready) return WK_OK;
  const size_t n = (size_t)wk_ctc_num_weights(&c->cfg);
  hipError_t e = c->opt_m.alloc(n);
  if (e == hipSuccess) e = c->opt_v.alloc(n);
  if (e == hipSuccess) e = c->opt_norm.alloc(1);
  if (e == hipSuccess) e = hipMemsetAsync(c->opt_m, 0, sizeof(float) * n, st);
  if (e == hipSuccess) e = hipMemsetAsync(c->opt_v, 0, sizeof(float) * n, st);
  if (e != hipSuccess) {
    c->opt_m.reset();
    c->opt_v.reset();
    c->opt_norm.reset();
    return e == hipErrorOutOfMemory ? fail(WK_ERR_NO_MEMORY, fn) : hip_fail(e, fn);
  }
  c->opt_step = 0;
  c->opt_ready = true;
  return WK_OK;
}

}  // namespace

wk_status wk_ctc_weights(wk_ctc* c, float* d_out, void* stream) {
  if (!c || !d_out) return invalid("wk_ctc_weights: null argument");
  if (const wk_status s = mutable_handle(c, "wk_ctc_weights")) return s;
  return on_device(c->cfg.device, [&]() -> wk_status {
    launch_ctc_gather(seg_table(c), d_out, c->n_cu, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_weights launch");
  });
}

wk_status wk_ctc_set_weights(wk_ctc* c, const float* d_blob, void* stream) {
  if (!c || !d_blob) return invalid("wk_ctc_set_weights: null argument");
  if (const wk_status s = mutable_handle(c, "wk_ctc_set_weights")) return s;
  return on_device(c->cfg.device, [&]() -> wk_status {
    launch_ctc_scatter(seg_table(c), d_blob, c->n_cu, (hipStream_t)stream);
    refresh_whh(c, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? WK_OK : hip_fail(e, "wk_ctc_set_weights launch");
  });
}

wk_status wk_ctc_adam_step(wk_ctc* c, const wk_ctc_adam* opt, const float* d_grads, const float* d_norm_or_null,
                           void* stream) {
  if (!c || !opt || !d_grads) return invalid("wk_ctc_adam_step: null argument");
  if (!std::isfinite(opt->lr) || opt->lr < 0.0f) return invalid("wk_ctc_adam_step: lr must be finite and >= 0");
  if (!(opt->beta1 >= 0.0f && opt->beta1 < 1.0f) || !(opt->beta2 >= 0.0f && opt->beta2 < 1.0f))
    return invalid("wk_ctc_adam_step: beta1 and beta2 must lie in [0, 1)");
  if (!(opt->eps > 0.0f)) return invalid("wk_ctc_adam_step: eps must be > 0");
  if (!(opt->weight_decay >= 0.0f)) return invalid("wk_ctc_adam_step: weight_decay must be >= 0");
  if (std::isnan(opt->max_norm)) return invalid("wk_ctc_adam_step: max_norm is NaN (<= 0 turns the clip off)");
  if (const wk_status s = mutable_handle(c, "wk_ctc_adam_step")) return s;
  return on_device(c->cfg.device, [&]() -> wk_status {
    hipStream_t st = (hipStream_t)stream;
    if (const wk_status s = ensure_optim(c, st, "wk_ctc_adam_step: optimiser state")) return s;
    const bool clip = opt->max_norm > 0.0f;
    const float* norm = clip ? d_norm_or_null : nullptr;
    if (clip && !norm) {
      launch_ctc_bwd_norm(d_grads, wk_ctc_num_weights(&c->cfg), c->opt_norm, st);
      norm = c->opt_norm;
    }
    const int64_t step = c->opt_step + 1;
    const double b1 = opt->beta1, b2 = opt->beta2;
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    const CtcAdamArgs a{opt->max_norm, opt->weight_decay,           opt->beta1,        (float)(1.0 - b1), opt->beta2,
                        (float)(1.0 - b2), (float)((double)opt->lr / bc1), (float)sqrt(bc2), opt->eps};
    launch_ctc_adam(seg_table(c), d_grads, c->opt_m, c->opt_v, norm, a, c->n_cu, st);
    refresh_whh(c, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "wk_ctc_adam_step launch");
    c->opt_step = step;
    return WK_OK;
  });
}

wk_status wk_ctc_optim_state(wk_ctc* c, float* d_m, float* d_v, int64_t* step, void* stream) {
  if (!c) return invalid("wk_ctc_optim_state: null handle");
  if (const wk_status s = mutable_handle(c, "wk_ctc_optim_state")) return s;
  return on_device(c->cfg.device, [&]() -> wk_status {
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = sizeof(float) * (size_t)wk_ctc_num_weights(&c->cfg);
    hipError_t e = hipSuccess;
    float* const out[2] = {d_m, d_v};
    const float* const src[2] = {c->opt_m, c->opt_v};
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {   // (a handle that never stepped: zeros, step 0)
      if (!out[i]) continue;
      e = c->opt_ready ? hipMemcpyAsync(out[i], src[i], bytes, hipMemcpyDeviceToDevice, st) : hipMemsetAsync(out[i], 0, bytes, st);
    }
    if (e != hipSuccess) return hip_fail(e, "wk_ctc_optim_state");
    if (step) *step = c->opt_ready ? c->opt_step : 0;
    return WK_OK;
  });
}

wk_status wk_ctc_set_optim_state(wk_ctc* c, const float* d_m_or_null, const float* d_v_or_null, int64_t step, void* stream) {
  if (!c) return invalid("wk_ctc_set_optim_state: null handle");
  if (step < 0) return invalid("wk_ctc_set_optim_state: negative step");
  if (const wk_status s = mutable_handle(c, "wk_ctc_set_optim_state")) return s;
  return on_device(c->cfg.device, [&]() -> wk_status {
    hipStream_t st = (hipStream_t)stream;
    if (const wk_status s = ensure_optim(c, st, "wk_ctc_set_optim_state: optimiser state")) return s;
    const size_t bytes = sizeof(float) * (size_t)wk_ctc_num_weights(&c->cfg);
    float* const dst[2] = {c->opt_m, c->opt_v};
    const float* const src[2] = {d_m_or_null, d_v_or_null};
    for (int i = 0; i < 2; ++i) {
      const hipError_t e = src[i] ? hipMemcpyAsync(dst[i], src[i], bytes, hipMemcpyDeviceToDevice, st)
                                  : hipMemsetAsync(dst[i], 0, bytes, st);
      if (e != hipSuccess) return hip_fail(e, "wk_ctc_set_optim_state");
    }
    c->opt_step = step;
    return WK_OK;
  });
}

}  // extern "C"
