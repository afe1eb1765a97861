// wk_ctc_train.hip -- the wk_ctc_* entry points that need an fp32 handle
// (wk_ctc_handle.h), no kernels: the forward that keeps its activations
// (wk_ctc_forward_train; with train-mode dropout over wk_ctc_dropout.hip,
// wk_ctc_forward_train_dropout and wk_ctc_dropout_masks), the entry to the
// backward pass of wk_ctc_bwd.hip (wk_ctc_backward), and the weights after
// creation and the optimiser over wk_ctc_optim.hip (wk_ctc_weights,
// wk_ctc_set_weights, wk_ctc_adam_step, wk_ctc_optim_state,
// wk_ctc_set_optim_state).  The forward is wk_ctc_forward's fp32 stage
// functions (wk_ctc.hip) on the training workspace: the same launches, so the
// same bits.
#include <cmath>
#include <string>

#include "wk_ctc_handle.h"

using namespace wk;

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
    CtcTrainWs& tn = c->tn;
    tn.batch = 0;   // (set once every stage is enqueued)
    if ((size_t)rows > tn.rows)   // grows on first use of a larger batch x T, as the inference workspace does
      if (const wk_status s = ctc_grow(st, tn.table(c->cfg.vocab, (size_t)rows), {{&tn.rows, (size_t)rows}},
                                       "wk_ctc_forward_train workspace"))
        return s;
    if (drop.on[1] && !tn.y0d)
      if (const wk_status s = ctc_grow(st, {{&tn.y0d, sizeof(float) * 2 * kH * tn.rows}}, {}, "wk_ctc_forward_train_dropout workspace"))
        return s;
    const hipError_t e = hipMemcpyAsync(tn.feats, d_feats, sizeof(float) * rows * kMels, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync");
    const Fwd f{c, st, batch, rows, T, false};   // (not bracketed: wk_ctc_stage_times covers features and forward)
    wk_status s = stage_encoder(f, d_feats, nullptr, tn.x0);
    if (s != WK_OK) return s;
    // site 0 in place: the backward's ReLU mask x0 > 0 holds for the dropped x0 (a kept positive stays positive)
    if (drop.on[0]) launch_ctc_dropout_fwd(drop, 0, tn.x0, tn.x0, rows, c->n_cu, st);
    if ((s = stage_gru(f, 0, tn.x0, tn.gi[0], tn.y[0])) != WK_OK) return s;
    // layer 1 reads the dropped copy of y0; y[0] stays undropped, layer 0's h_prev in the backward
    if (drop.on[1]) launch_ctc_dropout_fwd(drop, 1, tn.y[0], tn.y0d, rows, c->n_cu, st);
    if ((s = stage_gru(f, 1, drop.on[1] ? tn.y0d : tn.y[0], tn.gi[1], tn.y[1])) != WK_OK) return s;
    if ((s = stage_out32(f, tn.y[1], tn.logits, d_log_probs, nullptr)) != WK_OK) return s;
    if ((s = ctc_launched("wk_ctc_forward_train")) != WK_OK) return s;
    tn.batch = batch;
    tn.T = T;
    tn.drop = drop;
    return WK_OK;
  });
}

// The handle's weight buffers in blob order.
CtcSegTable seg_table(const wk_ctc* c) {
  const CtcWeights& w = c->w;
  const CtcBlob b = ctc_blob(c->cfg.vocab);
  float* p[kCtcSegs] = {w.enc_w, w.enc_b, w.ln_g, w.ln_b};
  for (int l = 0; l < 2; ++l)
    for (int d = 0; d < 2; ++d) {   // direction d is the second half of each of the layer's tensors
      float* const t[4] = {w.wih[l], w.whh[l], w.bih[l], w.bhh[l]};
      for (int k = 0; k < 4; ++k) {
        const int s = ctc_gru_seg(l, d, k);
        p[s] = t[k] + d * (b.off[s + 1] - b.off[s]);
      }
    }
  p[kSegOutW] = w.out_w;
  p[kSegOutB] = w.out_b;
  CtcSegTable t;
  for (int k = 0; k < kCtcSegs; ++k) t.s[k] = {b.off[k], b.off[k + 1] - b.off[k], p[k]};
  return t;
}

// Every W_hh layout an fp32 entry point reads, from whh[l].
void refresh_whh(const wk_ctc* c, hipStream_t st) {
  const CtcWeights& w = c->w;
  launch_ctc_refresh({{w.whh[0], w.whh[1]}, {w.whh_pk[0], w.whh_pk[1]}, {w.whht_pk[0], w.whht_pk[1]}}, st);
}

// The weight-changing calls: fp32 handles, and not the attribution mode (its fp16 out_w16 would go stale).
wk_status mutable_handle(const wk_ctc* c, const char* fn) {
  if (c->f16) return fail(WK_ERR_UNSUPPORTED, (std::string(fn) + ": fp32 handles only (precision 0)").c_str());
  if (c->mix) return fail(WK_ERR_UNSUPPORTED, (std::string(fn) + ": not on a handle created under WAKEWORD_CTC_MIX").c_str());
  return WK_OK;
}

size_t blob_bytes(const wk_ctc* c) { return sizeof(float) * (size_t)wk_ctc_num_weights(&c->cfg); }

// Adam's state, zeroed, on first use (stream-ordered; the allocation is what may block).
wk_status ensure_optim(wk_ctc* c, hipStream_t st, const char* fn) {
  CtcOptim& o = c->opt;
  if (o.ready) return WK_OK;
  hipError_t e = o.m.alloc_bytes(blob_bytes(c));
  if (e == hipSuccess) e = o.v.alloc_bytes(blob_bytes(c));
  if (e == hipSuccess) e = o.norm.alloc(1);
  if (e == hipSuccess) e = hipMemsetAsync(o.m, 0, blob_bytes(c), st);
  if (e == hipSuccess) e = hipMemsetAsync(o.v, 0, blob_bytes(c), st);
  if (e != hipSuccess) {
    o.m.reset();
    o.v.reset();
    o.norm.reset();
    return e == hipErrorOutOfMemory ? fail(WK_ERR_NO_MEMORY, fn) : hip_fail(e, fn);
  }
  o.step = 0;
  o.ready = true;
  return WK_OK;
}

// Both moments, blob-sized, on st: dst[i] <- src[i], or zeros where src[i] is null; a null dst[i] is skipped.
hipError_t copy_moments(const wk_ctc* c, float* const (&dst)[2], const float* const (&src)[2], hipStream_t st) {
  hipError_t e = hipSuccess;
  for (int i = 0; i < 2 && e == hipSuccess; ++i)
    if (dst[i])
      e = src[i] ? hipMemcpyAsync(dst[i], src[i], blob_bytes(c), hipMemcpyDeviceToDevice, st) : hipMemsetAsync(dst[i], 0, blob_bytes(c), st);
  return e;
}

}  // namespace

extern "C" {

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
  if (c->tn.batch <= 0) return invalid("wk_ctc_dropout_masks: no training forward on this handle yet");
  return on_device(c->cfg.device, [&]() -> wk_status {
    uint8_t* const out[2] = {d_mask_enc_or_null, d_mask_gru_or_null};
    for (int s = 0; s < 2; ++s)
      if (out[s]) launch_ctc_dropout_mask(c->tn.drop, s, out[s], c->tn.batch * (int64_t)c->tn.T, c->n_cu, (hipStream_t)stream);
    return ctc_launched("wk_ctc_dropout_masks");
  });
}

wk_status wk_ctc_backward(wk_ctc* c, int64_t batch, int32_t T, const float* d_dlogits, float* d_grads, float* d_grad_norm,
                          void* stream) {
  if (!c || !d_dlogits || !d_grads || batch <= 0 || T <= 0) return invalid("wk_ctc_backward: bad arguments");
  if (batch > INT32_MAX || batch * (int64_t)T > INT32_MAX) return invalid("wk_ctc_backward: batch x frames exceeds 2^31 rows");
  if (c->f16) return fail(WK_ERR_UNSUPPORTED, "wk_ctc_backward: fp32 handles only (precision 0)");
  if (batch != c->tn.batch || T != c->tn.T || (size_t)(batch * (int64_t)T) > c->tn.rows)
    return invalid("wk_ctc_backward: batch and T must be those of the handle's last wk_ctc_forward_train");
  return on_device(c->cfg.device, [&]() -> wk_status {
    launch_ctc_backward({batch, T, c->cfg.vocab, c->n_cu, d_dlogits, d_grads, d_grad_norm, c->tn, c->w}, (hipStream_t)stream);
    return ctc_launched("wk_ctc_backward");
  });
}

wk_status wk_ctc_weights(wk_ctc* c, float* d_out, void* stream) {
  if (!c || !d_out) return invalid("wk_ctc_weights: null argument");
  if (const wk_status s = mutable_handle(c, "wk_ctc_weights")) return s;
  return on_device(c->cfg.device, [&]() -> wk_status {
    launch_ctc_gather(seg_table(c), d_out, c->n_cu, (hipStream_t)stream);
    return ctc_launched("wk_ctc_weights");
  });
}

wk_status wk_ctc_set_weights(wk_ctc* c, const float* d_blob, void* stream) {
  if (!c || !d_blob) return invalid("wk_ctc_set_weights: null argument");
  if (const wk_status s = mutable_handle(c, "wk_ctc_set_weights")) return s;
  return on_device(c->cfg.device, [&]() -> wk_status {
    launch_ctc_scatter(seg_table(c), d_blob, c->n_cu, (hipStream_t)stream);
    refresh_whh(c, (hipStream_t)stream);
    return ctc_launched("wk_ctc_set_weights");
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
    CtcOptim& o = c->opt;
    if (const wk_status s = ensure_optim(c, st, "wk_ctc_adam_step: optimiser state")) return s;
    const bool clip = opt->max_norm > 0.0f;
    const float* norm = clip ? d_norm_or_null : nullptr;
    if (clip && !norm) {
      launch_ctc_bwd_norm(d_grads, wk_ctc_num_weights(&c->cfg), o.norm, st);
      norm = o.norm;
    }
    const int64_t step = o.step + 1;
    const double b1 = opt->beta1, b2 = opt->beta2;
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    const CtcAdamArgs a{opt->max_norm, opt->weight_decay,           opt->beta1,        (float)(1.0 - b1), opt->beta2,
                        (float)(1.0 - b2), (float)((double)opt->lr / bc1), (float)sqrt(bc2), opt->eps};
    launch_ctc_adam(seg_table(c), d_grads, o.m, o.v, norm, a, c->n_cu, st);
    refresh_whh(c, st);
    if (const wk_status s = ctc_launched("wk_ctc_adam_step")) return s;
    o.step = step;   // (only a step whose launches were accepted counts)
    return WK_OK;
  });
}

wk_status wk_ctc_optim_state(wk_ctc* c, float* d_m, float* d_v, int64_t* step, void* stream) {
  if (!c) return invalid("wk_ctc_optim_state: null handle");
  if (const wk_status s = mutable_handle(c, "wk_ctc_optim_state")) return s;
  return on_device(c->cfg.device, [&]() -> wk_status {
    const CtcOptim& o = c->opt;   // (a handle that never stepped: zeros, step 0)
    const hipError_t e = copy_moments(c, {d_m, d_v}, {o.ready ? o.m.get() : nullptr, o.ready ? o.v.get() : nullptr}, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "wk_ctc_optim_state");
    if (step) *step = o.ready ? o.step : 0;
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
    const hipError_t e = copy_moments(c, {c->opt.m, c->opt.v}, {d_m_or_null, d_v_or_null}, st);
    if (e != hipSuccess) return hip_fail(e, "wk_ctc_set_optim_state");
    c->opt.step = step;
    return WK_OK;
  });
}

}  // extern "C"
