"""References for the CTC head's parity tests (not a test module; CPU only).

* ``trained_like``: a seeded GRU_CTC_Model whose LayerNorm gamma / beta are not
  1 / 0, whose GRU saturates (|h| > 0.9 on a quarter to a third of the state
  values) and whose blank and last column win about a half and a tenth of the
  frames -- what a default ``nn`` initialisation never shows a kernel.
* ``features_case``: (B, T, 80) inputs for any T >= 1.
* ``ref64``: float64 log-probs from a hand-written forward (encoder, the four
  GRU equations in the header of wk_ctc_gru.hip, output layer, log_softmax).
* ``ref16``: the same forward with operands rounded to fp16 where the fp16
  kernels store or multiply in fp16; accumulations stay in float64.
* ``case``: one (vocab, B, T) with its float64 reference, ``e32`` (torch-CPU
  fp32 against ref64) and ``e16`` (ref16 against ref64): the parity bounds of
  tests/test_gpu_ctc_parity.py are K32 * e32 and K16 * e16 per case.
"""
import copy
import functools

import numpy as np
import torch

from oracle import wk_ctc_oracle as CO
from oracle import wk_oracle as O

H = 128
SEED = 8
VOCABS = (512, 4100)
T_CASES = tuple((35, t) for t in (1, 2, 5, 6, 7, 13, 64, 65, 129))
B_CASES = tuple((b, 13) for b in (1, 15, 16, 17, 31, 32, 33))
CASES = T_CASES + B_CASES
CAL = (35, 129)                # the calibration batch of trained_like

# Bounds: a device log-prob may be K times further from ref64 than the
# reference arithmetic of the same width is (e32: torch-CPU fp32; e16: ref16).
# Measured on the MI355X over VOCABS x CASES (profiles/ctc_parity_bounds.md):
# device-error / reference-error ratio 1.22 to 1.90 (fp32), 0.91 to 1.03
# (fp16), 0.94 to 1.14 (fp16, WAKEWORD_CTC_GEMM=1); K = twice the worst ratio.
K32 = 3.8
K16 = 2.3
MAX_EXCLUDED = 0.15            # of a case's frames, T >= 5
MAX_EXCLUDED_PER_UTT = 0.25    # of one utterance's frames, T >= 64
MIN_SHARE = 0.05               # blank / last-column share of the compared frames

_LOG2E = 1.4426950408889634
_GATE_SCALE = (-_LOG2E, -_LOG2E, 2.0 * _LOG2E)     # kCtcGateScale (wk_ctc_dev.h)


@functools.lru_cache(maxsize=None)
def audio_case(B):
    """B synthetic clips of 160 * 128 samples: a 129-frame map."""
    return O.synth_clips(41, 0, B, 160 * 128)


@functools.lru_cache(maxsize=None)
def _feature_map(B):
    return CO.features(torch.from_numpy(audio_case(B)))     # (B, 129, 80)


def features_case(B, T):
    """[:, :T] of the 129-frame z-scored log-mel map of B synthetic clips."""
    return _feature_map(B)[:, :T].contiguous()


# ---- the hand-written forward ---------------------------------------------------
def _r16(x):
    """Round to fp16 through fp32 (the kernels convert fp32 registers), back to float64."""
    return x.float().half().double()


def _ident(x):
    return x


def _params(model):
    return {k: v.detach().double() for k, v in model.state_dict().items()}


def _gate_scaled_r16(w):
    """ctc_pack_frag32 + upload_f16: gate g's rows times kCtcGateScale[g], then fp16."""
    out = torch.empty_like(w)
    for g, s in enumerate(_GATE_SCALE):
        rows = slice(g * H, (g + 1) * H)
        out[rows] = (w[rows] * s).float().half().double() / s
    return out


def gru_dir(x, wih, whh, bih, bhh, reverse, q_h=_ident, q_gi=_ident, bhn_outside=False):
    """One direction of one GRU layer, (B, T, D) -> (B, T, H), h0 = 0:
        r = s(Wir x + bir + Whr h + bhr), z = s(Wiz x + biz + Whz h + bhz),
        n = tanh(Win x + bin + r (Whn h + bhn)), h' = (1 - z) n + z h
    q_h rounds the state where it is the matrix operand, q_gi the gate inputs
    x W_ih^T.  bhn_outside is the classic wrong cell (b_hn outside r (...)):
    only the mutation test of tests/test_ctc_ref.py sets it."""
    B, T, _ = x.shape
    gi = q_gi(x @ wih.T)
    h = torch.zeros(B, H, dtype=x.dtype)
    out = torch.empty(B, T, H, dtype=x.dtype)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        gh = q_h(h) @ whh.T
        g = gi[:, t]
        r = torch.sigmoid(g[:, :H] + bih[:H] + gh[:, :H] + bhh[:H])
        z = torch.sigmoid(g[:, H:2 * H] + bih[H:2 * H] + gh[:, H:2 * H] + bhh[H:2 * H])
        if bhn_outside:
            n = torch.tanh(g[:, 2 * H:] + bih[2 * H:] + r * gh[:, 2 * H:] + bhh[2 * H:])
        else:
            n = torch.tanh(g[:, 2 * H:] + bih[2 * H:] + r * (gh[:, 2 * H:] + bhh[2 * H:]))
        h = (1.0 - z) * n + z * h
        out[:, t] = h
    return out


def forward(model, feats, mode=None, bhn_outside=False, return_states=False):
    """Float64 log-probs (B, T, V) of the hand-written model.  mode None: no
    rounding (ref64); "fp16", "gemm", "out16": see ref16."""
    p = _params(model)
    x = feats.double()
    f16 = mode in ("fp16", "gemm")
    q = _r16 if f16 else _ident
    q_w = {"fp16": _gate_scaled_r16, "gemm": _r16}.get(mode, _ident)
    a = q(x) @ q(p["audio_encoder.0.weight"]).T + p["audio_encoder.0.bias"]
    mu = a.mean(-1, keepdim=True)
    var = ((a - mu) ** 2).mean(-1, keepdim=True)                       # biased, as nn.LayerNorm
    a = (a - mu) / torch.sqrt(var + 1e-5) * p["audio_encoder.1.weight"] + p["audio_encoder.1.bias"]
    y = q(torch.relu(a))
    states = []
    for l in range(2):
        outs = []
        for sfx in ("", "_reverse"):
            outs.append(gru_dir(y, q_w(p[f"gru.weight_ih_l{l}{sfx}"]), q_w(p[f"gru.weight_hh_l{l}{sfx}"]),
                                p[f"gru.bias_ih_l{l}{sfx}"], p[f"gru.bias_hh_l{l}{sfx}"], sfx != "",
                                q_h=q, q_gi=_r16 if mode == "gemm" else _ident, bhn_outside=bhn_outside))
        y = torch.cat(outs, -1)
        states.append(y)
        y = q(y)
    if mode is None:
        logits = y @ p["output_layer.weight"].T + p["output_layer.bias"]
    else:
        logits = _r16(y) @ _r16(p["output_layer.weight"]).T + p["output_layer.bias"]
        if f16:
            logits = _r16(logits)
    lp = torch.log_softmax(logits, -1)
    return (lp, states) if return_states else lp


def ref64(model, feats):
    """Float64 log-probs of the module: the hand-written forward above, which
    tests/test_ctc_ref.py holds against a deep copy of the module in .double()
    (nn.GRU's own recurrence) to ~1e-13."""
    return forward(model, feats, None)


def module64(model, feats):
    """The module itself in double: torch's nn.GRU, LayerNorm and log_softmax."""
    with torch.no_grad():
        return copy.deepcopy(model).double()(feats.double())


def ref16(model, feats, mode="fp16"):
    """ref64 with operands rounded to fp16 where the kernels hold fp16;
    every accumulation, the gates and the state update stay float64.

    mode "fp16" (precision='fp16', the fused-projection recurrence):
      * features and encoder weight as MFMA operands -- ctc_encoder16_kernel
        (wk_ctc_dense.hip) converts the loaded rows (xb) and W (wf) to _Float16;
      * encoder output -- the same kernel stores y as _Float16 (x0h);
      * GRU W_ih, W_hh, each gate's rows times kCtcGateScale before the
        rounding -- ctc_pack_frag32 (wk_ctc_gru.hip) + upload_f16 (wk_ctc.hip);
      * the state as the matrix operand and as the layer output -- the h16
        image of ctc_gru16x_kernel (`o[q][i] = (_Float16)hn`), read back as the
        B fragments and stored as y0h / y1h; the state carried from step to
        step (`h[q][i]`) is fp32 and is not rounded here;
      * output weight -- out_w16 by upload_f16 (wk_ctc.hip); its input is y1h;
      * the logits, bias included, on the log-prob path --
        ctc_out_argmax16_kernel<LOGITS> stores them as fp16 for
        ctc_argmax_kernel<__half> (wk_ctc_out.hip).
    mode "gemm" (WAKEWORD_CTC_GEMM=1): GRU weights rounded unscaled
      (wih16, ctc_pack_whh16) and the gate inputs x W_ih^T, without bias,
      rounded -- ctc_gemm_nt_kernel<__half, __half> writes gi as fp16.
    mode "out16" (fp32 handle, WAKEWORD_CTC_MIX=out16): only y1
      (ctc_convert_kernel) and the output weight are rounded; that path
      decodes from the fp32 accumulators and has no log-probs.
    DESIGN 5.3 states the same list."""
    return forward(model, feats, mode)


# ---- the model ------------------------------------------------------------------
def _logits64(model, feats):
    p = _params(model)
    _, states = forward(model, feats, None, return_states=True)
    return states[1] @ p["output_layer.weight"].T + p["output_layer.bias"]


def trained_like(vocab, seed=SEED, out_scale=4.0, blank_bias=True):
    """CO.make_model(vocab, seed, out_scale) moved off the default init:
    LayerNorm weight ~ U(0.5, 1.5) and bias ~ U(-0.5, 0.5) from a generator of
    their own, every gru.* parameter times 3, then on the calibration batch
    features_case(*CAL) and in float64: bias[0] += the median over frames of
    (best non-blank logit - blank logit), and, for a ragged last tile
    (vocab % 64 != 0), bias[vocab - 1] += the 10 % quantile over frames of
    (best logit - that column's logit).  blank_bias=False leaves the first
    step out (the mutation test)."""
    m = CO.make_model(vocab, seed, out_scale=out_scale)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        ln = m.audio_encoder[1]
        ln.weight.copy_(0.5 + torch.rand(H, generator=g))
        ln.bias.copy_(torch.rand(H, generator=g) - 0.5)
        for prm in m.gru.parameters():
            prm.mul_(3.0)
        cal = features_case(*CAL)
        b = m.output_layer.bias
        if blank_bias:
            lg = _logits64(m, cal).reshape(-1, vocab)
            b[0] += float(torch.median(lg[:, 1:].max(-1).values - lg[:, 0]))
        if vocab % 64 != 0:
            lg = _logits64(m, cal).reshape(-1, vocab)
            b[vocab - 1] += float(torch.quantile(lg.max(-1).values - lg[:, vocab - 1], 0.10))
    return m


@functools.lru_cache(maxsize=None)
def model(vocab):
    return trained_like(vocab, SEED)


def plain_layernorm(m):
    """A copy of the model with gamma = 1, beta = 0 (nn.LayerNorm's init)."""
    c = copy.deepcopy(m)
    with torch.no_grad():
        c.audio_encoder[1].weight.fill_(1.0)
        c.audio_encoder[1].bias.zero_()
    return c


# ---- cases ----------------------------------------------------------------------
def _maxdiff(a, b):
    return float((a.double() - b).abs().max())


class Case:
    """One input of the parity tests: ref64's log-probs, argmax and top-2
    margin on it, and (computed when first asked for) the reference errors."""

    def __init__(self, vocab, feats):
        self.vocab, self.feats = vocab, feats
        self.B, self.T = feats.shape[:2]
        self.model = model(vocab)
        self.lp = ref64(self.model, feats)
        self.argmax = self.lp.argmax(-1)
        top2 = torch.topk(self.lp, 2, dim=-1).values
        self.margin = top2[..., 0] - top2[..., 1]
        self._err = {}

    def err(self, mode):
        if mode not in self._err:
            if mode == "fp32":
                with torch.no_grad():
                    self._err[mode] = _maxdiff(self.model(self.feats), self.lp)
            else:
                self._err[mode] = _maxdiff(ref16(self.model, self.feats, mode), self.lp)
        return self._err[mode]


@functools.lru_cache(maxsize=None)
def case(vocab, B, T):
    """The (vocab, B, T) case on features_case(B, T)."""
    return Case(vocab, features_case(B, T))


def e32(c):
    """max |torch-CPU fp32 log-probs - ref64| on the case."""
    return c.err("fp32")


def e16(c, mode="fp16"):
    """max |ref16(mode) - ref64| on the case."""
    return c.err(mode)


# device mode -> K; the reference error it multiplies is e32 (fp32) or e16 of that mode
MODES = {"fp32": K32, "fp16": K16, "gemm": K16, "out16": K16}


def bound(c, mode):
    """The log-prob bound of a device mode on a case: K * reference error.
    (out16 has no log-probs: its bound only sets the argmax gate.)"""
    return MODES[mode] * c.err(mode)


def gate(c, mode):
    """Frames whose argmax is compared: float64 top-2 margin > twice the bound."""
    return c.margin > 2.0 * bound(c, mode)


def check_gate(c, ok):
    """The gate's cap and coverage conditions on a case (asserted from the
    reference alone in tests/test_ctc_ref.py and again in the GPU tests):
    at T >= 5 at most 15 % of the frames are left out, at T >= 64 at most 25 %
    of any one utterance's; among the compared frames the blank and (ragged
    vocabularies) the last column each win at least 5 % and at least one."""
    n = int(ok.sum())
    assert n > 0
    if c.T >= 5:
        assert 1.0 - float(ok.float().mean()) <= MAX_EXCLUDED, (c.B, c.T, float(ok.float().mean()))
    if c.T >= 64:
        assert float(1.0 - ok.float().mean(-1).min()) <= MAX_EXCLUDED_PER_UTT
    cols = [0] + ([c.vocab - 1] if c.vocab % 64 != 0 else [])
    for col in cols:
        k = int((c.argmax[ok] == col).sum())
        assert k >= 1 and k >= MIN_SHARE * n, (c.B, c.T, col, k, n)


def saturated_share(m, feats):
    """Share of float64 GRU state values with |h| > 0.9 (both layers)."""
    _, states = forward(m, feats, None, return_states=True)
    return float(torch.cat([s.reshape(-1) for s in states]).abs().gt(0.9).float().mean())


# ---- decode patterns ------------------------------------------------------------
def greedy(pred):
    """decode_predictions on a (B, T) argmax map -> (tokens (B, T) padded with
    -1, lengths (B,)), through the oracle's greedy_decode."""
    pred = torch.as_tensor(pred).long()
    B, T = pred.shape
    lp = torch.full((B, T, int(pred.max()) + 1), -1.0)
    lp.scatter_(2, pred.unsqueeze(-1), 0.0)
    seqs = CO.greedy_decode(lp)
    tok = np.full((B, T), -1, np.int32)
    for b, s in enumerate(seqs):
        tok[b, :len(s)] = s
    return tok, np.array([len(s) for s in seqs], np.int32)


def patterns(pred):
    """Which of the greedy decode's edge patterns a (B, T) argmax map holds."""
    p = np.asarray(pred)
    T = p.shape[1]
    out = {"blank_at_0": bool((p[:, 0] == 0).any()),
           "all_blank": bool((p == 0).all(1).any()),
           "a_blank_a": bool(T >= 3 and ((p[:, :-2] != 0) & (p[:, 1:-1] == 0) & (p[:, 2:] == p[:, :-2])).any())}
    if T >= 65:
        out["repeat_63_64"] = bool(((p[:, 63] != 0) & (p[:, 63] == p[:, 64])).any())
        out["blank_63_64"] = bool(((p[:, 63] == 0) | (p[:, 64] == 0)).any())
    return out


# ---- features in float64 --------------------------------------------------------
def features64(x):
    """CO.features in float64: double audio and Hann window, the same fp32 mel
    filter bank widened, the same z-score."""
    x = torch.as_tensor(x).double()
    spec = torch.stft(x, n_fft=CO.N_FFT, hop_length=CO.HOP, win_length=CO.N_FFT,
                      window=torch.hann_window(CO.N_FFT, dtype=torch.float64), center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    mel = torch.log(torch.matmul(spec.abs().pow(2.0).transpose(-1, -2), CO.mel_fbanks().double()) + 1e-8)
    out = []
    for m in mel:
        if m.std() > 0:
            m = (m - m.mean()) / m.std()
        out.append(m)
    return torch.stack(out)
