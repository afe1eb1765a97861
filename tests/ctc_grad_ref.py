"""References for the GRU-CTC backward's tests (not a test module; CPU only).

* ``hand_backward``: a hand-written float64 backward of ``ctc_ref.forward`` up
  to the logits -- the equations of DESIGN 5.11, which are the kernels' -- held
  against torch.autograd on the module in ``.double()`` by
  tests/test_ctc_grad_ref.py.  ``MUTATIONS`` are the mistakes a BPTT kernel
  makes; each must move a tensor by more than twice the GPU bound.
* ``autograd``: gradients of ``(logits * D).sum()`` for every parameter by
  torch-CPU autograd in a given dtype (float64: the reference; float32: the
  yardstick e32).
* ``case``: one (vocab, B, T) with its seeded upstream gradient D, the
  utterances the ReLU rule zeroes, g64 and e32.

Bound, per tensor, with e = max|g - g64| / max|g64|:
    e_dev <= K * max(e32, FLOOR),  FLOOR = 16 * 2^-23 (tests/test_gpu_train.py)
K_BWD (backward alone, D given) and K_E2E (loss_and_grad, wk_ctc_loss's own
gradient error included) are twice the worst device / reference ratio of the
kernels' first complete run over every case (profiles/ctc_grad_bounds.md).

ReLU decisions: a pre-activation within rounding of 0 flips a whole gradient
term, so the reference alone zeroes an utterance that holds an element with
|a64| < 8 delta, delta = max|a32 - a64| over the case's pre-ReLU rows (a32:
torch-CPU fp32).  Its dlogits rows are zeroed (end to end: its input length
is set to 0); it stays in the batch.  At most a third of a case's utterances.
"""
import copy
import functools

import torch
import torch.nn.functional as F

import ctc_ref as R

H = R.H
FLOOR = 16 * 2.0 ** -23
K_BWD = 2.13                   # 2 x 1.06 (V = 4100, B = 17, T = 13)
K_E2E = 5.6                    # 2 x 2.79 (V = 512, B = 35, T = 65)
MAX_ZEROED = 1.0 / 3.0
VOCABS = (512, 4100)
CASES = tuple((35, t) for t in (1, 2, 5, 13, 64, 65)) + tuple((b, 13) for b in (1, 15, 16, 17, 33)) + ((8, 129),)
MUTATIONS = ("carry", "dn_r", "dx_rev", "ln_mean", "hprev_t", "bhn")


def keys(vocab):
    from wakeword.ctc import ctc_state_dict_spec
    return [k for k, _ in ctc_state_dict_spec(vocab)]


def _module(model, dtype):
    m = copy.deepcopy(model).to(dtype)
    m.eval()
    return m


def logits_of(m, x):
    y, _ = m.gru(m.audio_encoder(x))
    return m.output_layer(y)


def pre_relu(m, x):
    """The encoder's pre-ReLU rows (after LayerNorm's affine map), (B, T, 128)."""
    with torch.no_grad():
        return m.audio_encoder[1](m.audio_encoder[0](x))


def autograd(model, feats, D, dtype):
    """{key: d (logits * D).sum() / d parameter} by torch-CPU autograd in dtype."""
    m = _module(model, dtype)
    (logits_of(m, feats.to(dtype)) * D.to(dtype)).sum().backward()
    return {k: p.grad.detach() for k, p in m.named_parameters()}


def rel_err(g, ref):
    g, ref = torch.as_tensor(g).detach().cpu().double(), ref.double()
    top = float(ref.abs().max())
    if top == 0.0:      # (dW_hh at T = 1: h_prev = 0) exactly zero is asked for
        return 0.0 if float(g.abs().max()) == 0.0 else float("inf")
    return float((g.reshape(ref.shape) - ref).abs().max()) / top


# ---- the hand-written backward ---------------------------------------------------
def _gru_dir_saved(x, wih, whh, bih, bhh, reverse):
    B, T, _ = x.shape
    gi = x @ wih.T
    h = torch.zeros(B, H, dtype=x.dtype)
    s = {k: torch.empty(B, T, H, dtype=x.dtype) for k in ("r", "z", "n", "hn", "hprev", "h")}
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        gh = h @ whh.T
        g = gi[:, t]
        r = torch.sigmoid(g[:, :H] + bih[:H] + gh[:, :H] + bhh[:H])
        z = torch.sigmoid(g[:, H:2 * H] + bih[H:2 * H] + gh[:, H:2 * H] + bhh[H:2 * H])
        hn = gh[:, 2 * H:] + bhh[2 * H:]
        n = torch.tanh(g[:, 2 * H:] + bih[2 * H:] + r * hn)
        s["hprev"][:, t] = h
        h = (1.0 - z) * n + z * h
        for k, v in (("r", r), ("z", z), ("n", n), ("hn", hn), ("h", h)):
            s[k][:, t] = v
    return s


def hand_backward(model, feats, D, mutation=None):
    """{key: gradient} of (logits * D).sum() in float64, by hand:
        dn = dh (1 - z)(1 - n^2), dz = dh (h_prev - n) z (1 - z), dr = dn (W_hn h_prev + b_hn) r (1 - r)
        da_i = [dr, dz, dn], da_h = [dr, dz, dn r], dh_prev = dh z + W_hh^T da_h
    with dh of step t also receiving the layer's upstream gradient at t.
    mutation: one of MUTATIONS (a deliberately wrong backward)."""
    assert mutation is None or mutation in MUTATIONS
    p = R._params(model)
    x = feats.double()
    D = D.double()
    B, T, _ = x.shape
    W, b = p["audio_encoder.0.weight"], p["audio_encoder.0.bias"]
    gam, bet = p["audio_encoder.1.weight"], p["audio_encoder.1.bias"]
    a = x @ W.T + b
    c = a - a.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((c ** 2).mean(-1, keepdim=True) + 1e-5)
    xh = c * rstd
    pre = xh * gam + bet
    ins, saved = [torch.relu(pre)], []
    for l in range(2):
        ss = [_gru_dir_saved(ins[l], p[f"gru.weight_ih_l{l}{sfx}"], p[f"gru.weight_hh_l{l}{sfx}"],
                             p[f"gru.bias_ih_l{l}{sfx}"], p[f"gru.bias_hh_l{l}{sfx}"], sfx != "") for sfx in ("", "_reverse")]
        saved.append(ss)
        ins.append(torch.cat([s["h"] for s in ss], -1))
    g = {}
    V = D.shape[-1]
    D2 = D.reshape(-1, V)
    g["output_layer.bias"] = D2.sum(0)
    g["output_layer.weight"] = D2.T @ ins[2].reshape(-1, 2 * H)
    dy = (D2 @ p["output_layer.weight"]).reshape(B, T, 2 * H)
    for l in (1, 0):
        xin = ins[l]
        din = xin.shape[-1]
        dx = torch.zeros(B, T, din, dtype=x.dtype)
        for d, sfx in enumerate(("", "_reverse")):
            s = saved[l][d]
            wih, whh = p[f"gru.weight_ih_l{l}{sfx}"], p[f"gru.weight_hh_l{l}{sfx}"]
            dh = torch.zeros(B, H, dtype=x.dtype)
            da_i = torch.empty(B, T, 3 * H, dtype=x.dtype)
            da_h = torch.empty(B, T, 3 * H, dtype=x.dtype)
            for t in (range(T) if d else range(T - 1, -1, -1)):       # backward in the direction's own time
                r, z, n, hn, hp = (s[k][:, t] for k in ("r", "z", "n", "hn", "hprev"))
                dht = dh + dy[:, t, d * H:(d + 1) * H]
                dn = dht * (1.0 - z) * (1.0 - n * n)
                dz = dht * (hp - n) * z * (1.0 - z)
                dr = dn * hn * r * (1.0 - r)
                da_i[:, t] = torch.cat([dr, dz, dn], -1)
                da_h[:, t] = torch.cat([dr, dz, dn if mutation == "dn_r" else dn * r], -1)
                dh = da_h[:, t] @ whh
                if mutation != "carry":
                    dh = dh + dht * z
            ai, ah = da_i.reshape(-1, 3 * H), da_h.reshape(-1, 3 * H)
            g[f"gru.weight_ih_l{l}{sfx}"] = ai.T @ xin.reshape(-1, din)
            hp_all = s["h"] if mutation == "hprev_t" else s["hprev"]
            g[f"gru.weight_hh_l{l}{sfx}"] = ah.T @ hp_all.reshape(-1, H)
            g[f"gru.bias_ih_l{l}{sfx}"] = ai.sum(0)
            g[f"gru.bias_hh_l{l}{sfx}"] = (ai if mutation == "bhn" else ah).sum(0)
            if not (mutation == "dx_rev" and d == 1):
                dx = dx + da_i @ wih
        dy = dx
    dl = dy * (pre > 0)                                   # ReLU: 0 at a pre-activation <= 0
    g["audio_encoder.1.weight"] = (dl * xh).reshape(-1, H).sum(0)
    g["audio_encoder.1.bias"] = dl.reshape(-1, H).sum(0)
    dxh = dl * gam
    m1 = dxh.mean(-1, keepdim=True)
    m2 = (dxh * xh).mean(-1, keepdim=True)
    da = rstd * (dxh - (0.0 if mutation == "ln_mean" else m1) - xh * m2)
    g["audio_encoder.0.weight"] = da.reshape(-1, H).T @ x.reshape(-1, x.shape[-1])
    g["audio_encoder.0.bias"] = da.reshape(-1, H).sum(0)
    return g


# ---- cases -----------------------------------------------------------------------
def relu_zeroed(model, feats):
    """(indices of the utterances the ReLU rule zeroes, delta) on a batch."""
    a64 = pre_relu(_module(model, torch.float64), feats.double())
    a32 = pre_relu(_module(model, torch.float32), feats.float())
    delta = float((a32.double() - a64).abs().max())
    near = (a64.abs() < 8.0 * delta).flatten(1).any(1)
    return [int(i) for i in torch.nonzero(near).flatten()], delta


@functools.lru_cache(maxsize=None)
def features(vocab, B, T):
    """features_case(B, T), except (8, 129): eight of the 35 utterances, by
    index -- the first eight if the rule zeroes at most two of them, else the
    first six it keeps and the first two it zeroes (so that path stays covered)."""
    if (B, T) != (8, 129):
        return R.features_case(B, T)
    all35 = R.features_case(35, T)
    first = all35[:8].contiguous()
    if len(relu_zeroed(R.model(vocab), first)[0]) <= 2:
        return first
    bad = set(relu_zeroed(R.model(vocab), all35)[0])
    keep = [i for i in range(35) if i not in bad][:6] + sorted(bad)[:2]
    return all35[sorted(keep)].contiguous()


def dlogits(vocab, B, T):
    """The seeded upstream gradient at the logits, fp32 normal values."""
    g = torch.Generator().manual_seed(7000 + 131 * B + T + vocab)
    return torch.randn(B, T, vocab, generator=g, dtype=torch.float32)


class Case:
    def __init__(self, vocab, B, T):
        self.vocab, self.B, self.T = vocab, B, T
        self.model = R.model(vocab)
        self.feats = features(vocab, B, T)
        self.zeroed, self.delta = relu_zeroed(self.model, self.feats)
        self.D = dlogits(vocab, B, T)
        self.D[self.zeroed] = 0.0
        self._g = {}

    def check_cap(self):
        assert len(self.zeroed) <= MAX_ZEROED * self.B, (self.B, self.T, self.zeroed)
        assert len(self.zeroed) < self.B

    @property
    def g64(self):
        if "g64" not in self._g:
            self._g["g64"] = autograd(self.model, self.feats, self.D, torch.float64)
        return self._g["g64"]

    @property
    def e32(self):
        if "e32" not in self._g:
            g32 = autograd(self.model, self.feats, self.D, torch.float32)
            self._g["e32"] = {k: rel_err(g32[k], self.g64[k]) for k in self.g64}
        return self._g["e32"]

    def bound(self, key, K=None):
        return (K_BWD if K is None else K) * max(self.e32[key], FLOOR)


@functools.lru_cache(maxsize=None)
def case(vocab, B, T):
    return Case(vocab, B, T)


# ---- end to end --------------------------------------------------------------------
def e2e_targets(vocab, B, T, zeroed):
    """Labels for loss_and_grad on a (B, T) batch: ragged input lengths (some
    < T), repeated labels, the last column of the vocabulary, and utterance
    B - 1 (when B > 1 and T > 1) without a valid alignment: more labels than
    frames.  The utterances of `zeroed` get input length 0.  Returns (labels
    (B, S) int64, input lengths, label lengths) as lists."""
    g = torch.Generator().manual_seed(900 + 17 * B + T)
    S = max(1, min(12, T // 2))
    labels = torch.randint(1, vocab, (B, S + 1), generator=g)
    labels[:, 1::3] = labels[:, 0::3][:, :labels[:, 1::3].shape[1]]       # adjacent repeats
    labels[0, 2 if S >= 2 else 0] = vocab - 1
    il = [max(1, T - (3 * b) % max(1, T // 3)) for b in range(B)]      # T, T - 3, ... > 2 T / 3
    tl = [max(1, S - b % 3) for b in range(B)]                          # <= T / 2, a third of them repeats
    if B > 1 and T > 1:
        il[B - 1] = 1
        tl[B - 1] = min(S + 1, 2)                                         # 2 labels, 1 frame: no alignment
    for b in zeroed:
        il[b] = 0
        tl[b] = max(tl[b], 1)
    return labels, il, tl


def e2e_reference(model, feats, labels, il, tl, dtype):
    """(loss, per-utterance nll, {key: gradient}) of
    F.ctc_loss(log_softmax(module(feats)), reduction="mean", zero_infinity=True)
    by torch-CPU autograd in dtype.  An utterance of input length 0 has no
    alignment for its (non-empty) label and contributes 0, as every
    utterance without one: it is left out of the call and counted in the mean."""
    m = _module(model, dtype)
    B = feats.shape[0]
    live = [b for b in range(B) if il[b] > 0]
    lp = F.log_softmax(logits_of(m, feats.to(dtype)), -1)
    nll_live = F.ctc_loss(lp[live].transpose(0, 1), labels[live], torch.tensor([il[b] for b in live]),
                          torch.tensor([tl[b] for b in live]), blank=0, reduction="none", zero_infinity=True)
    nll = torch.zeros(B, dtype=dtype)
    nll[live] = nll_live
    loss = (nll / torch.tensor(tl, dtype=dtype).clamp(min=1)).mean()
    loss.backward()
    return loss.detach(), nll.detach(), {k: p.grad.detach() for k, p in m.named_parameters()}
