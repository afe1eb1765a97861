"""References for the tests of train-mode dropout in the GRU-CTC head (not a
test module; CPU only).

* ``philox4x32_10``: the generator in numpy, from its definition (multipliers
  D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85, ten rounds).
* ``masks``: the two keep masks of one training forward, addressed as
  include/wakeword.h states: key = (seed low, seed high), counter = (q low,
  q high, offset low, offset high | site << 31), q = e / 4, element e = row *
  width + unit takes word e % 4, kept iff word >= floor(double(float32(p)) 2^32).
* ``Masked``: the function the device trains -- the reference's encoder, then
  two single-layer bidirectional ``nn.GRU`` carrying the two layers' weights,
  with the explicit products ``x * m * s`` between them, s =
  double(float32(1) / (float32(1) - float32(p))) -- differentiated by torch-CPU
  autograd.  float64 is the reference, float32 the yardstick e32.
* ``hand_backward``: ctc_grad_ref.hand_backward with the two masks, held
  against ``Masked`` in float64 by tests/test_ctc_dropout_ref.py; it carries the
  ``MUTATIONS``, the mistakes a dropout implementation makes.

Bounds.  Per tensor (the log-probs count as one), e = max|x - x64| / max|x64|:
    e_dev <= K * max(e32, FLOOR),  FLOOR = 16 * 2^-23
K_BWD (backward alone, dlogits given), K_E2E (through wk_ctc_loss) and K_TRAJ
(the eight-step loss curve, in ctc_optim_ref's unit) are twice the worst
device / yardstick ratio of the kernels' first complete run over every case,
measured against the float64 reference (profiles/ctc_dropout_bounds.md).
"""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

import ctc_grad_ref as G
import ctc_optim_ref as O
import ctc_ref as R

H = R.H
FLOOR = G.FLOOR
K_BWD = 1.61                   # 2 x 0.805 (V = 512, B = 1, T = 13, p = (0.2, 0.2), gru.bias_hh_l0)
K_E2E = 5.92                   # 2 x 2.96 (V = 512, B = 8, T = 129, p = (0.2, 0.2), output_layer.bias)
K_TRAJ = 0.57                  # 2 x 0.284 (step 5 of 8: 1.02e-5 against the loss bound 3.6e-5)
WIDTH = (H, 2 * H)             # site 0: encoder output; site 1: layer 0's output as layer 1's input
CASES = ((512, 35, 1), (512, 35, 5), (512, 1, 13), (512, 16, 13), (512, 17, 13), (512, 8, 129), (4100, 17, 13))
PROBS = {case: ((0.2, 0.2),) for case in CASES}
PROBS[(512, 17, 13)] = ((0.2, 0.2), (0.5, 0.0), (0.0, 0.5))       # one site at a time: tells them apart
STREAMS = ((0, 0), (0x9E3779B97F4A7C15, 1), (7, 2 ** 32 + 3), (7, 2 ** 62 + 1))     # (seed, offset)
TRAJ = (512, 8, 33, 8)         # vocab, B, T, steps
MUTATIONS = ("bwd_mask0", "bwd_mask1", "no_scale", "hprev_dropped", "sites_swapped")

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr (..., 4) and key (2,) of 32-bit words -> (..., 4) uint32 words."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]          # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def threshold(p):
    """floor(double(float32(p)) * 2^32): an element is kept iff its word >= this."""
    return int(np.floor(float(np.float32(p)) * 2.0 ** 32))


def scale(p):
    """The factor of a kept element as the host computes it in float, widened."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def site_words(seed, offset, site, n):
    """The first n (a multiple of 4) words of a site's stream."""
    assert n % 4 == 0 and 0 <= offset < 2 ** 63 and 0 <= seed < 2 ** 64
    q = np.arange(n // 4, dtype=np.uint64)
    ctr = np.empty((n // 4, 4), np.uint64)
    ctr[:, 0], ctr[:, 1] = q & _LOW, q >> np.uint64(32)
    ctr[:, 2], ctr[:, 3] = offset & 0xFFFFFFFF, (offset >> 32) | (site << 31)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)


def masks(seed, offset, B, T, p_enc, p_gru, swap=False):
    """(m0 (B, T, 128), m1 (B, T, 256)) bool tensors, True = kept.  swap: the
    two sites' ids exchanged (the mutation)."""
    out = []
    for site, p in enumerate((p_enc, p_gru)):
        w = site_words(seed, offset, site ^ 1 if swap else site, B * T * WIDTH[site])
        out.append(torch.from_numpy(w >= np.uint32(threshold(p))).reshape(B, T, WIDTH[site]))     # (p = 0: all kept)
    return tuple(out)


# ---- the masked module ---------------------------------------------------------------
class Masked:
    """The trained-like model with the dropout products written out, in dtype."""

    def __init__(self, model, dtype):
        m = copy.deepcopy(model).to(dtype)
        m.eval()                                   # (the encoder's own nn.Dropout: identity)
        self.m, self.dtype = m, dtype
        self.layers = []
        for l in range(2):
            g = torch.nn.GRU(input_size=WIDTH[l], hidden_size=H, num_layers=1, batch_first=True, bidirectional=True).to(dtype)
            with torch.no_grad():
                for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    for sfx in ("", "_reverse"):
                        getattr(g, f"{name}_l0{sfx}").copy_(getattr(m.gru, f"{name}_l{l}{sfx}"))
            self.layers.append(g)

    def parameters(self):
        """{state-dict key of the model: parameter of this module}."""
        out = {k: p for k, p in self.m.named_parameters() if not k.startswith("gru.")}
        for l, g in enumerate(self.layers):
            for k, p in g.named_parameters():
                out["gru." + k.replace("_l0", f"_l{l}")] = p
        return out

    def logits(self, feats, m0, m1, p):
        s0, s1 = scale(p[0]), scale(p[1])
        x0 = self.m.audio_encoder(feats.to(self.dtype)) * m0.to(self.dtype) * s0
        y0, _ = self.layers[0](x0)
        y1, _ = self.layers[1](y0 * m1.to(self.dtype) * s1)
        return self.m.output_layer(y1)

    def grads(self):
        return {k: (p.grad.detach() if p.grad is not None else torch.zeros_like(p)) for k, p in self.parameters().items()}


def autograd(model, feats, D, m0, m1, p, dtype):
    """(log-probs, {key: d (logits * D).sum() / d parameter}) of the masked module in dtype."""
    mm = Masked(model, dtype)
    logits = mm.logits(feats, m0, m1, p)
    (logits * D.to(dtype)).sum().backward()
    return F.log_softmax(logits.detach(), -1), {k: mm.grads()[k] for k in G.keys(D.shape[-1])}


def e2e_reference(model, feats, labels, il, tl, m0, m1, p, dtype):
    """ctc_grad_ref.e2e_reference on the masked module: (loss, per-utterance nll, log-probs, {key: gradient})."""
    mm = Masked(model, dtype)
    B = feats.shape[0]
    live = [b for b in range(B) if il[b] > 0]
    lp = F.log_softmax(mm.logits(feats, m0, m1, p), -1)
    nll_live = F.ctc_loss(lp[live].transpose(0, 1), labels[live], torch.tensor([il[b] for b in live]),
                          torch.tensor([tl[b] for b in live]), blank=0, reduction="none", zero_infinity=True)
    nll = torch.zeros(B, dtype=dtype)
    nll[live] = nll_live
    loss = (nll / torch.tensor(tl, dtype=dtype).clamp(min=1)).mean()
    loss.backward()
    return loss.detach(), nll.detach(), lp.detach(), {k: mm.grads()[k] for k in G.keys(lp.shape[-1])}


# ---- the hand-written backward, with the masks and the mutations ------------------------
def hand_backward(model, feats, D, m0, m1, p, mutation=None):
    """ctc_grad_ref.hand_backward's equations in float64 with dropout:
        x0d = s0 m0 relu(pre) feeds layer 0; y0d = s1 m1 y0 feeds layer 1 (gi1, dW_ih1); the undropped y0 is
        layer 0's h_prev; dy0 = s1 m1 dx1; dx0 = s0 m0 dx0' before the ReLU mask.
    mutation: one of MUTATIONS but sites_swapped, which is a mutation of masks()."""
    assert mutation is None or mutation in MUTATIONS[:4]
    prm = R._params(model)
    x, D = feats.double(), D.double()
    B, T, _ = x.shape
    m = [m0.double(), m1.double()]
    s = [1.0, 1.0] if mutation == "no_scale" else [scale(p[0]), scale(p[1])]
    W, b = prm["audio_encoder.0.weight"], prm["audio_encoder.0.bias"]
    gam, bet = prm["audio_encoder.1.weight"], prm["audio_encoder.1.bias"]
    a = x @ W.T + b
    c = a - a.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((c ** 2).mean(-1, keepdim=True) + 1e-5)
    xh = c * rstd
    pre = xh * gam + bet
    ins, saved = [torch.relu(pre) * m[0] * s[0]], []
    for l in range(2):
        ss = [G._gru_dir_saved(ins[l], prm[f"gru.weight_ih_l{l}{sfx}"], prm[f"gru.weight_hh_l{l}{sfx}"],
                               prm[f"gru.bias_ih_l{l}{sfx}"], prm[f"gru.bias_hh_l{l}{sfx}"], sfx != "") for sfx in ("", "_reverse")]
        saved.append(ss)
        y = torch.cat([d["h"] for d in ss], -1)
        ins.append(y * m[1] * s[1] if l == 0 else y)
    g = {}
    V = D.shape[-1]
    D2 = D.reshape(-1, V)
    g["output_layer.bias"] = D2.sum(0)
    g["output_layer.weight"] = D2.T @ ins[2].reshape(-1, 2 * H)
    dy = (D2 @ prm["output_layer.weight"]).reshape(B, T, 2 * H)
    for l in (1, 0):
        xin = ins[l]
        din = xin.shape[-1]
        dx = torch.zeros(B, T, din, dtype=x.dtype)
        for d, sfx in enumerate(("", "_reverse")):
            sv = saved[l][d]
            hprev = sv["hprev"]
            if mutation == "hprev_dropped" and l == 0:       # h_prev read from the dropped y0: the shift of s1 m1 y0
                drop = sv["h"] * m[1][..., d * H:(d + 1) * H] * s[1]
                hprev = torch.zeros_like(drop)
                if d == 0:
                    hprev[:, 1:] = drop[:, :-1]
                else:
                    hprev[:, :-1] = drop[:, 1:]
            wih, whh = prm[f"gru.weight_ih_l{l}{sfx}"], prm[f"gru.weight_hh_l{l}{sfx}"]
            dh = torch.zeros(B, H, dtype=x.dtype)
            da_i = torch.empty(B, T, 3 * H, dtype=x.dtype)
            da_h = torch.empty(B, T, 3 * H, dtype=x.dtype)
            for t in (range(T) if d else range(T - 1, -1, -1)):
                r, z, n, hn = (sv[k][:, t] for k in ("r", "z", "n", "hn"))
                hp = hprev[:, t]
                dht = dh + dy[:, t, d * H:(d + 1) * H]
                dn = dht * (1.0 - z) * (1.0 - n * n)
                dz = dht * (hp - n) * z * (1.0 - z)
                dr = dn * hn * r * (1.0 - r)
                da_i[:, t] = torch.cat([dr, dz, dn], -1)
                da_h[:, t] = torch.cat([dr, dz, dn * r], -1)
                dh = da_h[:, t] @ whh + dht * z
            ai, ah = da_i.reshape(-1, 3 * H), da_h.reshape(-1, 3 * H)
            g[f"gru.weight_ih_l{l}{sfx}"] = ai.T @ xin.reshape(-1, din)
            g[f"gru.weight_hh_l{l}{sfx}"] = ah.T @ hprev.reshape(-1, H)
            g[f"gru.bias_ih_l{l}{sfx}"] = ai.sum(0)
            g[f"gru.bias_hh_l{l}{sfx}"] = ah.sum(0)
            dx = dx + da_i @ wih
        dy = dx * s[l] * (1.0 if mutation == f"bwd_mask{l}" else m[l])      # through site l, the layer's input
    dl = dy * (pre > 0)
    g["audio_encoder.1.weight"] = (dl * xh).reshape(-1, H).sum(0)
    g["audio_encoder.1.bias"] = dl.reshape(-1, H).sum(0)
    dxh = dl * gam
    m1_ = dxh.mean(-1, keepdim=True)
    m2_ = (dxh * xh).mean(-1, keepdim=True)
    da = rstd * (dxh - m1_ - xh * m2_)
    g["audio_encoder.0.weight"] = da.reshape(-1, H).T @ x.reshape(-1, x.shape[-1])
    g["audio_encoder.0.bias"] = da.reshape(-1, H).sum(0)
    return g


# ---- cases ---------------------------------------------------------------------------
class DropCase:
    """ctc_grad_ref.case(vocab, B, T) under given masks and probabilities:
    the float64 log-probs and gradients and the float32 yardstick, backward
    alone.  The zeroed utterances are the eval-mode case's: the ReLU rule
    reads features and weights only."""

    def __init__(self, vocab, B, T, p, m0, m1):
        self.c = G.case(vocab, B, T)
        self.vocab, self.B, self.T, self.p, self.m0, self.m1 = vocab, B, T, p, m0, m1
        lp64, g64 = autograd(self.c.model, self.c.feats, self.c.D, m0, m1, p, torch.float64)
        lp32, g32 = autograd(self.c.model, self.c.feats, self.c.D, m0, m1, p, torch.float32)
        self.ref = dict(g64, log_probs=lp64)
        self.e32 = {k: G.rel_err(v, self.ref[k]) for k, v in dict(g32, log_probs=lp32).items()}


def report(tag, ref, e32, got, K, label):
    """Prints every tensor's error, yardstick and ratio; returns (failures, worst ratio)."""
    bad, worst = [], 0.0
    for k in ref:
        e = G.rel_err(got[k], ref[k])
        unit = max(e32[k], FLOOR)
        worst = max(worst, e / unit)
        print(f"{tag} {label} {k}: e={e:.3g} e32={e32[k]:.3g} ratio={e / unit:.3g}")
        if not e <= K * unit:
            bad.append((k, e, K * unit))
    print(f"{tag} {label} worst ratio {worst:.3g} (K = {K})")
    return bad, worst


# ---- the training loop ------------------------------------------------------------------
def traj_batch(vocab, B, T):
    labels, il, tl = G.e2e_targets(vocab, B, T, zeroed=[])
    return R.features_case(B, T), labels, il, tl


def trajectory(vocab, B, T, step_masks, p, dtype):
    """ctc_optim_ref.trajectory on the masked module, step k under
    step_masks[k] = (m0, m1).  Returns (losses before each update, gradient
    norms before the clip)."""
    feats, labels, il, tl = traj_batch(vocab, B, T)
    mm = Masked(R.model(vocab), dtype)
    params = list(mm.parameters().values())
    opt = torch.optim.Adam(params, lr=O.HYPER["lr"], betas=O.HYPER["betas"], eps=O.HYPER["eps"])
    t_il, t_tl = torch.tensor(il), torch.tensor(tl)
    losses, norms = [], []
    for m0, m1 in step_masks:
        lp = F.log_softmax(mm.logits(feats, m0, m1, p), -1)
        loss = F.ctc_loss(lp.transpose(0, 1), labels, t_il, t_tl, blank=0, reduction="mean", zero_infinity=True)
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, O.HYPER["max_norm"])))
        opt.step()
        losses.append(float(loss.detach()))
    return losses, norms
