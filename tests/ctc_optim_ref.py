"""References for the GRU-CTC optimiser's tests (not a test module; CPU only).

* ``adam_ref``: clip_grad_norm_ then torch.optim.Adam (non-amsgrad, L2 weight
  decay) on the flat weight blob, written out in a given dtype -- float64 is
  the reference (held against torch itself by tests/test_ctc_optim_ref.py),
  float32 the yardstick e32.  ``MUTATIONS`` are the mistakes an Adam kernel
  makes; each must move a tensor by more than 100 times its bound.
* ``gradients``: the seeded gradients of the optimiser-alone tests.  Per tensor
  of the state-dict spec, normal values at a scale 10^(-6 u), u ~ U(0, 1); 1 %
  of the elements exactly 0 and another 1 % times 1e-12 (sqrt(v) near eps);
  then the whole blob rescaled to the 2-norms ``NORMS`` on steps 1 to 5: the
  clip on, on either side of max_norm = 5, and off.
* ``trajectory``: the reference's training loop (ctc.py:390-402) on one batch
  by torch-CPU autograd in a given dtype.

Bounds.  Per tensor, the weights use e = max|p - p64| / max|p64 - p0| (the
error against the displacement the steps made), m and v use
max|x - x64| / max|x64|, and
    e_dev <= K_OPT * max(e32, FLOOR),  FLOOR = 16 * 2^-23
with e32 adam_ref's float32 run by the same measure.  The trajectory compares
the loss curve: |loss_k - loss64_k| <= K_TRAJ * max(max_j |loss32_j - loss64_j|,
CTCModel.loss's bound on the batch).  K_OPT and K_TRAJ are twice the worst
device / yardstick ratio of the kernels' first complete run over every case
(profiles/ctc_optim_bounds.md), the rule of K_BWD.
"""
import copy
import functools

import torch
import torch.nn.functional as F

import ctc_grad_ref as G
import ctc_ref as R

FLOOR = G.FLOOR
K_OPT = 5.72                   # 2 x 2.86 (V = 4100, weight_decay run, m of output_layer.weight)
K_TRAJ = 0.11                  # 2 x 0.0551 (step 1 of 8: 1.72e-6 against the loss bound 3.12e-5)
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=5.0)     # ctc.py:368, :401
NORMS = (30.0, 12.0, 4.9, 5.1, 2.0)
RUNS = {"plain": {}, "weight_decay": {"weight_decay": 1e-2}, "no_clip": {"max_norm": 0.0}}
MUTATIONS = ("no_bias_correction", "no_clamp", "eps_in_sqrt", "decoupled_wd", "clip_update_only", "step_off_by_one")
TRAJ = (512, 17, 13, 8)        # vocab, B, T, steps


def spec(vocab):
    from wakeword.ctc import ctc_state_dict_spec
    return ctc_state_dict_spec(vocab)


def split(flat, vocab):
    from wakeword.ctc import unpack_grads
    return unpack_grads(flat, vocab)


def flat_weights(model, vocab, dtype=torch.float32):
    """The module's parameters as one blob of dtype in the spec's order."""
    sd = model.state_dict()
    return torch.cat([sd[k].detach().reshape(-1).to(dtype) for k, _ in spec(vocab)])


@functools.lru_cache(maxsize=None)
def p0(vocab):
    return flat_weights(R.model(vocab), vocab)


@functools.lru_cache(maxsize=None)
def gradients(vocab):
    """(list of fp32 gradient blobs, list of their 2-norms as fp32 scalars: the
    double-accumulated norm rounded to float, as wk_ctc_backward reports it)."""
    gen = torch.Generator().manual_seed(4200 + vocab)
    grads, norms = [], []
    for target in NORMS:
        parts = []
        for _, shape in spec(vocab):
            n = 1
            for s in shape:
                n *= s
            scale = 10.0 ** (-6.0 * float(torch.rand((), generator=gen)))
            g = torch.randn(n, generator=gen, dtype=torch.float64) * scale
            u = torch.rand(n, generator=gen)
            g[u < 0.01] = 0.0
            g[(u >= 0.01) & (u < 0.02)] *= 1e-12
            parts.append(g)
        g = torch.cat(parts)
        g = (g * (target / float(g.norm()))).float()
        grads.append(g)
        norms.append(g.double().norm().float())
    return grads, norms


def adam_ref(p, grads, norms, dtype, lr, betas, eps, weight_decay, max_norm, mutation=None, m=None, v=None, step0=0):
    """(p, m, v) after one step per gradient, in dtype.  p, m, v and the
    gradients are flat blobs; norms are the gradients' 2-norms (fp32 scalars,
    read as the device reads them).  mutation: one of MUTATIONS."""
    assert mutation is None or mutation in MUTATIONS
    b1, b2 = betas
    p = p.to(dtype).clone()
    m = torch.zeros_like(p) if m is None else m.to(dtype).clone()
    v = torch.zeros_like(p) if v is None else v.to(dtype).clone()
    for i, (g, norm) in enumerate(zip(grads, norms)):
        t = step0 + i + 1 + (1 if mutation == "step_off_by_one" else 0)
        g = g.to(dtype)
        coef = torch.ones((), dtype=dtype)
        if max_norm > 0:
            coef = max_norm / (norm.to(dtype) + 1e-6)
            if mutation != "no_clamp":
                coef = torch.where(coef > 1.0, torch.ones_like(coef), coef)     # (a NaN stays NaN)
        raw = g
        g = g * coef
        if mutation == "clip_update_only":
            gm = raw + weight_decay * p
        elif mutation == "decoupled_wd":
            gm = g
        else:
            gm = g + weight_decay * p
        m = b1 * m + (1.0 - b1) * gm
        v = b2 * v + (1.0 - b2) * (gm * gm)
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        if mutation == "no_bias_correction":
            bc1 = bc2 = 1.0
        if mutation == "eps_in_sqrt":
            denom = torch.sqrt(v / bc2 + eps)
        else:
            denom = torch.sqrt(v) / (bc2 ** 0.5) + eps
        upd = (lr / bc1) * m / denom
        if mutation == "clip_update_only":
            upd = upd * coef
        if mutation == "decoupled_wd":
            p = p * (1.0 - lr * weight_decay)
        p = p - upd
    return p, m, v


def abi_hyper(hyper):
    """The hyper-parameters as wk_ctc_adam carries them: rounded to fp32.  The
    device steps with beta2 = fl32(0.999), whose 1 - beta2 is 1.3e-5 (relative)
    off 0.001, and so must the reference it is compared with; v and its bias
    correction move together, so the update itself does not see the rounding."""
    r = lambda x: float(torch.tensor(x, dtype=torch.float32))
    return {k: tuple(r(b) for b in v) if k == "betas" else r(v) for k, v in hyper.items()}


def errors(got, ref, base, vocab):
    """{key: error} per tensor of the spec: against the displacement ref - base
    when base is given (weights), else against max|ref| (moments).  A tensor
    the steps did not move (or a zero moment) must be matched exactly."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), ref.double()
    g, r = split(got, vocab), split(ref, vocab)
    b = split(base.double(), vocab) if base is not None else None
    out = {}
    for k in r:
        top = float((r[k] - b[k]).abs().max()) if b is not None else float(r[k].abs().max())
        diff = float((g[k] - r[k]).abs().max())
        out[k] = (0.0 if diff == 0.0 else float("inf")) if top == 0.0 else diff / top
    return out


class OptCase:
    """One (vocab, run): the float64 result and the float32 yardstick."""

    def __init__(self, vocab, run):
        self.vocab, self.run = vocab, run
        self.hyper = abi_hyper(dict(HYPER, **RUNS[run]))
        self.grads, self.norms = gradients(vocab)
        self.p0 = p0(vocab)
        self.ref = adam_ref(self.p0, self.grads, self.norms, torch.float64, **self.hyper)
        r32 = adam_ref(self.p0, self.grads, self.norms, torch.float32, **self.hyper)
        self.e32 = self.measure(r32)

    def measure(self, pmv):
        """{"p" | "m" | "v": {key: error}} of a (p, m, v) triple against the float64 run."""
        return {"p": errors(pmv[0], self.ref[0], self.p0, self.vocab), "m": errors(pmv[1], self.ref[1], None, self.vocab),
                "v": errors(pmv[2], self.ref[2], None, self.vocab)}

    def bound(self, what, key, K=None):
        return (K_OPT if K is None else K) * max(self.e32[what][key], FLOOR)


@functools.lru_cache(maxsize=None)
def opt_case(vocab, run):
    return OptCase(vocab, run)


# ---- the training loop -------------------------------------------------------------
def traj_batch(vocab, B, T):
    """(features, labels, input lengths, label lengths) of the trajectory test."""
    labels, il, tl = G.e2e_targets(vocab, B, T, zeroed=[])
    return R.features_case(B, T), labels, il, tl


@functools.lru_cache(maxsize=None)
def trajectory(vocab, B, T, steps, dtype):
    """The reference's loop on one batch by torch-CPU autograd in dtype: eval
    mode (no dropout), nn.CTCLoss(blank=0, zero_infinity=True) on the mean,
    clip_grad_norm_(5.0), optim.Adam(lr=1e-3).  Returns (losses before each
    update, gradient norms before the clip, final flat weights)."""
    feats, labels, il, tl = traj_batch(vocab, B, T)
    m = copy.deepcopy(R.model(vocab)).to(dtype)
    m.eval()
    opt = torch.optim.Adam(m.parameters(), lr=HYPER["lr"], betas=HYPER["betas"], eps=HYPER["eps"])
    x, t_il, t_tl = feats.to(dtype), torch.tensor(il), torch.tensor(tl)
    losses, norms = [], []
    for _ in range(steps):
        lp = F.log_softmax(G.logits_of(m, x), -1)
        loss = F.ctc_loss(lp.transpose(0, 1), labels, t_il, t_tl, blank=0, reduction="mean", zero_infinity=True)
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(m.parameters(), HYPER["max_norm"])))
        opt.step()
        losses.append(float(loss.detach()))
    return losses, norms, flat_weights(m, vocab, dtype)
