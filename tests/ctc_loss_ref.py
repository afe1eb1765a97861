"""Cases and float64 references for wk_ctc_loss (not a test module; CPU only).

* ``SPECS`` / ``case(name, kind)``: seeded cases at the edges of the kernels --
  2S+1 either side of 64 and 128 lanes and at the register limit (S = 255),
  T = 1, 2, S and S + repeats, V = 3, 33 (no multiple of 4), 4000 and 16384,
  B = 1, 3, 35, ragged lengths inside a batch, runs of one label, the label
  V - 1 -- each with two kinds of logits: "random" (nll ~ T ln V) and
  "trained" (peaked along a random valid alignment plus noise: nll a few units).
* The float64 reference is F.log_softmax + F.ctc_loss on the CPU in float64 with
  the gradient taken at the logits (``Case.nll64``, ``Case.g64``); ``hand_ctc``
  is a hand-written float64 alpha / beta in the kernels' gradient convention,
  held against it by tests/test_ctc_loss_abi.py.
* ``e32``: torch-CPU fp32 on the same case against float64.  The device gets the
  same fp32 log-probs (``Case.lp32``) and is bounded by
      |nll_dev - nll_64|  <= K_LOSS max(e32_loss, eps32 |nll_64|)
      max |g_dev - g_64|  <= K_GRAD max(e32_grad, eps32 max(1, |nll_64|))
  per case (maxima over the case's utterances).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = float(np.finfo(np.float32).eps)

# Twice the worst device-error / reference-unit ratio of the kernels' first run
# on the MI355X over every case below (loss 1.00, gradient 12.91).  The committed
# kernels measure 0.01 to 1.31 (loss) and, for the gradient, 0.11 to 1.24 on
# random logits and 0.20 to 11.69 on trained-like ones, where torch-CPU's "fp32"
# gradient is within a rounding of float64 (1e-8 to 4e-7) and the device's fp32
# recursion is off by 1e-7 to 3e-6 (profiles/ctc_loss_bounds.md).
K_LOSS = 2.0
K_GRAD = 25.8

KINDS = ("random", "trained")


def _b35():
    """35 ragged utterances, S up to 64 (129 states: four per lane's pair of registers)."""
    g = np.random.default_rng(35)
    out = [(64, 129, "rand"), (0, 129, "rand"), (64, "min", "runs")]
    modes = ("rand", "runs", "last", "norepeat")
    for i in range(32):
        out.append((int(g.integers(0, 65)), "any", modes[i % 4]))
    return out


# name -> (V, T or None (= the longest input), [(S_b, T_b | "min" (= S_b + repeats) | "any", label mode)])
SPECS = {
    "S0-T1-V3-B1": (3, 1, [(0, 1, "rand")]),
    "S1-T1-V3-B1": (3, 1, [(1, 1, "rand")]),
    "S1-T2-V3-B3": (3, 2, [(1, 2, "rand"), (1, 1, "rand"), (0, 2, "rand")]),
    "S31-T70-V33-B3": (33, 70, [(31, 70, "rand"), (5, 33, "runs"), (17, 51, "last")]),
    "S31-T70-V3-B3": (3, 70, [(31, 70, "norepeat"), (20, 70, "rand"), (31, 31, "norepeat")]),
    "S32-T70-V33-B3": (33, 70, [(32, 70, "rand"), (31, 64, "rand"), (0, 9, "rand")]),
    "S63-T129-V33-B3": (33, 129, [(63, 129, "rand"), (40, 100, "runs"), (63, "min", "rand")]),
    "S64-T129-V33-B35": (33, 129, _b35()),
    "S255-T255-V33-B1": (33, 255, [(255, 255, "norepeat")]),
    "S255-Tmin-V3-B3": (3, None, [(255, "min", "rand"), (100, "min", "rand"), (64, 200, "norepeat")]),
    "same7-T70-V33-B3": (33, 70, [(20, 70, "same7"), (20, "min", "same7"), (10, 70, "last")]),
    "V4000-T40-B3": (4000, 40, [(12, 40, "last"), (7, 25, "runs"), (1, 40, "rand")]),
    "V16384-T2-B1": (16384, 2, [(1, 2, "last")]),
}
NAMES = tuple(SPECS)
CASES = tuple((n, k) for n in NAMES for k in KINDS)
CASE_IDS = [f"{n}-{k}" for n, k in CASES]


def _labels(g, mode, S, V):
    if S == 0:
        return []
    if mode == "same7":
        return [7] * S
    if mode == "norepeat":        # no two adjacent labels equal: T = S is feasible
        out = [int(g.integers(1, V))]
        while len(out) < S:
            out.append(1 + (out[-1] - 1 + int(g.integers(1, V - 1))) % (V - 1))
        return out
    if mode == "runs":            # runs of three equal labels
        vals = g.integers(1, V, size=(S + 2) // 3)
        return [int(vals[i // 3]) for i in range(S)]
    out = [int(v) for v in g.integers(1, V, size=S)]
    if mode == "last":
        out[0] = out[-1] = V - 1
    return out


def repeats(lab):
    return sum(1 for i in range(1, len(lab)) if lab[i] == lab[i - 1])


def _alignment(g, lab, Tb):
    """A random valid alignment: Tb frame classes that collapse to lab."""
    path = []
    for i, v in enumerate(lab):
        if i and lab[i - 1] == v:
            path.append(0)
        path.append(v)
    if not path:
        return [0] * Tb
    assert Tb >= len(path)
    # spread the spare frames: blanks before / between / after, or a symbol held longer
    slots = [0] * (2 * len(path) + 1)       # even: blanks around path[i]; odd: extra copies of path[i]
    for k in g.integers(0, len(slots), size=Tb - len(path)):
        slots[int(k)] += 1
    out = []
    for i, v in enumerate(path):
        out += [0] * slots[2 * i] + [v] * (1 + slots[2 * i + 1])
    return out + [0] * slots[-1]


class Case:
    def __init__(self, name, kind):
        V, T, utts = SPECS[name]
        g = np.random.default_rng(7 * sum(map(ord, name)) + KINDS.index(kind))
        labs, in_len = [], []
        for S, Tb, mode in utts:
            lab = _labels(g, mode, S, V)
            need = S + repeats(lab)
            if Tb == "min":
                Tb = max(need, 1)
            elif Tb == "any":
                Tb = int(g.integers(max(need, 1), (T or need) + 1))
            assert Tb >= need, (name, S, Tb, need)
            labs.append(lab)
            in_len.append(Tb)
        self.name, self.kind, self.V = name, kind, V
        self.B, self.T = len(utts), T if T is not None else max(in_len)
        assert max(in_len) <= self.T
        self.lab_len = [len(lab) for lab in labs]
        self.in_len = in_len
        self.S_max = max(max(self.lab_len), 1)
        self.labels = torch.zeros((self.B, self.S_max), dtype=torch.int64)
        for b, lab in enumerate(labs):
            self.labels[b, :len(lab)] = torch.tensor(lab, dtype=torch.int64)
        tg = torch.Generator().manual_seed(int(g.integers(1 << 30)))
        z = torch.randn((self.B, self.T, V), generator=tg, dtype=torch.float32)
        if kind == "trained":
            for b, lab in enumerate(labs):
                al = torch.tensor(_alignment(g, lab, in_len[b]), dtype=torch.int64)
                z[b, torch.arange(in_len[b]), al] += 8.0
        self.z32 = z
        self.lp32 = F.log_softmax(z, -1)                     # what the device is given
        self.nll64, self.g64 = torch_ctc(z.double(), self.labels, in_len, self.lab_len)
        self.nll32, self.g32 = torch_ctc(z, self.labels, in_len, self.lab_len)
        assert bool(torch.isfinite(self.nll64).all())
        self.nll_scale = float(self.nll64.abs().max())
        self.e32_loss = float((self.nll32.double() - self.nll64).abs().max())
        self.e32_grad = float((self.g32.double() - self.g64).abs().max())

    @property
    def loss_unit(self):
        return max(self.e32_loss, EPS32 * self.nll_scale)

    @property
    def grad_unit(self):
        return max(self.e32_grad, EPS32 * max(1.0, self.nll_scale))

    @property
    def loss_bound(self):
        return K_LOSS * self.loss_unit

    @property
    def grad_bound(self):
        return K_GRAD * self.grad_unit

    def concatenated(self):
        """torch's 1-D target form of the same labels."""
        return torch.cat([self.labels[b, :n] for b, n in enumerate(self.lab_len)])


@functools.lru_cache(maxsize=None)
def case(name, kind):
    return Case(name, kind)


def torch_ctc(z, labels, in_len, lab_len, reduction="sum", zero_infinity=False, grad_output=None):
    """F.log_softmax + F.ctc_loss(blank=0) on (B, T, V) logits in z's dtype ->
    (per-utterance nll (B,), the gradient at the logits of the reduced loss
    (times grad_output, per utterance for "none"))."""
    z = z.detach().clone().requires_grad_(True)
    lp = F.log_softmax(z, -1).transpose(0, 1)
    il, tl = torch.tensor(in_len, dtype=torch.int64), torch.tensor(lab_len, dtype=torch.int64)
    nll = F.ctc_loss(lp, labels, il, tl, blank=0, reduction="none", zero_infinity=zero_infinity)
    if reduction == "mean":
        out = (nll / tl.clamp(min=1).to(nll.dtype)).mean()
    else:
        out = nll if reduction == "none" else nll.sum()
    if grad_output is None:
        grad_output = torch.ones_like(out)
    out.backward(grad_output.to(out.dtype))
    return nll.detach(), z.grad


def reduce64(nll, lab_len, reduction):
    """nn.CTCLoss's reduction of per-utterance losses, in float64."""
    nll = torch.as_tensor(nll).double()
    if reduction == "mean":
        return float((nll / torch.tensor(lab_len, dtype=torch.float64).clamp(min=1)).mean())
    return float(nll.sum())


def hand_ctc(lp, labels, in_len, lab_len):
    """Float64 alpha / beta by hand on (B, T, V) log-probs, blank = 0:
        g[b,t,v] = exp(lp[b,t,v]) - exp(lse_{s: l'_s = v}(alpha_t(s) + beta_t(s)) + nll_b - lp[b,t,v]),
    0 at t >= in_len[b] -> (nll (B,), g (B, T, V))."""
    lp = lp.double()
    B, T, V = lp.shape
    ninf = float("-inf")
    nll = torch.zeros(B, dtype=torch.float64)
    g = torch.zeros_like(lp)
    for b in range(B):
        S, Tb = int(lab_len[b]), int(in_len[b])
        L = 2 * S + 1
        ext = torch.zeros(L, dtype=torch.int64)
        ext[1::2] = labels[b, :S]
        lpe = lp[b, :Tb][:, ext]
        skip_a = torch.zeros(L, dtype=torch.bool)          # alpha may come from s - 2
        skip_a[3::2] = ext[3::2] != ext[1:-2:2]
        skip_b = torch.zeros(L, dtype=torch.bool)          # beta may come from s + 2
        skip_b[1:-2:2] = ext[1:-2:2] != ext[3::2]
        pad1, pad2 = torch.full((1,), ninf, dtype=torch.float64), torch.full((2,), ninf, dtype=torch.float64)
        alpha = torch.full((Tb, L), ninf, dtype=torch.float64)
        beta = torch.full((Tb, L), ninf, dtype=torch.float64)
        alpha[0, :2] = lpe[0, :2]
        beta[Tb - 1, max(L - 2, 0):] = lpe[Tb - 1, max(L - 2, 0):]
        for t in range(1, Tb):
            p = alpha[t - 1]
            s2 = torch.where(skip_a, torch.cat([pad2, p[:-2]])[:L], pad1)
            alpha[t] = lpe[t] + torch.logsumexp(torch.stack([p, torch.cat([pad1, p[:-1]]), s2]), 0)
        for t in range(Tb - 2, -1, -1):
            p = beta[t + 1]
            s2 = torch.where(skip_b, torch.cat([p[2:], pad2])[-L:], pad1)
            beta[t] = lpe[t] + torch.logsumexp(torch.stack([p, torch.cat([p[1:], pad1]), s2]), 0)
        nll[b] = -torch.logsumexp(alpha[Tb - 1, max(L - 2, 0):], 0)
        ab = alpha + beta
        lcab = torch.full((Tb, V), ninf, dtype=torch.float64)
        for s in range(L):
            lcab[:, ext[s]] = torch.logaddexp(lcab[:, ext[s]], ab[:, s])
        g[b, :Tb] = torch.exp(lp[b, :Tb]) - torch.exp(lcab + nll[b] - lp[b, :Tb])
    return nll, g
