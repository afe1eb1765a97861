"""Cases and float64 references for the inference CNN (not a test module; CPU only):
the CNN role of wk_fused_kernel / wk_cnn_fused_kernel in fp32 (Winograd F(2,3)),
bf16 and split bf16, tests/test_gpu_cnn_parity.py.

* ``forward64``: LightweightKWS.forward (ml_models/src/wakeModel.py:4-34) in
  float64.  ``forward32`` is the same network in fp32 with one of three
  convolutions -- F.conv1d, a tap-by-tap sum, and a restatement of the kernel's
  Winograd F(2,3) (wk_cnn_dev.h: G1 = (g0 + g1 + g2) / 2 packed by the host,
  G2 = (g0 + g2) - G1) -- three summation orders of the same arithmetic.
* ``unit32`` = max(max over the three of max|z32 - z64|, 16 * 2^-23 * max|z64|)
  is the yardstick of every bound; it comes from the reference alone.
* ``emul_bf16`` / ``emul_bf16x3``: the network with the kernels' roundings -- the
  conv weights and each conv's input activations rounded to nearest even to
  bf16 (wk_kernels.h to_bf16_rne, wk_cnn_dev.h bf16_bits); conv3's output, the
  pooled mean and the classifier stay unrounded -- in float64 or in fp32.  In
  float64 the rounding is done on the bf16 grid (``bf16_grid``).  The split
  form takes xh = bf16(x), xl = bf16(x - xh) of activations and weights and the
  products xh wh + xl wh + xh wl (xl wl is dropped, conv_pair_bf3).
* ``Ref(W, x)``: every per-clip figure of one (weights, features) pair, computed
  once; ``ref(name, kind)`` is the cached one of a seeded feature kind, and a
  batch of B clips is its prefix ``[:B]``.
* The bounds (``check``), u = unit32 of the batch:
      fp32     max|z_dev - z64|        <= 8 u
      bf16x3   max|z_dev - z_emul3_64| <= 8 max(u, max|z_emul3_32 - z_emul3_64|)
      bf16     every clip |z_dev - z_emul_64| <= 0.25 Q, Q = max|z_emul_64 - z64|
               (over the batch if B >= 1024, else over the 1024-clip seeded set
               whose prefix it is), and for B >= 1024 at most 5 % of the clips
               above 8 u
  8 is this project's factor for another summation order of the same arithmetic
  (tests/test_gpu_train.py).  bf16 needs the two-part form because a rounding
  that falls the other way in fp32 than in float64 moves a logit by a bf16 ulp
  of one activation: the fp32 emulation itself has 1 to 2 % of its clips above
  8 u and reaches 0.06 to 0.10 Q; tests/test_cnn_ref.py holds the reference to
  the two caps.
* ``probe_set(j)``: one-hot weights with which every precision is exact.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from test_gpu_train import KEYS, weight_set as _trained_sets

WEIGHT_SETS = ("xiaoa", "default")
PRECISIONS = ("fp32", "bf16", "bf16x3")
KINDS = ("normal", "wide", "impulse")
CONVS = ("conv1d", "taps", "wino")
K_ORDER = 8                  # another summation order of the same arithmetic (test_gpu_train.py)
FLOOR = 16 * 2.0 ** -23
SHARE_CAP = 0.05             # bf16: clips above K_ORDER u
Q_CAP = 0.25                 # bf16: every clip, in units of the quantisation effect Q
Q_SET = 1024                 # bf16 at small B: Q is taken over this many clips of the seeded set
SEEDS = {"normal": 4101, "wide": 4102, "impulse": 4103}
IMPULSE_C = (0, 11, 12)      # 12: the image row's 13th element, written on its own; conv1's K padding follows it
IMPULSE_T = (0, 1, 30, 31, 32, 60, 61, 62)   # 0: the zero left pad; 62 reaches output 61 only


def weight_set(name):
    """name -> {key: float32 torch tensor}: "xiaoa" (tests/golden/xiaoa.onnx) or
    "default" (wakeword.train.default_init(seed=11))."""
    return {k: torch.from_numpy(v) for k, v in _trained_sets(name).items()}


# ---- batch sizes ------------------------------------------------------------
# launch_fused (wk_fused.hip; launch_fused_as, wk_fused_dev.h): grid = min(B, n_cu) workgroups; workgroup w takes
# clips w, w + grid, ... (n_mine = (B - 1 - w) / grid + 1) in batches of NBF = 4.
# With C = n_cu, 4C + 1 gives workgroup 0 a second batch of nv = 1 beside
# single-batch workgroups; 5C + 3: nv = 2 (w < 3) and 1; 6C + C/2: nv = 3 and 2;
# 9C + 7: a third batch of nv = 2 (w < 7) and 1 after two whole ones.
def sizes_fused(C):
    return (4 * C + 1, 5 * C + 3, 6 * C + C // 2, 9 * C + 7)


# launch_cnn_fused: roles = ceil(B / 4), grid = min(ceil(roles / 2), n_cu)
# workgroups of two CNN roles; role r = 2 * block + {0, 1} takes clips r,
# r + 2 grid, ...  B = 1: the second role of the only workgroup has n_mine = 0;
# 2 to 4: both roles, nv = 1 or 2; 5 to 8: nv up to 4 in one batch; 9: two
# workgroups, the last role with one clip.  Second batches need B > 8C:
# 8C + 1 (nv = 1 in one role), 10C + 3 (nv = 2 and 1), 15C (nv = 4 and 3).
def sizes_cnn(C):
    return (1, 2, 3, 4, 5, 7, 8, 9, 8 * C + 1, 10 * C + 3, 15 * C)


# ---- features ----------------------------------------------------------------
def features(kind, n):
    """Seeded [n][13][63] fp32 features; clip i does not depend on n for
    "impulse", and for the random kinds batches are cut from one call."""
    if kind == "impulse":
        x = torch.zeros(n, 13, 63)
        i = torch.arange(n)
        nt = len(IMPULSE_T)
        x[i, torch.tensor(IMPULSE_C)[(i // nt) % len(IMPULSE_C)], torch.tensor(IMPULSE_T)[i % nt]] = 1.0
        return x
    g = torch.Generator().manual_seed(SEEDS[kind])
    x = torch.randn(n, 13, 63, generator=g)
    return x * 8.0 if kind == "wide" else x      # CMVN'd values reach +-sqrt(62)


# ---- roundings ---------------------------------------------------------------
def bf16_grid(x):
    """Round to nearest even onto the bf16 grid (8 significant bits), keeping the
    dtype: frexp, round half to even at 8 bits, ldexp.  On fp32 inputs (normal
    range) bit-equal to x.bfloat16()."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)     # torch.round: half to even


def bf16_trunc(x):
    """The mutant rounding: toward zero at 8 bits."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.trunc(m * 256.0) / 256.0, e)


def bf16_torch(x):
    return x.bfloat16().to(x.dtype)


def split_bf16(x, rnd):
    h = rnd(x)
    return h, rnd(x - h)


# ---- convolutions (k = 3, padding 1, no bias) ----------------------------------
def conv_conv1d(h, w):
    return F.conv1d(h, w, padding=1)


def conv_taps(h, w):
    hp = F.pad(h, (1, 1))
    T = h.shape[2]
    out = 0
    for k in (2, 0, 1):
        out = out + torch.einsum("oc,bct->bot", w[:, :, k], hp[:, :, k:k + T])
    return out


def conv_wino(h, w):
    """wk_cnn_dev.h conv_wino_v / epi_wino_pool: per output pair (2p, 2p + 1)
    from input rows d_r = x[2p - 1 + r]."""
    T = h.shape[2]
    P = (T + 1) // 2
    hp = F.pad(h, (1, 2))
    d = [hp[:, :, r:r + 2 * P:2] for r in range(4)]
    g0, g1, g2 = w[:, :, 0], w[:, :, 1], w[:, :, 2]
    G1 = (0.5 * (g0.double() + g1.double() + g2.double())).to(w.dtype)   # pack_fragments (wk_kernels.h)
    G2 = (g0 + g2) - G1

    def mm(g, x):
        return torch.einsum("oc,bct->bot", g, x)
    m0, m1, m2, m3 = mm(g0, d[0] - d[2]), mm(G1, d[1] + d[2]), mm(G2, d[2] - d[1]), mm(g2, d[1] - d[3])
    y = torch.stack([m0 + m1 + m2, m1 - m2 - m3], dim=3).reshape(h.shape[0], w.shape[0], 2 * P)
    return y[:, :, :T]


_CONV = {"conv1d": conv_conv1d, "taps": conv_taps, "wino": conv_wino}


def gap(h):
    """maxpool(2) (floor) of conv3's ReLU'd output and the mean over time."""
    return F.max_pool1d(h, 2).mean(dim=2)


def network(x, W, conv=conv_conv1d, rnd=None, split=False, drop=None, conv_of=None, gap_fn=gap):
    """LightweightKWS.forward -> logits (B,) in x's dtype.  rnd: the rounding of
    each conv's weights and input (None: none); split: the xh / xl form; drop:
    the layer whose xl wh product is left out (a mutant); conv_of(layer) ->
    convolution, gap_fn: for mutants."""
    W = {k: v.to(x.dtype) for k, v in W.items()}
    h = x
    for layer, k in enumerate(KEYS[:3]):
        c = conv_of(layer) if conv_of else conv
        w = W[k]
        if split:
            xh, xl = split_bf16(h, rnd)
            wh, wl = split_bf16(w, rnd)
            y = c(xh, wl) if drop == layer else c(xh, wl) + c(xl, wh)
            y = y + c(xh, wh)
        else:
            y = c(rnd(h), rnd(w)) if rnd else c(h, w)
        y = F.relu(y)
        h = F.max_pool1d(y, 2) if layer < 2 else gap_fn(y)
    return F.linear(F.relu(F.linear(h, W[KEYS[3]])), W[KEYS[4]])[:, 0]


def forward64(x, W):
    with torch.no_grad():
        return network(x.double(), W)


def forward32(x, W, conv="conv1d"):
    with torch.no_grad():
        return network(x.float(), W, _CONV[conv])


def _rnd(dtype):
    return bf16_grid if dtype == torch.float64 else bf16_torch


def emul_bf16(x, W, dtype, conv="conv1d"):
    with torch.no_grad():
        return network(x.to(dtype), W, _CONV[conv], rnd=_rnd(dtype))


def emul_bf16x3(x, W, dtype, conv="conv1d"):
    with torch.no_grad():
        return network(x.to(dtype), W, _CONV[conv], rnd=_rnd(dtype), split=True)


# ---- per-clip reference figures -----------------------------------------------
class Ref:
    """Everything the bounds need for one (weights, features) pair, per clip."""

    def __init__(self, W, x):
        x = x.detach().cpu().float().contiguous()
        self.n = x.shape[0]
        self.z64 = forward64(x, W)
        self.zb64 = emul_bf16(x, W, torch.float64)
        self.z3_64 = emul_bf16x3(x, W, torch.float64)
        # per-clip error of each summation order: fp32, and the fp32 emulations
        self.e32 = {c: (forward32(x, W, c).double() - self.z64).abs() for c in CONVS}
        self.eb32 = {c: (emul_bf16(x, W, torch.float32, c).double() - self.zb64).abs() for c in CONVS}
        self.e3_32 = {c: (emul_bf16x3(x, W, torch.float32, c).double() - self.z3_64).abs() for c in CONVS[:2]}

    def unit32(self, B=None):
        B = self.n if B is None else B
        e = max(float(v[:B].max()) for v in self.e32.values())
        return max(e, FLOOR * float(self.z64[:B].abs().max()))

    def unit3(self, B=None):
        B = self.n if B is None else B
        return max(self.unit32(B), max(float(v[:B].max()) for v in self.e3_32.values()))

    def q(self, B=None):
        """The bf16 quantisation effect the batch is measured in."""
        B = self.n if B is None else B
        n = B if B >= Q_SET else min(Q_SET, self.n)
        return float((self.zb64[:n] - self.z64[:n]).abs().max())

    def target(self, precision):
        return {"fp32": self.z64, "bf16": self.zb64, "bf16x3": self.z3_64}[precision]


@functools.lru_cache(maxsize=None)
def _ref(name, kind, n):
    return Ref(weight_set(name), features(kind, n))


def ref(name, kind, n):
    """The cached Ref of features(kind, n'), n' >= max(n, Q_SET) (impulse: n)."""
    if kind != "impulse":
        n = max(n, Q_SET)
    return _ref(name, kind, n)


def check(tag, precision, z_dev, r, B=None, rows=None):
    """Print the device's figures against the units of Ref r's first B clips,
    then assert the bounds of the module docstring.  rows: a list that receives
    the table row (profiles/cnn_parity_bounds.md)."""
    B = r.n if B is None else B
    z = torch.as_tensor(z_dev).detach().cpu().double().reshape(-1)
    assert z.shape[0] == B and bool(torch.isfinite(z).all()), (tag, z.shape, B)
    e = (z - r.target(precision)[:B]).abs()
    u = r.unit32(B)
    if precision == "fp32":
        unit, bound = u, K_ORDER * u
        row = f"{tag} {precision} B={B}: e_dev={float(e.max()):.3e} u={u:.3e} e_dev/u={float(e.max()) / u:.2f}"
        bad = not float(e.max()) <= bound
    elif precision == "bf16x3":
        unit = r.unit3(B)
        row = (f"{tag} {precision} B={B}: e_dev={float(e.max()):.3e} u={u:.3e} u3={unit:.3e} "
               f"e_dev/u3={float(e.max()) / unit:.2f}")
        bad = not float(e.max()) <= K_ORDER * unit
    else:
        Q = r.q(B)
        share = float((e > K_ORDER * u).double().mean())
        row = (f"{tag} {precision} B={B}: e_dev max={float(e.max()):.3e} median={float(e.median()):.3e} u={u:.3e} "
               f"Q={Q:.3e} max/Q={float(e.max()) / Q:.3f} share(>8u)={share:.4f}")
        bad = not float(e.max()) <= Q_CAP * Q or (B >= Q_SET and not share <= SHARE_CAP)
    print(row)
    if rows is not None:
        rows.append(row)
    assert not bad, row


# ---- the exact probe -------------------------------------------------------------
PROBE_SHAPES = ((32, 13), (64, 32), (128, 64))      # (cout, cin) of the three convs
PROBE_SEED = 9400         # chosen so that every PROBE_POINTS impulse reaches a pooled channel (test_cnn_ref.py)
PROBE_N = 64 + 3          # terms of the standard summation bound: classifier.2's 64 and its 3 butterfly adds


def _probe_layout(j):
    """Per conv layer, for each output channel its one (ci, tap, weight).
    conv1: 39 (ci, tap) pairs over the 4 x 32 output channels of j = 0..3 in a
    seeded order, each pair's first use positive.  conv2 / conv3 (cout = 2 cin):
    every ci is read twice in each j: by one of the first cin output channels at
    a seeded tap, a quarter of them with weight < 0, and by one of the others at
    tap 2 with weight > 0 (frame 62 reaches the pooled features through tap 2
    of every layer only).  Magnitudes 1 and 0.5."""
    g = np.random.default_rng(9000)
    perm39 = g.permutation(39)
    out = []
    s = j * 32 + np.arange(32)
    pair = perm39[s % 39]
    sign = np.where((s // 39) % 2 == 0, 1.0, -1.0)
    mag = np.where(g.integers(0, 2, size=128)[s] == 0, 1.0, 0.5)
    out.append((pair // 3, pair % 3, sign * mag))
    for layer, (cout, cin) in enumerate(PROBE_SHAPES[1:], 1):
        gj = np.random.default_rng(PROBE_SEED + 10 * layer + j)
        ci = np.concatenate([gj.permutation(cin), gj.permutation(cin)])
        tap = np.concatenate([gj.integers(0, 3, size=cin), np.full(cin, 2)])
        sign = np.concatenate([np.where(gj.integers(0, 4, size=cin) == 0, -1.0, 1.0), np.ones(cin)])
        mag = np.where(gj.integers(0, 2, size=cout) == 0, 1.0, 0.5)
        out.append((ci, tap, sign * mag))
    return out


def probe_set(j, watch=None):
    """One-hot weights: with integer features in [-8, 8] every conv output is
    a small dyadic number (|k| / 8, |k| <= 64), exact in fp32, in Winograd's
    transforms and in bf16 (so xl = 0), and the pooled sums are exact.
    classifier.0 selects one pooled channel per output with weight 1 (256 slots
    over j = 0..3 cover the 128 channels twice); classifier.2 is +-2^k.
    watch = ch: classifier.0's output 0 selects pooled channel ch and
    classifier.2 is (1, 0, ..., 0): the logit is relu(h[ch]) itself."""
    W = {}
    for key, (cout, cin), (ci, tap, val) in zip(KEYS[:3], PROBE_SHAPES, _probe_layout(j)):
        w = np.zeros((cout, cin, 3), np.float32)
        w[np.arange(cout), ci, tap] = val
        W[key] = torch.from_numpy(w)
    g = np.random.default_rng(9200)
    sel = g.permutation(128)[(j * 64 + np.arange(64)) % 128]
    w2 = np.where(g.integers(0, 2, size=64) == 0, 1.0, -1.0) * 2.0 ** g.integers(-3, 4, size=64)
    if watch is not None:
        sel[0] = watch
        w2 = np.zeros(64)
        w2[0] = 1.0
    f1 = np.zeros((64, 128), np.float32)
    f1[np.arange(64), sel] = 1.0
    W[KEYS[3]] = torch.from_numpy(f1)
    W[KEYS[4]] = torch.from_numpy(w2.astype(np.float32).reshape(1, 64))
    return W


def probe_features(n, seed=77):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (n, 13, 63), generator=g).float()


def probe_pooled(x, W):
    """Exact pooled sums s [B][128] (float64) of conv3's ReLU'd, max-pooled output."""
    x = x.double()
    h = x
    for layer, k in enumerate(KEYS[:3]):
        h = F.max_pool1d(F.relu(F.conv1d(h, W[k].double(), padding=1)), 2)
        if layer == 2:
            return h.sum(dim=2)


def probe_expect(x, W):
    """-> (h [B][128] fp32 = fp32(s * fp32(1/7)) as epi_gap / epi_wino_gap form it,
    logits64 [B], bound [B] = PROBE_N 2^-24 sum|w h|)."""
    s = probe_pooled(x, W)
    s32 = s.float()
    assert bool((s32.double() == s).all())
    h = (s32.numpy() * np.float32(1.0 / 7.0)).astype(np.float32)
    h64 = torch.from_numpy(h).double()
    hid = F.relu(F.linear(h64, W[KEYS[3]].double()))
    w2 = W[KEYS[4]].double()[0]
    z = hid @ w2
    bound = PROBE_N * 2.0 ** -24 * (hid * w2.abs()).sum(dim=1)
    return torch.from_numpy(h), z, bound


def impulse_clip(c, t):
    x = torch.zeros(13, 63)
    x[c, t] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def probe_reach(c, t):
    """(j, ch): the first probe set and pooled channel that a single 1 at
    (c, t) of an otherwise zero clip reaches (None if none)."""
    for j in range(4):
        s = probe_pooled(impulse_clip(c, t)[None], probe_set(j))[0]
        nz = torch.nonzero(s).flatten()
        if nz.numel():
            return j, int(nz[0])
    return None


PROBE_POINTS = tuple((c, t) for c in IMPULSE_C for t in (0, 1, 31, 62))
