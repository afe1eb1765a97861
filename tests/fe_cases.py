"""Degenerate inputs of the mode-B front-end, by construction, and their float64
references (not a test module; CPU only): tests/test_fe_cases.py and
tests/test_gpu_fe_degenerate.py.

A wake-word detector hears these all the time -- a muted microphone, a
zero-padded clip, a clipped ADC, a quiet room -- and none of them looks like the
0.1 N(0,1) noise the other GPU tests feed the kernels.

* ``CASES``: name -> 16000 float32 samples, drawn from ``default_rng(0)`` in the
  order of ``NAMES``.  ``int16_form(name)``: the same clip as int16 where every
  sample is a multiple of 1/32768 inside the int16 range (None otherwise: +1.0
  is 32768, so ``dc1``, ``fullscale_sq`` and ``impulse`` have none).
* ``Ref(x)``: the float64 figures of a batch of clips and the bound they give:
      raw64   O.mfcc_torchaudio(x)                          [B][13][63]
      f64     O.features_mode_b(x)
      s       per-row std of raw64 (ddof = 1)                [B][13]
      e_host  max|wakeword.host.mfcc(x, cmvn=False) - raw64| per clip
      eps     max(8 e_host, 16 2^-23 max|raw64|)             per clip
  The host library is an independent fp32 restatement of the same formulas
  (libm logf, its own FFT) that tests/test_host.py pins to the oracle; 8 and the
  floor are the project's own (tests/test_gpu_train.py): another summation
  order of the same arithmetic.
* The CMVN'd features divide by the row's std, so their bound is the raw bound
  carried through f = (m - mean) / s: a raw perturbation |delta| <= eps moves
  the centred value by at most 2 eps and s by at most eps sqrt(63/62), hence to
  first order
      |df| <= eps (2 + |f|) / (s + 1e-8) + 2^-22 |f|
  (the last term is the rounding of f itself), on every row with s >= eps.
  Rows below that are constant to within the raw bound: only silence has any
  (tests/test_fe_cases.py), and the convention for them is exactly 0.0.
"""
import functools

import numpy as np

from oracle import wk_oracle as O

N = 16000
K_ORDER = 8                   # tests/test_gpu_train.py
FLOOR = 16 * 2.0 ** -23       # tests/test_gpu_train.py
NAMES = ("silence", "dc0.5", "dc1", "int16_min", "fullscale_sq", "fullscale_sine1k", "quiet1lsb", "quiet1e-4",
         "quiet1e-6", "half_silence", "impulse", "noise0.1")


def _build():
    rng = np.random.default_rng(0)
    t = np.arange(N)
    c = {}
    c["silence"] = np.zeros(N)
    c["dc0.5"] = np.full(N, 0.5)
    c["dc1"] = np.full(N, 1.0)
    c["int16_min"] = np.full(N, -1.0)
    c["fullscale_sq"] = np.where((t // 20) % 2 == 0, 1.0, -1.0)
    c["fullscale_sine1k"] = np.sin(2.0 * np.pi * 1000.0 * t / 16000.0)
    c["quiet1lsb"] = rng.integers(-1, 2, size=N) / 32768.0
    c["quiet1e-4"] = 1e-4 * rng.standard_normal(N)
    c["quiet1e-6"] = 1e-6 * rng.standard_normal(N)
    c["half_silence"] = np.concatenate([0.1 * rng.standard_normal(N // 2), np.zeros(N // 2)])
    imp = np.zeros(N)
    imp[8000] = 1.0
    c["impulse"] = imp
    c["noise0.1"] = 0.1 * rng.standard_normal(N)
    assert tuple(c) == NAMES
    return {k: np.ascontiguousarray(v, np.float32) for k, v in c.items()}


CASES = _build()


def int16_form(name):
    q = CASES[name].astype(np.float64) * 32768.0
    if not np.array_equal(q, np.round(q)) or q.min() < -32768 or q.max() > 32767:
        return None
    return q.astype(np.int16)


INT16_NAMES = tuple(n for n in NAMES if int16_form(n) is not None)


class Ref:
    """The float64 figures and bounds of a batch of clips x [B][16000] (float32)."""

    def __init__(self, x):
        from wakeword import host
        x = np.ascontiguousarray(x, np.float32)
        x = x[None] if x.ndim == 1 else x
        self.x = x
        self.raw64 = O.mfcc_torchaudio(x)
        self.f64 = O.normalize_mfcc(self.raw64, "cmvn")
        self.s = self.raw64.std(axis=-1, ddof=1)
        self.host_raw = host.mfcc(x, cmvn=False)
        self.e_host = np.abs(self.host_raw - self.raw64).max(axis=(1, 2))
        self.eps = np.maximum(K_ORDER * self.e_host, FLOOR * np.abs(self.raw64).max(axis=(1, 2)))
        self.kept = self.s >= self.eps[:, None]                                # rows the CMVN comparison keeps

    def cmvn_bound(self):
        """The per-element bound of the module docstring, [B][13][63]."""
        a = np.abs(self.f64)
        return self.eps[:, None, None] * (2.0 + a) / (self.s[:, :, None] + 1e-8) + 2.0 ** -22 * a

    def cmvn_ratio(self, got):
        """max over the kept rows of |got - f64| / bound, per clip (0 where no row is kept)."""
        r = np.abs(np.asarray(got, np.float64) - self.f64) / self.cmvn_bound()
        r = np.where(self.kept[:, :, None], r, 0.0)
        return r.max(axis=(1, 2))

    def cmvn_err(self, got):
        """max over the kept rows of |got - f64|, per clip."""
        e = np.where(self.kept[:, :, None], np.abs(np.asarray(got, np.float64) - self.f64), 0.0)
        return e.max(axis=(1, 2))


@functools.lru_cache(maxsize=None)
def ref():
    """The Ref of the 12 cases, in NAMES order."""
    return Ref(np.stack([CASES[n] for n in NAMES]))


# ---- the fp32 reduction of the device's CMVN --------------------------------------
def wave_sum32(v):
    """wk_common.h wave_sum in numpy float32: the DPP butterflies inside each
    16-lane row (quad_perm xor 1, xor 2, row_half_mirror, row_mirror), then
    (r0 + r1) + (r2 + r3) of the four row sums.  v [..., 64]."""
    v = np.asarray(v, np.float32)
    i = np.arange(64)
    for src in (i ^ 1, i ^ 2, (i & ~7) | (7 - (i & 7)), (i & ~15) | (15 - (i & 15))):
        v = (v + v[..., src]).astype(np.float32)
    return ((v[..., 0] + v[..., 16]).astype(np.float32) + (v[..., 32] + v[..., 48]).astype(np.float32)).astype(np.float32)


def cmvn_lane32(v, n=63, flat_rule=True):
    """cmvn_lane (wk_fe_dev.h) on rows v [..., 63] in numpy float32, one lane
    per frame and a zero 64th lane.  flat_rule: a row of equal values is taken
    as a row of zeros (cmvn_row_is_flat); False is the kernel before that rule."""
    f32 = np.float32
    v = np.asarray(v, f32)
    if flat_rule:
        v = np.where((v == v[..., :1]).all(axis=-1, keepdims=True), f32(0.0), v)
    lanes = np.zeros(v.shape[:-1] + (64,), f32)
    lanes[..., :n] = v
    mean = (wave_sum32(lanes) / f32(n)).astype(f32)
    d = (lanes - mean[..., None]).astype(f32)
    d[..., n:] = 0
    sd = np.sqrt((wave_sum32((d * d).astype(f32)) / f32(n - 1)).astype(f32)).astype(f32)
    sd = np.where(sd == 0, f32(1.0), sd)
    return (d * (f32(1.0) / (sd + f32(1e-8)))[..., None]).astype(f32)[..., :n]


def neighbours32(v, k=50):
    """The 2k + 1 float32 values within k ulps of v."""
    b = np.array([v], np.float32).view(np.int32)[0]
    return (b + np.arange(-k, k + 1, dtype=np.int32)).astype(np.int32).view(np.float32)
