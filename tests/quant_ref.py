"""References for the post-training quantisation tests (not a test module).

* ``forward_int8``: the int8 network of oracle.kws_forward_int8 with every
  exponent a parameter (a spec = dict with e_in, e_w[5], e_act[6]).
* ``calib_reference``: the float64 forward of the float network with the seven
  observed tensors, their power-of-2 histograms and the exponents a percentile
  picks -- what wk_calibrate computes in fp32 on the device.
"""
import math
from fractions import Fraction

import numpy as np

from oracle import wk_oracle as O

KEYS = ("conv_layers.0.weight", "conv_layers.3.weight", "conv_layers.6.weight",
        "classifier.0.weight", "classifier.2.weight")
DEFAULT = {"e_in": -4, "e_w": [-8, -9, -9, -9, -9], "e_act": [-5, -5, -4, -5, -4, -3]}
PER_CLIP = (13 * 63, 32 * 63, 64 * 31, 128 * 15, 128, 64, 1)
E_MIN, E_MAX, N_BINS = -24, 7, 32


def as_dict(spec):
    return spec if isinstance(spec, dict) else spec.to_dict()


def shifts(spec):
    s = as_dict(spec)
    e_x = (s["e_in"], s["e_act"][0], s["e_act"][1], s["e_act"][3], s["e_act"][4])
    e_out = (s["e_act"][0], s["e_act"][1], s["e_act"][2], s["e_act"][4], s["e_act"][5])
    return [o - x - w for o, x, w in zip(e_out, e_x, s["e_w"])]


# ---- the int8 network at any spec ------------------------------------------------
def quantize_weights(sd, spec):
    """sat8(rne(w * 2^-e_w)) per tensor, int64 arrays in state-dict shapes."""
    return {k: np.clip(np.round(np.asarray(sd[k], np.float64) * 2.0 ** (-e)), -128, 127).astype(np.int64)
            for k, e in zip(KEYS, as_dict(spec)["e_w"])}


def quantize_input(feats, spec):
    """Round half away from zero, saturate (TensorBase::assign) at exponent e_in."""
    v = np.asarray(feats, np.float64) * 2.0 ** (-as_dict(spec)["e_in"])
    return np.clip(np.sign(v) * np.floor(np.abs(v) + 0.5), -128, 127).astype(np.int64)


def _rq(acc, s):
    return np.clip(np.round(acc / float(1 << s)), -128, 127).astype(np.int64)   # exact in float64; s = 0: saturate


def _rne_div(num, den):
    """round-half-even of num / den for int64 arrays num >= 0 and an int den > 0, in integers."""
    q = num // den
    r2 = 2 * (num - q * den)
    return q + ((r2 > den) | ((r2 == den) & (q % 2 == 1))).astype(np.int64)


def forward_int8_q(q_in, qw, spec):
    """q_in (B, 13, 63) int -> the int8 logit (B,) at exponent e_act[5]."""
    s = shifts(spec)
    sp = as_dict(spec)
    d = sp["e_act"][2] - sp["e_act"][3]
    x = np.asarray(q_in, np.int64)

    def conv(a, W):
        T = a.shape[-1]
        ap = np.pad(a, ((0, 0), (0, 0), (1, 1)))
        return sum(np.einsum("oc,bct->bot", W[:, :, k], ap[:, :, k:k + T]) for k in range(3))

    for key, sh in zip(KEYS[:3], s[:3]):
        x = np.maximum(_rq(conv(x, qw[key]), sh), 0)
        T = x.shape[-1] // 2
        x = np.maximum(x[..., 0:2 * T:2], x[..., 1:2 * T:2])
    tot = x.sum(-1)
    g = np.clip(_rne_div(tot << max(d, 0), 7 << max(-d, 0)), -128, 127)
    h = np.maximum(_rq(g @ qw[KEYS[3]].T, s[3]), 0)
    return _rq(h @ qw[KEYS[4]].T, s[4])[:, 0]


def forward_int8(feats, sd, spec):
    """Float features (B, 13, 63) -> float32 logits (B,), as a WK_PREC_INT8 handle at `spec` gives them."""
    q = forward_int8_q(quantize_input(feats, spec), quantize_weights(sd, spec), spec)
    return (q * 2.0 ** as_dict(spec)["e_act"][5]).astype(np.float32)


# ---- exponents and bins -------------------------------------------------------
def hold_exp_exact(a):
    """min{e : a <= 127 * 2^e} = ceil(log2(a / 127)) for a > 0, in exact rational arithmetic."""
    a = Fraction(float(a))
    e = math.frexp(float(a))[1] - 7          # a starting point; the loops settle it exactly
    while a > 127 * Fraction(2) ** e:
        e += 1
    while a <= 127 * Fraction(2) ** (e - 1):
        e -= 1
    return e


def hold_exp_bits(a):
    """The same from the float32 bit pattern (the kernel's rule), unclamped."""
    u = int(np.float32(a).view(np.uint32)) & 0x7FFFFFFF
    return (u >> 23) - 127 - (6 if (u & 0x7FFFFF) <= 0x7E0000 else 5)


def hold_exp(a):
    """Vectorised, float64 input (exact: frexp): clamped to [-24, 7], zeros lowest."""
    a = np.abs(np.asarray(a, np.float64))
    m, ex = np.frexp(a)
    e = ex - 7 + (m > 127.0 / 128.0)
    return np.where(a == 0, E_MIN, np.clip(e, E_MIN, E_MAX)).astype(np.int64)


def weight_exponents(sd):
    return [int(hold_exp(np.abs(np.asarray(sd[k], np.float32)).max())) for k in KEYS]


# ---- float64 calibration reference ----------------------------------------------
def observed_tensors(feats, sd):
    """The seven observed tensors of a float64 direct-form forward, each flattened."""
    x = np.asarray(feats, np.float64)
    out = [x.reshape(-1)]
    for key in KEYS[:3]:
        y = np.maximum(O._conv1d_k3p1(x, np.asarray(sd[key], np.float64)), 0.0)
        out.append(y.reshape(-1))
        x = O._maxpool2(y)
    g = x.mean(axis=-1)
    h = np.maximum(g @ np.asarray(sd[KEYS[3]], np.float64).T, 0.0)
    z = h @ np.asarray(sd[KEYS[4]], np.float64).T
    return out + [g.reshape(-1), h.reshape(-1), z.reshape(-1)]


def calib_reference(feats, sd, near=1e-4):
    """dict: counts (7, 32), max_abs (7,), sorted |values| per tensor, and
    near (7, 32): how many values lie within `near` relative of each bin's upper threshold 127 * 2^e."""
    tensors = [np.abs(t) for t in observed_tensors(feats, sd)]
    counts = np.zeros((7, N_BINS), np.int64)
    nearc = np.zeros((7, N_BINS), np.int64)
    for i, a in enumerate(tensors):
        counts[i] = np.bincount(hold_exp(a) - E_MIN, minlength=N_BINS)
        for b in range(N_BINS):
            thr = 127.0 * 2.0 ** (b + E_MIN)
            nearc[i, b] = int((np.abs(a - thr) <= near * thr).sum())
    return {"counts": counts, "near": nearc, "max_abs": np.array([a.max() for a in tensors]),
            "sorted": [np.sort(a) for a in tensors]}


def kth(n, percentile):
    k = n if percentile >= 100.0 else int(math.ceil(percentile / 100.0 * float(n)))
    return min(max(k, 1), n)


def spec_from_counts(counts, sd, percentile, pin_e_in=-4):
    e = []
    for i in range(7):
        cum = np.cumsum(counts[i])
        e.append(int(np.argmax(cum >= kth(int(cum[-1]), percentile))) + E_MIN)
    return {"e_in": e[0] if pin_e_in is None else pin_e_in, "e_w": weight_exponents(sd), "e_act": e[1:]}


def kth_margin(ref, percentile):
    """Per tensor, the relative distance of the reference's k-th smallest |value| from the nearest threshold
    127 * 2^e (zeros: inf -- they sit in the lowest bin whatever the rounding)."""
    out = []
    for a in ref["sorted"]:
        v = a[kth(a.size, percentile) - 1]
        if v == 0:
            out.append(math.inf)
            continue
        e = int(hold_exp(v))
        out.append(min(abs(v - 127.0 * 2.0 ** e) / v, abs(v - 127.0 * 2.0 ** (e - 1)) / v))
    return out
