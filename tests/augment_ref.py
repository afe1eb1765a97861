"""Reference for the tests of wk_augment_batch (not a test module; CPU only).

``reference`` states include/wakeword.h's rules for output row r = i*K + v in
numpy: Philox from ``ctc_dropout_ref.philox4x32_10``; the interpolation's
indices and weights (i0, l1, l0) in float32 exactly as the kernel forms them;
sample values, Gaussians, the two means and the scale in `dtype`: float64 is
the reference, float32 (every operation rounded on its own) is what the noise-
free rows must equal bit for bit.  ``snr_stage_torch`` is add_random_noise's
own lines (extract_mfcc.py:25-45) in torch-CPU, on a given noise and uniform
draw: in float64 it checks ``reference``'s step 4, in float32 it is the
yardstick of the device's step 4.

Bounds (``check_rows``):
  * steps 1-3 with pad noise: |out - ref64| <= ATOL_PAD = 5e-7.  A Gaussian from
    <= 4-ulp logf / sincosf with rho <= 5.77 is within 1e-5 (ATOL_GAUSS, checked
    through a pad_noise = 1, len = 0 row), so a pad sample at level 0.005 is
    within 5e-8; a blend of magnitude <= 1 has three roundings (1.8e-7); times
    1.3 and one more rounding gives 3.8e-7.
  * step 4: e = max over the case's rows of |out - ref64|, e32 the same for the
    float32 yardstick; e <= K_SNR * e32.  K_SNR is twice the largest ratio the
    kernel showed on the MI355X over every case of CASES, against the yardstick
    (profiles/augment_bounds.md).
``MUTATIONS`` are the mistakes an implementation makes; each must fail
``check_rows`` on CASES (tests/test_augment_ref.py).
"""
import collections
import functools

import numpy as np
import torch

from ctc_dropout_ref import philox4x32_10

REFERENCE_VARIANTS = ((1.0, 1.0), (0.8, 1.0), (1.2, 1.0), (1.0, 0.7), (1.0, 1.3))
# At out_len = 1 speed 0.8 resamples to int(0.8) = 0 samples, which wk_augment_batch refuses by its own rule (the
# device test asserts that); the one-sample cases run the list with 0.8 replaced by 1.25, K = 5 as everywhere.
VARIANTS_LEN1 = ((1.0, 1.0), (1.25, 1.0), (1.2, 1.0), (1.0, 0.7), (1.0, 1.3))
SNR = (0.01, 5.0, 20.0)
PAD = 0.005
ATOL_PAD = 5e-7
ATOL_GAUSS = 1e-5
K_SNR = 4.68                   # 2 x 2.34 (CASES[4]: n = 3, out_len = 257, float32 input, lengths (1, 257, 256))
SEEDS = ((0, 0), (0x9E3779B97F4A7C15, 1), (7, 2 ** 32 - 1))
MUTATIONS = ("align_corners", "streams_1_2_swapped", "stream0_by_row", "snr_db_over_10", "volume_before_pad",
             "sin_cos_swapped")

Case = collections.namedtuple("Case", "n out_len lengths i16 seed epoch variants")


def _cases():
    out, k = [], 0
    for out_len in (16000, 257, 4099, 1):
        in_len = out_len + 37
        opts = (0, 1, out_len - 1, out_len, in_len)
        for n, pick in ((3, (2, 0, 4)), (3, (1, 3, 2)), (1, (3,) if k % 2 else (4,))):
            seed, epoch = SEEDS[k % 3]
            out.append(Case(n, out_len, tuple(opts[p] for p in pick), k % 2 == 1, seed, epoch,
                            REFERENCE_VARIANTS if out_len > 1 else VARIANTS_LEN1))
            k += 1
    for out_len in (4099, 257):       # speed and volume in one variant: the pad behind the clip is multiplied too
        out.append(Case(3, out_len, (0, out_len - 1, out_len + 37), False, 7, 2 ** 32 - 1, ((0.5, 2.0),)))
    return tuple(out)


CASES = _cases()


def case_audio(c):
    """(raw (n, in_len) float32 or int16 as the device takes it, the same as float32 samples).  Amplitude 0.9:
    volume 1.3 clamps some samples."""
    in_len = c.out_len + 37
    rng = np.random.default_rng(1000 + c.out_len + 7 * c.n + c.i16)
    if c.i16:
        raw = rng.integers(-29491, 29492, size=(c.n, in_len)).astype(np.int16)
        return raw, raw.astype(np.float32) / np.float32(32768.0)
    raw = rng.uniform(-0.9, 0.9, size=(c.n, in_len)).astype(np.float32)
    return raw, raw


# ---- noise --------------------------------------------------------------------------------
def words(seed, epoch, stream, row, n_blocks):
    """Blocks 0..n_blocks-1 of a stream: (n_blocks, 4) uint32."""
    ctr = np.zeros((n_blocks, 4), np.uint64)
    ctr[:, 0] = np.arange(n_blocks, dtype=np.uint64)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = row, epoch, stream
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def gauss(seed, epoch, stream, row, n, swap=False):
    """Samples 0..n-1 of g(stream, row, .) in float64.  swap: the sin / cos mutation."""
    w = words(seed, epoch, stream, row, (n + 3) // 4).reshape(-1, 2).astype(np.float64)
    u1 = (np.floor(w[:, 0] / 256.0) + 1.0) * 2.0 ** -24
    u2 = np.floor(w[:, 1] / 256.0) * 2.0 ** -24
    rho = np.sqrt(-2.0 * np.log(u1))
    c, s = rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)
    return np.stack((s, c) if swap else (c, s), -1).reshape(-1)[:n]


def uniform(seed, epoch, row):
    """The SNR draw of a row: word 0 of block 0 of stream 3."""
    return float(int(words(seed, epoch, 3, row, 1)[0, 0]) >> 8) * 2.0 ** -24


# ---- the stages ---------------------------------------------------------------------------
def resample_plan(out_len, speed, align_corners=False):
    """(m, i0, i1, l0, l1) of step 2 for j < min(m, out_len), indices and weights in float32."""
    f = np.float32
    m = int(float(out_len) * float(f(speed)))
    j = np.arange(min(m, out_len), dtype=np.float32)
    if align_corners:
        src = j * (f(out_len - 1) / f(max(m - 1, 1)))
    else:
        scale = f(out_len) / f(m)
        src = np.maximum(scale * (j + f(0.5)) - f(0.5), f(0.0))
    i0 = np.minimum(src.astype(np.int32), out_len - 1)
    i1 = i0 + (i0 < out_len - 1)
    l1 = src - i0.astype(np.float32)
    l0 = f(1.0) - l1
    assert src.dtype == l0.dtype == l1.dtype == np.float32
    return m, i0, i1, l0, l1


def snr_stage(b, z, u, lo, hi, div=20.0):
    """Step 4 in b's dtype (float64: the reference) on noise z = snr_noise * g and draw u."""
    t = b.dtype.type
    snr = t(10.0) ** ((t(lo) + t(u) * (t(hi) - t(lo))) / t(div))
    ps, pn = np.mean(b * b, dtype=t), np.mean(z * z, dtype=t)
    if pn > 0:
        z = z * np.sqrt(ps / (pn * snr))
    return np.clip(b + z, t(-1.0), t(1.0))


def snr_stage_torch(b, z, u, lo, hi, dtype):
    """add_random_noise (extract_mfcc.py:29-45), its own lines in its own order, on a given noise and draw."""
    waveform, noise = torch.as_tensor(np.asarray(b)).to(dtype), torch.as_tensor(np.asarray(z)).to(dtype)
    snr_db = torch.tensor([u], dtype=dtype) * (hi - lo) + lo
    snr = 10 ** (snr_db / 20)
    signal_power = torch.mean(waveform ** 2)
    noise_power = torch.mean(noise ** 2)
    if noise_power > 0:
        scale_factor = torch.sqrt(signal_power / (noise_power * snr))
        noise = noise * scale_factor
    return torch.clamp(waveform + noise, -1.0, 1.0).numpy()


Rows = collections.namedtuple("Rows", "out b z u")


def reference(x, lengths, variants, pad_noise, snr, seed, epoch, out_len, dtype=np.float64, mutation=None):
    """Rows (n*K, out_len) of wk_augment_batch for float32 clips x (n, in_len).  Returns Rows(out, b = steps 1-3,
    z = snr_noise * g of step 4 (None with the stage off), u = the rows' SNR draws)."""
    assert mutation is None or mutation in MUTATIONS
    t = np.dtype(dtype).type
    f = np.float32
    x = np.asarray(x, np.float32)
    n, in_len = x.shape
    K = len(variants)
    swap = mutation == "sin_cos_swapped"
    s_pad, s_snr = (2, 1) if mutation == "streams_1_2_swapped" else (1, 2)
    pad = t(f(pad_noise))
    out, bs, zs, us = [], [], [], []
    for i in range(n):
        ln = in_len if lengths is None else min(max(int(lengths[i]), 0), in_len)
        lim = min(ln, out_len)
        for v, (speed, volume) in enumerate(variants):
            r = i * K + v
            a = np.zeros(out_len, t)
            a[:lim] = x[i, :lim]
            if pad_noise > 0:
                key_row = r if mutation == "stream0_by_row" else i
                a[lim:] = pad * gauss(seed, epoch, 0, key_row, out_len, swap).astype(t)[lim:]
            vol = t(f(volume))
            if f(speed) != f(1.0):
                m, i0, i1, l0, l1 = resample_plan(out_len, speed, mutation == "align_corners")
                b = np.zeros(out_len, t)
                if pad_noise > 0:
                    b[:] = pad * gauss(seed, epoch, s_pad, r, out_len, swap).astype(t)
                head = l0.astype(t) * a[i0] + l1.astype(t) * a[i1]
                if mutation == "volume_before_pad" and f(volume) != f(1.0):
                    head = np.clip(head * vol, t(-1.0), t(1.0))
                b[:len(head)] = head
                if mutation == "volume_before_pad":
                    vol = t(1.0)
            else:
                b = a
            if vol != t(1.0):
                b = np.clip(b * vol, t(-1.0), t(1.0))
            assert b.dtype == t
            bs.append(b)
            if snr is not None and snr[0] > 0:
                z = t(f(snr[0])) * gauss(seed, epoch, s_snr, r, out_len, swap).astype(t)
                u = uniform(seed, epoch, r)
                us.append(u)
                zs.append(z)
                out.append(snr_stage(b, z, u, f(snr[1]), f(snr[2]), 10.0 if mutation == "snr_db_over_10" else 20.0))
            else:
                out.append(b)
    return Rows(np.stack(out), np.stack(bs), np.stack(zs) if zs else None, np.asarray(us))


def yardstick(ref, snr):
    """Step 4 in torch float32 on the float64 reference's b, z and u, each rounded to float32 once."""
    return np.stack([snr_stage_torch(ref.b[r].astype(np.float32), ref.z[r].astype(np.float32), ref.u[r],
                                     float(np.float32(snr[1])), float(np.float32(snr[2])), torch.float32)
                     for r in range(ref.out.shape[0])])


# ---- the cases' references, made once and left unchanged -------------------------------------
@functools.lru_cache(maxsize=None)
def case_refs(k):
    """(quiet32: noise off in float32, pad64: steps 1-3 with pad noise, snr64: all four steps, e32: the yardstick's
    error on snr64) of CASES[k]."""
    c = CASES[k]
    _, x = case_audio(c)
    quiet = reference(x, c.lengths, c.variants, 0.0, None, c.seed, c.epoch, c.out_len, np.float32).out
    pad = reference(x, c.lengths, c.variants, PAD, None, c.seed, c.epoch, c.out_len).out
    full = reference(x, c.lengths, c.variants, PAD, SNR, c.seed, c.epoch, c.out_len)
    e32 = float(np.abs(yardstick(full, SNR).astype(np.float64) - full.out).max())
    for a in (quiet, pad, full.out):
        a.setflags(write=False)
    return quiet, pad, full.out, e32


def check_rows(k, quiet, pad, full, K=None, tag="device"):
    """The GPU checks 1-3 on CASES[k] for three outputs (any may be None: not checked): prints every figure, returns
    (failures, step 4's ratio or None)."""
    K = K_SNR if K is None else K
    q32, p64, s64, e32 = case_refs(k)
    bad, ratio = [], None
    if quiet is not None:
        same = np.array_equal(np.asarray(quiet, np.float32).view(np.uint32), q32.view(np.uint32))
        print(f"{tag} case {k} noise off: bit-equal {same}")
        if not same:
            bad.append(("noise off", k))
    if pad is not None:
        e = float(np.abs(np.asarray(pad, np.float64) - p64).max())
        print(f"{tag} case {k} pad noise: max|d| = {e:.3g} (bound {ATOL_PAD:g})")
        if not e <= ATOL_PAD:
            bad.append(("pad noise", k, e))
    if full is not None:
        e = float(np.abs(np.asarray(full, np.float64) - s64).max())
        ratio = 0.0 if e == 0.0 else (e / e32 if e32 > 0 else float("inf"))
        print(f"{tag} case {k} snr: e = {e:.3g} e32 = {e32:.3g} ratio = {ratio:.3g} (K = {K})")
        if K is not None and not ratio <= K:
            bad.append(("snr", k, ratio))
    return bad, ratio
