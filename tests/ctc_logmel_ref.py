"""References and checks for the CTC log-mel stage's parity tests (not a test
module; CPU only): csrc/wk_ctc_logmel.hip against float64.

* ``layout`` / ``batch_for``: ctc_logmel_layout restated, to choose the batch
  at which a launch deals its waves ranges of R passes.
* ``raw64`` / ``raw32``: ln(mel + 1e-8) before the z-score, float64 and
  torch-CPU fp32; ``zscore``: ctc.py:101-104 on such a map.
* ``audio``: seeded band-limited noise plus a tone, |x| <= 0.5, every utterance
  its own stream, tone and level (0 to -20 dB), cheap at 20,000 utterances.
* ``check_features``, ``check_zero_frames``, ``check_raw``, ``check_stats``:
  what tests/test_gpu_ctc_logmel.py asserts of a device result.  They take the
  result as an array, so tests/test_ctc_logmel_ref.py can hand them a result
  with a known defect and see them fail.
"""
import collections

import numpy as np
import torch

from oracle import wk_ctc_oracle as CO

HOP, N_FFT, N_MELS = CO.HOP, CO.N_FFT, CO.N_MELS
ROWS_PER_PASS, WAVES = 6, 12          # kRowsPerPass, kF2Waves (wk_ctc_logmel.hip)

FEAT_ATOL = 2e-3      # tests/test_ctc.py's feature tolerance: here only the conditioning check
KFEAT = 14.0          # tests/test_gpu_ctc_parity.py: twice the worst device / torch-CPU-fp32 ratio
FEAT_FLOOR = 1e-4     # five times the device error of profiles/ctc_parity_bounds.md (1.6e-5 to 2.0e-5)
FEAT_CAP = 2e-4       # no family constant may lift a bound above this
# The floor ln(1e-8f), correctly rounded.  The kernel's is v_log_f32(1e-8f) * ln 2
# in fp32: 1 ulp of log2 (at 26.6: 1.9e-6) and the product's rounding, so it may
# sit up to 2 ulp (3.8e-6) away; FLOOR_TOL is that.
LN_FLOOR = float(np.log(np.float64(np.float32(1e-8))))
FLOOR_TOL = 2 * float(np.spacing(np.float32(abs(LN_FLOOR))))
MEAN_RTOL = 1e-5                  # |mean - mean64| <= MEAN_RTOL |mean64 - ln 1e-8|
ISTD_FACTOR = 16 * 2.0 ** -23     # |istd std64 - 1| <= ISTD_FACTOR ms / var

Layout = collections.namedtuple("Layout", "passes grid R MS")


def frames(n_samples):
    return 1 + n_samples // HOP


def layout(n_cu, rows, T):
    """ctc_logmel_layout: passes of 6 rows, at most one 12-wave workgroup per
    CU, each wave a range of R passes, MS statistics slots per wave."""
    passes = -(-rows // ROWS_PER_PASS)
    grid = min(-(-passes // WAVES), n_cu)
    nw = grid * WAVES
    R = -(-passes // nw)
    return Layout(passes, grid, R, (ROWS_PER_PASS * R - 1) // T + 2)


def batch_for(n_cu, T, R):
    """The smallest batch whose launch has ranges of R passes."""
    B = 1 if R == 1 else (ROWS_PER_PASS * WAVES * n_cu * (R - 1)) // T + 1
    while B > 1 and layout(n_cu, (B - 1) * T, T).R >= R:
        B -= 1
    while layout(n_cu, B * T, T).R < R:
        B += 1
    return B


# ---- audio ----------------------------------------------------------------------
AUDIO_RANGE = 11.0


def _candidates(seed, chunk, B, L):
    rng = np.random.default_rng([seed, chunk, B, L])
    w = rng.standard_normal((B, L + 4))
    c = np.cumsum(w, axis=1)
    noise = (c[:, 4:] - c[:, :-4]) / 4.0 + 0.1 * w[:, 4:]     # 4-tap box (below ~4 kHz) over a -20 dB white floor
    noise /= np.abs(noise).max(axis=1, keepdims=True)
    f = rng.uniform(300.0, 3500.0, (B, 1))
    ph = rng.uniform(0.0, 2.0 * np.pi, (B, 1))
    tone = np.sin(2.0 * np.pi * f / CO.SR * np.arange(L)[None, :] + ph)
    gain = 10.0 ** (-rng.uniform(0.0, 20.0, (B, 1)) / 20.0)
    return (0.5 * gain * (0.85 * noise + 0.15 * tone)).astype(np.float32)


def _range(x):
    """Per utterance, the largest ln(frame's strongest bin / frame's weakest mel value), float64."""
    spec = torch.stft(torch.from_numpy(x).double(), n_fft=N_FFT, hop_length=HOP, win_length=N_FFT,
                      window=torch.hann_window(N_FFT, dtype=torch.float64), center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    p = spec.abs().pow(2.0).transpose(-1, -2)
    mel = torch.matmul(p, CO.mel_fbanks().double())
    return (torch.log(p.max(-1).values) - torch.log(mel.min(-1).values)).max(-1).values.numpy()


def audio(seed, B, L):
    """(B, L) float32, |x| <= 0.5: low-passed white noise (a running sum: no
    FFT) plus a tone of the utterance's own frequency and phase, every
    utterance from its own part of the stream and at its own level of 0 to
    -20 dB, so neighbours differ by up to 20 dB.
    Only well-conditioned utterances are kept, judged in float64 alone (the
    same choice on every machine): those in which no mel value lies more than
    e^AUDIO_RANGE in power (245 in amplitude) below its frame's strongest bin;
    the next candidate moves up.  An fp32 transform is a few 6e-8 of the
    strongest bin off in every bin, so ~1e-4 of such a value's amplitude at
    most.  (A reflect-padded edge frame is symmetric and its spectrum real;
    next to a sign change a one-bin mel filter holds almost no power.  Among
    20,000 utterances of two frames hundreds have such a value, where every
    fp32 transform is 1e-3 off and the bound K e32 says nothing.)"""
    kept, n, chunk = [], 0, 0
    while n < B:
        x = _candidates(seed, chunk, B // 2 + 16, L)
        x = x[_range(x) <= AUDIO_RANGE]
        kept.append(x)
        n += len(x)
        chunk += 1
        assert chunk < 64, (seed, B, L, n)
    return np.ascontiguousarray(np.concatenate(kept)[:B])


# ---- log-mel --------------------------------------------------------------------
def _logmel(x, n_samples, dtype, fbank=None):
    x = CO.pad_or_trim(torch.as_tensor(np.asarray(x)), n_samples).to(dtype)
    spec = torch.stft(x, n_fft=N_FFT, hop_length=HOP, win_length=N_FFT, window=torch.hann_window(N_FFT, dtype=dtype),
                      center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    fb = (CO.mel_fbanks() if fbank is None else fbank).to(dtype)
    return torch.log(torch.matmul(spec.abs().pow(2.0).transpose(-1, -2), fb) + 1e-8)


def raw64(x, n_samples):
    """ctc_ref.features64 without the z-score: (B, T, 80) float64."""
    return _logmel(x, n_samples, torch.float64)


def raw32(x, n_samples, fbank=None):
    """The same in torch-CPU fp32 (CO.features without the z-score)."""
    return _logmel(x, n_samples, torch.float32, fbank)


def zscore(mel):
    """ctc.py:101-104 per utterance: mean and unbiased std over the whole map,
    applied only where std > 0."""
    mean = mel.mean(dim=(1, 2), keepdim=True)
    std = mel.std(dim=(1, 2), keepdim=True)
    return torch.where(std > 0, (mel - mean) / torch.where(std > 0, std, torch.ones_like(std)), mel)


def zero_frames(x, n_samples):
    """(B, T) bool: the frames whose 400 samples, after pad / trim and the
    reflect pad, are all exactly zero -- found from the input."""
    p = CO.pad_or_trim(torch.as_tensor(np.asarray(x, np.float32)), n_samples).numpy()
    p = np.pad(p, ((0, 0), (N_FFT // 2, N_FFT // 2)), mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(p != 0, N_FFT, axis=1)[:, ::HOP]
    return ~win.any(-1)


# ---- checks ---------------------------------------------------------------------
def feature_bound(e32, k=KFEAT):
    """max(KFEAT e32, FEAT_FLOOR); a family's own constant k > KFEAT only up to FEAT_CAP."""
    b = max(KFEAT * e32, FEAT_FLOOR)
    return b if k <= KFEAT else max(b, min(k * e32, FEAT_CAP))


def _where(err):
    b, t, m = np.unravel_index(int(np.argmax(err)), err.shape)
    return f"utt={b} frame={t} mel={m}"


class Ref:
    """The float64 and torch-CPU fp32 log-mel of one input, computed once."""

    def __init__(self, x, n_samples):
        self.x, self.n_samples, self.T = x, n_samples, frames(n_samples)
        self.raw = raw64(x, n_samples)
        self.feats = zscore(self.raw)
        self.e32 = float((zscore(raw32(x, n_samples)).double() - self.feats).abs().max())
        self.std = self.raw.std(dim=(1, 2)).numpy()
        self.bound = feature_bound(self.e32)


def check_features(tag, got, ref, k=KFEAT):
    """Z-scored device features (B, T, 80) against features64:
    err <= max(k e32, FEAT_FLOOR), capped at FEAT_CAP."""
    got = torch.as_tensor(np.asarray(got)).double()
    assert got.shape == ref.feats.shape, (tuple(got.shape), tuple(ref.feats.shape))
    assert bool(torch.isfinite(got).all()), tag
    err = (got - ref.feats).abs().numpy()
    dev, bound = float(err.max()), feature_bound(ref.e32, k)
    per_utt = err.reshape(err.shape[0], -1).max(1)
    print(f"ctc-logmel {tag} B={err.shape[0]} T={ref.T} dev={dev:.3e} ref={ref.e32:.3e} ratio={dev / ref.e32:.2f} "
          f"bound={bound:.3e} worst: {_where(err)} (utterances over the bound: {int((per_utt > bound).sum())})")
    assert ref.e32 < FEAT_ATOL, (tag, ref.e32)      # else the input is ill-conditioned and proves nothing
    assert dev <= bound, (tag, dev, bound, _where(err))
    return dev


def check_zero_frames(tag, got, ref):
    """Every all-zero input frame of an utterance carries one and the same
    device value in all its mels (bit for bit).  -> the number of such frames."""
    got = np.ascontiguousarray(np.asarray(got, np.float32))
    z = zero_frames(ref.x, ref.n_samples)
    for b in range(got.shape[0]):
        v = got[b][z[b]].view(np.uint32)
        if v.size:
            bad = v != v.flat[0]
            t_bad = np.flatnonzero(z[b])[np.flatnonzero(bad.any(1))]
            assert not bad.any(), (tag, b, "frames", t_bad[:8].tolist(), float(got[b][z[b]].max()), float(got[b][z[b]].min()))
    print(f"ctc-logmel {tag} all-zero frames per utterance: {z.sum(1).tolist()}")
    return int(z.sum())


def check_raw(tag, raw, ref, k=KFEAT):
    """Un-normalised device rows (B, T, 80) against raw64: an error d there is
    d / std in the z-scored value, so utterance b's bound is the feature
    bound times its float64 std."""
    raw = torch.as_tensor(np.asarray(raw)).double()
    assert raw.shape == ref.raw.shape and bool(torch.isfinite(raw).all()), tag
    assert (ref.std > 0).all(), tag
    err = (raw - ref.raw).abs().numpy() / ref.std[:, None, None]
    dev, bound = float(err.max()), feature_bound(ref.e32, k)
    print(f"ctc-logmel {tag} raw B={err.shape[0]} T={ref.T} dev/std={dev:.3e} ref={ref.e32:.3e} ratio={dev / ref.e32:.2f} "
          f"bound={bound:.3e} worst: {_where(err)}")
    assert ref.e32 < FEAT_ATOL, (tag, ref.e32)
    assert dev <= bound, (tag, dev, bound, _where(err))
    return dev


def stats64(raw):
    """Float64 two-pass statistics of (B, T, 80) rows -> mean, unbiased std,
    and ms, the mean of (x - ln 1e-8)^2."""
    r = np.asarray(raw, np.float64).reshape(len(raw), -1)
    mean = r.mean(1)
    var = ((r - mean[:, None]) ** 2).sum(1) / (r.shape[1] - 1)
    return mean, np.sqrt(var), ((r - LN_FLOOR) ** 2).mean(1)


def check_stats(tag, zs, raw, mean_rtol=MEAN_RTOL, istd_factor=ISTD_FACTOR):
    """The device's {mean, 1/std} (B, 2) against the float64 statistics of its
    own raw rows (so the FFT's error does not enter):
        |mean - mean64| <= mean_rtol |mean64 - ln 1e-8|
        |(1/std) std64 - 1| <= istd_factor ms / var
    A pass of 6 rows lost, doubled or given to a neighbour moves the mean by
    >= 6/T of mean64 - ln 1e-8."""
    zs = np.asarray(zs, np.float64)
    mean, std, ms = stats64(raw)
    assert (std > 0).all(), tag
    rm = np.abs(zs[:, 0] - mean) / np.abs(mean - LN_FLOOR)
    rs = np.abs(zs[:, 1] * std - 1.0) / (ms / std ** 2)
    print(f"ctc-logmel {tag} stats B={len(zs)} mean ratio={rm.max() / mean_rtol:.3f} (utt {int(rm.argmax())}) "
          f"1/std ratio={rs.max() / istd_factor:.3f} (utt {int(rs.argmax())})")
    assert rm.max() <= mean_rtol, (tag, int(rm.argmax()), float(rm.max()))
    assert rs.max() <= istd_factor, (tag, int(rs.argmax()), float(rs.max()))
    return float(rm.max()), float(rs.max())
