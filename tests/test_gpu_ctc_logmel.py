"""The CTC log-mel stage (csrc/wk_ctc_logmel.hip: ctc_logmel_fft2_kernel,
ctc_zscore_kernel, ctc_zstats_kernel) against float64 where it can go wrong:
ranges of more than one 6-row pass per wave (R = 2, 3) down to T = 2, ragged
last passes and dead partner rows, strided and trimmed batches through the raw
ABI, zero padding at synth level and at int16 scale (an all-zero frame sharing
a complex FFT with a loud one), and, through wk_ctc_transcribe_stats, the
un-normalised rows and the fused {mean, 1/std} of the fp16 one-call path.

Bounds (tests/ctc_logmel_ref.py): z-scored features within
max(KFEAT e32, FEAT_FLOOR) of features64, e32 being torch-CPU fp32's error on
the same input; raw rows within that times the utterance's float64 std; the
statistics against the float64 statistics of the device's own rows.  Measured
figures: profiles/ctc_parity_bounds.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ctc_logmel_ref as LR
from oracle import wk_ctc_oracle as CO
from oracle import wk_oracle as O

pytestmark = pytest.mark.gpu
V = 512


@functools.lru_cache(maxsize=None)
def handle(precision):
    import wakeword
    return wakeword.CTCModel(CO.flat_weights(CO.make_model(V, seed=7)), V, precision=precision)


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    yield
    handle.cache_clear()
    padded_ref.cache_clear()


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def n_samples_for(T):
    """201, 320, 480, ...: the fewest samples the reflect pad takes at T = 2, then 160 (T - 1)."""
    return 201 if T == 2 else LR.HOP * (T - 1)


# ---- a. ranges and small T ---------------------------------------------------------
RANGE_CASES = [(2, T) for T in (2, 3, 4, 5, 6, 7, 13)] + [(3, 2), (3, 7)]
RAGGED_CASES = [(1, 2), (2, 2), (3, 3), (1, 5), (1, 7), (5, 7), (1, 13)]       # rows mod 6: 2, 4, 3, 5, 1, 5, 1


@pytest.mark.parametrize("R,T", RANGE_CASES, ids=[f"R{r}-T{t}" for r, t in RANGE_CASES])
def test_features_in_ranges_of_several_passes(gpu, R, T):
    """Every utterance of the smallest batch whose waves take R passes each: at
    T < 6 the utterance-advance loops step more than once per pass, at
    6 <= T <= 11 every range starts mid-utterance."""
    B, n = LR.batch_for(n_cu(), T, R), n_samples_for(T)
    assert LR.frames(n) == T and LR.layout(n_cu(), B * T, T).R == R
    x = LR.audio(100 * R + T, B, n)
    got = handle("fp32").features(x, n_samples=n).cpu().numpy()
    LR.check_features(f"R={R}", got, LR.Ref(x, n))


@pytest.mark.parametrize("B,T", RAGGED_CASES, ids=[f"B{b}-T{t}" for b, t in RAGGED_CASES])
def test_features_ragged_last_pass(gpu, B, T):
    """R = 1 with a last pass of 1 to 5 rows; with an odd row count the last
    live row shares its FFT with a dead one."""
    n = n_samples_for(T)
    assert LR.frames(n) == T and LR.layout(n_cu(), B * T, T).R == 1 and (B * T) % 6 != 0
    x = LR.audio(7 * B + T, B, n)
    got = handle("fp32").features(x, n_samples=n).cpu().numpy()
    LR.check_features(f"ragged rows%6={(B * T) % 6}", got, LR.Ref(x, n))


# ---- b. stride and trim through the raw ABI ------------------------------------------
def raw_features(buf, batch, n_valid, n_samples, stride):
    from wakeword._lib import check, lib
    g = handle("fp32")
    out = torch.empty((batch, LR.frames(n_samples), 80), dtype=torch.float32, device=buf.device)
    check(lib().wk_ctc_features(g._h, C.c_void_p(buf.data_ptr()), batch, n_valid, n_samples, stride,
                                C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(0).cuda_stream)),
          "wk_ctc_features")
    return out.cpu().numpy()


def strided(x, stride):
    """x's rows `stride` apart in one device buffer, 1e30 in between."""
    B, L = x.shape
    buf = torch.full((B * stride,), 1e30, dtype=torch.float32)
    buf.view(B, stride)[:, :L] = torch.from_numpy(x)
    return buf.cuda()


@pytest.mark.parametrize("n_valid,n_samples", [(1920, 1920), (60000, 48000)], ids=["stride", "trim"])
def test_strided_batch_is_bit_identical_to_contiguous(gpu, n_valid, n_samples):
    """stride = n_valid + 3: rows off 16-byte alignment, with values between
    them that must not be read.  With n_valid > n_samples the rows are also
    trimmed: the same bits as the pre-trimmed contiguous batch."""
    B = 7
    x = LR.audio(31, B, n_valid)
    got = raw_features(strided(x, n_valid + 3), B, n_valid, n_samples, n_valid + 3)
    keep = min(n_valid, n_samples)
    want = raw_features(torch.from_numpy(np.ascontiguousarray(x[:, :keep])).cuda(), B, keep, n_samples, keep)
    assert np.isfinite(got).all() and np.abs(got).max() < 100.0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    LR.check_features(f"stride n_valid={n_valid}", got, LR.Ref(x, n_samples))


def test_zero_valid_samples_give_the_floor(gpu):
    """n_valid = 0: every sample is padding, every value ln(1e-8f), left
    un-normalised (std 0); the audio buffer is not read."""
    got = raw_features(torch.full((8,), 1e30, dtype=torch.float32).cuda(), 3, 0, 1920, 0)
    bits = got.view(np.uint32)
    print(f"ctc-logmel floor: device {got.flat[0]!r} ln(1e-8f) {np.float32(LR.LN_FLOOR)!r}")
    assert (bits == bits.flat[0]).all()
    assert abs(float(got.flat[0]) - LR.LN_FLOOR) <= LR.FLOOR_TOL


# ---- c. padding at both levels ---------------------------------------------------------
PAD_CASES = [(amp, nv, 48000, 5) for amp in (1.0, 32768.0) for nv in (30000, 30080)] + [(32768.0, 1000, 1920, 6)]
PAD_IDS = [f"amp{a:g}-{nv}of{n}" for a, nv, n, _ in PAD_CASES]


def padded_audio(amp, n_valid, B):
    return (O.synth_clips(11, 0, B, n_valid) * np.float32(amp)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def padded_ref(amp, n_valid, n_samples, B):
    return LR.Ref(padded_audio(amp, n_valid, B), n_samples)


@pytest.mark.parametrize("amp,n_valid,n_samples,B", PAD_CASES, ids=PAD_IDS)
def test_zero_padded_utterances(gpu, amp, n_valid, n_samples, B):
    """Short utterances zero-padded to n_samples, at synth level and as
    int16-valued floats.  The first all-zero frame is 189 or 190 (8 at
    n_valid = 1000), so over b = 0..4 it falls on both row parities, and with
    T odd the zero tail of an even utterance shares an FFT with the head of
    the next.  The float64 reference gives the floor ln(1e-8) in such a frame;
    so must the device: every value of the utterance's all-zero frames equal."""
    ref = padded_ref(amp, n_valid, n_samples, B)
    got = handle("fp32").features(ref.x, n_samples=n_samples).cpu().numpy()
    nz = LR.check_zero_frames(f"pad amp={amp:g} n_valid={n_valid}", got, ref)
    assert nz >= B * (ref.T - 2 - n_valid // 160)
    LR.check_features(f"pad amp={amp:g} n_valid={n_valid}", got, ref)


# ---- d. un-normalised rows and fused statistics -----------------------------------------
def one_call(x, n_samples):
    """decode_audio on the fp16 handle, then the read-back -> (zs, raw) arrays."""
    g = handle("fp16")
    B, T = x.shape[0], LR.frames(n_samples)
    g.decode_audio(x, n_samples=n_samples)
    zs, raw = g.transcribe_stats(B, T, return_raw=True)
    return zs.cpu().numpy(), raw.cpu().numpy()


STATS_CASES = [(1, 35, T) for T in (6, 7, 8, 11, 13)] + [(2, None, 7), (3, None, 7), (1, 7, 301)]


@pytest.mark.parametrize("R,B,T", STATS_CASES, ids=[f"R{r}-T{t}" for r, _, t in STATS_CASES])
def test_raw_rows_and_fused_statistics(gpu, R, B, T):
    """The fused path's raw rows against raw64 and its {mean, 1/std} against
    the float64 statistics of those rows, where passes straddle utterances in
    every pattern (T = 6 to 13), in ranges of 2 and 3 passes, and at T = 301."""
    if B is None:
        B = LR.batch_for(n_cu(), T, R)
    n = n_samples_for(T)
    assert LR.frames(n) == T and LR.layout(n_cu(), B * T, T).R == R
    x = LR.audio(1000 * R + T, B, n)
    zs, raw = one_call(x, n)
    LR.check_raw(f"R={R}", raw, LR.Ref(x, n))
    LR.check_stats(f"R={R} T={T}", zs, raw)


@pytest.mark.parametrize("amp,n_valid,n_samples,B", [PAD_CASES[2], PAD_CASES[4]], ids=[PAD_IDS[2], PAD_IDS[4]])
def test_raw_rows_and_fused_statistics_padded(gpu, amp, n_valid, n_samples, B):
    """The same on the int16-scaled zero-padded utterances: the all-zero frames
    are exactly the floor and add exactly 0 to the partial sums."""
    ref = padded_ref(amp, n_valid, n_samples, B)
    zs, raw = one_call(ref.x, n_samples)
    z = LR.zero_frames(ref.x, n_samples)
    floor = raw[z]
    assert floor.size and (floor.view(np.uint32) == floor.view(np.uint32).flat[0]).all()
    assert abs(float(floor.flat[0]) - LR.LN_FLOOR) <= LR.FLOOR_TOL
    LR.check_raw(f"pad amp={amp:g} n_valid={n_valid}", raw, ref)
    LR.check_stats(f"pad amp={amp:g} n_valid={n_valid}", zs, raw)


# ---- e. constant utterances ------------------------------------------------------------
def test_silent_utterances_through_the_read_back(gpu):
    """Digital silence: zs == (0, 1) exactly, every raw value the floor's bits."""
    zs, raw = one_call(np.zeros((4, 8000), np.float32), 8000)
    assert np.array_equal(zs, np.tile(np.float32([0.0, 1.0]), (4, 1)))
    bits = raw.view(np.uint32)
    assert (bits == bits.flat[0]).all() and abs(float(raw.flat[0]) - LR.LN_FLOOR) <= LR.FLOOR_TOL


def test_dc_utterances_through_the_read_back(gpu):
    """A DC offset: the variance is within the partials' rounding, so the
    statistics come from the exact two-pass fallback -- 1e-6 relative to the
    float64 statistics of the device's own rows."""
    zs, raw = one_call(np.full((4, 8000), 0.25, np.float32), 8000)
    mean, std, _ = LR.stats64(raw)
    print(f"ctc-logmel dc: mean {zs[:, 0].tolist()} 1/std {zs[:, 1].tolist()} std64 {std.tolist()}")
    assert (std > 0).all()
    assert np.abs(zs[:, 0] - mean).max() <= 1e-6 * np.abs(mean).max()
    assert np.abs(zs[:, 1] * std - 1.0).max() <= 1e-6


def test_dc_and_silent_batch_at_odd_T(gpu):
    """DC and silent utterances alternating at T = 51: the last frame of one
    shares its FFT with the first of the next.  The silent ones are exactly the
    floor on both paths and left un-normalised, and the one-call and two-call
    frame argmax agree."""
    B, n, T = 4, 8000, 51
    x = np.zeros((B, n), np.float32)
    x[0::2] = 0.25
    g = handle("fp16")
    g.decode_audio(x, n_samples=n)
    one = g.frame_argmax(B, T).cpu()
    zs, raw = g.transcribe_stats(B, T, return_raw=True)
    zs, raw = zs.cpu().numpy(), raw.cpu().numpy()
    feats = g.features(x, n_samples=n)
    g.decode(feats)
    two = g.frame_argmax(B, T).cpu()
    f = feats.cpu().numpy()
    for silent in (raw[1::2], f[1::2]):
        bits = silent.view(np.uint32)
        assert (bits == bits.flat[0]).all() and abs(float(silent.flat[0]) - LR.LN_FLOOR) <= LR.FLOOR_TOL
    assert np.array_equal(zs[1::2], np.tile(np.float32([0.0, 1.0]), (2, 1)))
    assert torch.equal(one, two)


# ---- f. refusals -----------------------------------------------------------------------
def test_transcribe_stats_refusals(gpu):
    """Only after a fused wk_ctc_transcribe of the same batch and T."""
    import wakeword
    w = CO.flat_weights(CO.make_model(V, seed=7))
    x = LR.audio(5, 3, 1920)
    g16 = wakeword.CTCModel(w, V, precision="fp16")
    with pytest.raises(wakeword.WakewordError, match="no wk_ctc_transcribe"):
        g16.transcribe_stats(3, 13)
    g32 = wakeword.CTCModel(w, V, precision="fp32")
    g32.decode_audio(x, n_samples=1920)
    with pytest.raises(wakeword.WakewordError, match="batch 3, T 13, not fused .fp32 handle"):
        g32.transcribe_stats(3, 13)
    g16.decode_audio(x[:, :480], n_samples=480)
    with pytest.raises(wakeword.WakewordError, match="batch 3, T 4, not fused .T < 6"):
        g16.transcribe_stats(3, 4)
    g16.decode_audio(x, n_samples=1920)
    for batch, T in ((2, 13), (3, 12), (4, 13)):
        with pytest.raises(wakeword.WakewordError, match="batch 3, T 13 .fused."):
            g16.transcribe_stats(batch, T)
    zs, raw = g16.transcribe_stats(3, 13, return_raw=True)
    assert zs.shape == (3, 2) and raw.shape == (3, 13, 80) and bool(torch.isfinite(raw).all())
    LR.check_stats("after refusals", zs.cpu().numpy(), raw.cpu().numpy())
