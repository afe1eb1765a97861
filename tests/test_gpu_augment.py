"""wk_augment_batch on the MI355X against tests/augment_ref.py (its docstring
has the bounds): the waveform stage of extract_features for a batch of clips.

Streams 1-3 (the pad behind a sped-up clip, the SNR noise, the SNR draw) are
keyed by the output row r = i*K + v, so a variant's noisy rows depend on its
position v in the list: by design, and checked here.  At out_len = 1 the
reference list's speed 0.8 resamples to int(0.8) = 0 samples, which the entry
point refuses by its own rule; that refusal is asserted and the one-sample cases
run with 0.8 replaced by 1.25 (augment_ref.VARIANTS_LEN1)."""
import ctypes as C

import numpy as np
import pytest

import augment_ref as A

pytestmark = pytest.mark.gpu


def run(gpu, c, pad_noise, snr, epoch=None, **kw):
    import wakeword
    raw, _ = A.case_audio(c)
    out = wakeword.augment_batch(raw, np.asarray(c.lengths, np.int32), variants=c.variants, pad_noise=pad_noise, snr=snr,
                                 seed=c.seed, epoch=c.epoch if epoch is None else epoch, out_len=c.out_len, **kw)
    assert out.shape == (c.n * len(c.variants), c.out_len) and out.dtype == gpu.float32 and out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize("k", range(len(A.CASES)))
def test_rows_against_the_reference(gpu, k):
    """Checks 1-3: noise off bit-equal; pad noise within 5e-7; the SNR stage within K_SNR of the float32 yardstick."""
    c = A.CASES[k]
    bad, _ = A.check_rows(k, run(gpu, c, 0.0, None), run(gpu, c, A.PAD, None), run(gpu, c, A.PAD, A.SNR))
    assert A.K_SNR is not None
    assert not bad, bad


def test_raw_gaussians(gpu):
    """A pad_noise = 1, len = 0 row is the generator itself: within 1e-5 of float64."""
    import wakeword
    for seed, epoch in A.SEEDS:
        got = wakeword.augment_batch(np.zeros((2, 8), np.float32), [0, 0], variants=((1.0, 1.0),), pad_noise=1.0,
                                     seed=seed, epoch=epoch, out_len=4099).cpu().numpy()
        for i in range(2):
            e = np.abs(got[i] - A.gauss(seed, epoch, 0, i, 4099)).max()
            print(f"raw gaussians seed {seed:#x} epoch {epoch} clip {i}: max|d| = {e:.3g}")
            assert e <= A.ATOL_GAUSS


def test_seventeen_variants_and_an_empty_resample_are_refused(gpu):
    import wakeword
    x = np.zeros((1, 16), np.float32)
    with pytest.raises(ValueError):
        wakeword.augment_batch(x, variants=((1.0, 1.0),) * 17, out_len=16)
    from wakeword import _lib
    d = gpu.zeros(64, device="cuda")
    var = (_lib.WkAugVariant * 17)(*[_lib.WkAugVariant(1.0, 1.0)] * 17)
    spec = _lib.WkAugSpec(0.0, 0.0, 0.0, 0.0, 0, 0)
    assert _lib.lib().wk_augment_batch(C.c_void_p(d.data_ptr()), 0, None, 1, 16, 16, var, 17, C.byref(spec), 16,
                                       C.c_void_p(d.data_ptr() + 128), None) == 1
    with pytest.raises(wakeword.WakewordError):
        wakeword.augment_batch(x, out_len=1)            # REFERENCE_VARIANTS: int(1 * 0.8) = 0


def test_zero_signal_stays_zero(gpu):
    """len = 0 and no pad noise: Ps = 0 scales the SNR noise to exactly 0."""
    import wakeword
    for out_len in (1, 257, 16000):
        variants = A.REFERENCE_VARIANTS if out_len > 1 else A.VARIANTS_LEN1
        out = wakeword.augment_batch(np.ones((3, 40), np.float32), [0, 0, 0], variants=variants, pad_noise=0.0, snr=A.SNR,
                                     seed=7, epoch=2, out_len=out_len)
        assert out.shape == (15, out_len) and not out.view(gpu.int32).any()


def test_determinism_and_epochs(gpu):
    c = A.CASES[7]                      # n = 3, out_len = 4099, lengths (1, 4099, 4098)
    one, two = run(gpu, c, A.PAD, A.SNR), run(gpu, c, A.PAD, A.SNR)
    assert np.array_equal(one.view(np.uint32), two.view(np.uint32))
    other = run(gpu, c, A.PAD, A.SNR, epoch=c.epoch + 1)
    assert all((one[r] != other[r]).any() for r in range(one.shape[0]))     # every noisy row is drawn afresh
    # SNR off: the samples that hold no noise (j < len of variant (1, 1)) do not move with the epoch, the pad does
    quiet0, quiet1 = run(gpu, c, A.PAD, None), run(gpu, c, A.PAD, None, epoch=c.epoch + 1)
    _, x = A.case_audio(c)
    for i, ln in enumerate(c.lengths):
        lim = min(ln, c.out_len)
        r = i * len(c.variants)
        assert np.array_equal(quiet0[r, :lim], x[i, :lim]) and np.array_equal(quiet1[r, :lim], x[i, :lim])
        if lim < c.out_len:
            assert (quiet0[r, lim:] != quiet1[r, lim:]).all()
    # another seed is another draw as well
    import wakeword
    raw, _ = A.case_audio(c)
    reseeded = wakeword.augment_batch(raw, list(c.lengths), variants=c.variants, pad_noise=A.PAD, snr=A.SNR,
                                      seed=c.seed + 1, epoch=c.epoch, out_len=c.out_len).cpu().numpy()
    assert all((one[r] != reseeded[r]).any() for r in range(one.shape[0]))


def test_layout(gpu):
    """A clip's rows depend on its index, not on n or on the other clips; a variant's noisy rows depend on its
    position in the list (streams 1-3 are keyed by the row)."""
    import wakeword
    c = A.CASES[6]                      # n = 3, out_len = 4099
    raw, _ = A.case_audio(c)
    lens = list(c.lengths)
    kw = dict(variants=c.variants, pad_noise=A.PAD, snr=A.SNR, seed=c.seed, epoch=c.epoch, out_len=c.out_len)
    K = len(c.variants)
    full = wakeword.augment_batch(raw, lens, **kw).cpu().numpy()
    first = wakeword.augment_batch(raw[:1], lens[:1], **kw).cpu().numpy()
    assert np.array_equal(full[:K].view(np.uint32), first.view(np.uint32))
    changed = raw.copy()
    changed[1] = changed[1][::-1]
    mixed = wakeword.augment_batch(changed, [lens[0], 17, lens[2]], **kw).cpu().numpy()
    for i in (0, 2):
        assert np.array_equal(full[i * K:(i + 1) * K].view(np.uint32), mixed[i * K:(i + 1) * K].view(np.uint32))
    assert (full[K:2 * K] != mixed[K:2 * K]).any()
    # two variants exchanged: with all noise off the rows move with them, with noise on they are other rows
    a, b = (0.8, 1.0), (1.0, 1.3)
    q = dict(pad_noise=0.0, snr=None, seed=c.seed, epoch=c.epoch, out_len=c.out_len)
    ab, ba = (wakeword.augment_batch(raw, lens, variants=v, **q).cpu().numpy() for v in ((a, b), (b, a)))
    assert np.array_equal(ab[0::2], ba[1::2]) and np.array_equal(ab[1::2], ba[0::2])
    kw.pop("variants")
    ab, ba = (wakeword.augment_batch(raw, lens, variants=v, **kw).cpu().numpy() for v in ((a, b), (b, a)))
    assert (ab[0::2] != ba[1::2]).any() and (ab[1::2] != ba[0::2]).any()


@pytest.mark.parametrize("i16", [False, True])
def test_out_of_range_lengths_and_the_stride_gap(gpu, i16):
    """d_len entries of in_len + 5 and -3 behave as in_len and 0; the 64 elements between clips (1e30, or 32767 for
    int16) are never read; nothing exceeds 1.3 in magnitude."""
    from wakeword import _lib
    n, in_len, out_len, K = 3, 300, 257, 5
    rng = np.random.default_rng(11)
    if i16:
        buf = np.full((n, in_len + 64), 32767, np.int16)
        buf[:, :in_len] = rng.integers(-29491, 29492, size=(n, in_len))
        x = buf[:, :in_len].astype(np.float32) / np.float32(32768.0)
    else:
        buf = np.full((n, in_len + 64), 1e30, np.float32)
        buf[:, :in_len] = rng.uniform(-0.9, 0.9, size=(n, in_len))
        x = buf[:, :in_len]
    in_len_short = 200                 # a clip shorter than out_len: reading past it would reach the gap
    d_buf = gpu.from_numpy(buf).cuda()
    var = (_lib.WkAugVariant * K)(*[_lib.WkAugVariant(s, v) for s, v in A.REFERENCE_VARIANTS])
    spec = _lib.WkAugSpec(A.PAD, A.SNR[0], A.SNR[1], A.SNR[2], 7, 5)

    def call(lengths, L):
        d_len = gpu.tensor(lengths, dtype=gpu.int32, device="cuda")
        out = gpu.empty((n * K, out_len), dtype=gpu.float32, device="cuda")
        st = _lib.lib().wk_augment_batch(C.c_void_p(d_buf.data_ptr()), 1 if i16 else 0, C.c_void_p(d_len.data_ptr()), n, L,
                                         in_len + 64, var, K, C.byref(spec), out_len, C.c_void_p(out.data_ptr()),
                                         C.c_void_p(gpu.cuda.current_stream().cuda_stream))
        assert st == 0
        return out.cpu().numpy()

    for L in (in_len, in_len_short):
        wild, tame = call([L + 5, -3, 100], L), call([L, 0, 100], L)
        assert np.array_equal(wild.view(np.uint32), tame.view(np.uint32))
        assert np.abs(wild).max() <= 1.3
        ref = A.reference(x[:, :L], [L, 0, 100], A.REFERENCE_VARIANTS, A.PAD, None, 7, 5, out_len)
        spec.snr_noise = 0.0
        quiet = call([L + 5, -3, 100], L)
        spec.snr_noise = A.SNR[0]
        assert np.abs(quiet - ref.out).max() <= A.ATOL_PAD


def test_python_layer(gpu):
    """extract_features = mfcc(augment_batch(...)) bitwise, labels K times; step_augmented = step on those features."""
    import wakeword
    rng = np.random.default_rng(12)
    x = rng.uniform(-0.5, 0.5, size=(4, 12000)).astype(np.float32)
    lens = [12000, 9000, 1, 0]
    feats, labels = wakeword.extract_features(x, lens, label=1, is_noise=True, seed=3, epoch=4)
    wave = wakeword.augment_batch(x, lens, snr=(0.01, 5, 20), seed=3, epoch=4)
    assert wave.shape == (20, 16000) and feats.shape == (20, 13, 63) and labels.shape == (20,)
    assert gpu.equal(feats.view(gpu.int32), wakeword.mfcc(wave, mode="torchaudio", cmvn=True).view(gpu.int32))
    assert labels.dtype == gpu.int64 and bool((labels == 1).all())
    plain, plain_labels = wakeword.extract_features(x, lens, augment_audio=False, add_noise_to_pad=False)
    assert plain.shape == (4, 13, 63) and plain_labels.shape == (4,) and not plain_labels.any()
    assert gpu.equal(plain, wakeword.mfcc(wakeword.augment_batch(x, lens, variants=((1, 1),), pad_noise=0.0)))

    y = np.array([1, 0, 1, 0], np.float32)
    t1, t2 = wakeword.Trainer(seed=5), wakeword.Trainer(seed=5)
    for epoch in (4, 5):
        feats, _ = wakeword.extract_features(x, lens, is_noise=True, seed=3, epoch=epoch)
        want = t1.step(feats, np.repeat(y, 5))
        got = t2.step_augmented(x, lens, y, epoch, is_noise=True, seed=3)
        assert gpu.equal(want.view(gpu.int32), got.view(gpu.int32)) and bool(gpu.isfinite(got))
    assert gpu.equal(t1.weights(), t2.weights())
