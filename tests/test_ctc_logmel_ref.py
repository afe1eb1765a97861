"""tests/ctc_logmel_ref.py on the CPU: the layout restatement, the audio
generator, and the mutation check of the checks themselves -- a stand-in for
the device result (torch-CPU fp32 log-mel, float64 statistics rounded to fp32)
passes them, and the same result with one defect of the kind the log-mel
kernel could have fails the check named beside it."""
import numpy as np
import pytest
import torch

import ctc_logmel_ref as LR
from oracle import wk_ctc_oracle as CO

B, T, N = 9, 13, 1920


def test_layout_and_batch_for():
    # 256 CUs: 3072 waves, R = 2 from 18,433 rows on (the figures of wk_ctc_logmel.hip's layout)
    assert LR.layout(256, 18432, 2) == LR.Layout(3072, 256, 1, 4)
    assert LR.layout(256, 18434, 2).R == 2 and LR.layout(256, 7, 7) == LR.Layout(2, 1, 1, 2)
    assert LR.layout(256, 2 * 18432 + 1, 7) == LR.Layout(6145, 256, 3, 4)
    for n_cu in (256, 304, 64):
        for t in (2, 3, 5, 7, 13, 301):
            assert LR.batch_for(n_cu, t, 1) == 1
            for r in (2, 3):
                b = LR.batch_for(n_cu, t, r)
                assert LR.layout(n_cu, b * t, t).R == r and LR.layout(n_cu, (b - 1) * t, t).R == r - 1


def test_audio_generator():
    x = LR.audio(3, 64, 1920)
    assert x.dtype == np.float32 and x.shape == (64, 1920) and np.abs(x).max() <= 0.5
    assert np.array_equal(x, LR.audio(3, 64, 1920)) and not np.array_equal(x, LR.audio(4, 64, 1920))
    rms_db = 20.0 * np.log10(np.sqrt((x.astype(np.float64) ** 2).mean(1)))
    assert np.abs(np.diff(rms_db)).max() > 10.0 and rms_db.max() - rms_db.min() < 26.0
    c = np.corrcoef(x[:8])
    assert np.abs(c - np.eye(8)).max() < 0.3          # every utterance its own stream
    # well-conditioned by construction, down to T = 2 and at a batch that takes R = 2
    for n, b in ((201, 9217), (320, 40), (960, 40), (48000, 7)):
        assert LR.Ref(LR.audio(n, b, n), n).e32 < 1e-4


@pytest.fixture(scope="module")
def stand_in():
    x = LR.audio(17, B, N)
    ref = LR.Ref(x, N)
    raw = LR.raw32(x, N)
    mean, std, _ = LR.stats64(raw.numpy())
    zs = np.stack([mean, 1.0 / std], 1).astype(np.float32)
    return ref, raw.numpy(), LR.zscore(raw).numpy(), zs


def test_stand_in_passes(stand_in):
    ref, raw, feats, zs = stand_in
    LR.check_features("stand-in", feats, ref)
    LR.check_raw("stand-in", raw, ref)
    LR.check_stats("stand-in", zs, raw)


def test_a_zeroed_pass_fails_check_features_and_check_raw(stand_in):
    ref, raw, feats, _ = stand_in
    for good, check in ((feats, LR.check_features), (raw, LR.check_raw)):
        bad = good.reshape(B * T, 80).copy()
        bad[30:36] = 0.0                              # pass 5: rows 30..35, utterances 2
        with pytest.raises(AssertionError):
            check("zeroed pass", bad.reshape(B, T, 80), ref)


def test_rows_swapped_across_an_utterance_boundary_fail(stand_in):
    ref, raw, feats, _ = stand_in
    for good, check in ((feats, LR.check_features), (raw, LR.check_raw)):
        bad = good.reshape(B * T, 80).copy()
        bad[[T - 1, T]] = bad[[T, T - 1]]             # the last row of utterance 0 and the first of utterance 1
        with pytest.raises(AssertionError):
            check("swapped rows", bad.reshape(B, T, 80), ref)


def test_a_dropped_low_weight_mel_tap_fails(stand_in):
    """One filter tap of weight < 0.05 left out (a window cut one bin short):
    inside the old 2e-3 tolerance or not, outside the new bound."""
    ref, _, _, _ = stand_in
    fb = CO.mel_fbanks().clone()
    small = ((fb > 0) & (fb < 0.05)).nonzero()
    assert len(small) >= 8
    caught = 0
    for k, m in small.tolist():
        cut = fb.clone()
        assert 0.0 < float(cut[k, m]) < 0.05
        cut[k, m] = 0.0
        raw = LR.raw32(ref.x, N, cut)
        for good, check in ((LR.zscore(raw).numpy(), LR.check_features), (raw.numpy(), LR.check_raw)):
            with pytest.raises(AssertionError):
                check(f"dropped tap bin {k} mel {m} w={float(fb[k, m]):.4f}", good, ref)
        caught += 1
    assert caught == len(small)


def test_a_mean_off_by_a_pass_fails_check_stats(stand_in):
    """One 6-row pass lost from, or counted twice in, an utterance's sums."""
    _, raw, _, zs = stand_in
    for sign in (-1.0, 1.0):
        bad = zs.copy()
        bad[4, 0] += np.float32(sign * 6.0 / T * (zs[4, 0] - LR.LN_FLOOR))
        with pytest.raises(AssertionError):
            LR.check_stats("mean off by 6/T", bad, raw)
    # and at T = 301, where a pass is 2 % of the utterance
    x = LR.audio(19, 2, 48000)
    raw = LR.raw32(x, 48000).numpy()
    mean, std, _ = LR.stats64(raw)
    zs = np.stack([mean, 1.0 / std], 1).astype(np.float32)
    LR.check_stats("T=301", zs, raw)
    zs[1, 0] -= np.float32(6.0 / 301 * (zs[1, 0] - LR.LN_FLOOR))
    with pytest.raises(AssertionError):
        LR.check_stats("T=301 mean off by 6/T", zs, raw)


def test_zero_frames_are_found_from_the_input():
    x = np.ones((2, 1000), np.float32)
    x[1, 500:] = 0.0
    z = LR.zero_frames(x, 1920)
    assert z.shape == (2, 13)
    assert z[0].tolist() == [False] * 8 + [True] * 5          # frame t covers 160 t - 200 .. 160 t + 199
    assert z[1].tolist() == [False] * 5 + [True] * 8
    ref = LR.Ref(x * 3.0, 1920)
    good = LR.zscore(LR.raw64(x * 3.0, 1920)).numpy().astype(np.float32)
    assert LR.check_zero_frames("floor", good, ref) == 13
    bad = good.copy()
    bad[1, 6, 3] += 1e-3                                      # leakage into one all-zero frame
    with pytest.raises(AssertionError):
        LR.check_zero_frames("leak", bad, ref)
