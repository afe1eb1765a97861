"""CPU tests of the keyword-spotting definition (tests/ctc_spot_ref.py, the
oracle of the GPU tests): the recurrence equals the brute-force maximum over
all segments, a planted keyword scores exactly 0 on its span, and the tie
rules (tight start, first maximum) hold."""
import numpy as np
import pytest

import ctc_spot_ref as R


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalized"])
def test_reference_equals_brute_force(normalize):
    """float64, T <= 8, V <= 4, S <= 3: the score is the maximum of seg64 over
    all segments, the span attains it, and its end is the first that does."""
    rng = np.random.default_rng(20 + normalize)
    finite = 0
    for _ in range(120):
        T, V, S = int(rng.integers(1, 9)), int(rng.integers(2, 5)), int(rng.integers(1, 4))
        kw = rng.integers(1, V, size=S)
        lp = R.log_softmax(rng.standard_normal((T, V)))
        if rng.random() < 0.3:
            lp[rng.random((T, V)) < 0.2] = -np.inf
        score, span, e = R.spot(lp, kw, normalize, np.float64)
        tab = R.brute64(lp, kw, normalize)
        assert score == tab.max()
        assert np.array_equal(e, tab[:, 1:].max(axis=0))            # the trace: the best segment ending at each frame
        if score == -np.inf:
            assert span == (-1, -1)
            continue
        finite += 1
        assert 0 <= span[0] < span[1] <= T
        assert tab[span[0], span[1]] == score
        assert tab[:, :span[1]].max() < score                        # no earlier end attains it
    assert finite > 60


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_keyword_scores_zero(dtype):
    kw = [3, 1, 1, 4]
    lp, want = R.planted(30, 6, kw, start=7, hold=3, gap=1)
    score, span, e = R.spot(lp, kw, True, dtype)
    # frames: 3 at 7-9, blank, 1 at 11-13, blank, 1 at 15-17, blank, 4 from 19
    assert score == 0.0 and score.dtype == dtype and span == want == (7, 20)
    assert e[span[1] - 1] == 0.0 and (e[:span[1] - 1] == -np.inf).all()
    # on soft rows that the keyword's path wins everywhere the score is still exactly 0
    soft = R.log_softmax(np.where(lp == 0.0, 9.0, 0.0) + np.random.default_rng(0).standard_normal(lp.shape))
    score, span, _ = R.spot(soft, kw, True, dtype)
    assert score == 0.0 and span == want
    raw, span_raw, _ = R.spot(soft, kw, False, dtype)
    assert raw < 0.0 and span_raw == (9, 20)      # raw mode: every frame costs, so the start is tight (the first label's last frame)


def test_raw_mode_tight_start_and_first_maximum():
    """Uniform rows, normalize off: every frame costs -ln V, so the best segment
    is the shortest, S frames; among the equal ones the first end wins."""
    V, T = 5, 9
    lp = np.full((T, V), -np.log(np.float32(V)), dtype=np.float32)
    score, span, e = R.spot(lp, [1, 2, 3], False)
    assert span == (0, 3) and score == e[2] and (e[:2] == -np.inf).all()
    assert (e[2:] == score).all()                       # every later end ties and loses to the first
    # normalize on: every path ties at exactly 0; stay is preferred, so the start stays at frame 0
    score, span, e = R.spot(lp, [1, 2, 3], True)
    assert score == 0.0 and span == (0, 3)


def test_repeated_labels_need_a_blank():
    V, T = 4, 6
    lp = np.full((T, V), -np.inf, dtype=np.float32)
    lp[:, 2] = 0.0                                      # label 2 at every frame, never a blank
    assert R.spot(lp, [2, 2], True)[0] == -np.inf
    assert R.spot(lp, [2], True)[:2] == (0.0, (0, 1))
    lp[3, 2], lp[3, 0] = -np.inf, 0.0                   # one blank at frame 3
    score, span, _ = R.spot(lp, [2, 2], True)
    assert score == 0.0 and span == (0, 5)              # stay is preferred: the start stays at 0
    lat, skip = R.lattice([2, 2, 3])
    assert lat.tolist() == [2, 0, 2, 0, 3] and skip.tolist() == [False, False, False, False, True]


@pytest.mark.parametrize("kw,need", [([1, 2, 3], 3), ([1, 1, 3], 4), ([2, 2, 2], 5), ([3], 1)])
def test_too_few_frames_is_no_occurrence(kw, need):
    """Tb < S + the number of adjacent equal labels gives -inf, Tb equal to it a finite score."""
    rng = np.random.default_rng(need)
    lp = R.log_softmax(rng.standard_normal((need, 5)))
    for normalize in (False, True):
        score, span, e = R.spot(lp[:need - 1], kw, normalize)
        assert score == -np.inf and span == (-1, -1) and (e == -np.inf).all()
        score, span, _ = R.spot(lp, kw, normalize)
        assert np.isfinite(score) and span == (0, need)


def test_spot_batch_conventions():
    rng = np.random.default_rng(3)
    lp = R.log_softmax(rng.standard_normal((2, 7, 5)))
    kws = np.array([[1, 2, 0], [9, 1, 0], [3, 0, 0], [4, 4, 4]])
    out = R.spot_batch(lp, kws, [2, 2, 0, 3], in_len=[7, 0])
    assert out["scores"].shape == (2, 4) and out["spans"].shape == (2, 4, 2) and out["trace"].shape == (2, 4, 7)
    assert np.isfinite(out["scores"][0, [0, 3]]).all()
    assert (out["scores"][0, [1, 2]] == -np.inf).all() and (out["spans"][0, [1, 2]] == -1).all()      # invalid label, empty
    assert (out["scores"][1] == -np.inf).all() and (out["trace"][1] == -np.inf).all()                  # Tb = 0
