"""CPU tests of the numpy reference the GPU tests of wk_ctc_cer compare against
(tests/ctc_cer_ref.py): the int64-key row recurrence equals a lexicographic
(d, s) tuple DP and the exhaustive enumeration of alignments, keeps the
invariants of an edit distance, and its collapse is the greedy CTC decode."""
import numpy as np
import pytest

import ctc_cer_ref as R


def pairs(seed, count, max_len, alphabet):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        n, m = rng.integers(0, max_len + 1, size=2)
        yield rng.integers(1, alphabet + 1, size=n), rng.integers(1, alphabet + 1, size=m)


@pytest.mark.parametrize("alphabet", [2, 3, 5, 50])
def test_equals_tuple_dp(alphabet):
    for h, r in pairs(alphabet, 150, 40, alphabet):
        assert R.edit_stats(h, r)[:2] == R.tuple_dp(h.tolist(), r.tolist()), (h, r)


@pytest.mark.parametrize("alphabet", [2, 3])
def test_equals_exhaustive_enumeration(alphabet):
    for h, r in pairs(10 + alphabet, 120, 6, alphabet):
        assert R.edit_stats(h, r)[:2] == R.exhaustive(h.tolist(), r.tolist()), (h, r)
    h = np.array([1, 2, 1, 2, 1, 2])
    assert R.edit_stats(h, h[::-1])[:2] == R.exhaustive(h.tolist(), h[::-1].tolist())       # N = M = 6


def test_invariants():
    for alphabet in (2, 3, 5, 50):
        for h, r in pairs(100 + alphabet, 100, 40, alphabet):
            d, s, dele, ins = R.edit_stats(h, r)
            n, m = len(h), len(r)
            assert d == s + dele + ins and ins - dele == n - m and min(s, dele, ins) >= 0
            assert abs(n - m) <= d <= max(n, m)
            assert R.edit_stats(h, h) == (0, 0, 0, 0)
            ds, ss, dels, inss = R.edit_stats(r, h)
            assert (ds, ss, dels, inss) == (d, s, ins, dele)                  # symmetric: the roles of ins and del swap


def test_known_values():
    assert R.edit_stats([1, 2, 3], [1, 2, 3]) == (0, 0, 0, 0)
    assert R.edit_stats([], [4, 5]) == (2, 0, 2, 0) and R.edit_stats([4, 5], []) == (2, 0, 0, 2)
    assert R.edit_stats([], []) == (0, 0, 0, 0)
    assert R.edit_stats([1, 2, 3], [1, 9, 3]) == (1, 1, 0, 0)
    assert R.edit_stats([1, 3], [1, 2, 3]) == (1, 0, 1, 0)
    # "ab" vs "ba": two substitutions or one deletion and one insertion, both d = 2; the fewest substitutions is 0
    assert R.edit_stats([1, 2], [2, 1]) == (2, 0, 1, 1)
    # kitten / sitting
    k, s = [ord(c) for c in "kitten"], [ord(c) for c in "sitting"]
    assert R.edit_stats(k, s)[0] == 3


def test_collapse_is_the_greedy_decode():
    from wakeword.ctc import greedy_tokens
    rng = np.random.default_rng(7)
    for T in (0, 1, 2, 63, 64, 65, 130):
        for V in (2, 3, 7):
            labels = rng.integers(0, V, size=T)
            lp = np.full((T, V), -30.0, dtype=np.float32)
            lp[np.arange(T), labels] = 0.0                                  # one-hot log-probs
            want = greedy_tokens(lp[None])[0] if T else []
            assert R.collapse(labels).tolist() == want
    assert R.collapse([0, 3, 3, 0, 3, 4, 4, 4, 0, 0, 5]).tolist() == [3, 3, 4, 5]


def test_batch_totals_and_oracle():
    hyp = np.array([[[1, 2, 3, 0], [1, 9, 3, 0], [1, 2, 3, 7]],
                    [[5, 5, 0, 0], [6, 0, 0, 0], [5, 6, 0, 0]],
                    [[7, 7, 7, 7], [8, 0, 0, 0], [0, 0, 0, 0]]])
    hyp_len = [3, 3, 4, 2, 1, 2, 4, 1, -1]
    ref = np.array([[1, 9, 3], [5, 6, 0], [0, 0, 0]])
    got = R.cer_batch(hyp, hyp_len, ref, [3, 2, 0])
    assert got["stats"][0].tolist() == [[1, 1, 0, 0], [0, 0, 0, 0], [2, 1, 0, 1]]
    assert got["stats"][1].tolist() == [[1, 1, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0]]
    assert got["stats"][2].tolist() == [[4, 0, 0, 4], [1, 0, 0, 1], [0, 0, 0, 0]]      # M = 0: every token an insertion
    assert got["best"].tolist() == [1, 2, 2]
    assert got["totals"].tolist() == [[6, 2, 0, 4, 5, 9, 3, 3], [0, 0, 0, 0, 5, 5, 0, 3]]


def test_equals_torchaudio():
    F = pytest.importorskip("torchaudio.functional")
    for h, r in pairs(3, 50, 40, 4):
        assert R.edit_stats(h, r)[0] == F.edit_distance(h.tolist(), r.tolist())
