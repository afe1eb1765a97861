"""CPU tests of the forced-alignment reference (tests/ctc_align_ref.py): it
equals brute-force enumeration on tiny problems, score and tie rule; it
recovers a planted alignment; and on every case of the table the float32 and
float64 paths are the same path -- a condition on the INPUTS, which keeps the
GPU tests' "bit-equal to the float32 reference" from hiding a near-tie."""
import numpy as np
import pytest

import ctc_align_ref as A

TINY = [(T, labels) for T in range(1, 8) for labels in ([], [1], [2], [1, 2], [1, 1], [2, 2], [1, 2, 1], [2, 2, 1], [1, 1, 1],
                                                        [2, 1, 1])]


def _f32_path_score(lp, labels, path):
    """The recurrence's own arithmetic along one path: x_t + (the sum so far), in float32."""
    ext = A.extended(labels)
    acc = np.float32(lp[0, ext[path[0]]])
    for t in range(1, len(path)):
        acc = np.float32(lp[t, ext[path[t]]]) + acc
    return acc


@pytest.mark.parametrize("T,labels", TINY, ids=[f"T{T}-{'_'.join(map(str, lab)) or 'empty'}" for T, lab in TINY])
def test_reference_equals_brute_force(T, labels):
    """V = 3.  Dyadic log-probs (multiples of 1/4 in [-2, 0]: every sum is
    exact in either precision and ties are plentiful): the score is the
    maximum over all valid paths and the path is, among the optimal ones, the
    one the tie rule picks -- exact arithmetic makes every prefix of an optimal
    path optimal, so preferring L-1 at the exit and then s over s-1 over s-2 at
    each step back is the largest path in reverse-lexicographic order.  Random
    normal log-probs: the float32 score is the maximum of the paths' float32
    scores (rounding is monotone, so max and add commute)."""
    rng = np.random.default_rng(100 * T + len(labels) + 7 * sum(labels))
    paths = A.all_paths(labels, T)
    for trial in range(6):
        lp = -rng.integers(0, 9, size=(T, 3)).astype(np.float32) / 4.0
        if trial == 0:
            lp[:] = -0.25                                  # every path ties
        for dtype in (np.float32, np.float64):
            score, states = A.viterbi(lp, labels, dtype)
            if not paths:
                assert states is None and score == -np.inf
                continue
            scored = [(A.path_score64(lp, labels, p), tuple(reversed(p))) for p in paths]
            best = max(scored)
            assert float(score) == best[0]
            assert tuple(reversed(states.tolist())) == best[1]
            assert A.valid_alignment(states, labels, T)
    lp = A.log_softmax(rng.standard_normal((T, 3)))
    score, states = A.viterbi(lp, labels, np.float32)
    if paths:
        assert score == max(_f32_path_score(lp, labels, p) for p in paths)
        assert _f32_path_score(lp, labels, states) == score
        s64, st64 = A.viterbi(lp, labels, np.float64)
        assert abs(s64 - max(A.path_score64(lp, labels, p) for p in paths)) <= 1e-12
    else:
        assert states is None


def test_infeasible_and_empty():
    lp = np.zeros((4, 5), np.float32)
    assert A.viterbi(lp[:0], [1], np.float32)[1] is None              # Tb = 0
    assert A.viterbi(lp[:2], [1, 1], np.float32)[1] is None           # needs 3 frames
    assert A.viterbi(lp[:3], [1, 1], np.float32)[1].tolist() == [1, 2, 3]
    assert A.viterbi(lp, [], np.float32)[1].tolist() == [0, 0, 0, 0]  # S = 0: all blanks
    broken = lp.copy()
    broken[1, :] = -np.inf
    assert A.viterbi(broken, [1, 2], np.float32) == (-np.inf, None)   # every path through a -inf
    out = A.align_batch(np.zeros((2, 4, 5), np.float32), [[5, 1], [1, 2]], [4, 3], [2, 2])
    assert out["scores"][0] == -np.inf and (out["states"][0] == -1).all() and (out["spans"][0] == -1).all()
    # all ties: the trailing blank at the exit, then the nearest reachable predecessor at each step back
    assert out["states"][1].tolist() == [1, 3, 4, -1] and out["spans"][1].tolist() == [[0, 1], [1, 2]]
    assert out["tokens"][1].tolist() == [1, 2, 0, -1] and out["scores"][1] == 0.0


def test_tie_rule_example():
    """Uniform rows: labels [2, 2, 5], T = 12 -> states 1, 2, 3, 5, 6, 6, ..."""
    lp = np.full((12, 7), -np.log(7.0), dtype=np.float32)
    _, states = A.viterbi(lp, [2, 2, 5], np.float32)
    assert states.tolist() == [1, 2, 3, 5] + [6] * 8


@pytest.mark.parametrize("case", A.CASES, ids=A.CASE_IDS)
def test_table_float32_and_float64_paths_agree(case):
    lp, labels, planted = A.case(*case)
    T = lp.shape[0]
    s32, p32 = A.viterbi(lp, labels, np.float32)
    s64, p64 = A.viterbi(lp, labels, np.float64)
    assert p32 is not None and A.valid_alignment(p32, labels, T)
    assert np.array_equal(p32, p64)
    rel = abs(float(s32) - s64) / abs(s64)
    print(f"ctc-align-ref {case} score64={s64:.6f} rel32={rel:.2e}")
    assert rel <= 2 * T * A.EPS32                       # T adds, each within 2^-24 of a partial sum
    assert abs(A.path_score64(lp, labels, p64) - s64) <= 1e-9 * abs(s64)
    if planted is not None:
        assert np.array_equal(p32, planted)             # the planted alignment is recovered exactly
