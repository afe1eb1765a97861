"""CPU tests of the prefix beam search reference (tests/ctc_beam_ref.py), the
specification wk_ctc_beam is held to: exhaustive search against brute force,
the float32 run within the pinned E32 of the float64 run, the cap on
indecisive utterances for every case of the table, the merge by hand, the tie
rules on uniform rows and Tb = 0."""
import numpy as np
import pytest

import ctc_beam_ref as R


def test_exhaustive_search_equals_brute_force():
    """T = 5, V = 3, W = 64, K = 2: nothing is pruned, so the beam holds every
    label sequence with a path and each score is the exact CTC log-likelihood.
    (Of the 63 label sequences of length <= 5 over two labels, those with a
    path in 5 frames are the 25 with length + adjacent repeats <= 5.)"""
    for seed in range(4):
        lp = R.log_softmax(2.0 * np.random.default_rng(seed).standard_normal((5, 3)))
        hyps, _ = R.beam_search(lp, 64, 2, np.float64)
        exact = R.brute_force(lp, 5)
        assert len(exact) == 25 and {h[0] for h in hyps} == set(exact)
        for l, _, _, p in hyps:
            assert abs(p - exact[l]) <= 1e-12, (l, p, exact[l])
        assert hyps[0][0] == max(exact, key=exact.get)
        assert [h[3] for h in hyps] == sorted((h[3] for h in hyps), reverse=True)


def test_float32_within_pinned_error():
    worst = 0.0
    for shape in R.SHAPES:
        e, n = R.score_error32(shape)
        print(f"ctc-beam-ref {shape}: float32 against float64 over {n} hypotheses: {e:.3e}")
        assert n >= R.BATCH
        worst = max(worst, e)
    print(f"ctc-beam-ref E32 measured {worst:.3e}, pinned {R.E32:.3e}, tau {R.TAU:.3e}")
    assert worst <= R.E32
    assert worst >= 0.5 * R.E32          # the pinned constant is the measurement, not a loose bound


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.CASE_IDS)
def test_decisive_share(shape):
    """At most 25 % of a case's utterances may be indecisive (margin <= tau), and none may have zero decisive ones."""
    _, margins = R.case_reference(shape)
    decisive = int((margins > R.TAU).sum())
    print(f"ctc-beam-ref {shape}: decisive {decisive}/{R.BATCH}, smallest margin {margins.min():.3e}")
    assert decisive > 0 and R.BATCH - decisive <= R.BATCH // 4


def test_merge_by_hand():
    """Two frames, V = 2 (a = 1): after frame 0 both () and (a) live; in frame 1
    the extension of () by a is the live prefix (a) and adds to its stay."""
    p = np.log(np.array([[0.6, 0.4], [0.3, 0.7]]))
    hyps, cand = R.beam_search(p, 4, 1, np.float64)
    got = {h[0]: h for h in hyps}
    assert cand.tolist() == [[1], [1]]
    # (): blank, blank
    assert np.isclose(np.exp(got[()][3]), 0.6 * 0.3, rtol=1e-14, atol=0)
    # (a): pb = a blank; pnb = a a (its own stay) + blank a (the merged extension of ())
    assert np.isclose(np.exp(got[(1,)][1]), 0.4 * 0.3, rtol=1e-14, atol=0)
    assert np.isclose(np.exp(got[(1,)][2]), 0.4 * 0.7 + 0.6 * 0.7, rtol=1e-14, atol=0)
    # (a, a) needs a blank between: no path in two frames, so it is dropped, not kept at -inf
    assert set(got) == {(), (1,)}
    assert sum(np.exp(h[3]) for h in hyps) == pytest.approx(1.0, abs=1e-14)
    assert hyps[0][0] == (1,)


def test_tie_rules_on_uniform_rows():
    V = 5
    lp = np.full((2, V), -np.log(V))
    # candidates: ties to the lower id, in selection order
    assert R.candidates(lp[0], 3).tolist() == [1, 2, 3]
    assert R.candidates(np.array([0.0, -1.0, -0.5, -0.5, -1.0]), 3).tolist() == [2, 3, 1]
    assert R.candidates(np.array([0.0, -np.inf, -np.inf]), 8).tolist() == [1, 2]
    # frame 0: the stay () and the extensions (1), (2), (3) all total log(1/5): candidate order decides
    h1, _ = R.beam_search(lp[:1], 3, 3, np.float64)
    assert [h[0] for h in h1] == [(), (1,), (2,)]
    assert len({h[3] for h in h1}) == 1
    # frame 1 from (), (1), (2), (3): the stays (1), (2), (3) triple (label, then blank or label again, and the merged
    # extension of ()) and lead in slot order; then the equal singles: the stay () first, then the extensions by
    # parent slot, then token id ((1, 1) needs a blank between and has no path)
    h2, _ = R.beam_search(lp, 6, 3, np.float64)
    assert [h[0] for h in h2] == [(1,), (2,), (3,), (), (1, 2), (1, 3)]
    assert h2[0][3] == h2[1][3] == h2[2][3] > h2[3][3] == h2[4][3] == h2[5][3]
    # a replacement must be strictly greater: W = 1 keeps the first of the equal candidates
    assert R.beam_search(lp[:1], 1, 3, np.float64)[0][0][0] == ()


def test_zero_frames_and_fill():
    lp = R.log_softmax(np.random.default_rng(5).standard_normal((2, 6, 4)))
    out = R.beam_batch(lp, [0, 6], 4, 2, 3, 2, np.float64)
    assert out["lengths"][0].tolist() == [0, -1, -1] and out["scores"][0].tolist() == [0.0, -np.inf, -np.inf]
    assert (out["tokens"][0] == -1).all() and (out["cand"][0] == -1).all()
    assert out["hyps"][0] == [((), 0.0, -np.inf, 0.0)]
    # max_len = 2 cuts the tokens, the lengths stay whole
    for i in range(3):
        l = out["hyps"][1][i][0]
        assert out["lengths"][1, i] == len(l) and out["tokens"][1, i].tolist() == (list(l[:2]) + [-1, -1])[:2]
    assert R.margin(lp[0, :0], 4, 2) == np.inf


def test_margin_reads_both_boundaries():
    lp = np.log(np.array([[0.5, 0.3, 0.15, 0.05]]))
    # K = 2 of 3 non-blank: the K-th against the (K+1)-th lp; W = 8 never binds
    assert R.margin(lp, 8, 2) == pytest.approx(np.log(0.15) - np.log(0.05), abs=1e-12)
    # K = 3 takes all; W = 2 of 4 candidates (0.5, 0.3, 0.15, 0.05): the W-th against the (W+1)-th total
    assert R.margin(lp, 2, 3) == pytest.approx(np.log(0.3) - np.log(0.15), abs=1e-12)


def test_case_table_has_a_recreated_parent():
    """The table reaches the merge whose parent prefix left the beam and came
    back (the same prefix under another search-tree node)."""
    n = [sum(R.recreated_merges(R.case(s)[b], s[2], s[3]) for b in range(R.BATCH)) for s in R.SHAPES]
    print("ctc-beam-ref recreated-parent merges per case:", n)
    assert n[-1] > 0
