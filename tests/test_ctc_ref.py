"""CPU tests of tests/ctc_ref.py, the references of tests/test_gpu_ctc_parity.py:
the hand-written float64 model against torch's own modules in double, the
trained-like model's coverage conditions and the argmax gate's cap at every
case, from the reference alone, and the mutations the parity bounds must see."""
import copy

import numpy as np
import pytest
import torch

import ctc_ref as R
from oracle import wk_ctc_oracle as CO

ALL = [(v, b, t) for v in R.VOCABS for b, t in R.CASES]


@pytest.mark.parametrize("vocab", R.VOCABS)
def test_handwritten_model_matches_torch_double(vocab):
    """ref64 (hand-written encoder, GRU cell, output layer) against the module
    in .double() -- nn.GRU's recurrence -- on a saturating model: rounding only."""
    m = R.model(vocab)
    feats = R.features_case(17, 65)
    assert float((R.ref64(m, feats) - R.module64(m, feats)).abs().max()) < 1e-12
    x = feats.double()
    with torch.no_grad():
        want, _ = copy.deepcopy(m.gru).double()(copy.deepcopy(m.audio_encoder).double()(x))
    _, states = R.forward(m, feats, None, return_states=True)
    assert float((states[1] - want).abs().max()) < 1e-13


@pytest.mark.parametrize("vocab", R.VOCABS)
def test_trained_like_leaves_the_default_init(vocab):
    """What make_model's init never shows: LayerNorm parameters off 1 / 0, a
    saturated GRU, the blank winning about half and (ragged V) the last column
    about a tenth of the calibration batch's frames."""
    m = R.model(vocab)
    w, b = m.audio_encoder[1].weight.detach(), m.audio_encoder[1].bias.detach()
    assert float((w - 1).abs().min()) > 0 and float(w.min()) >= 0.5 and float(w.max()) <= 1.5
    assert float(b.abs().max()) <= 0.5 and float(b.abs().mean()) > 0.1
    assert 0.2 <= R.saturated_share(m, R.features_case(*R.CAL)) <= 0.4
    assert R.saturated_share(CO.make_model(vocab, R.SEED), R.features_case(*R.CAL)) < 1e-3
    c = R.case(vocab, *R.CAL)
    assert 0.4 <= float((c.argmax == 0).float().mean()) <= 0.55
    if vocab % 64:
        assert 0.08 <= float((c.argmax == vocab - 1).float().mean()) <= 0.12
    assert len(torch.unique(c.argmax)) >= 16


def test_reference_errors_are_rounding_sized():
    """e32 is a few fp32 ulps of a log-prob, e16 a few fp16 ulps: the figures
    the bounds multiply (measured: 1.6e-6 to 7.5e-6, depending on the host's
    fp32 GEMM, and 2.3e-3 to 7.2e-3)."""
    for v, b, t in ALL:
        c = R.case(v, b, t)
        assert 5e-7 < R.e32(c) < 2e-5, (v, b, t, R.e32(c))
        for mode in ("fp16", "gemm"):
            assert 1.5e-3 < R.e16(c, mode) < 1e-2, (v, b, t, mode, R.e16(c, mode))
        assert R.e16(c, "out16") < R.e16(c, "fp16")       # a subset of its roundings


@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("vocab,B,T", ALL)
def test_gate_cap_and_coverage(vocab, B, T, mode):
    """From the reference alone: the argmax gate (margin > 2 K e) leaves out at
    most 15 % of a case's frames (T >= 5) and 25 % of any utterance's (T >= 64),
    and the blank and the last ragged column are among the frames it keeps."""
    c = R.case(vocab, B, T)
    R.check_gate(c, R.gate(c, mode))


@pytest.mark.parametrize("vocab", R.VOCABS)
def test_decode_patterns_in_the_reference(vocab):
    """The greedy decode's edges are in the reference's argmax maps: a blank at
    t = 0, "a, blank, a", a repeat and a blank across the 64-frame ballot
    boundary (T = 65, 129), all-blank utterances (T = 1, 2)."""
    for T in (65, 129):
        p = R.patterns(R.case(vocab, 35, T).argmax.numpy())
        assert all(p[k] for k in ("blank_at_0", "a_blank_a", "repeat_63_64", "blank_63_64")), (T, p)
    for T in (1, 2):
        assert R.patterns(R.case(vocab, 35, T).argmax.numpy())["all_blank"]


def test_greedy_on_hand_made_sequences():
    pred = np.array([[0, 3, 3, 0, 3, 5, 5, 1, 1], [0, 0, 0, 0, 0, 0, 0, 0, 0], [2, 2, 2, 2, 0, 0, 2, 4, 0]])
    tok, ln = R.greedy(pred)
    assert ln.tolist() == [4, 0, 3]
    assert tok[0].tolist() == [3, 3, 5, 1, -1, -1, -1, -1, -1]       # the blank separates equal tokens
    assert (tok[1] == -1).all()
    assert tok[2, :3].tolist() == [2, 2, 4]
    p = R.patterns(pred)
    assert p["blank_at_0"] and p["all_blank"] and p["a_blank_a"]
    assert not R.patterns(pred[2:, :4])["a_blank_a"]


# ---- mutations: a reference broken on the CPU must leave the bound ----------------
# A device output within K e of ref64 is further than K e from anything that is
# more than 2 K e from ref64, so each mutation below would fail the GPU test.
def _worst_bound(c):
    return max(R.bound(c, mode) for mode in ("fp32", "fp16", "gemm"))


@pytest.mark.parametrize("vocab", R.VOCABS)
def test_bounds_see_layernorm_parameters(vocab):
    """gamma / beta reset to 1 / 0 and gamma, beta swapped: both far outside
    the widest bound, at the smallest and the largest case."""
    m = R.model(vocab)
    swapped = copy.deepcopy(m)
    with torch.no_grad():
        swapped.audio_encoder[1].weight.copy_(m.audio_encoder[1].bias)
        swapped.audio_encoder[1].bias.copy_(m.audio_encoder[1].weight)
    for B, T in ((35, 1), (35, 129)):
        c = R.case(vocab, B, T)
        for broken in (R.plain_layernorm(m), swapped):
            assert float((R.ref64(broken, c.feats) - c.lp).abs().max()) > 20 * _worst_bound(c)


@pytest.mark.parametrize("vocab", R.VOCABS)
def test_bounds_see_gru_cell_and_blank_bias(vocab):
    """b_hn moved outside r (...) and the blank bias left out."""
    m = R.model(vocab)
    for B, T in ((35, 1), (35, 129)):
        c = R.case(vocab, B, T)
        assert float((R.forward(m, c.feats, None, bhn_outside=True) - c.lp).abs().max()) > 2 * _worst_bound(c)
        no_blank = R.ref64(R.trained_like(vocab, R.SEED, blank_bias=False), c.feats)
        assert float((no_blank - c.lp).abs().max()) > 2 * _worst_bound(c)
        ok = R.gate(c, "fp16")
        assert (no_blank.argmax(-1) != c.argmax)[ok].any()


def test_decode_equality_sees_a_collapsed_blank():
    """A decode that collapses "a, blank, a" to "a" differs from greedy() on the
    reference's own argmax maps (the equality the GPU test asserts)."""
    for vocab in R.VOCABS:
        pred = R.case(vocab, 35, 129).argmax.numpy()
        tok, ln = R.greedy(pred)
        wrong = [[t for i, t in enumerate(s) if i == 0 or t != s[i - 1]] for s in ([x for x in row if x != 0] for row in pred)]
        assert [len(w) for w in wrong] != ln.tolist()
