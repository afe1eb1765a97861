"""CPU tests of the GRU-CTC backward's references (tests/ctc_grad_ref.py): the
hand-written float64 backward equals torch.autograd on the module in double;
each mutation of it moves a tensor by more than twice the GPU test's bound (so
the bound sees what it is for); the ReLU exclusion rule, computed from the
reference alone, zeroes at most a third of every case's utterances."""
import pytest
import torch

import ctc_grad_ref as G


@pytest.mark.parametrize("vocab,B,T", [(512, 17, 13), (512, 35, 5), (4100, 3, 2), (512, 2, 1)])
def test_hand_backward_equals_autograd(vocab, B, T):
    c = G.Case(vocab, B, T)
    hand = G.hand_backward(c.model, c.feats, c.D)
    assert set(hand) == set(c.g64) == set(G.keys(vocab))
    for k in G.keys(vocab):
        assert hand[k].shape == c.g64[k].shape, k
        assert G.rel_err(hand[k], c.g64[k]) <= 1e-10, (k, G.rel_err(hand[k], c.g64[k]))


@pytest.fixture(scope="module")
def mcase():
    return G.case(512, 35, 13)


@pytest.mark.parametrize("mutation", G.MUTATIONS)
def test_mutation_exceeds_twice_the_bound(mcase, mutation):
    """Some tensor moves by more than 2 K max(e32, FLOOR) for both K: K times
    the yardstick stays below half the smallest mutation error."""
    c = mcase
    wrong = G.hand_backward(c.model, c.feats, c.D, mutation)
    worst = max((G.rel_err(wrong[k], c.g64[k]) / c.bound(k, max(G.K_BWD, G.K_E2E)), k) for k in c.g64)
    print(f"mutation {mutation}: error / bound = {worst[0]:.3g} on {worst[1]}")
    assert worst[0] > 2.0, worst


def test_mutations_are_mistakes_not_noise(mcase):
    c = mcase
    right = G.hand_backward(c.model, c.feats, c.D)
    assert max(G.rel_err(right[k], c.g64[k]) for k in c.g64) <= 1e-10
    assert max(c.e32.values()) < 1e-4      # the yardstick itself is fp32 rounding


@pytest.mark.parametrize("vocab", G.VOCABS)
def test_relu_rule_cap(vocab):
    counts = {}
    for B, T in G.CASES:
        feats = G.features(vocab, B, T)
        assert tuple(feats.shape) == (B, T, 80)
        zeroed, delta = G.relu_zeroed(G.R.model(vocab), feats)
        assert 0.0 < delta < 1e-4
        assert len(zeroed) <= G.MAX_ZEROED * B and len(zeroed) < B, (B, T, zeroed)
        counts[(B, T)] = len(zeroed)
    print(f"V={vocab} zeroed utterances: {counts}")
    assert any(counts.values())            # the rule is exercised somewhere


def test_e2e_targets_hold_the_edges():
    labels, il, tl = G.e2e_targets(512, 35, 65, [3])
    assert il[3] == 0 and min(il[:3]) > 0 and len(set(il)) > 2 and max(il) == 65
    assert il[34] < tl[34]                                   # no valid alignment
    assert bool((labels[:, 0] == labels[:, 1]).all())        # repeats
    assert int(labels.max()) == 511
    m = G.R.model(512)
    loss, nll, g = G.e2e_reference(m, G.R.features_case(3, 13), *G.e2e_targets(512, 3, 13, []), torch.float64)
    assert float(nll[2]) == 0.0 and float(nll[0]) > 0.0 and torch.isfinite(loss)
    assert all(torch.isfinite(v).all() for v in g.values())
