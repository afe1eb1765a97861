"""CPU tests of the dropout references (tests/ctc_dropout_ref.py): the numpy
Philox against its known answers, the masks' statistics and addressing, the
masked module against the eval-mode reference, the hand-written masked
backward against autograd, and the mutations against the GPU bound."""
import re

import numpy as np
import pytest
import torch

import ctc_dropout_ref as DR
import ctc_grad_ref as G

KNOWN = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
CASE = (512, 17, 13)           # vocab, B, T of the module tests
P = (0.2, 0.2)


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    got = DR.philox4x32_10(np.array(ctr, np.uint64), key)
    assert " ".join(f"{int(w):08x}" for w in got) == want


def test_known_answers_are_those_of_the_device_header():
    """csrc/wk_philox.h quotes the same three answers and constants."""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    txt = open(os.path.join(here, "..", "esp32-wake-word_amd", "csrc", "wk_philox.h")).read()
    for _, _, want in KNOWN:
        assert want in txt
    for const in ("0xD2511F53u", "0xCD9E8D57u", "0x9E3779B9u", "0xBB67AE85u"):
        assert const in txt
    assert not re.search(r"\basm\b", txt)


def test_threshold_and_scale_are_the_abi_floats():
    assert DR.threshold(0.0) == 0
    assert DR.threshold(0.5) == 2 ** 31
    assert DR.threshold(0.2) == int(np.floor(float(np.float32(0.2)) * 2.0 ** 32)) == 858993472      # fl32(0.2) > 0.2
    assert DR.scale(0.5) == 2.0 and DR.scale(0.0) == 1.0
    assert DR.scale(0.2) == float(np.float32(1.0) / np.float32(0.8))


def test_kept_share():
    n = 2 ** 20
    kept = int((DR.site_words(0, 0, 0, n) >= DR.threshold(0.2)).sum())
    sigma = (0.16 / n) ** 0.5
    assert abs(kept / n - 0.8) <= 4.0 * sigma, (kept / n, sigma)


def test_masks_differ_by_offset_site_and_seed():
    B, T = 17, 13
    a0, a1 = DR.masks(7, 0, B, T, *P)
    b0, b1 = DR.masks(7, 1, B, T, *P)
    c0, _ = DR.masks(8, 0, B, T, *P)
    h0, _ = DR.masks(7, 2 ** 32, B, T, *P)          # the offset's high word enters
    assert a0.shape == (B, T, 128) and a1.shape == (B, T, 256) and a0.dtype == torch.bool
    assert not torch.equal(a0, b0) and not torch.equal(a1, b1) and not torch.equal(a0, c0) and not torch.equal(a0, h0)
    n = a0.numel()
    assert not torch.equal(a0.reshape(-1), a1.reshape(-1)[:n])         # the two sites on their common prefix
    s0, s1 = DR.masks(7, 0, B, T, *P, swap=True)
    assert torch.equal(s0.reshape(-1), a1.reshape(-1)[:n]) and torch.equal(s1.reshape(-1)[:n], a0.reshape(-1))
    on0, on1 = DR.masks(7, 0, B, T, 0.0, 0.0)
    assert bool(on0.all()) and bool(on1.all())
    # one Philox block is four adjacent elements: block q of a longer stream is block q of a shorter one
    assert np.array_equal(DR.site_words(7, 3, 1, 64)[:32], DR.site_words(7, 3, 1, 32))


def test_all_ones_masks_give_the_eval_mode_gradients():
    c = G.case(*CASE)
    ones = (torch.ones(c.B, c.T, 128, dtype=torch.bool), torch.ones(c.B, c.T, 256, dtype=torch.bool))
    _, g = DR.autograd(c.model, c.feats, c.D, *ones, (0.0, 0.0), torch.float64)
    for k in G.keys(c.vocab):
        assert G.rel_err(g[k], c.g64[k]) <= 1e-12, k


@pytest.fixture(scope="module")
def masked():
    c = G.case(*CASE)
    m0, m1 = DR.masks(3, 5, c.B, c.T, *P)
    return c, m0, m1, DR.DropCase(*CASE, P, m0, m1)


def test_hand_backward_is_autograd_of_the_masked_module(masked):
    c, m0, m1, dc = masked
    g = DR.hand_backward(c.model, c.feats, c.D, m0, m1, P)
    for k in G.keys(c.vocab):
        assert G.rel_err(g[k], dc.ref[k]) <= 1e-12, k
    assert G.rel_err(dc.ref["gru.weight_ih_l1"], c.g64["gru.weight_ih_l1"]) > 0.01        # the masks change the function


# The factor by which each mutation exceeds the GPU bound K_BWD * max(e32, FLOOR) on its worst tensor.  Reached with
# K_BWD = 1.61: 1.52e5, 1.93e5, 1.51e5, 2.99e5, 4.3e5; asserted at a tenth of that (the CPU's BLAS may reorder e32's sums).
REACHED = {"bwd_mask0": 1.5e4, "bwd_mask1": 1.9e4, "no_scale": 1.5e4, "hprev_dropped": 2.9e4, "sites_swapped": 4.3e4}


@pytest.mark.parametrize("mutation", DR.MUTATIONS)
def test_mutations_exceed_the_gpu_bound(masked, mutation):
    c, m0, m1, dc = masked
    if mutation == "sites_swapped":
        g = DR.hand_backward(c.model, c.feats, c.D, *DR.masks(3, 5, c.B, c.T, *P, swap=True), P)
    else:
        g = DR.hand_backward(c.model, c.feats, c.D, m0, m1, P, mutation)
    factor = max(G.rel_err(g[k], dc.ref[k]) / (DR.K_BWD * max(dc.e32[k], DR.FLOOR)) for k in G.keys(c.vocab))
    print(f"{mutation}: {factor:.3g} x the bound")
    assert factor > 2.0 and factor >= REACHED[mutation], factor
