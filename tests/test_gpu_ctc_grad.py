"""GPU tests of wk_ctc_forward_train / wk_ctc_backward (CTCModel.forward_train,
backward, loss_and_grad) against float64 autograd on the CPU.

Backward alone: the same seeded dlogits D go to a float64 reference,
(logits64 * D).sum() through autograd, and to wk_ctc_backward, so wk_ctc_loss's
own error does not enter.  Per tensor e = max|g - g64| / max|g64| must satisfy
    e <= K_BWD * max(e32, 16 * 2^-23)
e32 being torch-CPU fp32 autograd's e on the same case (tests/ctc_grad_ref.py;
how K_BWD and K_E2E were set: profiles/ctc_grad_bounds.md).  End to end:
loss_and_grad against float64 F.ctc_loss(log_softmax(module64(feats))), the
loss within CTCModel.loss's bound (tests/test_gpu_ctc_loss.py), the gradients
within K_E2E * max(e32, floor).  Utterances with a ReLU pre-activation within
rounding of 0 are zeroed by the reference alone (ctc_grad_ref.relu_zeroed).

Cases: the trained-like model at V = 512 and 4100 (ragged last V tile); the
16-utterance tile edges, one row in all, row counts that are no multiple of a
tile, T past 128 and row counts on both sides of the split of a reduction."""
import ctypes as C
import functools

import pytest
import torch

import ctc_grad_ref as G
import ctc_loss_ref as LR
import ctc_ref as H

pytestmark = pytest.mark.gpu

E2E_CASES = ((512, 35, 65), (512, 8, 129), (4100, 33, 13), (4100, 35, 64))


@functools.lru_cache(maxsize=None)
def dev_model(vocab, precision="fp32"):
    import wakeword
    return wakeword.CTCModel(H.model(vocab).state_dict(), vocab, precision=precision)


def _report(tag, c, got, K):
    """Prints every tensor's error, yardstick and ratio; returns the failures."""
    bad, worst = [], 0.0
    for k in G.keys(c.vocab):
        e = G.rel_err(got[k], c_ref(c, tag)[k])
        unit = max(c_e32(c, tag)[k], G.FLOOR)
        worst = max(worst, e / unit)
        print(f"{tag} V={c.vocab} B={c.B} T={c.T} {k}: e={e:.3g} e32={c_e32(c, tag)[k]:.3g} ratio={e / unit:.3g}")
        if not e <= K * unit:
            bad.append((k, e, K * unit))
    print(f"{tag} V={c.vocab} B={c.B} T={c.T} worst ratio {worst:.3g} (K = {K})")
    return bad


_e2e = {}


def c_ref(c, tag):
    return c.g64 if tag == "bwd" else _e2e[(c.vocab, c.B, c.T)]["g64"]


def c_e32(c, tag):
    return c.e32 if tag == "bwd" else _e2e[(c.vocab, c.B, c.T)]["e32"]


@pytest.mark.parametrize("B,T", G.CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("vocab", G.VOCABS)
def test_backward_parity(gpu, vocab, B, T):
    import wakeword
    c = G.case(vocab, B, T)
    c.check_cap()
    m = dev_model(vocab)
    lp = m.forward_train(c.feats)
    flat, norm = m.backward(c.D, return_norm=True)
    flat2 = m.backward(c.D)
    _, _, lp_inf = m.decode(c.feats, return_log_probs=True)
    torch.cuda.synchronize()
    assert torch.equal(lp, lp_inf)                     # bit for bit wk_ctc_forward's log-probs
    assert torch.equal(flat, flat2)                    # the same inputs give the same bits
    assert bool(torch.isfinite(flat).all())
    want = float(flat.double().norm())
    assert abs(float(norm) - want) <= 1e-6 * want
    bad = _report("bwd", c, wakeword.unpack_grads(flat.cpu(), vocab), G.K_BWD)
    assert not bad, bad


@pytest.mark.parametrize("vocab,B,T", E2E_CASES)
def test_loss_and_grad_end_to_end(gpu, vocab, B, T):
    c = G.case(vocab, B, T)
    c.check_cap()
    labels, il, tl = G.e2e_targets(vocab, B, T, c.zeroed)
    assert any(i < T for i in il if i > 1) and il[B - 1] < tl[B - 1]
    loss64, nll64, g64 = G.e2e_reference(c.model, c.feats, labels, il, tl, torch.float64)
    loss32, nll32, g32 = G.e2e_reference(c.model, c.feats, labels, il, tl, torch.float32)
    _e2e[(vocab, B, T)] = {"g64": g64, "e32": {k: G.rel_err(g32[k], g64[k]) for k in g64}}
    m = dev_model(vocab)
    loss, grads, norm = m.loss_and_grad(c.feats, labels, il, tl, reduction="mean", zero_infinity=True)
    torch.cuda.synchronize()
    # the loss: CTCModel.loss's bound (test_gpu_ctc_loss.test_ctc_model_loss), per utterance, then the mean's
    t_il, t_tl = torch.tensor(il), torch.tensor(tl)
    own = LR.K_LOSS * torch.maximum((nll32.double() - nll64).abs().max(), LR.EPS32 * nll64.abs())
    hc = H.Case(vocab, c.feats)
    bound = t_il.double() * H.bound(hc, "fp32") + own
    mean_bound = float((bound / t_tl.clamp(min=1)).mean())
    print(f"e2e V={vocab} B={B} T={T} loss err={abs(float(loss) - float(loss64)):.3g} bound={mean_bound:.3g}")
    assert abs(float(loss) - float(loss64)) <= mean_bound
    flat = torch.cat([grads[k].reshape(-1) for k in G.keys(vocab)])
    want = float(flat.double().norm())
    assert abs(float(norm) - want) <= 1e-6 * want
    bad = _report("e2e", c, {k: v.cpu() for k, v in grads.items()}, G.K_E2E)
    assert not bad, bad


def test_inference_unchanged_by_training_calls(gpu):
    """wk_ctc_forward and wk_ctc_frame_argmax give, after a forward_train +
    backward pair on the same handle (at another geometry), what they gave
    before: the training workspace is apart from theirs."""
    vocab = 512
    m = dev_model(vocab)
    c, other = G.case(vocab, 17, 13), G.case(vocab, 35, 5)
    tok, ln, lp = m.decode(c.feats, return_log_probs=True)
    pred = m.frame_argmax(17, 13)
    before = [t.clone() for t in (tok, ln, lp, pred)]
    m.forward_train(other.feats)
    m.backward(other.D)
    pred_after = m.frame_argmax(17, 13)                 # still the last wk_ctc_forward's
    tok2, ln2, lp2 = m.decode(c.feats, return_log_probs=True)
    torch.cuda.synchronize()
    for a, b in zip(before, (tok2, ln2, lp2, pred_after)):
        assert torch.equal(a, b)


def test_refusals(gpu):
    from wakeword import _lib
    L = _lib.lib()
    vocab = 512
    m = dev_model(vocab)
    c = G.case(vocab, 17, 13)
    m.forward_train(c.feats)
    n = L.wk_ctc_num_weights(C.byref(m.cfg))
    out = torch.empty(n, device="cuda:0")
    d = c.D.to("cuda:0")
    for batch, T in ((17, 12), (16, 13), (13, 17)):
        assert L.wk_ctc_backward(m._h, batch, T, C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), None, None) == 1
        assert b"last wk_ctc_forward_train" in L.wk_last_error()
    with pytest.raises(_lib.WakewordError):
        m.backward(c.D[:, :12])
    m.backward(c.D)                                     # the matching geometry is still accepted
    h = dev_model(vocab, "fp16")
    f = c.feats.to("cuda:0")
    lp = torch.empty((17, 13, vocab), device="cuda:0")
    assert L.wk_ctc_forward_train(h._h, C.c_void_p(f.data_ptr()), 17, 13, C.c_void_p(lp.data_ptr()), None) == 4
    assert L.wk_ctc_backward(h._h, 17, 13, C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), None, None) == 4
    torch.cuda.synchronize()
