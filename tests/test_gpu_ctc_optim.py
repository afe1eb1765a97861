"""GPU tests of the GRU-CTC optimiser (wk_ctc_adam_step, wk_ctc_weights,
wk_ctc_set_weights, wk_ctc_optim_state; CTCModel.adam_step, CTCTrainer).

Optimiser alone: five generated gradients (tests/ctc_optim_ref.py) through
wk_ctc_adam_step against adam_ref in float64, per tensor within
K_OPT * max(e32, 16 * 2^-23), e32 being adam_ref in float32.  Consistency: after
steps or a set_weights, a handle computes bit for bit what a fresh handle
created from its exported blob computes -- inference, training forward and
backward -- so every layout wk_ctc_create derives on the host was rebuilt on the
device.  Then composition, resume, the loss curve of eight steps against the
reference's loop in float64 torch, and the refusals.

Every test that steps or sets weights creates its own handle."""
import ctypes as C
import os

import pytest
import torch

import ctc_grad_ref as G
import ctc_loss_ref as LR
import ctc_optim_ref as O
import ctc_ref as H

pytestmark = pytest.mark.gpu


def new_model(vocab, blob=None, precision="fp32"):
    import wakeword
    return wakeword.CTCModel((O.p0(vocab) if blob is None else blob).numpy(), vocab, precision=precision)


def new_trainer(vocab, **kw):
    import wakeword
    return wakeword.CTCTrainer(O.p0(vocab).numpy(), vocab, **kw)


def dev(t):
    return t.to("cuda:0")


# ---- 1. the optimiser alone ----------------------------------------------------------
@pytest.mark.parametrize("run", list(O.RUNS))
@pytest.mark.parametrize("vocab", G.VOCABS)
def test_optimiser_alone(gpu, vocab, run):
    c = O.opt_case(vocab, run)
    m = new_model(vocab)
    for g, n in zip(c.grads, c.norms):
        m.adam_step(dev(g), dev(n), **c.hyper)
    p = m.weights()
    mm, vv, step = m.optim_state()
    torch.cuda.synchronize()
    assert step == len(c.grads)
    assert bool(torch.isfinite(p).all())
    e = c.measure((p.cpu(), mm.cpu(), vv.cpu()))
    bad, worst = [], (0.0, None)
    for what in ("p", "m", "v"):
        for k in e[what]:
            unit = max(c.e32[what][k], O.FLOOR)
            ratio = e[what][k] / unit
            worst = max(worst, (ratio, f"{what} {k}"))
            print(f"opt V={vocab} {run} {what} {k}: e={e[what][k]:.3g} e32={c.e32[what][k]:.3g} ratio={ratio:.3g}")
            if not e[what][k] <= c.bound(what, k):
                bad.append((what, k, e[what][k], c.bound(what, k)))
    print(f"opt V={vocab} {run} worst ratio {worst[0]:.3g} at {worst[1]} (K_OPT = {O.K_OPT})")
    assert not bad, bad


# ---- 2. the norm paths ---------------------------------------------------------------
def test_norm_paths_and_determinism(gpu):
    """The norm computed by the step (d_norm NULL) and the one wk_ctc_backward
    returned for the same gradients give the same bits, as do two handles
    given the same inputs; both sides of the clip are met."""
    vocab = 512
    c = G.case(vocab, 17, 13)
    a, b, b2 = new_model(vocab), new_model(vocab), new_model(vocab)
    clipped = []
    for scale in (1.0, 1e-6):                       # a large gradient (clipped), then a small one (not)
        b.forward_train(c.feats)
        flat, norm = b.backward(c.D * scale, return_norm=True)
        clipped.append(float(norm) > O.HYPER["max_norm"])
        a.adam_step(flat, None, **O.HYPER)
        b.adam_step(flat, norm, **O.HYPER)
        b2.adam_step(flat.clone(), norm.clone(), **O.HYPER)
        wa, wb, wb2 = a.weights(), b.weights(), b2.weights()
        torch.cuda.synchronize()
        assert torch.equal(wa, wb) and torch.equal(wb, wb2)
    assert clipped == [True, False], clipped
    for x, y in zip(a.optim_state(), b.optim_state()):
        assert torch.equal(x, y) if torch.is_tensor(x) else x == y


def test_unaligned_blob_pointers(gpu):
    """A gradient, a blob or an output that is not 16-byte aligned takes the
    kernels' scalar path: the same bits as the 16-byte one."""
    from wakeword import _lib
    L = _lib.lib()
    vocab = 512
    c = O.opt_case(vocab, "plain")
    a, b = new_model(vocab), new_model(vocab)
    n = a.num_weights()

    def shifted(t):                      # the same values, one float past a 16-byte boundary
        buf = torch.empty(n + 1, device="cuda:0")
        buf[1:] = t
        assert buf[1:].data_ptr() % 16 == 4
        return buf[1:]

    g, norm = dev(c.grads[0]), dev(c.norms[0])
    assert g.data_ptr() % 16 == 0
    a.adam_step(g, norm, **c.hyper)
    b.adam_step(shifted(g), norm, **c.hyper)
    wa, wb = a.weights(), b.weights()
    out = shifted(torch.zeros(n))
    assert L.wk_ctc_weights(b._h, C.c_void_p(out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(wa, wb) and torch.equal(out, wb)
    b.set_weights(shifted(dev(O.p0(vocab))))
    assert torch.equal(b.weights().cpu(), O.p0(vocab))


# ---- 3. every layout is rebuilt ------------------------------------------------------
def _same_function(m, fresh, vocab, B, T):
    feats, D = G.features(vocab, B, T), G.dlogits(vocab, B, T)
    out = []
    for x in (m, fresh):
        tok, ln, lp = x.decode(feats, return_log_probs=True)
        lpt = x.forward_train(feats)
        flat = x.backward(D)
        out.append((tok, ln, lp, lpt, flat))
    torch.cuda.synchronize()
    for name, u, v in zip(("tokens", "lengths", "log-probs", "forward_train", "backward"), *out):
        assert torch.equal(u, v), name
    return out[0]


@pytest.mark.parametrize("vocab,B,T", [(512, 17, 13), (4100, 3, 5)])
def test_refresh_matches_a_fresh_handle(gpu, vocab, B, T):
    import wakeword
    c = O.opt_case(vocab, "plain")
    m = new_model(vocab)
    w0 = m.weights()
    torch.cuda.synchronize()
    assert torch.equal(w0.cpu(), O.p0(vocab))                      # an unstepped handle gives its blob back
    before = m.decode(G.features(vocab, B, T), return_log_probs=True)[2].clone()
    for g, n in zip(c.grads[:3], c.norms[:3]):
        m.adam_step(dev(g), dev(n), **c.hyper)
    w = m.weights().cpu()
    assert not torch.equal(w, O.p0(vocab))
    fresh = wakeword.CTCModel(w.numpy(), vocab)                    # the host packers
    after = _same_function(m, fresh, vocab, B, T)
    assert not torch.equal(before, after[2])                       # wk_ctc_forward runs on the new weights
    # set_weights of another blob on the used handle (state dict form), against a fresh handle of it
    gen = torch.Generator().manual_seed(77 + vocab)
    other = (O.p0(vocab) * 0.9 + 0.02 * torch.randn(O.p0(vocab).shape, generator=gen)).contiguous()
    m.set_weights(wakeword.unpack_grads(other, vocab))
    assert torch.equal(m.weights().cpu(), other)
    _same_function(m, wakeword.CTCModel(other.numpy(), vocab), vocab, B, T)
    sd = m.state_dict()
    assert list(sd) == [k for k, _ in O.spec(vocab)]
    assert all((sd[k] == v.numpy()).all() for k, v in wakeword.unpack_grads(other, vocab).items())


# ---- 4. composition -------------------------------------------------------------------
def test_trainer_step_is_loss_and_grad_then_adam_step(gpu):
    vocab, B, T, _ = O.TRAJ
    feats, labels, il, tl = O.traj_batch(vocab, B, T)
    a, b = new_trainer(vocab, zero_infinity=True), new_trainer(vocab, zero_infinity=True)
    for _ in range(3):
        la = a.step(feats, labels, il, tl)
        lb, grads, norm = b.model.loss_and_grad(feats, labels, il, tl, zero_infinity=True)
        b.model.adam_step(grads, norm, **b.hyper)
        wa, wb = a.weights(), b.weights()
        torch.cuda.synchronize()
        assert la.dim() == 0 and la.is_cuda and torch.equal(la, lb)
        assert torch.equal(wa, wb)


# ---- 5. resume ----------------------------------------------------------------------
def test_resume_from_exported_state(gpu):
    vocab, B, T, _ = O.TRAJ
    feats, labels, il, tl = O.traj_batch(vocab, B, T)
    import wakeword
    a = new_trainer(vocab, zero_infinity=True)
    for _ in range(4):
        a.step(feats, labels, il, tl)
    b = new_trainer(vocab, zero_infinity=True)
    for _ in range(2):
        b.step(feats, labels, il, tl)
    w, (m, v, step) = b.weights().cpu().numpy(), b.optim_state()
    assert step == 2
    r = wakeword.CTCTrainer(w, vocab, zero_infinity=True)
    r.load_optim_state(m, v, step)
    for _ in range(2):
        r.step(feats, labels, il, tl)
    wa, wr = a.weights(), r.weights()
    sa, sr = a.optim_state(), r.optim_state()
    torch.cuda.synchronize()
    assert torch.equal(wa, wr)
    assert torch.equal(sa[0], sr[0]) and torch.equal(sa[1], sr[1]) and sa[2] == sr[2] == 4
    r.load_optim_state(None, None, 0)                             # reset
    m0, v0, s0 = r.optim_state()
    assert s0 == 0 and not bool(m0.any()) and not bool(v0.any())


# ---- 6. the loss curve ----------------------------------------------------------------
def test_training_trajectory(gpu):
    """Eight steps at the reference's hyper-parameters against the same loop
    in float64 torch-CPU.  The loss curve is compared, not the weights: Adam
    turns a gradient's sign into a step of lr, so fp32 noise on a near-zero
    gradient moves single weights by up to 2 lr, which the loss does not see
    to first order."""
    import wakeword
    vocab, B, T, steps = O.TRAJ
    feats, labels, il, tl = O.traj_batch(vocab, B, T)
    loss64, norm64, w64 = O.trajectory(vocab, B, T, steps, torch.float64)
    loss32, _, w32 = O.trajectory(vocab, B, T, steps, torch.float32)
    e32 = max(abs(a - b) for a, b in zip(loss32, loss64))
    # CTCModel.loss's bound on this batch (tests/test_gpu_ctc_grad.py), at the initial weights
    _, nll64, _ = G.e2e_reference(H.model(vocab), feats, labels, il, tl, torch.float64)
    _, nll32, _ = G.e2e_reference(H.model(vocab), feats, labels, il, tl, torch.float32)
    own = LR.K_LOSS * torch.maximum((nll32.double() - nll64).abs().max(), LR.EPS32 * nll64.abs())
    per_utt = torch.tensor(il).double() * H.bound(H.Case(vocab, feats), "fp32") + own
    loss_bound = float((per_utt / torch.tensor(tl).clamp(min=1)).mean())
    unit = max(e32, loss_bound)
    assert all(b < a for a, b in zip(loss64, loss64[1:])), loss64
    assert max(norm64) > O.HYPER["max_norm"] > min(norm64), norm64      # the clip on and off

    t = new_trainer(vocab, zero_infinity=True)
    got, norms = [], []
    for _ in range(steps):
        loss, _, norm = t.grad(feats, labels, il, tl)
        t.apply()
        got.append(loss)
        norms.append(norm)
    w = t.weights().cpu().double()
    got, norms = [float(x) for x in got], [float(x) for x in norms]
    worst = 0.0
    for k, (a, b) in enumerate(zip(got, loss64)):
        worst = max(worst, abs(a - b) / unit)
        print(f"traj step {k}: loss={a:.7g} loss64={b:.7g} err={abs(a - b):.3g} norm={norms[k]:.4g} norm64={norm64[k]:.4g}")
    print(f"traj e32={e32:.3g} loss bound={loss_bound:.3g} worst ratio {worst:.3g} (K_TRAJ = {O.K_TRAJ})")
    p0 = O.p0(vocab).double()
    for k in (k for k, _ in O.spec(vocab)):       # for the record only
        d64 = wakeword.unpack_grads(w64 - p0, vocab)[k]
        rms = lambda x: float(x.pow(2).mean().sqrt())
        print(f"traj {k}: rms displacement {rms(d64):.3g}, rms error device {rms(wakeword.unpack_grads(w - w64, vocab)[k]):.3g}, "
              f"torch fp32 {rms(wakeword.unpack_grads(w32.double() - w64, vocab)[k]):.3g}")
    assert all(b < a for a, b in zip(got, got[1:])), got
    assert max(norms) > O.HYPER["max_norm"] > min(norms), norms
    assert all(abs(a - b) <= O.K_TRAJ * unit for a, b in zip(got, loss64)), (got, loss64, unit)


# ---- 7. limits --------------------------------------------------------------------------
def _all_five(L, h, n):
    from wakeword import _lib
    buf = torch.zeros(n, device="cuda:0")
    buf2 = torch.zeros(n, device="cuda:0")
    opt = _lib.WkCtcAdam(1e-3, 0.9, 0.999, 1e-8, 0.0, 5.0)
    step = C.c_int64(0)
    p, p2 = C.c_void_p(buf.data_ptr()), C.c_void_p(buf2.data_ptr())
    return [L.wk_ctc_weights(h, p, None), L.wk_ctc_set_weights(h, p, None), L.wk_ctc_adam_step(h, C.byref(opt), p, None, None),
            L.wk_ctc_optim_state(h, p, p2, C.byref(step), None), L.wk_ctc_set_optim_state(h, None, None, 0, None)]


def test_limits(gpu):
    import wakeword
    from wakeword import _lib
    L = _lib.lib()
    vocab = 512
    h = new_model(vocab, precision="fp16")
    n = h.num_weights()
    assert _all_five(L, h._h, n) == [4] * 5
    assert b"fp32 handles only" in L.wk_last_error()
    os.environ["WAKEWORD_CTC_MIX"] = "out16"
    try:
        mixed = new_model(vocab)
    finally:
        del os.environ["WAKEWORD_CTC_MIX"]
    assert _all_five(L, mixed._h, n) == [4] * 5
    assert b"WAKEWORD_CTC_MIX" in L.wk_last_error()
    # a trained model reaches the fp16 inference path
    _, B, T, _ = O.TRAJ
    feats, labels, il, tl = O.traj_batch(vocab, B, T)
    t = new_trainer(vocab, zero_infinity=True)
    t.step(feats, labels, il, tl)
    m16 = t.to_model("fp16")
    tok, ln, _ = m16.decode(feats)
    torch.cuda.synchronize()
    assert tok.shape == (B, T) and bool((ln >= 0).all()) and bool((ln <= T).all())
    with pytest.raises(ValueError):
        t.model.adam_step(torch.zeros(n - 1), None)
    with pytest.raises(ValueError):
        wakeword.CTCTrainer(O.p0(vocab).numpy(), vocab, lr=-1.0)
