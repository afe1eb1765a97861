"""GPU tests of train-mode dropout in the GRU-CTC head
(wk_ctc_forward_train_dropout, wk_ctc_dropout_masks; CTCModel.forward_train /
loss_and_grad with dropout=, CTCModel.dropout_masks, CTCTrainer(dropout=)).

Mask bits: the exported masks equal the numpy Philox masks exactly.  Dropout
off: p = (0, 0) gives wk_ctc_forward_train / wk_ctc_backward's bits, and a
handle that ran dropout computes afterwards what one that never did computes.
Parity: log-probs and every parameter gradient against the float64 masked
module of tests/ctc_dropout_ref.py fed the exported masks, the backward alone
(seeded dlogits) and end to end through wk_ctc_loss, per tensor
    e <= K * max(e32, 16 * 2^-23)
with e32 the same module in float32 on the CPU (how K_BWD, K_E2E and K_TRAJ
were set: profiles/ctc_dropout_bounds.md).  Utterances with a ReLU
pre-activation within rounding of 0 are zeroed by the reference alone, as in
tests/test_gpu_ctc_grad.py: the set depends on features and weights only.
Then determinism, the refusals, and the trainer: composition, resume with the
RNG state, the eval-mode validation loss and an eight-step loss curve."""
import ctypes as C
import functools

import pytest
import torch

import ctc_dropout_ref as DR
import ctc_grad_ref as G
import ctc_loss_ref as LR
import ctc_optim_ref as O
import ctc_ref as H

pytestmark = pytest.mark.gpu

CASE_P = [(v, B, T, p) for (v, B, T) in DR.CASES for p in DR.PROBS[(v, B, T)]]
SEED, OFFSET = DR.STREAMS[1]


@functools.lru_cache(maxsize=None)
def dev_model(vocab, precision="fp32"):
    import wakeword
    return wakeword.CTCModel(H.model(vocab).state_dict(), vocab, precision=precision)


@functools.lru_cache(maxsize=None)
def plain_model(vocab):
    """A handle that no dropout call ever touches."""
    import wakeword
    return wakeword.CTCModel(H.model(vocab).state_dict(), vocab)


def exported(m):
    m0, m1 = m.dropout_masks()
    return m0.cpu(), m1.cpu()


def assert_masks(m, seed, offset, B, T, p):
    m0, m1 = exported(m)
    w0, w1 = DR.masks(seed, offset, B, T, *p)
    assert m0.dtype == torch.bool and m0.shape == (B, T, 128) and m1.shape == (B, T, 256)
    assert torch.equal(m0, w0) and torch.equal(m1, w1), (seed, offset, B, T, p)
    return m0, m1


# ---- 1. the mask bits ------------------------------------------------------------------
@pytest.mark.parametrize("vocab,B,T", DR.CASES)
def test_mask_bits(gpu, vocab, B, T):
    m = dev_model(vocab)
    feats = G.features(vocab, B, T)
    for p in DR.PROBS[(vocab, B, T)]:
        for seed, offset in DR.STREAMS:
            m.forward_train(feats, dropout=p, seed=seed, offset=offset)
            m0, m1 = assert_masks(m, seed, offset, B, T, p)
            for mask, q in ((m0, p[0]), (m1, p[1])):
                assert bool(mask.all()) == (q == 0.0)               # a site that is off exports all ones
    m.forward_train(feats)                                          # a plain forward records "none"
    m0, m1 = exported(m)
    assert bool(m0.all()) and bool(m1.all())


# ---- 2. dropout off --------------------------------------------------------------------
@pytest.mark.parametrize("vocab,B,T", DR.CASES)
def test_dropout_off_is_the_plain_path(gpu, vocab, B, T):
    c = G.case(vocab, B, T)
    m, fresh = dev_model(vocab), plain_model(vocab)
    lp0 = fresh.forward_train(c.feats)
    g0, n0 = fresh.backward(c.D, return_norm=True)
    lp = m.forward_train(c.feats, dropout=(0.0, 0.0), seed=SEED, offset=OFFSET)
    g, n = m.backward(c.D, return_norm=True)
    torch.cuda.synchronize()
    assert torch.equal(lp, lp0) and torch.equal(g, g0) and torch.equal(n, n0)
    # after a dropout forward and backward, the plain pair again
    lpd = m.forward_train(c.feats, dropout=0.2, seed=SEED, offset=OFFSET)
    gd = m.backward(c.D)
    lp = m.forward_train(c.feats)
    g, n = m.backward(c.D, return_norm=True)
    _, _, lp_inf = m.decode(c.feats, return_log_probs=True)
    torch.cuda.synchronize()
    assert not torch.equal(lpd, lp0) and not torch.equal(gd, g0)
    assert torch.equal(lp, lp0) and torch.equal(g, g0) and torch.equal(n, n0) and torch.equal(lp_inf, lp0)


# ---- 3. parity -------------------------------------------------------------------------
@pytest.mark.parametrize("vocab,B,T,p", CASE_P, ids=lambda v: str(v))
def test_backward_parity(gpu, vocab, B, T, p):
    import wakeword
    c = G.case(vocab, B, T)
    c.check_cap()
    m = dev_model(vocab)
    lp = m.forward_train(c.feats, dropout=p, seed=SEED, offset=OFFSET)
    flat, norm = m.backward(c.D, return_norm=True)
    m0, m1 = assert_masks(m, SEED, OFFSET, B, T, p)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(flat).all())
    want = float(flat.double().norm())
    assert abs(float(norm) - want) <= 1e-6 * want
    dc = DR.DropCase(vocab, B, T, p, m0, m1)
    got = dict(wakeword.unpack_grads(flat.cpu(), vocab), log_probs=lp.cpu())
    bad, _ = DR.report("drop-bwd", dc.ref, dc.e32, got, DR.K_BWD, f"V={vocab} B={B} T={T} p={p}")
    assert not bad, bad


@pytest.mark.parametrize("vocab,B,T,p", CASE_P, ids=lambda v: str(v))
def test_loss_and_grad_end_to_end(gpu, vocab, B, T, p):
    c = G.case(vocab, B, T)
    c.check_cap()
    labels, il, tl = G.e2e_targets(vocab, B, T, c.zeroed)
    m = dev_model(vocab)
    lp = m.forward_train(c.feats, dropout=p, seed=SEED, offset=OFFSET)
    loss, grads, norm = m.loss_and_grad(c.feats, labels, il, tl, reduction="mean", zero_infinity=True, dropout=p, seed=SEED,
                                        offset=OFFSET)
    m0, m1 = assert_masks(m, SEED, OFFSET, B, T, p)
    torch.cuda.synchronize()
    loss64, nll64, lp64, g64 = DR.e2e_reference(c.model, c.feats, labels, il, tl, m0, m1, p, torch.float64)
    loss32, nll32, lp32, g32 = DR.e2e_reference(c.model, c.feats, labels, il, tl, m0, m1, p, torch.float32)
    ref = dict(g64, log_probs=lp64)
    e32 = {k: G.rel_err(v, ref[k]) for k, v in dict(g32, log_probs=lp32).items()}
    # the loss: test_gpu_ctc_grad's form, with the masked function's own log-prob bound
    lp_bound = DR.K_E2E * max(e32["log_probs"], DR.FLOOR) * float(lp64.abs().max())
    own = LR.K_LOSS * torch.maximum((nll32.double() - nll64).abs().max(), LR.EPS32 * nll64.abs())
    mean_bound = float(((torch.tensor(il).double() * lp_bound + own) / torch.tensor(tl).clamp(min=1)).mean())
    print(f"drop-e2e V={vocab} B={B} T={T} p={p} loss err={abs(float(loss) - float(loss64)):.3g} bound={mean_bound:.3g}")
    assert abs(float(loss) - float(loss64)) <= mean_bound
    flat = torch.cat([grads[k].reshape(-1) for k in G.keys(vocab)])
    want = float(flat.double().norm())
    assert abs(float(norm) - want) <= 1e-6 * want
    got = dict({k: v.cpu() for k, v in grads.items()}, log_probs=lp.cpu())
    bad, _ = DR.report("drop-e2e", ref, e32, got, DR.K_E2E, f"V={vocab} B={B} T={T} p={p}")
    assert not bad, bad


# ---- 4. determinism and the refusals ------------------------------------------------------
def test_same_stream_same_bits_other_offset_other_mask(gpu):
    vocab, B, T = 512, 17, 13
    c = G.case(vocab, B, T)
    m = dev_model(vocab)
    runs = []
    for offset in (5, 5, 6):
        lp = m.forward_train(c.feats, dropout=0.2, seed=3, offset=offset)
        runs.append((lp, m.backward(c.D), *m.dropout_masks()))
    torch.cuda.synchronize()
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0], runs[2]):
        assert not torch.equal(a, b)


def test_refusals(gpu):
    import wakeword
    from wakeword import _lib
    L = _lib.lib()
    vocab, B, T = 512, 17, 13
    c = G.case(vocab, B, T)
    new = wakeword.CTCModel(H.model(vocab).state_dict(), vocab)
    f = c.feats.to("cuda:0")
    lp = torch.empty((B, T, vocab), device="cuda:0")
    m0 = torch.empty((B, T, 128), dtype=torch.uint8, device="cuda:0")

    def fwd(h, drop):
        return L.wk_ctc_forward_train_dropout(h, C.c_void_p(f.data_ptr()), B, T, C.byref(drop) if drop is not None else None,
                                              C.c_void_p(lp.data_ptr()), None)

    assert L.wk_ctc_dropout_masks(new._h, C.c_void_p(m0.data_ptr()), None, None) == 1      # before any training forward
    assert b"no training forward" in L.wk_last_error()
    with pytest.raises(ValueError):
        new.dropout_masks()
    assert fwd(new._h, None) == 1
    for pe, pg, off in ((-0.5, 0.2, 0), (0.2, 1.0, 0), (float("nan"), 0.2, 0), (0.2, 0.2, 2 ** 63)):
        assert fwd(new._h, _lib.WkCtcDropout(pe, pg, 0, off)) == 1, (pe, pg, off)
    assert L.wk_ctc_dropout_masks(new._h, C.c_void_p(m0.data_ptr()), None, None) == 1      # a refused forward is none
    for bad in (1.0, (0.2, -0.1)):
        with pytest.raises(ValueError):
            new.forward_train(c.feats, dropout=bad)
    with pytest.raises(ValueError):
        new.forward_train(c.feats, dropout=0.2, offset=2 ** 63)
    assert fwd(new._h, _lib.WkCtcDropout(0.2, 0.2, 0, 2 ** 63 - 1)) == 0
    assert L.wk_ctc_dropout_masks(new._h, C.c_void_p(m0.data_ptr()), None, None) == 0      # either pointer may be null
    h = dev_model(vocab, "fp16")
    assert fwd(h._h, _lib.WkCtcDropout(0.2, 0.2, 0, 0)) == 4
    assert L.wk_ctc_dropout_masks(h._h, C.c_void_p(m0.data_ptr()), None, None) == 4
    torch.cuda.synchronize()


# ---- 5. the trainer -------------------------------------------------------------------------
def new_trainer(vocab, **kw):
    import wakeword
    return wakeword.CTCTrainer(O.p0(vocab).numpy(), vocab, zero_infinity=True, **kw)


def test_trainer_step_is_loss_and_grad_then_adam_step(gpu):
    vocab, B, T, _ = DR.TRAJ
    feats, labels, il, tl = DR.traj_batch(vocab, B, T)
    a, b = new_trainer(vocab, dropout=0.2, seed=11), new_trainer(vocab)
    assert a.dropout == (0.2, 0.2) and a.rng_state() == (11, 0) and b.dropout == (0.0, 0.0)
    for k in range(3):
        la = a.step(feats, labels, il, tl)
        lb, grads, norm = b.model.loss_and_grad(feats, labels, il, tl, zero_infinity=True, dropout=0.2, seed=11, offset=k)
        b.model.adam_step(grads, norm, **b.hyper)
        wa, wb = a.weights(), b.weights()
        torch.cuda.synchronize()
        assert la.dim() == 0 and la.is_cuda and torch.equal(la, lb)
        assert torch.equal(wa, wb)
        assert a.rng_state() == (11, k + 1)
    assert_masks(a.model, 11, 2, B, T, (0.2, 0.2))                  # the third grad() drew at offset 2


def test_train_ctc_passes_dropout_through(gpu):
    import wakeword
    vocab, B, T, _ = DR.TRAJ
    batch = DR.traj_batch(vocab, B, T)
    t, train_losses, val_losses, _ = wakeword.train_ctc([batch], [batch], vocab, num_epochs=1, weights=O.p0(vocab).numpy(),
                                                        zero_infinity=True, dropout=0.2, seed=11)
    ref = new_trainer(vocab, dropout=0.2, seed=11)
    first = ref.step(*batch)
    assert t.dropout == (0.2, 0.2) and t.rng_state() == (11, 1)
    assert train_losses == [float(first)] and val_losses == [float(ref.val_loss(*batch))]
    plain, _, _, _ = wakeword.train_ctc([batch], [batch], vocab, num_epochs=1, weights=O.p0(vocab).numpy())
    assert plain.dropout == (0.0, 0.0)                              # the default: today's callers see no change


def test_resume_with_rng_state(gpu):
    import wakeword
    vocab, B, T, _ = DR.TRAJ
    feats, labels, il, tl = DR.traj_batch(vocab, B, T)
    a = new_trainer(vocab, dropout=0.2, seed=5)
    for _ in range(4):
        a.step(feats, labels, il, tl)
    b = new_trainer(vocab, dropout=0.2, seed=5)
    for _ in range(2):
        b.step(feats, labels, il, tl)
    w, (m, v, step), rng = b.weights().cpu().numpy(), b.optim_state(), b.rng_state()
    assert step == 2 and rng == (5, 2)
    r = wakeword.CTCTrainer(w, vocab, zero_infinity=True, dropout=0.2)
    r.load_optim_state(m, v, step)
    r.load_rng_state(*rng)
    for _ in range(2):
        r.step(feats, labels, il, tl)
    wa, wr = a.weights(), r.weights()
    sa, sr = a.optim_state(), r.optim_state()
    torch.cuda.synchronize()
    assert torch.equal(wa, wr)
    assert torch.equal(sa[0], sr[0]) and torch.equal(sa[1], sr[1]) and sa[2] == sr[2] == 4
    assert a.rng_state() == r.rng_state() == (5, 4)
    with pytest.raises(ValueError):
        r.load_rng_state(0, 2 ** 63)


def test_val_loss_is_the_eval_mode_loss(gpu):
    import wakeword
    vocab, B, T, _ = DR.TRAJ
    feats, labels, il, tl = DR.traj_batch(vocab, B, T)
    t = new_trainer(vocab, dropout=0.2, seed=1)
    t.step(feats, labels, il, tl)
    got = t.val_loss(feats, labels, il, tl)
    want = wakeword.CTCModel(t.weights().cpu().numpy(), vocab).loss(feats, labels, il, tl)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_training_trajectory(gpu):
    """Eight dropout steps at the reference's hyper-parameters against the
    same loop in float64 torch-CPU fed each step's exported masks; the unit
    and form of test_gpu_ctc_optim.test_training_trajectory."""
    vocab, B, T, steps = DR.TRAJ
    p = (0.2, 0.2)
    feats, labels, il, tl = DR.traj_batch(vocab, B, T)
    t = new_trainer(vocab, dropout=p, seed=2)
    got, step_masks = [], []
    for _ in range(steps):
        got.append(t.step(feats, labels, il, tl))
        step_masks.append(exported(t.model))
    got = [float(x) for x in got]
    for k, (m0, m1) in enumerate(step_masks):
        w0, w1 = DR.masks(2, k, B, T, *p)
        assert torch.equal(m0, w0) and torch.equal(m1, w1), k
    loss64, norm64 = DR.trajectory(vocab, B, T, step_masks, p, torch.float64)
    loss32, _ = DR.trajectory(vocab, B, T, step_masks, p, torch.float32)
    e32 = max(abs(a - b) for a, b in zip(loss32, loss64))
    _, nll64, _ = G.e2e_reference(H.model(vocab), feats, labels, il, tl, torch.float64)
    _, nll32, _ = G.e2e_reference(H.model(vocab), feats, labels, il, tl, torch.float32)
    own = LR.K_LOSS * torch.maximum((nll32.double() - nll64).abs().max(), LR.EPS32 * nll64.abs())
    per_utt = torch.tensor(il).double() * H.bound(H.Case(vocab, feats), "fp32") + own
    loss_bound = float((per_utt / torch.tensor(tl).clamp(min=1)).mean())
    unit = max(e32, loss_bound)
    worst = 0.0
    for k, (a, b) in enumerate(zip(got, loss64)):
        worst = max(worst, abs(a - b) / unit)
        print(f"drop-traj step {k}: loss={a:.7g} loss64={b:.7g} err={abs(a - b):.3g} norm64={norm64[k]:.4g}")
    print(f"drop-traj e32={e32:.3g} loss bound={loss_bound:.3g} worst ratio {worst:.3g} (K_TRAJ = {DR.K_TRAJ})")
    assert loss64[-1] < loss64[0] and got[-1] < got[0]
    assert all(abs(a - b) <= DR.K_TRAJ * unit for a, b in zip(got, loss64)), (got, loss64, unit)
