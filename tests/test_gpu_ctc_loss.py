"""wk_ctc_loss / wakeword.ctc_loss / CTCModel.loss on the MI355X against float64
(tests/ctc_loss_ref.py: the cases, the references and the bounds).

Parity, per case: |nll_dev - nll_64| <= K_LOSS max(e32_loss, eps32 |nll_64|) and
max |g_dev - g_64| <= K_GRAD max(e32_grad, eps32 max(1, |nll_64|)), e32 being
torch-CPU fp32's own error on the case; measured ratios and the constants:
profiles/ctc_loss_bounds.md.  Exact properties on every case: zero rows past the
input length, rows summing to zero within the gradient bound, two calls giving
the same bits, d_loss the reduction of d_nll.  Each case is one call (run once,
shared)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import ctc_loss_ref as R

RED = {"none": 0, "sum": 1, "mean": 2}


def raw(lp, labels, in_len, lab_len, reduction="sum", zero_infinity=False, grad_scale=1.0, want_grad=True):
    """One wk_ctc_loss call through the C ABI on (B, T, V) device log-probs ->
    (nll, loss, grad) on the host; the outputs start as NaN, so anything the
    call leaves unwritten shows."""
    from wakeword import _lib
    L = _lib.lib()
    dev = lp.device
    B, T, V = lp.shape
    labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    smax = labels.shape[1] if max(lab_len) > 0 else 0
    il = torch.tensor(in_len, dtype=torch.int32, device=dev)
    tl = torch.tensor(lab_len, dtype=torch.int32, device=dev)
    ws = torch.empty(L.wk_ctc_loss_workspace_bytes(B, T, smax), dtype=torch.uint8, device=dev)
    nll = torch.full((B,), float("nan"), device=dev)
    loss = torch.full((1,), float("nan"), device=dev)
    grad = torch.full_like(lp, float("nan")) if want_grad else None
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    _lib.check(L.wk_ctc_loss(p(lp), B, T, V, p(labels), labels.shape[1], p(il), p(tl), smax, RED[reduction],
                             int(zero_infinity), grad_scale, p(ws), p(nll), p(loss), p(grad) if want_grad else None,
                             dev.index or 0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "wk_ctc_loss")
    return nll.cpu(), loss.cpu(), grad.cpu() if want_grad else None


@functools.lru_cache(maxsize=None)
def run(name, kind, reduction="sum"):
    c = R.case(name, kind)
    return raw(c.lp32.to("cuda:0"), c.labels, c.in_len, c.lab_len, reduction)


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    run.cache_clear()


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", R.CASES, ids=R.CASE_IDS)
def test_parity_with_float64(gpu, name, kind):
    c = R.case(name, kind)
    nll, _, g = run(name, kind)
    assert bool(torch.isfinite(nll).all()) and bool(torch.isfinite(g).all())
    e_loss = float((nll.double() - c.nll64).abs().max())
    e_grad = float((g.double() - c.g64).abs().max())
    print(f"ctc-loss {name}-{kind} nll~{c.nll_scale:.4g} loss: dev={e_loss:.3e} e32={c.e32_loss:.3e} unit={c.loss_unit:.3e} "
          f"ratio={e_loss / c.loss_unit:.2f} grad: dev={e_grad:.3e} e32={c.e32_grad:.3e} unit={c.grad_unit:.3e} "
          f"ratio={e_grad / c.grad_unit:.2f}")
    assert e_loss <= c.loss_bound
    assert e_grad <= c.grad_bound


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", R.CASES, ids=R.CASE_IDS)
def test_exact_properties(gpu, name, kind):
    c = R.case(name, kind)
    nll, loss, g = run(name, kind)
    worst = 0.0
    for b, tb in enumerate(c.in_len):
        assert not bool(g[b, tb:].any())                      # exactly 0 past the input length
        worst = max(worst, float(g[b, :tb].double().sum(-1).abs().max()))
    print(f"ctc-loss {name}-{kind} max|sum_v g|={worst:.3e} bound={c.grad_bound:.3e}")
    assert worst <= c.grad_bound
    nll2, loss2, g2 = raw(c.lp32.to("cuda:0"), c.labels, c.in_len, c.lab_len, "sum")
    assert torch.equal(nll, nll2) and torch.equal(loss, loss2) and torch.equal(g, g2)


@pytest.mark.gpu
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("name,kind", R.CASES, ids=R.CASE_IDS)
def test_loss_is_the_reduction_of_nll(gpu, name, kind, reduction):
    """d_loss against the reduction in float64 of the device's own d_nll, to one
    fp32 rounding (NONE: the sum); d_nll itself does not depend on the reduction,
    and MEAN's gradient is SUM's times 1 / (B max(S_b, 1)), to one more rounding."""
    c = R.case(name, kind)
    nll_s, _, g_s = run(name, kind)
    nll, loss, g = run(name, kind, reduction)
    assert torch.equal(nll, nll_s)
    want = R.reduce64(nll, c.lab_len, reduction)
    assert abs(float(loss[0]) - want) <= R.EPS32 * abs(want)
    if reduction == "mean":
        f = 1.0 / (c.B * torch.tensor(c.lab_len, dtype=torch.float64).clamp(min=1))
        want_g = g_s.double() * f.reshape(-1, 1, 1)
        assert bool(((g.double() - want_g).abs() <= 2.0 * R.EPS32 * want_g.abs() + 1e-44).all())
    else:
        assert torch.equal(g, g_s)


# ---- utterances without an alignment ---------------------------------------------
def _infeasible():
    """B = 4, V = 33, T = 20: utterances 1 (fifteen equal labels need 29 frames)
    and 2 (T_b = 2 < S_b = 3) have no alignment; 0 and 3 do."""
    g = torch.Generator().manual_seed(5)
    z = torch.randn((4, 20, 33), generator=g)
    labels = torch.zeros((4, 15), dtype=torch.int64)
    labels[0, :5] = torch.tensor([3, 3, 9, 32, 1])
    labels[1, :] = 7
    labels[2, :3] = torch.tensor([4, 5, 6])
    labels[3, :2] = torch.tensor([2, 2])
    return z, labels, [20, 20, 2, 3], [5, 15, 3, 2]


@pytest.mark.gpu
def test_infeasible_utterances(gpu):
    z, labels, il, tl = _infeasible()
    lp = F.log_softmax(z, -1).to("cuda:0")
    nll64, g64 = R.torch_ctc(z.double(), labels, il, tl, zero_infinity=True)
    nll32, g32 = R.torch_ctc(z, labels, il, tl, zero_infinity=True)
    inf64, _ = R.torch_ctc(z.double(), labels, il, tl, zero_infinity=False)
    bad = torch.isinf(inf64)
    assert bad.tolist() == [False, True, True, False]
    scale = float(nll64.abs().max())
    loss_bound = R.K_LOSS * max(float((nll32.double() - nll64).abs().max()), R.EPS32 * scale)
    grad_bound = R.K_GRAD * max(float((g32.double() - g64).abs().max()), R.EPS32 * max(1.0, scale))
    for zi in (False, True):
        nll, loss, g = raw(lp, labels, il, tl, "sum", zero_infinity=zi)
        if zi:
            assert not bool(nll[bad].any()) and bool(torch.isfinite(loss).all())
        else:
            assert bool((nll[bad] == float("inf")).all()) and float(loss[0]) == float("inf")
        assert not bool(g[bad].any())                          # exactly 0 (required with zero_infinity)
        assert float((nll[~bad].double() - nll64[~bad]).abs().max()) <= loss_bound
        assert float((g[~bad].double() - g64[~bad]).abs().max()) <= grad_bound


@pytest.mark.gpu
def test_label_out_of_range_is_no_alignment(gpu):
    """A label outside [1, V) (V itself, the blank, a negative) gives nll = +inf
    for its utterance and is never an index; the others keep their bits."""
    c = R.case("S31-T70-V33-B3", "trained")
    lp = c.lp32.to("cuda:0")
    clean = raw(lp, c.labels, c.in_len, c.lab_len)
    for value in (33, 0, -5, 1 << 30):
        labels = c.labels.clone()
        labels[1, 2] = value
        nll, _, g = raw(lp, labels, c.in_len, c.lab_len)
        assert float(nll[1]) == float("inf") and not bool(g[1].any())
        for b in (0, 2):
            assert torch.equal(nll[b], clean[0][b]) and torch.equal(g[b], clean[2][b])


# ---- autograd ---------------------------------------------------------------------
AUTOGRAD_CASES = [("S32-T70-V33-B3", "trained"), ("S32-T70-V33-B3", "random"), ("V4000-T40-B3", "trained")]


@pytest.mark.gpu
@pytest.mark.parametrize("batch_first", [False, True], ids=["TBV", "BTV"])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("name,kind", AUTOGRAD_CASES, ids=[f"{n}-{k}" for n, k in AUTOGRAD_CASES])
def test_autograd_matches_float64(gpu, name, kind, reduction, batch_first):
    """wakeword.ctc_loss(F.log_softmax(z, -1), ...).backward(): z.grad against
    float64 autograd on the CPU, within the case's gradient bound times the
    largest upstream factor (1 / (B max(S_b, 1)) for mean, |grad_output| for
    none).  The (T, B, V) runs pass torch's 1-D concatenated targets."""
    import wakeword
    c = R.case(name, kind)
    go = torch.randn(c.B, generator=torch.Generator().manual_seed(3)) if reduction == "none" else None
    _, want = R.torch_ctc(c.z32.double(), c.labels, c.in_len, c.lab_len, reduction=reduction, grad_output=go)
    z = c.z32.to("cuda:0").requires_grad_(True)
    lp = F.log_softmax(z, -1)
    il, tl = torch.tensor(c.in_len), torch.tensor(c.lab_len)
    if batch_first:
        out = wakeword.ctc_loss(lp, c.labels, il, tl, reduction=reduction, batch_first=True)
    else:
        out = wakeword.CTCLoss(reduction=reduction)(lp.transpose(0, 1), c.concatenated(), il, tl)
    if reduction == "none":
        assert out.shape == (c.B,)
        out.backward(go.to("cuda:0"))
        factor = float(go.abs().max())
        want_out = c.nll64
    else:
        assert out.dim() == 0
        out.backward()
        factor = 1.0 if reduction == "sum" else float((1.0 / (c.B * tl.clamp(min=1).double())).max())
        want_out = torch.tensor(R.reduce64(c.nll64, c.lab_len, reduction))
    assert float((out.detach().cpu().double() - want_out).abs().max()) <= c.loss_bound
    err = float((z.grad.cpu().double() - want).abs().max())
    print(f"ctc-loss autograd {name}-{kind} {reduction} err={err:.3e} bound={c.grad_bound * factor:.3e}")
    assert err <= c.grad_bound * factor


@pytest.mark.gpu
def test_non_default_stream(gpu):
    import wakeword
    c = R.case("S64-T129-V33-B35", "trained")
    res = []
    for stream in (None, torch.cuda.Stream()):
        z = c.z32.to("cuda:0").requires_grad_(True)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            out = wakeword.ctc_loss(F.log_softmax(z, -1), c.labels, c.in_len, c.lab_len, batch_first=True)
            out.backward()
        torch.cuda.synchronize()
        res.append((out.detach().cpu(), z.grad.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert abs(float(res[0][0]) - R.reduce64(c.nll64, c.lab_len, "mean")) <= c.loss_bound


# ---- CTCModel.loss ----------------------------------------------------------------
@pytest.mark.gpu
def test_ctc_model_loss(gpu):
    """CTCModel.loss on ctc_ref's trained-like model (V = 512, B = 3, T = 70): equal,
    bit for bit, to wakeword.ctc_loss on the model's own log-probs, and within the
    head's log-prob bound propagated through the frames of float64 end to end:
    d nll / d lp[t, v] = -gamma_t(v) with sum_v gamma_t(v) = 1, so to first order
        |nll_dev - nll_64| <= T_b max|d lp| + (the loss kernel's own bound)
                           <= T_b K32 e32_head + K_LOSS max(e32_loss, eps32 |nll_64|)."""
    import ctc_ref as H
    import wakeword
    hc = H.case(512, 3, 70)
    model = wakeword.CTCModel(H.model(512).state_dict(), 512)
    labels = torch.zeros((3, 12), dtype=torch.int64)
    labels[0] = torch.tensor([5, 5, 17, 511, 2, 300, 300, 300, 9, 1, 44, 45])
    labels[1, :5] = torch.tensor([511, 7, 7, 8, 100])
    il, tl = [70, 50, 64], [12, 5, 0]
    _, _, lp = model.decode(hc.feats, return_log_probs=True)
    for reduction in ("mean", "none"):
        got = model.loss(hc.feats, labels, il, tl, reduction=reduction)
        assert torch.equal(got, wakeword.ctc_loss(lp, labels, il, tl, reduction=reduction, batch_first=True))
    nll = got.cpu().double()
    t_il, t_tl = torch.tensor(il), torch.tensor(tl)
    nll64 = F.ctc_loss(hc.lp.transpose(0, 1), labels, t_il, t_tl, blank=0, reduction="none")
    nll32 = F.ctc_loss(hc.lp.float().transpose(0, 1), labels, t_il, t_tl, blank=0, reduction="none")
    own = R.K_LOSS * torch.maximum((nll32.double() - nll64).abs().max(), R.EPS32 * nll64.abs())
    bound = t_il.double() * H.bound(hc, "fp32") + own
    print(f"ctc-model-loss err={(nll - nll64).abs().tolist()} bound={bound.tolist()}")
    assert bool(((nll - nll64).abs() <= bound).all())
    mean = float(model.loss(hc.feats, labels, il, tl))
    assert abs(mean - R.reduce64(nll64, tl, "mean")) <= float((bound / t_tl.clamp(min=1)).mean())
