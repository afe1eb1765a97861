"""CPU tests of wk_ctc_loss's surface: the symbols are exported, bad arguments
are rejected before any device work, the workspace size grows with the problem,
the Python wrapper pads targets, and the references of tests/ctc_loss_ref.py
agree with each other (hand-written float64 alpha / beta in the kernels'
gradient convention against torch's F.ctc_loss in float64)."""
import ctypes as C

import pytest
import torch

import ctc_loss_ref as R


@pytest.fixture(scope="module")
def L():
    from wakeword import _lib
    return _lib.lib()


def test_symbols_exported(L):
    from wakeword import _lib
    for name in ("wk_ctc_loss_workspace_bytes", "wk_ctc_loss"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    import wakeword
    assert callable(wakeword.ctc_loss) and callable(wakeword.CTCLoss()) and hasattr(wakeword.CTCModel, "loss")


def _call(L, **over):
    """wk_ctc_loss with fake (never dereferenced) device pointers and a valid
    shape, but for the overrides."""
    p = C.c_void_p(4096)
    a = dict(lp=p, batch=2, T=5, vocab=7, labels=p, label_stride=3, in_len=p, lab_len=p, max_label_len=3, reduction=2,
             zero_infinity=0, grad_scale=1.0, ws=p, nll=p, loss=p, grad=p, device=0, stream=None)
    a.update(over)
    return L.wk_ctc_loss(a["lp"], a["batch"], a["T"], a["vocab"], a["labels"], a["label_stride"], a["in_len"], a["lab_len"],
                         a["max_label_len"], a["reduction"], a["zero_infinity"], a["grad_scale"], a["ws"], a["nll"],
                         a["loss"], a["grad"], a["device"], a["stream"])


@pytest.mark.parametrize("over", [dict(lp=None), dict(labels=None), dict(in_len=None), dict(lab_len=None), dict(ws=None),
                                  dict(nll=None), dict(loss=None), dict(batch=0), dict(batch=-1), dict(T=0), dict(T=-3),
                                  dict(vocab=0), dict(vocab=-1), dict(label_stride=2), dict(reduction=3), dict(reduction=-1),
                                  dict(max_label_len=256, label_stride=256), dict(vocab=65537),
                                  dict(batch=1 << 20, T=1 << 9), dict(ws=C.c_void_p(4100))],
                         ids=lambda o: "-".join(f"{k}={getattr(v, 'value', v)}" for k, v in o.items()))
def test_bad_arguments_rejected_without_gpu(L, over):
    assert _call(L, **over) == 1
    assert b"wk_ctc_loss" in L.wk_last_error()


def test_workspace_bytes(L):
    f = L.wk_ctc_loss_workspace_bytes
    base = f(8, 801, 40)
    assert base > 0
    assert f(9, 801, 40) > base and f(8, 802, 40) > base
    # in label length: every step at fixed (batch, T) costs something, and the
    # 64-lane steps of 2S+1 (S = 31 -> 32, 63 -> 64, 127 -> 128) cost a row width
    sizes = [f(300, 7, s) for s in range(0, 256)]
    assert 0 < sizes[0] <= sizes[1]
    assert all(b > a for a, b in zip(sizes[1:], sizes[2:]))
    for s in (31, 63, 127):
        assert sizes[s + 1] - sizes[s] > 3 * 4 * 300 * 7 * 64
    # alpha, beta and the gathered log-probs: three fp32 rows of >= 2S+1 per frame
    assert base >= 3 * 4 * 8 * 801 * 81
    for bad in ((0, 801, 40), (8, 0, 40), (8, 801, -1), (8, 801, 256), (1 << 20, 1 << 9, 1)):
        assert f(*bad) == 0


def test_workspace_bytes_pinned(L):
    """The sizes themselves, at each register layout's last and first label
    length (31 | 32, 127, 255) and at T = 801: the layout is the kernels'
    contract with their callers' buffers, so a change of it shows here."""
    f = L.wk_ctc_loss_workspace_bytes
    assert f(8, 801, 31) == 4923648 and f(8, 801, 32) == 9844992
    assert f(3, 17, 127) == 160000 and f(257, 5, 255) == 8424704


def test_pad_targets_concatenated_equals_padded():
    import wakeword
    c = R.case("S32-T70-V33-B3", "random")       # lengths 32, 31, 0
    padded = wakeword.pad_targets(c.labels, c.lab_len)
    concat = wakeword.pad_targets(c.concatenated(), torch.tensor(c.lab_len))
    assert padded.dtype == concat.dtype == torch.int32
    assert padded.shape == concat.shape == (3, 32)
    assert torch.equal(padded, concat)
    # all-empty labels keep one (unused) column, so the device array is never empty
    assert wakeword.pad_targets(torch.zeros((2, 0), dtype=torch.int64), [0, 0]).shape == (2, 1)
    assert wakeword.pad_targets(torch.zeros((0,), dtype=torch.int64), [0, 0]).shape == (2, 1)
    with pytest.raises(ValueError):
        wakeword.pad_targets(c.concatenated(), [32, 30, 0])


def test_wrapper_rejects_bad_arguments():
    import wakeword
    lp = torch.zeros((2, 3, 4))
    with pytest.raises(ValueError, match="reduction"):
        wakeword.ctc_loss(lp, torch.ones((3, 1)), [2, 2, 2], [1, 1, 1], reduction="avg")
    with pytest.raises(ValueError, match="HIP device"):
        wakeword.ctc_loss(lp, torch.ones((3, 1)), [2, 2, 2], [1, 1, 1])


@pytest.mark.parametrize("name,kind", R.CASES, ids=R.CASE_IDS)
def test_hand_written_reference_agrees_with_torch(name, kind):
    """nll, the gradient convention (torch's float64 gradient at the logits is
    exp(lp) - exp(lse(alpha + beta) + nll - lp), 0 past the input length) and the
    'mean' formula mean_b(nll_b / max(S_b, 1)), to 1e-10 relative to the size of
    nll (float64 rounding of sums of that size)."""
    c = R.case(name, kind)
    lp64 = torch.log_softmax(c.z32.double(), -1)
    nll, g = R.hand_ctc(lp64, c.labels, c.in_len, c.lab_len)
    tol = 1e-10 * max(1.0, c.nll_scale)
    assert float((nll - c.nll64).abs().max()) <= tol
    assert float((g - c.g64).abs().max()) <= tol
    for b, tb in enumerate(c.in_len):
        assert not bool(c.g64[b, tb:].any()) and not bool(g[b, tb:].any())
    il, tl = torch.tensor(c.in_len), torch.tensor(c.lab_len)
    for red in ("mean", "sum"):
        want = float(torch.nn.functional.ctc_loss(lp64.transpose(0, 1), c.labels, il, tl, blank=0, reduction=red))
        assert abs(R.reduce64(nll, c.lab_len, red) - want) <= tol


def test_cases_cover_the_edges():
    smax = {max(s for s, _, _ in R.SPECS[n][2]) for n in R.NAMES}
    assert {0, 1, 31, 32, 63, 64, 255} <= smax
    assert {R.case(n, "random").B for n in R.NAMES} == {1, 3, 35}
    assert {3, 33, 4000} <= {R.SPECS[n][0] for n in R.NAMES}
    assert {1, 2, 70, 129} <= {R.case(n, "random").T for n in R.NAMES}
    c = R.case("V4000-T40-B3", "random")
    assert int(c.labels.max()) == 3999 and c.T <= 40
    c = R.case("same7-T70-V33-B3", "trained")
    assert c.labels[0, :20].tolist() == [7] * 20 and c.in_len[1] == 39 and len(set(c.in_len)) > 1
    # the two kinds are two regimes: nll ~ T ln V against a few units per utterance
    for n in ("S63-T129-V33-B3", "S64-T129-V33-B35"):
        assert float(R.case(n, "random").nll64.max()) > 100.0
        assert float(R.case(n, "trained").nll64.max()) < 30.0
