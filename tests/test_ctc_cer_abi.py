"""CPU tests of wk_ctc_cer's surface: the symbols are exported and typed, bad
arguments are rejected before any device work (fake pointers, never
dereferenced), the workspace size is 0 beyond the limits and holds no DP
matrix, the Python side rejects what the kernel does not take, and train_ctc
takes history= (a stub trainer, no GPU)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def L():
    from wakeword import _lib
    return _lib.lib()


def test_symbols_exported(L):
    import wakeword
    from wakeword import _lib
    for name in ("wk_ctc_cer_workspace_bytes", "wk_ctc_cer"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert L.wk_ctc_cer_workspace_bytes.restype is C.c_int64
    assert L.wk_ctc_cer_workspace_bytes.argtypes == [C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    assert len(L.wk_ctc_cer.argtypes) == 16 and L.wk_ctc_cer.restype is C.c_int32
    assert L.wk_ctc_cer.argtypes[2] is C.c_int64 and L.wk_ctc_cer.argtypes[3] is C.c_int32
    assert callable(wakeword.edit_distance) and callable(wakeword.error_rate)
    assert wakeword.EditStats._fields == ("distance", "substitutions", "deletions", "insertions", "best", "totals")
    assert hasattr(wakeword.EditStats, "sentence_error_rate")
    assert hasattr(wakeword.CTCModel, "cer") and hasattr(wakeword.CTCModel, "cer_audio") and hasattr(wakeword.CTCTrainer, "val_cer")
    assert L.wk_abi_version() == 1


def _call(L, **over):
    """wk_ctc_cer with fake (never dereferenced) device pointers and a valid shape, but for the overrides."""
    p = C.c_void_p(4096)
    a = dict(hyp=p, hyp_len=p, batch=2, n_hyp=3, hyp_stride=7, ref=p, ref_stride=5, ref_len=p, max_ref_len=5, collapse=0, ws=p,
             stats=p, best=p, totals=p, device=0, stream=None)
    a.update(over)
    return L.wk_ctc_cer(a["hyp"], a["hyp_len"], a["batch"], a["n_hyp"], a["hyp_stride"], a["ref"], a["ref_stride"], a["ref_len"],
                        a["max_ref_len"], a["collapse"], a["ws"], a["stats"], a["best"], a["totals"], a["device"], a["stream"])


@pytest.mark.parametrize("over", [dict(hyp=None), dict(hyp_len=None), dict(ref=None), dict(ref_len=None), dict(ws=None),
                                  dict(stats=None), dict(batch=0), dict(batch=-1), dict(n_hyp=0), dict(n_hyp=-2), dict(n_hyp=65),
                                  dict(hyp_stride=0), dict(hyp_stride=-1), dict(hyp_stride=32768), dict(max_ref_len=0),
                                  dict(max_ref_len=-1), dict(max_ref_len=1025, ref_stride=1025), dict(ref_stride=4),
                                  dict(ref_stride=-1), dict(batch=(1 << 24) + 1, n_hyp=1, hyp_stride=1),
                                  dict(batch=1 << 23, n_hyp=3, hyp_stride=1), dict(batch=1 << 20, n_hyp=1, hyp_stride=1025),
                                  dict(batch=1 << 40, n_hyp=1, hyp_stride=1), dict(ws=C.c_void_p(4100)), dict(ws=C.c_void_p(4104)),
                                  dict(device=-1), dict(collapse=1, hyp=None), dict(collapse=1, device=-1)],
                         ids=lambda o: "-".join(f"{k}={getattr(v, 'value', v)}" for k, v in o.items()))
def test_bad_arguments_rejected_without_gpu(L, over):
    assert _call(L, **over) == 1
    assert b"wk_ctc_cer" in L.wk_last_error()


def test_null_hyp_lengths_is_about_collapse(L):
    """Null d_hyp_lengths: rejected with collapse = 0 for that reason; with
    collapse != 0 it is not the reason (another bad argument is named instead)."""
    assert _call(L, hyp_len=None) == 1 and b"d_hyp_lengths" in L.wk_last_error()
    assert _call(L, hyp_len=None, collapse=1, device=-1) == 1
    assert b"device" in L.wk_last_error() and b"d_hyp_lengths" not in L.wk_last_error()


def test_workspace_bytes(L):
    f = L.wk_ctc_cer_workspace_bytes
    for bad in ((0, 1, 8, 8), (-1, 1, 8, 8), (8, 0, 8, 8), (8, -1, 8, 8), (8, 65, 8, 8), (8, 1, 0, 8), (8, 1, -1, 8),
                (8, 1, 32768, 8), (8, 1, 8, 0), (8, 1, 8, -1), (8, 1, 8, 1025), ((1 << 24) + 1, 1, 1, 1), (1 << 23, 3, 1, 1),
                (1 << 20, 1, 1025, 1), (1 << 16, 64, 257, 1), (1 << 40, 1, 1, 1)):
        assert f(*bad) == 0, bad
    # the limits themselves
    assert f(1 << 24, 1, 64, 1024) > 0 and f(1 << 18, 64, 64, 1) > 0 and f(1 << 15, 1, 32767, 1024) > 0 and f(1, 64, 32767, 1024) > 0
    # non-decreasing in every argument
    for b, h, n, m in ((1, 1, 1, 1), (3, 2, 17, 5), (257, 7, 5, 64), (8, 16, 255, 40), (8, 1, 801, 1023), (5, 63, 100, 256)):
        here = f(b, h, n, m)
        assert here > 0
        assert f(b + 1, h, n, m) >= here and f(b, h + 1, n, m) >= here and f(b, h, n + 1, m) >= here and f(b, h, n, m + 1) >= here
    sizes = [f(8, 16, 255, m) for m in range(1, 1025)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    sizes = [f(8, 16, n, 40) for n in range(1, 2000, 7)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    # no DP matrix: what the reference's length adds does not grow with the hypothesis's
    extra = [f(8, 16, n, 1024) - f(8, 16, n, 1) for n in (1, 64, 801, 8191)]
    assert max(extra) <= f(8, 16, 1, 1024)
    assert f(8, 16, 8191, 1024) <= f(8, 16, 1, 1024) + 4 * 8 * 16 * 8191 + 256      # at most the collapsed hypotheses


def test_workspace_bytes_pinned(L):
    """The sizes themselves: (batch, n_hyp, hyp_stride, max_ref_len), 801-frame hypotheses among them."""
    f = L.wk_ctc_cer_workspace_bytes
    assert f(8, 1, 801, 40) == 256 and f(1, 1, 1, 1) == 256
    assert f(3, 64, 17, 1024) == 1536 and f(257, 4, 5, 9) == 8448


def test_wrapper_rejects_bad_arguments():
    import wakeword
    from wakeword import ctc
    hyp = torch.zeros((2, 3, 5), dtype=torch.int32)
    ref, rl, hl = np.array([[1, 2], [3, 0]]), [2, 1], [5] * 6
    with pytest.raises(ValueError, match="HIP device"):
        wakeword.edit_distance(hyp, hl, ref, rl)
    with pytest.raises(ValueError, match="HIP device"):
        wakeword.edit_distance(hyp.numpy(), hl, ref, rl)
    for bad in (hyp.long(), hyp.float(), hyp[0, 0], hyp.reshape(1, 2, 3, 5), hyp.numpy(), [[1, 2]]):
        with pytest.raises(ValueError, match="int32 tensor"):
            ctc._cer_args(bad, hl, ref, rl, False)
    with pytest.raises(ValueError, match="hyp_lengths is required"):
        ctc._cer_args(hyp, None, ref, rl, False)
    with pytest.raises(ValueError, match="5 hypothesis lengths"):
        ctc._cer_args(hyp, [5] * 5, ref, rl, False)
    with pytest.raises(ValueError, match="batch of 2"):
        ctc._cer_args(hyp, hl, ref[:1], rl, False)
    with pytest.raises(ValueError, match="batch of 2"):
        ctc._cer_args(hyp, hl, ref, [2], False)
    with pytest.raises(ValueError, match="ref must be"):
        ctc._cer_args(hyp, hl, np.array([1, 2]), rl, False)
    with pytest.raises(ValueError, match="ref must be"):
        ctc._cer_args(hyp, hl, ref.astype(np.float32), rl, False)
    with pytest.raises(ValueError, match="at most 64"):
        ctc._cer_args(torch.zeros((2, 65, 5), dtype=torch.int32), [5] * 130, ref, rl, False)
    with pytest.raises(ValueError, match="at most 32767"):
        ctc._cer_args(torch.zeros((2, 1, 32768), dtype=torch.int32), [5] * 2, ref, rl, False)
    with pytest.raises(ValueError, match="positive"):
        ctc._cer_args(torch.zeros((2, 3, 0), dtype=torch.int32), hl, ref, rl, False)
    with pytest.raises(ValueError, match="2\\^30"):
        ctc._cer_args(torch.zeros((1 << 16, 64, 1), dtype=torch.int32).expand(1 << 16, 64, 257), [0], ref, rl, False)
    with pytest.raises(ValueError, match="at most 1024"):
        ctc._cer_args(hyp, hl, np.ones((2, 1025), dtype=np.int64), [1025, 3], False)


def test_argument_handling():
    """(B, N) is one hypothesis per utterance; lengths and references become
    int32 on hyp's device; None lengths pass with collapse; padding wider than
    1024 is cut to the longest reference; an empty reference array gets a column."""
    from wakeword import ctc
    hyp = torch.arange(10, dtype=torch.int32).reshape(2, 5)
    h, hl, r, rl, m = ctc._cer_args(hyp, torch.tensor([5, 2]), [[1, 2, 3], [4, 0, 0]], np.array([3, 1]), False)
    assert h.shape == (2, 1, 5) and h.is_contiguous() and torch.equal(h[:, 0], hyp)
    assert hl.dtype == r.dtype == rl.dtype == torch.int32
    assert hl.tolist() == [5, 2] and r.tolist() == [[1, 2, 3], [4, 0, 0]] and rl.tolist() == [3, 1] and m == 3
    h, hl, r, rl, m = ctc._cer_args(hyp, None, torch.tensor([[1], [2]]), [1, 1], True)
    assert hl is None and m == 1
    h, hl, r, rl, m = ctc._cer_args(hyp.reshape(1, 2, 5), [[5, 2]], np.ones((1, 2000), dtype=np.int64), [900], False)
    assert h.shape == (1, 2, 5) and r.shape == (1, 2000) and m == 900
    h, hl, r, rl, m = ctc._cer_args(hyp, [5, 2], np.zeros((2, 0), dtype=np.int64), [0, 0], False)
    assert r.shape == (2, 1) and m == 1


def test_error_rate():
    import wakeword
    totals = torch.tensor([[6, 2, 0, 4, 5, 9, 3, 3], [1, 0, 0, 1, 5, 5, 1, 3]])
    assert wakeword.error_rate(totals) == 6 / 5 and wakeword.error_rate(totals, oracle=True) == 1 / 5
    assert wakeword.error_rate(totals[0]) == 6 / 5 and wakeword.error_rate(totals.numpy()) == 6 / 5
    st = wakeword.EditStats(None, None, None, None, None, totals)
    assert wakeword.error_rate(st, oracle=True) == 1 / 5 and st.error_rate() == 6 / 5
    assert st.sentence_error_rate() == 1.0 and st.sentence_error_rate(oracle=True) == 1 / 3
    assert math.isnan(wakeword.error_rate(torch.tensor([0, 0, 0, 0, 0, 0, 0, 2])))
    assert wakeword.error_rate(torch.tensor([3, 0, 0, 3, 0, 3, 1, 2])) == math.inf
    with pytest.raises(ValueError, match="oracle"):
        wakeword.error_rate(totals[0], oracle=True)
    with pytest.raises(ValueError, match="totals"):
        wakeword.error_rate(torch.zeros(7, dtype=torch.int64))


class _StubTrainer:
    """What train_ctc needs of a trainer, on the host."""

    def __init__(self):
        self.steps = self.cers = 0

    def step(self, *batch):
        self.steps += 1
        return torch.tensor(1.0 / self.steps)

    def val_loss(self, *batch):
        return torch.tensor(2.0 / self.steps)

    def val_cer(self, feats, targets, input_lengths, target_lengths):
        self.cers += 1
        return torch.tensor([self.cers, 0, 0, self.cers, 4, 4 + self.cers, 1, 2])

    def state_dict(self):
        return {"steps": self.steps}


def test_train_ctc_history():
    import wakeword
    batch = (None, None, None, None)
    plain = wakeword.train_ctc([batch] * 2, [batch] * 3, vocab=5, num_epochs=2, trainer=_StubTrainer())
    assert len(plain) == 4 and plain[0].cers == 0                     # without history: no val_cer call, the same 4-tuple
    hist = {}
    trainer, tr, va, best = wakeword.train_ctc([batch] * 2, [batch] * 3, vocab=5, num_epochs=2, trainer=_StubTrainer(), history=hist)
    assert (tr, va, best) == plain[1:]
    assert trainer.cers == 6 and list(hist) == ["val_cer"]
    assert hist["val_cer"] == [(1 + 2 + 3) / 12, (4 + 5 + 6) / 12]
    hist = {"val_cer": [0.5]}                                         # an existing list is extended
    wakeword.train_ctc([batch], [batch], vocab=5, num_epochs=1, trainer=_StubTrainer(), history=hist)
    assert hist["val_cer"] == [0.5, 1 / 4]
