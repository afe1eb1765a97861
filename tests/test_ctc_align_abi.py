"""CPU tests of wk_ctc_align's surface: the symbols are exported and typed, bad
arguments are rejected before any device work (fake pointers, never
dereferenced), the workspace size is 0 beyond the limits and grows with the
problem, and the Python side handles its arguments (span_seconds, padded and
concatenated targets, batch_first)."""
import ctypes as C

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
    for name in ("wk_ctc_align_workspace_bytes", "wk_ctc_align"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert L.wk_ctc_align_workspace_bytes.restype is C.c_int64 and len(L.wk_ctc_align.argtypes) == 17
    assert callable(wakeword.ctc_align) and callable(wakeword.span_seconds)
    assert hasattr(wakeword.CTCModel, "align") and hasattr(wakeword.CTCModel, "align_audio")
    assert wakeword.Alignment._fields == ("states", "tokens", "frame_log_probs", "spans", "scores")


def _call(L, **over):
    """wk_ctc_align with fake (never dereferenced) device pointers and a valid shape, but for the overrides."""
    p = C.c_void_p(4096)
    a = dict(lp=p, batch=2, T=5, vocab=7, labels=p, label_stride=3, in_len=p, lab_len=p, max_label_len=3, ws=p, states=p,
             tokens=p, frame_lp=p, spans=p, score=p, device=0, stream=None)
    a.update(over)
    return L.wk_ctc_align(a["lp"], a["batch"], a["T"], a["vocab"], a["labels"], a["label_stride"], a["in_len"], a["lab_len"],
                          a["max_label_len"], a["ws"], a["states"], a["tokens"], a["frame_lp"], a["spans"], a["score"],
                          a["device"], a["stream"])


@pytest.mark.parametrize("over", [dict(lp=None), dict(labels=None), dict(in_len=None), dict(lab_len=None), dict(ws=None),
                                  dict(states=None), dict(score=None), dict(batch=0), dict(batch=-1), dict(T=0), dict(T=-3),
                                  dict(vocab=0), dict(vocab=-1), dict(label_stride=2), dict(max_label_len=-1),
                                  dict(max_label_len=256, label_stride=256), dict(vocab=65537),
                                  dict(batch=1 << 20, T=1 << 9), dict(ws=C.c_void_p(4100)), dict(device=-1)],
                         ids=lambda o: "-".join(f"{k}={getattr(v, 'value', v)}" for k, v in o.items()))
def test_bad_arguments_rejected_without_gpu(L, over):
    assert _call(L, **over) == 1
    assert b"wk_ctc_align" in L.wk_last_error()


def test_workspace_bytes(L):
    f = L.wk_ctc_align_workspace_bytes
    base = f(8, 801, 40)
    assert base > 0
    assert f(9, 801, 40) > base and f(8, 802, 40) > base
    sizes = [f(300, 7, s) for s in range(0, 256)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:]))          # non-decreasing in the label length
    for s in (31, 63, 127):                                                       # a wider state row at each 64-lane step
        assert sizes[s + 1] - sizes[s] >= 4 * 300 * 7 * 64
    for b, t in ((1, 1), (3, 17), (257, 5)):
        assert f(b + 1, t, 9) >= f(b, t, 9) and f(b, t + 1, 9) >= f(b, t, 9)
    # the gathered log-probs (>= 2S+1 floats per frame) and one back-pointer row of 64 words per frame
    assert base >= 4 * 8 * 801 * (81 + 64)
    # no alpha rows: well under wk_ctc_loss's three rows per frame at the same shape
    assert base < L.wk_ctc_loss_workspace_bytes(8, 801, 40)
    for bad in ((0, 801, 40), (8, 0, 40), (8, 801, -1), (8, 801, 256), (1 << 20, 1 << 9, 1)):
        assert f(*bad) == 0


def test_workspace_bytes_pinned(L):
    """The sizes themselves, at each register layout's last and first label
    length (31 | 32, 127, 255) and at T = 801."""
    f = L.wk_ctc_align_workspace_bytes
    assert f(8, 801, 31) == 3314944 and f(8, 801, 32) == 4955392
    assert f(3, 17, 127) == 99840 and f(257, 5, 255) == 3259904


def test_span_seconds():
    import wakeword
    spans = np.array([[[0, 3], [3, 50]], [[-1, -1], [-1, -1]]], dtype=np.int32)
    want = np.array([[[0.0, 0.03], [0.03, 0.5]], [[-1, -1], [-1, -1]]])
    got = wakeword.span_seconds(spans)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.allclose(got, want, rtol=0, atol=1e-15)
    got_t = wakeword.span_seconds(torch.from_numpy(spans))
    assert torch.is_tensor(got_t) and got_t.dtype == torch.float64 and np.array_equal(got_t.numpy(), got)
    # another front-end: hop 256 at 16 kHz
    assert wakeword.span_seconds(np.array([[[2, 4]]]), hop=256, sample_rate=16000).tolist() == [[[0.032, 0.064]]]


def test_wrapper_rejects_bad_arguments():
    import wakeword
    lp = torch.zeros((2, 3, 4))
    with pytest.raises(ValueError, match="HIP device"):
        wakeword.ctc_align(lp, torch.ones((3, 1)), [2, 2, 2], [1, 1, 1])
    with pytest.raises(ValueError, match="HIP device"):
        wakeword.ctc_align(lp.double(), torch.ones((3, 1)), [2, 2, 2], [1, 1, 1])


def test_argument_handling_padded_concatenated_batch_first():
    """ctc_align's argument handling (wakeword.ctc._align_args; the device check
    is ctc_align's own): (T, B, V) and batch-first give the same (B, T, V)
    tensor, padded and concatenated targets the same labels, lengths int32."""
    from wakeword import ctc
    lp = torch.randn((5, 3, 4), generator=torch.Generator().manual_seed(0))        # (T, B, V)
    padded = torch.tensor([[1, 2, 3], [3, 0, 0], [0, 0, 0]])
    lens = [3, 1, 0]
    concat = torch.tensor([1, 2, 3, 3])
    a = ctc._align_args(lp, padded, [5, 4, 0], lens, batch_first=False)
    b = ctc._align_args(lp.transpose(0, 1).contiguous(), concat, torch.tensor([5, 4, 0]), torch.tensor(lens), batch_first=True)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert a[0].shape == (3, 5, 4) and a[0].is_contiguous() and torch.equal(a[0], lp.transpose(0, 1))
    assert a[1].dtype == a[2].dtype == a[3].dtype == torch.int32
    assert a[1].tolist() == padded.tolist() and a[2].tolist() == [5, 4, 0] and a[3].tolist() == lens
    assert a[4] == b[4] == 3
    with pytest.raises(ValueError, match="batch of 3"):
        ctc._align_args(lp, padded, [5, 4], lens, batch_first=False)
    with pytest.raises(ValueError, match="target_lengths sum"):
        ctc._align_args(lp, concat, [5, 4, 0], [3, 2, 0], batch_first=False)
