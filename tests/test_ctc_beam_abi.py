"""CPU tests of wk_ctc_beam's surface: the symbols are exported and typed, bad
arguments are rejected before any device work (fake pointers, never
dereferenced), the workspace size is 0 beyond the limits and grows with the
problem, and the Python side handles its arguments (ValueErrors, (T, B, V)
and batch_first, beam_texts)."""
import ctypes as C
import inspect

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
    for name in ("wk_ctc_beam_workspace_bytes", "wk_ctc_beam"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert L.wk_ctc_beam_workspace_bytes.restype is C.c_int64 and len(L.wk_ctc_beam_workspace_bytes.argtypes) == 4
    assert len(L.wk_ctc_beam.argtypes) == 16
    assert callable(wakeword.ctc_beam_search) and callable(wakeword.beam_texts)
    assert hasattr(wakeword.CTCModel, "beam_decode") and hasattr(wakeword.CTCModel, "beam_decode_audio")
    assert wakeword.BeamResult._fields == ("tokens", "lengths", "scores", "candidates")
    sig = inspect.signature(wakeword.ctc_beam_search)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [
        ("input_lengths", None), ("beam", 16), ("top_k", 16), ("n_best", 1), ("max_len", None), ("batch_first", False),
        ("return_candidates", False)]
    for fn in (wakeword.CTCModel.transcribe, wakeword.CTCModel.transcribe_text):
        assert inspect.signature(fn).parameters["beam"].default is None


def _call(L, **over):
    """wk_ctc_beam with fake (never dereferenced) device pointers and a valid shape, but for the overrides."""
    p = C.c_void_p(4096)
    a = dict(lp=p, batch=2, T=5, vocab=7, in_len=p, beam=4, top_k=3, n_best=2, max_len=5, ws=p, tokens=p, lengths=p, scores=p,
             cand=p, device=0, stream=None)
    a.update(over)
    return L.wk_ctc_beam(a["lp"], a["batch"], a["T"], a["vocab"], a["in_len"], a["beam"], a["top_k"], a["n_best"], a["max_len"],
                         a["ws"], a["tokens"], a["lengths"], a["scores"], a["cand"], a["device"], a["stream"])


@pytest.mark.parametrize("over", [dict(lp=None), dict(ws=None), dict(tokens=None), dict(lengths=None), dict(scores=None),
                                  dict(batch=0), dict(batch=-1), dict(T=0), dict(T=-3), dict(vocab=1), dict(vocab=0),
                                  dict(vocab=-1), dict(vocab=65537), dict(beam=0), dict(beam=65, n_best=1), dict(beam=-1),
                                  dict(top_k=0), dict(top_k=33), dict(top_k=-1), dict(n_best=0), dict(n_best=5),
                                  dict(n_best=-1), dict(max_len=0), dict(max_len=-2), dict(batch=1 << 20, T=1 << 9),
                                  dict(batch=(1 << 28) + 1, T=1), dict(ws=C.c_void_p(4100)), dict(ws=C.c_void_p(4104)),
                                  dict(device=-1)],
                         ids=lambda o: "-".join(f"{k}={getattr(v, 'value', v)}" for k, v in o.items()))
def test_bad_arguments_rejected_without_gpu(L, over):
    assert _call(L, **over) == 1
    assert b"wk_ctc_beam" in L.wk_last_error()


def test_workspace_bytes(L):
    f = L.wk_ctc_beam_workspace_bytes
    base = f(8, 801, 16, 16)
    assert base > 0
    assert f(9, 801, 16, 16) > base and f(8, 802, 16, 16) > base and f(8, 801, 17, 16) > base and f(8, 801, 16, 17) > base
    for b, t in ((1, 1), (3, 17), (257, 5)):
        by_w = [f(b, t, w, 7) for w in range(1, 65)]
        by_k = [f(b, t, 9, k) for k in range(1, 33)]
        assert by_w[0] > 0 and by_k[0] > 0
        assert all(y >= x for x, y in zip(by_w, by_w[1:])) and all(y >= x for x, y in zip(by_k, by_k[1:]))
        assert f(b + 1, t, 9, 7) >= f(b, t, 9, 7) and f(b, t + 1, 9, 7) >= f(b, t, 9, 7)
    # per frame: the K candidates with their values, the blank's value, and a row of W search-tree nodes
    assert base >= 8 * 801 * (4 * (2 * 16 + 1) + 8 * 16)
    # far below the log-probs it decodes (V = 4000)
    assert base < 8 * 801 * 4000 * 4 // 16
    # the largest legal problem has a size (int64)
    assert f(1, 1 << 28, 64, 32) > (1 << 28) * (8 * 64 + 4 * 65)
    for bad in ((0, 801, 16, 16), (8, 0, 16, 16), (-1, 801, 16, 16), (8, 801, 0, 16), (8, 801, 65, 16), (8, 801, 16, 0),
                (8, 801, 16, 33), (1 << 20, 1 << 9, 16, 16), ((1 << 28) + 1, 1, 1, 1)):
        assert f(*bad) == 0


def test_workspace_bytes_pinned(L):
    """The sizes themselves: (batch, T, beam, top_k), T = 801 among them."""
    f = L.wk_ctc_beam_workspace_bytes
    assert f(8, 801, 16, 16) == 1666304 and f(1, 1, 1, 1) == 256
    assert f(3, 17, 64, 32) == 39424 and f(257, 5, 5, 3) == 89600


def test_wrapper_rejects_bad_arguments():
    import wakeword
    from wakeword import ctc
    lp = torch.zeros((2, 3, 4))
    with pytest.raises(ValueError, match="HIP device"):
        wakeword.ctc_beam_search(lp)
    with pytest.raises(ValueError, match="HIP device"):
        wakeword.ctc_beam_search(lp.double())
    with pytest.raises(ValueError, match="HIP device"):
        wakeword.ctc_beam_search(np.zeros((2, 3, 4), np.float32))
    good = dict(input_lengths=None, beam=4, top_k=3, n_best=2, max_len=None, batch_first=False)
    for bad, what in ((dict(beam=0), "beam"), (dict(beam=65), "beam"), (dict(beam=4.0), "beam"), (dict(top_k=0), "top_k"),
                      (dict(top_k=33), "top_k"), (dict(n_best=0), "n_best"), (dict(n_best=5), "n_best"),
                      (dict(max_len=0), "max_len"), (dict(max_len=2.5), "max_len"), (dict(input_lengths=[3]), "batch of 3"),
                      (dict(beam=True), "beam")):
        with pytest.raises(ValueError, match=what):
            ctc._beam_args(lp, **{**good, **bad})
    with pytest.raises(ValueError, match="V at least 2"):
        ctc._beam_args(torch.zeros((3, 2, 1)), **good)


def test_argument_handling_layouts():
    """(T, B, V) and batch-first give the same (B, T, V) tensor; lengths become
    int32 on the log-probs' device; max_len defaults to T."""
    from wakeword import ctc
    lp = torch.randn((5, 3, 4), generator=torch.Generator().manual_seed(0))        # (T, B, V)
    a = ctc._beam_args(lp, [5, 4, 0], 4, 3, 2, None, batch_first=False)
    b = ctc._beam_args(lp.transpose(0, 1).contiguous(), torch.tensor([5, 4, 0]), 4, 3, 2, 7, batch_first=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].shape == (3, 5, 4) and a[0].is_contiguous() and torch.equal(a[0], lp.transpose(0, 1))
    assert a[1].dtype == torch.int32 and a[1].tolist() == [5, 4, 0]
    assert a[2] == 5 and b[2] == 7
    assert ctc._beam_args(lp, None, 4, 3, 2, None, batch_first=False)[1] is None
    src = lp.transpose(0, 1).contiguous()
    assert ctc._beam_args(src, None, 1, 1, 1, None, batch_first=True)[0].data_ptr() == src.data_ptr()      # no copy


def test_beam_texts():
    import wakeword
    tokens = np.array([[[3, 1, -1], [2, -1, -1]], [[-1, -1, -1], [-1, -1, -1]], [[1, 2, 3], [9, 9, 1]]], dtype=np.int32)
    lengths = np.array([[2, 1], [0, -1], [5, 3]], dtype=np.int32)        # (utterance 2: a hypothesis longer than the rows)
    res = wakeword.BeamResult(tokens, lengths, np.zeros((3, 2), np.float32))
    chars = {1: "a", 2: "b", 3: "c"}
    assert wakeword.beam_texts(res, chars) == [["ca", "b"], [""], ["abc", "<unk><unk>a"]]
    as_t = wakeword.BeamResult(torch.from_numpy(tokens), torch.from_numpy(lengths), None)
    assert wakeword.beam_texts(as_t, chars) == wakeword.beam_texts(res, chars)
    assert res.candidates is None
