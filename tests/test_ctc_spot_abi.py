"""CPU tests of wk_ctc_spot's surface: the symbols are exported and typed, bad
arguments are rejected before any device work (fake pointers, never
dereferenced), the workspace size is 0 beyond the limits, grows with nothing
per (utterance, keyword) pair, and the Python side handles its arguments
(keyword_tokens, padded keywords and lists, batch_first, rejections)."""
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
    for name in ("wk_ctc_spot_workspace_bytes", "wk_ctc_spot"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert L.wk_ctc_spot_workspace_bytes.restype is C.c_int64 and len(L.wk_ctc_spot_workspace_bytes.argtypes) == 4
    assert len(L.wk_ctc_spot.argtypes) == 17
    assert callable(wakeword.ctc_spot) and callable(wakeword.keyword_tokens) and callable(wakeword.KeywordSpotter)
    assert hasattr(wakeword.CTCModel, "spot") and hasattr(wakeword.CTCModel, "spot_audio")
    assert wakeword.Spot._fields == ("scores", "spans", "frame_scores")
    assert wakeword.Detection._fields == ("utterance", "keyword", "confidence", "start_s", "end_s")


def _call(L, **over):
    """wk_ctc_spot with fake (never dereferenced) device pointers and a valid shape, but for the overrides."""
    p = C.c_void_p(4096)
    a = dict(lp=p, batch=2, T=5, vocab=7, in_len=p, kw=p, kw_stride=3, kw_len=p, n_keywords=4, max_keyword_len=3, normalize=1,
             ws=p, scores=p, spans=p, trace=p, device=0, stream=None)
    a.update(over)
    return L.wk_ctc_spot(a["lp"], a["batch"], a["T"], a["vocab"], a["in_len"], a["kw"], a["kw_stride"], a["kw_len"],
                         a["n_keywords"], a["max_keyword_len"], a["normalize"], a["ws"], a["scores"], a["spans"], a["trace"],
                         a["device"], a["stream"])


@pytest.mark.parametrize("over", [dict(lp=None), dict(kw=None), dict(kw_len=None), dict(ws=None), dict(scores=None),
                                  dict(spans=None), dict(batch=0), dict(batch=-1), dict(T=0), dict(T=-3), dict(vocab=0),
                                  dict(vocab=-1), dict(n_keywords=0), dict(n_keywords=-2), dict(kw_stride=2),
                                  dict(max_keyword_len=0), dict(max_keyword_len=-1), dict(max_keyword_len=33, kw_stride=33),
                                  dict(vocab=65537), dict(batch=1 << 20, T=1 << 9), dict(batch=1 << 29, T=1),
                                  dict(batch=1 << 20, n_keywords=17), dict(ws=C.c_void_p(4100)), dict(device=-1)],
                         ids=lambda o: "-".join(f"{k}={getattr(v, 'value', v)}" for k, v in o.items()))
def test_bad_arguments_rejected_without_gpu(L, over):
    assert _call(L, **over) == 1
    assert b"wk_ctc_spot" in L.wk_last_error()


def test_workspace_bytes(L):
    f = L.wk_ctc_spot_workspace_bytes
    base = f(8, 801, 1, 32)
    assert base >= 4 * 8 * 801                                   # the row maxima, [batch][T]
    for bad in ((0, 801, 1, 4), (8, 0, 1, 4), (8, 801, 0, 4), (8, 801, 1, 0), (8, 801, 1, 33), (1 << 20, 1 << 9, 1, 4),
                ((1 << 28) + 1, 1, 1, 4), (1 << 20, 1, 17, 4), (-1, 801, 1, 4), (8, -1, 1, 4), (8, 801, -1, 4), (8, 801, 1, -1)):
        assert f(*bad) == 0, bad
    assert f(1 << 20, 1 << 8, 16, 32) > 0 and f(1, 1, 1 << 24, 1) > 0      # the limits themselves
    # non-decreasing in every argument
    for b, t, k, s in ((1, 1, 1, 1), (3, 17, 2, 5), (257, 5, 7, 31), (8, 801, 63, 8)):
        here = f(b, t, k, s)
        assert here > 0
        assert f(b + 1, t, k, s) >= here and f(b, t + 1, k, s) >= here and f(b, t, k + 1, s) >= here and f(b, t, k, s + 1) >= here
    sizes = [f(8, 801, 64, s) for s in range(1, 33)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert f(9, 801, 1, 32) > base and f(8, 900, 1, 32) > base
    # nothing scales with batch * T * n_keywords: no gathered [batch][K][T][L] buffer, no per-pair rows
    assert f(8, 801, 64, 32) - f(8, 801, 1, 32) <= f(1, 1, 64, 32)
    # no gathered rows and no back-pointers: well under the forced alignment's at the same shape
    assert f(8, 801, 1, 4) < L.wk_ctc_align_workspace_bytes(8, 801, 4)


def test_workspace_bytes_pinned(L):
    """The sizes themselves: (batch, T, n_keywords, max_keyword_len), T = 801 among them."""
    f = L.wk_ctc_spot_workspace_bytes
    assert f(8, 801, 3, 5) == 25856 and f(1, 1, 1, 1) == 256
    assert f(3, 17, 2, 32) == 256 and f(257, 5, 7, 9) == 5376


def test_keyword_tokens():
    import wakeword
    c2i = {"a": 1, "b": 2, "c": 3, "小": 4}
    tok, ln = wakeword.keyword_tokens(["abc", "b", "小a"], c2i)
    assert tok.dtype == np.int32 and ln.dtype == np.int32
    assert tok.tolist() == [[1, 2, 3], [2, 0, 0], [4, 1, 0]] and ln.tolist() == [3, 1, 2]
    tok, ln = wakeword.keyword_tokens("ab", c2i)                  # one word
    assert tok.tolist() == [[1, 2]] and ln.tolist() == [2]
    with pytest.raises(KeyError):
        wakeword.keyword_tokens(["abz"], c2i)
    with pytest.raises(ValueError, match="length"):
        wakeword.keyword_tokens(["a", ""], c2i)
    with pytest.raises(ValueError, match="length"):
        wakeword.keyword_tokens(["a" * 33], c2i)
    assert wakeword.keyword_tokens(["a" * 32], c2i)[1].tolist() == [32]
    with pytest.raises(ValueError, match="no keywords"):
        wakeword.keyword_tokens([], c2i)


def test_wrapper_rejects_bad_arguments():
    import wakeword
    lp = torch.zeros((2, 3, 4))
    with pytest.raises(ValueError, match="HIP device"):
        wakeword.ctc_spot(lp, [[1, 2]])
    with pytest.raises(ValueError, match="HIP device"):
        wakeword.ctc_spot(lp.double(), [[1, 2]])
    with pytest.raises(ValueError, match="HIP device"):
        wakeword.ctc_spot(np.zeros((2, 3, 4), np.float32), [[1, 2]])
    with pytest.raises(ValueError, match="threshold"):
        wakeword.KeywordSpotter(None, {"a": 1}, ["a"], threshold=1.0)
    with pytest.raises(KeyError):
        wakeword.KeywordSpotter(None, {"a": 1}, ["ab"])


def test_argument_handling():
    """ctc_spot's argument handling (wakeword.ctc._spot_args; the device check
    is ctc_spot's own): (T, B, V) and batch-first give the same (B, T, V)
    tensor; a padded array with lengths, a tensor and a list of lists the same
    keywords; lengths int32; padding wider than 32 is cut to the longest keyword."""
    from wakeword import ctc
    lp = torch.randn((5, 3, 4), generator=torch.Generator().manual_seed(0))        # (T, B, V)
    padded = np.array([[1, 2, 3], [3, 0, 0], [2, 2, 0]])
    a = ctc._spot_args(lp, padded, [3, 1, 2], [5, 4, 0], batch_first=False)
    b = ctc._spot_args(lp.transpose(0, 1).contiguous(), torch.from_numpy(padded), torch.tensor([3, 1, 2]), torch.tensor([5, 4, 0]),
                       batch_first=True)
    c = ctc._spot_args(lp, [[1, 2, 3], [3], [2, 2]], None, [5, 4, 0], batch_first=False)
    for other in (b, c):
        for x, y in zip(a[:4], other[:4]):
            assert torch.equal(x, y)
        assert other[4] == 3
    assert a[0].shape == (3, 5, 4) and a[0].is_contiguous() and torch.equal(a[0], lp.transpose(0, 1))
    assert a[1].dtype == a[2].dtype == a[3].dtype == torch.int32
    assert a[1].tolist() == padded.tolist() and a[2].tolist() == [3, 1, 2] and a[3].tolist() == [5, 4, 0] and a[4] == 3
    # no lengths: every row is a whole keyword; no input lengths: None goes to the kernel
    d = ctc._spot_args(lp, padded[:1], None, None, batch_first=False)
    assert d[2].tolist() == [3] and d[3] is None
    wide = np.zeros((2, 40), dtype=np.int64)
    wide[0, :5], wide[1, :2] = 1, 2
    e = ctc._spot_args(lp, wide, [5, 2], None, batch_first=False)
    assert e[1].shape == (2, 40) and e[4] == 5
    with pytest.raises(ValueError, match="at most 32"):
        ctc._spot_args(lp, wide, [40, 2], None, batch_first=False)
    with pytest.raises(ValueError, match="3 keywords"):
        ctc._spot_args(lp, padded, [3, 1], None, batch_first=False)
    with pytest.raises(ValueError, match="batch of 3"):
        ctc._spot_args(lp, padded, [3, 1, 2], [5, 4], batch_first=False)
    with pytest.raises(ValueError, match="keywords must be"):
        ctc._spot_args(lp, np.array([1, 2, 3]), None, None, batch_first=False)
    with pytest.raises(ValueError, match="keywords must be"):
        ctc._spot_args(lp, [], None, None, batch_first=False)


def test_detections_from_a_spot():
    """KeywordSpotter.detections: exp(score) > threshold, times from span_seconds."""
    import wakeword
    sp = wakeword.KeywordSpotter(None, {"a": 1, "b": 2}, ["ab", "b"], threshold=0.5, hop=160, sample_rate=16000)
    assert sp.tokens.tolist() == [[1, 2], [2, 0]] and sp.lengths.tolist() == [2, 1]
    spot = wakeword.Spot(torch.tensor([[0.0, -np.inf], [np.log(0.4), np.log(0.75)]], dtype=torch.float32),
                         torch.tensor([[[10, 25], [-1, -1]], [[3, 9], [40, 41]]], dtype=torch.int32))
    got = sp.detections(spot)
    assert [(d.utterance, d.keyword) for d in got] == [(0, "ab"), (1, "b")]
    assert got[0].confidence == 1.0 and (got[0].start_s, got[0].end_s) == (0.1, 0.25)
    assert abs(got[1].confidence - 0.75) < 1e-6 and (got[1].start_s, got[1].end_s) == (0.4, 0.41)
