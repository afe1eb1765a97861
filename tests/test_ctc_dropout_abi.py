"""CPU tests of the surface of train-mode dropout: the symbols are exported and
declared, bad arguments are rejected before any device work (the handle is a
fake, never dereferenced pointer), and the Python keywords exist and validate."""
import ctypes as C
import math
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "wakeword.h")


@pytest.fixture(scope="module")
def L():
    from wakeword import _lib
    return _lib.lib()


def test_symbols_exported_and_declared(L):
    from wakeword import _lib
    for name in ("wk_ctc_forward_train_dropout", "wk_ctc_dropout_masks"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    txt = open(HEADER).read()
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+p_enc,\s*p_gru;\s*uint64_t\s+seed,\s*offset;\s*\}\s*wk_ctc_dropout;", txt)
    assert C.sizeof(_lib.WkCtcDropout) == 24 and _lib.WkCtcDropout.seed.offset == 8 and _lib.WkCtcDropout.offset.offset == 16
    assert "captured graph" in txt[txt.index("train-mode dropout"):txt.index("wk_ctc_dropout;")]


P = C.c_void_p(4096)


def _call(L, drop, c=P, feats=P, batch=2, T=5, lp=P):
    return L.wk_ctc_forward_train_dropout(c, feats, batch, T, C.byref(drop) if drop is not None else None, lp, None)


@pytest.mark.parametrize("p_enc,p_gru,offset", [(-0.1, 0.2, 0), (0.2, -1e-9, 0), (1.0, 0.2, 0), (0.2, 1.5, 0), (math.nan, 0.2, 0),
                                                (0.2, math.nan, 0), (0.2, 0.2, 2 ** 63), (0.0, 0.0, 2 ** 64 - 1)])
def test_bad_dropout_is_rejected_without_gpu(L, p_enc, p_gru, offset):
    from wakeword import _lib
    assert _call(L, _lib.WkCtcDropout(p_enc, p_gru, 1, offset)) == 1
    assert b"wk_ctc_forward_train_dropout" in L.wk_last_error()


def test_null_drop_and_the_existing_argument_rules(L):
    from wakeword import _lib
    assert _call(L, None) == 1
    assert b"null drop" in L.wk_last_error()
    ok = _lib.WkCtcDropout(0.2, 0.2, 1, 2 ** 63 - 1)
    for over in (dict(c=None), dict(feats=None), dict(lp=None), dict(batch=0), dict(T=0), dict(batch=1 << 20, T=1 << 11)):
        assert _call(L, ok, **over) == 1, over
    assert L.wk_ctc_dropout_masks(None, P, P, None) == 1


def test_python_keywords():
    import inspect

    import wakeword
    from wakeword.ctc import dropout_pair
    for fn in (wakeword.CTCModel.forward_train, wakeword.CTCModel.loss_and_grad):
        prm = inspect.signature(fn).parameters
        assert prm["dropout"].default is None and prm["seed"].default == 0 and prm["offset"].default == 0
    prm = inspect.signature(wakeword.CTCTrainer.__init__).parameters
    assert prm["dropout"].default == 0.0 and prm["seed"].default == 0
    for name in ("rng_state", "load_rng_state"):
        assert callable(getattr(wakeword.CTCTrainer, name))
    assert callable(wakeword.CTCModel.dropout_masks)
    assert "0.2" in wakeword.train_ctc.__doc__ and "dropout" in wakeword.train_ctc.__doc__
    assert dropout_pair(None) == (0.0, 0.0) and dropout_pair(0.2) == (0.2, 0.2) and dropout_pair((0.5, 0)) == (0.5, 0.0)
    for bad in (1.0, -0.1, (0.2,), (0.2, 0.2, 0.2), "0.2", math.nan, True):
        with pytest.raises(ValueError):
            dropout_pair(bad)
