"""CPU tests of the surface of wk_ctc_forward_train / wk_ctc_backward: the
symbols are exported and declared, bad arguments are rejected before any device
work (the handle is a fake, never dereferenced pointer), and the Python names
exist with unpack_grads following the state-dict spec."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from wakeword import _lib
    return _lib.lib()


def test_symbols_exported(L):
    from wakeword import _lib
    for name in ("wk_ctc_forward_train", "wk_ctc_backward"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    import wakeword
    for name in ("forward_train", "backward", "loss_and_grad"):
        assert callable(getattr(wakeword.CTCModel, name))
    assert callable(wakeword.unpack_grads)


P = C.c_void_p(4096)


@pytest.mark.parametrize("over", [dict(c=None), dict(feats=None), dict(lp=None), dict(batch=0), dict(batch=-1), dict(T=0),
                                  dict(T=-2), dict(batch=1 << 20, T=1 << 11), dict(batch=1 << 40, T=1 << 30)],
                         ids=lambda o: "-".join(f"{k}={getattr(v, 'value', v)}" for k, v in o.items()))
def test_forward_train_rejects_bad_arguments_without_gpu(L, over):
    a = dict(c=P, feats=P, batch=2, T=5, lp=P)
    a.update(over)
    assert L.wk_ctc_forward_train(a["c"], a["feats"], a["batch"], a["T"], a["lp"], None) == 1
    assert b"wk_ctc_forward_train" in L.wk_last_error()


@pytest.mark.parametrize("over", [dict(c=None), dict(dlogits=None), dict(grads=None), dict(batch=0), dict(batch=-1), dict(T=0),
                                  dict(T=-2), dict(batch=1 << 20, T=1 << 11), dict(batch=1 << 40, T=1 << 30)],
                         ids=lambda o: "-".join(f"{k}={getattr(v, 'value', v)}" for k, v in o.items()))
def test_backward_rejects_bad_arguments_without_gpu(L, over):
    a = dict(c=P, batch=2, T=5, dlogits=P, grads=P)
    a.update(over)
    assert L.wk_ctc_backward(a["c"], a["batch"], a["T"], a["dlogits"], a["grads"], None, None) == 1
    assert b"wk_ctc_backward" in L.wk_last_error()


def test_unpack_grads_follows_the_spec(L):
    import wakeword
    from wakeword import _lib
    V = 37
    cfg = _lib.WkCtcConfig(V, 128, 2, 80, 0, 0)
    n = L.wk_ctc_num_weights(C.byref(cfg))
    flat = np.arange(n, dtype=np.float32)
    g = wakeword.unpack_grads(flat, V)
    spec = wakeword.ctc_state_dict_spec(V)
    assert list(g) == [k for k, _ in spec]
    off = 0
    for k, shape in spec:
        assert g[k].shape == shape and g[k].reshape(-1)[0] == off and np.shares_memory(g[k], flat)
        off += int(np.prod(shape))
    assert off == n
    # a state dict and its gradient share one layout
    assert np.array_equal(wakeword.pack_state_dict(g, V), flat)
    with pytest.raises(ValueError):
        wakeword.unpack_grads(flat[:-1], V)
