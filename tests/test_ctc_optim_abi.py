"""CPU tests of the surface of the GRU-CTC optimiser (wk_ctc_adam_step,
wk_ctc_weights, wk_ctc_set_weights, wk_ctc_optim_state, wk_ctc_set_optim_state):
the symbols are exported and declared, bad arguments are rejected before any
device work (the handle is a fake, never dereferenced pointer), the Python
names exist, and CTCTrainer refuses bad hyper-parameters before it touches the
GPU."""
import ctypes as C
import math
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wakeword.h")
NAMES = ("wk_ctc_weights", "wk_ctc_set_weights", "wk_ctc_adam_step", "wk_ctc_optim_state", "wk_ctc_set_optim_state")


@pytest.fixture(scope="module")
def L():
    from wakeword import _lib
    return _lib.lib()


def test_symbols_exported(L):
    from wakeword import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    txt = open(HEADER).read()
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+lr,\s*beta1,\s*beta2,\s*eps,\s*weight_decay,\s*max_norm;\s*\}\s*wk_ctc_adam;", txt)
    assert [f[0] for f in _lib.WkCtcAdam._fields_] == ["lr", "beta1", "beta2", "eps", "weight_decay", "max_norm"]
    assert C.sizeof(_lib.WkCtcAdam) == 24
    import wakeword
    for name in ("weights", "state_dict", "set_weights", "adam_step", "optim_state", "set_optim_state"):
        assert callable(getattr(wakeword.CTCModel, name))
    for name in ("grad", "apply", "step", "val_loss", "weights", "state_dict", "optim_state", "load_optim_state", "to_model"):
        assert callable(getattr(wakeword.CTCTrainer, name))
    assert callable(wakeword.train_ctc)


P = C.c_void_p(4096)
GOOD = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=5.0)


def _id(o):
    return "-".join(f"{k}={getattr(v, 'value', v)}" for k, v in o.items())


@pytest.mark.parametrize("over", [dict(c=None), dict(opt=None), dict(grads=None), dict(lr=-1e-3), dict(lr=math.inf),
                                  dict(lr=math.nan), dict(beta1=-0.1), dict(beta1=1.0), dict(beta1=math.nan), dict(beta2=1.0),
                                  dict(beta2=-1e-6), dict(beta2=1.5), dict(eps=0.0), dict(eps=-1e-8), dict(eps=math.nan),
                                  dict(weight_decay=-1e-2), dict(weight_decay=math.nan), dict(max_norm=math.nan)], ids=_id)
def test_adam_step_rejects_bad_arguments_without_gpu(L, over):
    from wakeword import _lib
    h = dict(GOOD)
    h.update({k: v for k, v in over.items() if k in GOOD})
    opt = _lib.WkCtcAdam(h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["max_norm"])
    a = dict(c=P, opt=C.byref(opt), grads=P)
    a.update({k: v for k, v in over.items() if k in a})
    assert L.wk_ctc_adam_step(a["c"], a["opt"], a["grads"], None, None) == 1
    assert b"wk_ctc_adam_step" in L.wk_last_error()


def test_blob_and_state_calls_reject_bad_arguments_without_gpu(L):
    step = C.c_int64(0)
    for call, name in ((lambda: L.wk_ctc_weights(None, P, None), "wk_ctc_weights"),
                       (lambda: L.wk_ctc_weights(P, None, None), "wk_ctc_weights"),
                       (lambda: L.wk_ctc_set_weights(None, P, None), "wk_ctc_set_weights"),
                       (lambda: L.wk_ctc_set_weights(P, None, None), "wk_ctc_set_weights"),
                       (lambda: L.wk_ctc_optim_state(None, P, P, C.byref(step), None), "wk_ctc_optim_state"),
                       (lambda: L.wk_ctc_set_optim_state(None, None, None, 0, None), "wk_ctc_set_optim_state"),
                       (lambda: L.wk_ctc_set_optim_state(P, P, P, -1, None), "wk_ctc_set_optim_state"),
                       (lambda: L.wk_ctc_set_optim_state(P, None, None, -(1 << 40), None), "wk_ctc_set_optim_state")):
        assert call() == 1
        assert name.encode() in L.wk_last_error()


@pytest.mark.parametrize("over", [dict(lr=-1.0), dict(lr=math.inf), dict(lr=math.nan), dict(lr="fast"), dict(betas=(0.9,)),
                                  dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=0.0), dict(eps=-1.0),
                                  dict(weight_decay=-1e-3), dict(max_norm=math.nan)], ids=_id)
def test_trainer_rejects_bad_hyper_parameters_without_gpu(over):
    """(the message names the hyper-parameter: the blob's size check, which comes later, is not what raised)"""
    import numpy as np
    import wakeword
    with pytest.raises(ValueError, match=r"^(lr|betas|eps|weight_decay|max_norm) must"):
        wakeword.CTCTrainer(np.zeros(8, np.float32), vocab=16, device=99, **over)
