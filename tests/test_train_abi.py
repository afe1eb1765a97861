"""CPU tests of the training entry points (wk_trainer_*): declared in the
header, exported, and rejecting bad arguments before any device work."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wakeword.h")
FUNCS = ("wk_trainer_create", "wk_trainer_destroy", "wk_trainer_grad", "wk_trainer_step", "wk_trainer_weights")


def test_header_declares_the_trainer():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = set(re.findall(r"\b([A-Za-z_]\w*)\s*\([^;{]*\)\s*;", txt))
    for name in FUNCS:
        assert name in fns, name
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+lr,\s*beta1,\s*beta2,\s*eps,\s*weight_decay;\s*\}\s*wk_adamw;", txt)
    assert "#define WK_ABI_VERSION 1" in txt


def test_null_arguments_rejected_without_gpu():
    from wakeword import _lib
    L = _lib.lib()
    h = C.c_void_p()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    opt = _lib.WkAdamW(5e-4, 0.9, 0.99, 1e-7, 1e-3)
    assert L.wk_trainer_create(0, None, C.byref(h)) == 1 and not h
    assert L.wk_trainer_create(0, p, None) == 1
    assert L.wk_trainer_destroy(None) == 1
    assert L.wk_trainer_grad(None, p, p, 1, p, None, None, None) == 1
    assert L.wk_trainer_step(None, C.byref(opt), None, None) == 1
    assert L.wk_trainer_weights(None, p, None) == 1
    assert b"null" in L.wk_last_error()


def test_train_module_imports():
    import wakeword
    from wakeword import train
    assert wakeword.Trainer is train.Trainer and wakeword.train_model is train.train_model
    sd = train.default_init(3)
    assert [tuple(sd[k].shape) for k in wakeword.api.STATE_KEYS] == [(32, 13, 3), (64, 32, 3), (128, 64, 3), (64, 128), (1, 64)]
    for k, v in sd.items():
        bound = 1.0 / (v[0].size ** 0.5)
        assert v.dtype.name == "float32" and abs(v).max() <= bound and abs(v).max() > 0.9 * bound
    assert all((train.default_init(3)[k] == sd[k]).all() for k in sd)
