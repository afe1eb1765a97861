"""GPU test: destroying a handle or a stream object gives its device memory back.

The handle structs own their device and pinned memory through the owner types
of csrc/wk_devmem.h, and a destroy is a `delete` with the device current.  The
driver's free-memory figure can see two of the objects:
  * a mode-B wk_handle with weights: its feature workspace alone is
    16,384 x 819 x 4 B, about 54 MB;
  * a wk_stream of capacity 4,000,000 samples, hop 480: its mirrored device
    ring is 2 x 4,000,000 x 4 B = 32 MB.
For each: free memory f0; create one object, read f1, destroy it; then 16
create -> use once -> destroy cycles; read f2.  f0 - f1 > 0 shows that the probe
sees the footprint, and f0 - f2 <= 2 (f0 - f1) allows one footprint of
allocator slack (code objects loaded on first launch, the runtime's pools) where
a struct that stopped freeing would be short of 16 footprints, 8 x the bound.
The factor 2 is a condition, not a measurement.

Everything goes through ctypes, not through Python objects whose finalisers run
late.  wk_ctc, wk_trainer and wk_esp_mfcc objects are too small to see this way
(a few MB at most, within the runtime's own noise): their release rests on the
same owner types and on review.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIN = 16000
CYCLES = 16


def _free_bytes(torch):
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _create_handle(L, _lib, blob):
    cfg = _lib.WkConfig(_lib.WK_MODE_TORCHAUDIO_CMVN, _lib.WK_PREC_FP32, 1, 0, 1)
    h = C.c_void_p()
    _lib.check(L.wk_create(C.byref(cfg), blob.ctypes.data_as(C.c_void_p), C.byref(h)), "wk_create")
    return h


def _check_returned(f0, f1, f2, what):
    foot, lost = f0 - f1, f0 - f2
    print(f"{what}: footprint {foot / 1e6:.1f} MB, after {CYCLES} cycles {lost / 1e6:.1f} MB short of the start")
    assert foot > 0, (what, f0, f1)
    assert lost <= 2 * foot, (what, f0, f1, f2)


@pytest.fixture(scope="module")
def blob(xiaoa_sd):
    from wakeword.api import pack_weights
    return pack_weights(xiaoa_sd)


def test_handle_memory_comes_back(gpu, blob):
    torch = gpu
    from wakeword import _lib
    L = _lib.lib()
    clips = torch.zeros(4, WIN, dtype=torch.float32, device="cuda:0")
    logits = torch.empty(4, dtype=torch.float32, device="cuda:0")
    f0 = _free_bytes(torch)
    h = _create_handle(L, _lib, blob)
    f1 = _free_bytes(torch)
    _lib.check(L.wk_destroy(h), "wk_destroy")
    for _ in range(CYCLES):
        h = _create_handle(L, _lib, blob)
        _lib.check(L.wk_forward(h, C.c_void_p(clips.data_ptr()), _lib.WK_DTYPE_F32, 4, WIN, WIN,
                                C.c_void_p(logits.data_ptr()), None, None), "wk_forward")
        torch.cuda.synchronize()
        _lib.check(L.wk_destroy(h), "wk_destroy")
    f2 = _free_bytes(torch)
    assert bool(torch.isfinite(logits).all())
    _check_returned(f0, f1, f2, "wk_handle")


def test_stream_memory_comes_back(gpu, blob):
    torch = gpu
    from wakeword import _lib
    L = _lib.lib()
    cap, hop, n = 4_000_000, 480, 16_480   # one push of 16,480 samples completes windows 0 and 1
    samples = np.zeros(n, np.float32)
    out = np.empty(8, np.float32)
    n_out = C.c_int32()
    fp = C.POINTER(C.c_float)

    def create():
        s = C.c_void_p()
        _lib.check(L.wk_stream_create(h, hop, cap, None, C.byref(s)), "wk_stream_create")
        return s

    h = _create_handle(L, _lib, blob)
    try:
        f0 = _free_bytes(torch)
        s = create()
        f1 = _free_bytes(torch)
        _lib.check(L.wk_stream_destroy(s), "wk_stream_destroy")
        for _ in range(CYCLES):
            s = create()
            _lib.check(L.wk_stream_push(s, samples.ctypes.data_as(fp), n, out.ctypes.data_as(fp), None, 8,
                                        C.byref(n_out)), "wk_stream_push")
            assert n_out.value == 2
            _lib.check(L.wk_stream_destroy(s), "wk_stream_destroy")
        f2 = _free_bytes(torch)
    finally:
        L.wk_destroy(h)
    _check_returned(f0, f1, f2, "wk_stream")
