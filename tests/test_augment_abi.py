"""CPU tests of wk_augment_batch's C surface: every argument rule of
include/wakeword.h is refused before any device work (no device is present
here), n == 0 is WK_OK, and the header's structs are the binding's."""
import ctypes as C
import math
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wakeword.h")
PTR = 0x1000          # a non-NULL device address: never read by a refused call, nor by n == 0


@pytest.fixture(scope="module")
def L():
    from wakeword import _lib
    return _lib.lib()


def call(L, audio=PTR, dtype=0, lens=None, n=2, in_len=16000, in_stride=16000, variants=((1.0, 1.0), (0.8, 1.0)),
         n_variants=None, spec=(0.005, 0.01, 5.0, 20.0, 0, 0), out_len=16000, out=PTR + 0x100000):
    from wakeword import _lib
    var = None
    if variants is not None:
        var = (_lib.WkAugVariant * max(len(variants), 1))(*[_lib.WkAugVariant(s, v) for s, v in variants])
    sp = C.byref(_lib.WkAugSpec(*spec)) if spec is not None else None
    K = len(variants or ()) if n_variants is None else n_variants
    return L.wk_augment_batch(C.c_void_p(audio), dtype, lens, n, in_len, in_stride, var, K, sp, out_len, C.c_void_p(out), None)


def test_n_zero_is_ok(L):
    assert call(L, n=0) == 0
    assert call(L, n=0, dtype=1, out_len=1, in_len=0, in_stride=0, variants=((1.0, 1.0),)) == 0


INF, NAN = math.inf, math.nan
REJECTED = {
    "null audio": dict(audio=None), "null out": dict(out=None), "null variants": dict(variants=None, n_variants=1),
    "null spec": dict(spec=None),
    "n < 0": dict(n=-1), "in_len < 0": dict(in_len=-1, in_stride=0), "stride < len": dict(in_stride=15999),
    "no variants": dict(variants=(), n_variants=0), "17 variants": dict(variants=((1.0, 1.0),) * 17),
    "speed 0": dict(variants=((0.0, 1.0),)), "speed < 0": dict(variants=((-1.0, 1.0),)),
    "speed nan": dict(variants=((NAN, 1.0),)), "speed inf": dict(variants=((INF, 1.0),)),
    "volume 0": dict(variants=((1.0, 0.0),)), "volume < 0": dict(variants=((1.0, -0.5),)),
    "volume nan": dict(variants=((1.0, NAN),)), "volume inf": dict(variants=((1.0, INF),)),
    "m = 0": dict(variants=((1e-5, 1.0),)), "m = 2^31": dict(variants=((2.0 ** 31 / 16000, 1.0),)),
    "pad < 0": dict(spec=(-0.005, 0.01, 5.0, 20.0, 0, 0)), "pad nan": dict(spec=(NAN, 0.01, 5.0, 20.0, 0, 0)),
    "pad inf": dict(spec=(INF, 0.01, 5.0, 20.0, 0, 0)),
    "snr < 0": dict(spec=(0.005, -0.01, 5.0, 20.0, 0, 0)), "snr nan": dict(spec=(0.005, NAN, 5.0, 20.0, 0, 0)),
    "snr inf": dict(spec=(0.005, INF, 5.0, 20.0, 0, 0)),
    "lo > hi": dict(spec=(0.005, 0.01, 20.0, 5.0, 0, 0)), "lo nan": dict(spec=(0.005, 0.01, NAN, 20.0, 0, 0)),
    "hi inf": dict(spec=(0.005, 0.01, 5.0, INF, 0, 0)), "lo -inf": dict(spec=(0.005, 0.01, -INF, 20.0, 0, 0)),
    "out_len 0": dict(out_len=0), "out_len < 0": dict(out_len=-4), "out_len > max": dict(out_len=16385),
    "dtype i8": dict(dtype=2), "dtype < 0": dict(dtype=-1),
    "n K = 2^32": dict(n=2 ** 31),
}


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_rejected_before_any_device_work(L, name):
    assert call(L, **REJECTED[name]) == 1, name
    assert call(L, n=0, **{k: v for k, v in REJECTED[name].items() if k != "n"}) == (0 if name.startswith("n ") else 1)
    assert b"wk_augment_batch" in L.wk_last_error() or name.startswith("n ")


def test_largest_accepted_resampled_length(L):
    """int(out_len * speed) = 2^31 - 128 (the largest float below 2^31 / 16000 times 16000) is in range."""
    assert call(L, n=0, variants=((134217.72, 1.0),)) == 0


def test_header_declares_the_surface_and_struct_sizes_match():
    from wakeword import _lib
    txt = open(HEADER).read()
    assert re.search(r"#define\s+WK_AUG_MAX_VARIANTS\s+16\b", txt)
    m = re.search(r"#define\s+WK_AUG_MAX_LEN\s+(\d+)", txt)
    assert m and int(m.group(1)) >= 16000 and int(m.group(1)) == _lib.WK_AUG_MAX_LEN
    assert re.search(r"typedef struct \{ float speed, volume; \} wk_aug_variant;", txt)
    body = re.search(r"typedef struct \{([^}]*)\} wk_aug_spec;", txt).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, [n.strip() for n in names.split(",")]) for t, names in re.findall(r"(\w+)\s+([\w, ]+);", body)]
    assert fields == [("float", ["pad_noise"]), ("float", ["snr_noise"]), ("float", ["snr_lo_db", "snr_hi_db"]),
                      ("uint64_t", ["seed"]), ("uint32_t", ["epoch"])]
    assert [n for n, _ in _lib.WkAugSpec._fields_] == [n for _, names in fields for n in names]
    # C layout: four floats (16), the 8-aligned seed (8), epoch (4), tail padding to 8 -> 32; the variant: 8
    assert C.sizeof(_lib.WkAugSpec) == 32 and _lib.WkAugSpec.seed.offset == 16 and _lib.WkAugSpec.epoch.offset == 24
    assert C.sizeof(_lib.WkAugVariant) == 8
    assert "wk_augment_batch" in _lib.EXPORTS and re.search(r"wk_status wk_augment_batch\(const void\* d_audio", txt)
    assert _lib.WK_AUG_MAX_VARIANTS == 16


def test_python_surface():
    import wakeword
    assert wakeword.REFERENCE_VARIANTS == ((1, 1), (0.8, 1), (1.2, 1), (1, 0.7), (1, 1.3))
    assert callable(wakeword.augment_batch) and callable(wakeword.extract_features)
    assert callable(wakeword.Trainer.step_augmented)
