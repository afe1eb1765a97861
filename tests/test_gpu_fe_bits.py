"""Bit identity of everything the MFCC front-end's device code feeds, against
tests/golden/fe_bits.npz.

The fixture was recorded on an MI355X from commit cb038a7 (the last one with
slot-major LDS twiddle tables, the split twiddle w0 in registers and the flat
window copy) with

    WAKEWORD_LIB=<libwakeword.so of that commit> python tools/record_fe_bits.py tests/golden/fe_bits.npz

tools/record_fe_bits.py defines the inputs and the calls; this test repeats
them on the current build and requires every array to be equal bit for bit.
Laying tables out differently, or reading them with other instructions, moves
no arithmetic, so any difference is a wrong table entry, a wrong lane or a
wrong edge path:

  - the fused kernel at B = 1, 3 and 5 (ragged CNN batches, both edge frames of
    every clip) in fp32 (packed front-end unit), bf16 and bf16x3 (scalar unit);
  - the standalone front-end in mode B (2 clips) and mode A (2 clips of 1 s and
    2 of 5,000 samples: a last chunk with fewer frames than frame slots);
  - wk_scan of a 5-window recording (frame store + per-window edge frames)."""
import importlib.util
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_fe_bits", os.path.join(REPO, "tools", "record_fe_bits.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)

KEYS = ([f"fused_{p}_B{n}_{w}" for p in REC.PRECISIONS for n in REC.FUSED_B for w in ("logits", "feats")]
        + ["scan_logits", "scan_feats", "mfcc_b", "mfcc_a_full", "mfcc_a_short"])


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "fe_bits.npz"))
    return {k: g[k] for k in g.files}


def test_fixture_is_complete(golden):
    """Not a GPU test: the fixture holds every array the recorder names, with the shapes of its calls."""
    assert sorted(golden) == sorted(KEYS)
    for p in REC.PRECISIONS:
        for n in REC.FUSED_B:
            assert golden[f"fused_{p}_B{n}_logits"].shape == (n,)
            assert golden[f"fused_{p}_B{n}_feats"].shape == (n, 13, 63)
    assert golden["scan_feats"].shape == (REC.SCAN_WINDOWS, 13, 63)
    assert golden["mfcc_a_short"].shape == (2, (REC.SHORT - 320) // 256 + 1, 13)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in golden.values())


@pytest.fixture(scope="module")
def current(gpu):
    return REC.record()


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_bit_identical(current, golden, key):
    got, want = current[key], golden[key]
    assert got.shape == want.shape and got.dtype == want.dtype
    diff = got.view(np.uint32) != want.view(np.uint32)
    print(f"{key}: {int(diff.sum())} of {diff.size} values differ")
    assert not diff.any(), (key, int(diff.sum()), np.argwhere(diff)[:4].tolist())
