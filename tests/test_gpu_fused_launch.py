"""Every instantiation the fused kernel's launcher can pick (launch_fused_as,
csrc/wk_fused_dev.h): audio type float32 / int16 x precision fp32 / bf16 /
bf16x3 x with / without the feature output, each pinned to bits.

tests/test_gpu_fe_bits.py pins the float32, with-features kernels to
tests/golden/fe_bits.npz.  Here, on the same clips (tools/record_fe_bits.py)
at B = 1 and B = 5 (a ragged second CNN batch):

  (a) the kernel without the feature stores gives the fixture's logits, bit
      for bit (the feature output moves no arithmetic of the logit);
  (b) int16 audio xi = round(32767 x) gives the bits of the float32 audio
      xf = xi / 32768 (exact in float32: the int16 kernel scales by 2^-15),
      logits without features, logits and features with them.

The launcher chooses a kernel and computes nothing, so any difference is a
wrong instantiation or wrong launch arguments."""
import importlib.util
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_fe_bits", os.path.join(REPO, "tools", "record_fe_bits.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)

BATCHES = (1, 5)


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "fe_bits.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module", params=REC.PRECISIONS)
def runs(request, gpu):
    """(precision, {(B, audio type, with features): (logits, features or None)}) of one model."""
    import wakeword
    x = REC.clips()
    xi = np.round(32767.0 * x).astype(np.int16)
    xf = xi.astype(np.float32) / np.float32(32768.0)
    assert np.array_equal(xf.astype(np.float64) * 32768.0, xi.astype(np.float64))   # xf is exact
    model = wakeword.load_onnx(os.path.join(REPO, "tests", "golden", "xiaoa.onnx"), precision=request.param)
    out = {}
    for n in BATCHES:
        out[n, "x", False] = (model.detect(x[:n]).cpu().numpy(), None)
        for name, a in (("i16", xi), ("f32", xf)):
            out[n, name, False] = (model.detect(a[:n]).cpu().numpy(), None)
            logits, feats = model.detect(a[:n], return_features=True)
            out[n, name, True] = (logits.cpu().numpy(), feats.cpu().numpy())
    model.check_device_errors()
    return request.param, out


def _differing(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    diff = got.view(np.uint32) != want.view(np.uint32)
    return int(diff.sum()), np.argwhere(diff)[:4].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("n", BATCHES)
def test_logits_without_features_match_fixture(runs, golden, n):
    prec, out = runs
    bad, where = _differing(out[n, "x", False][0], golden[f"fused_{prec}_B{n}_logits"])
    print(f"{prec} B={n}: {bad} of {n} logits differ from the fixture")
    assert bad == 0, (prec, n, where)


@pytest.mark.gpu
@pytest.mark.parametrize("n", BATCHES)
def test_int16_audio_equals_scaled_float(runs, n):
    prec, out = runs
    for feats in (False, True):
        (li, fi), (lf, ff) = out[n, "i16", feats], out[n, "f32", feats]
        bad, where = _differing(li, lf)
        print(f"{prec} B={n} features={feats}: {bad} of {n} logits differ between int16 and float32 audio")
        assert bad == 0, (prec, n, feats, where)
        if feats:
            assert fi.shape == (n, 13, 63)
            bad, where = _differing(fi, ff)
            print(f"{prec} B={n}: {bad} of {fi.size} features differ between int16 and float32 audio")
            assert bad == 0, (prec, n, where)
