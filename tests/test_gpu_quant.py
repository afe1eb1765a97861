"""Post-training int8 calibration on the device (wk_calibrate), run-time
exponents in the int8 network (wk_set_quant), and the Python surface that
closes train -> quantise -> int8 evaluate (ml_models/main.py:71-129).

References: tests/quant_ref.py -- the numpy int8 network at any spec (equal to
oracle.kws_forward_int8 at the default one, tests/test_quant_ref.py) and the
float64 calibration."""
import os
import subprocess
import sys

import numpy as np
import pytest

import quant_gpu_checks as Q
import quant_ref as R
from oracle import wk_oracle as O

pytestmark = pytest.mark.gpu

PER_CLIP = np.array(R.PER_CLIP, np.int64)


@pytest.fixture(scope="module")
def g24():
    return Q.golden_feats()


@pytest.fixture(scope="module")
def f600(g24):
    """The golden features tiled to 600 clips with seeded N(0, 0.05^2) perturbation: more clips than workgroups."""
    rng = np.random.default_rng(7)
    return (np.tile(g24, (25, 1, 1)) + rng.normal(0.0, 0.05, (600, 13, 63))).astype(np.float32)


@pytest.fixture(scope="module")
def ref24(g24, xiaoa_sd):
    return R.calib_reference(g24, xiaoa_sd)


@pytest.fixture(scope="module")
def fp32_model(gpu, xiaoa_sd):
    import wakeword
    return wakeword.KWSModel(xiaoa_sd)


@pytest.fixture(scope="module")
def cal24(fp32_model, g24):
    import wakeword
    return wakeword.calibrate(fp32_model, g24)


@pytest.mark.parametrize("B", [1, 3, 17, 600])
def test_calibration_counts_every_value_once(fp32_model, f600, xiaoa_sd, B):
    """Per tensor the counts add up to B x (819, 2016, 1984, 1920, 128, 64, 1) exactly: the padded columns of the
    64 / 32 / 16-wide tiles and the guard rows are not counted, and no clip is skipped or counted twice when the
    workgroups walk more clips than there are of them.  Two calls agree; the maxima are the float64 reference's."""
    import wakeword
    feats = f600[:B]
    spec, st = wakeword.calibrate(fp32_model, feats, return_stats=True)
    totals = st["counts"].sum(axis=1)
    print("totals", totals.tolist())
    np.testing.assert_array_equal(totals, B * PER_CLIP)
    assert st["n_clips"] == B and (st["counts"] >= 0).all()
    spec2, st2 = wakeword.calibrate(fp32_model, feats, return_stats=True)
    np.testing.assert_array_equal(st2["counts"], st["counts"])
    np.testing.assert_array_equal(st2["max_abs"], st["max_abs"])
    assert spec2 == spec
    want = np.array([np.abs(t).max() for t in R.observed_tensors(feats, xiaoa_sd)])
    rel = np.abs(st["max_abs"].astype(np.float64) - want) / want
    print("max rel", rel.tolist())
    assert (rel <= 1e-5).all(), rel


def test_calibration_counts_against_float64(fp32_model, g24, ref24, xiaoa_sd):
    """Every cumulative bin count is the float64 reference's up to the reference values within 1e-4 relative of
    that bin's threshold, and the exponents picked at the 99.9th percentile and at the maximum are the reference's
    (whose k-th values are first checked to lie at least 1 % from a threshold)."""
    import wakeword
    for pct in (99.9, 100.0):
        margins = R.kth_margin(ref24, pct)
        print(pct, "margins", margins)
        assert min(margins) >= 0.01, (pct, margins)
    _, st = wakeword.calibrate(fp32_model, g24, return_stats=True)
    cum, cum_ref = np.cumsum(st["counts"], axis=1), np.cumsum(ref24["counts"], axis=1)
    print("|cum - ref| max per tensor", np.abs(cum - cum_ref).max(axis=1).tolist(), "allowed", ref24["near"].max(axis=1).tolist())
    assert (np.abs(cum - cum_ref) <= ref24["near"]).all()
    for pct in (99.9, 100.0):
        for pin in (-4, None):
            got = wakeword.calibrate(fp32_model, g24, percentile=pct, pin_input_exp=pin)
            assert got.to_dict() == R.spec_from_counts(ref24["counts"], xiaoa_sd, pct, pin), (pct, pin)
    # any precision's handle calibrates alike (the fp32 weights are used), and a state dict does as a model
    m8 = wakeword.KWSModel(xiaoa_sd, precision="int8")
    assert wakeword.calibrate(m8, g24) == wakeword.calibrate(xiaoa_sd, g24) == wakeword.calibrate(fp32_model, g24)


def test_calibration_and_trainer_share_one_forward(gpu, g24, xiaoa_sd):
    """Calibration and the trainer run the same direct-form forward (csrc/wk_direct_dev.h), so the logit maximum
    calibration observes has the bits of the trainer's |logit|: clip by clip (B = 1, one workgroup, one clip) and over
    the 24 clips at once (a multi-clip walk), for xiaoa's weights and for a default initialisation."""
    import wakeword
    from wakeword.train import default_init
    labels = (np.arange(24) % 2).astype(np.float32)
    for name, sd in (("xiaoa", xiaoa_sd), ("default_init(0)", default_init(0))):
        logit = np.abs(wakeword.Trainer(sd).grad(g24, labels)[1].cpu().numpy())
        assert logit.dtype == np.float32 and logit.shape == (24,)
        for i in (0, 11, 23):
            _, st = wakeword.calibrate(sd, g24[i:i + 1], return_stats=True)
            print(name, "clip", i, "trainer |logit|", logit[i].view(np.uint32), "calibration", st["max_abs"][6].view(np.uint32))
            assert st["max_abs"][6].view(np.uint32) == logit[i].view(np.uint32), (name, i)
        _, st = wakeword.calibrate(sd, g24, return_stats=True)
        print(name, "24 clips: trainer max |logit|", logit.max().view(np.uint32), "calibration", st["max_abs"][6].view(np.uint32))
        assert st["max_abs"][6].view(np.uint32) == logit.max().view(np.uint32), name


def test_run_time_exponents_bit_exact_mfma(gpu, xiaoa_sd, cal24):
    Q.check_entry_points(xiaoa_sd, cal24)


def test_run_time_exponents_bit_exact_valu_kernel(gpu):
    """The same comparisons with the one-block-per-clip VALU kernel, which a process selects for its lifetime."""
    env = dict(os.environ, WAKEWORD_INT8_VALU="1")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "quant_gpu_checks.py")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "quant_gpu_checks: ok VALU" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_set_quant_refuses_other_precisions_and_bad_specs(fp32_model, xiaoa_sd):
    import wakeword
    with pytest.raises(ValueError):
        wakeword.KWSModel(xiaoa_sd, precision="bf16", quant=wakeword.QuantSpec.default())
    assert fp32_model.quant is None
    with pytest.raises(wakeword.WakewordError, match="shift"):
        wakeword.KWSModel(xiaoa_sd, precision="int8", quant=wakeword.QuantSpec(-4, (-8, -9, -9, -9, -9), (-13, -5, -4, -5, -4, -3)))
    m = wakeword.KWSModel(xiaoa_sd, precision="int8")
    assert m.quant == wakeword.QuantSpec.default()


def test_power_of_2_rescaling_is_absorbed_by_calibration(fp32_model, xiaoa_sd, g24, cal24):
    """conv1's weights x 4 and conv2's x 1/4 leave the float network unchanged bit for bit (ReLU and the pool
    commute with a positive power of 2).  Calibration follows: the same spec with e_w[0] and e_act[conv1] two
    higher and e_w[1] two lower, and the same int8 logits.  At the default spec the rescaled network saturates."""
    import wakeword
    sd2 = {k: v.copy() for k, v in xiaoa_sd.items()}
    sd2["conv_layers.0.weight"] *= np.float32(4.0)
    sd2["conv_layers.3.weight"] *= np.float32(0.25)
    a = fp32_model(g24).reshape(-1).cpu().numpy()
    b = wakeword.KWSModel(sd2)(g24).reshape(-1).cpu().numpy()
    np.testing.assert_array_equal(a, b)
    cal2 = wakeword.calibrate(sd2, g24)
    e_w, e_act = list(cal24.e_w), list(cal24.e_act)
    e_w[0] += 2
    e_w[1] -= 2
    e_act[0] += 2
    assert cal2 == wakeword.QuantSpec(cal24.e_in, tuple(e_w), tuple(e_act))
    q1 = wakeword.KWSModel(xiaoa_sd, precision="int8", quant=cal24)(g24).reshape(-1).cpu().numpy()
    q2 = wakeword.KWSModel(sd2, precision="int8", quant=cal2)(g24).reshape(-1).cpu().numpy()
    np.testing.assert_array_equal(q1, q2)
    np.testing.assert_array_equal(q1, R.forward_int8(g24, xiaoa_sd, cal24))
    d1 = wakeword.KWSModel(xiaoa_sd, precision="int8")(g24).reshape(-1).cpu().numpy()
    d2 = wakeword.KWSModel(sd2, precision="int8")(g24).reshape(-1).cpu().numpy()
    assert not np.array_equal(d1, d2)


def test_train_then_quantise(gpu, xiaoa_sd, g24):
    """Trainer -> to_model('int8', calib=feats): the int8 network at the calibrated spec, bit for bit the numpy
    reference, and as close to the float network as xiaoa's int8 network is at xiaoa.info's exponents: at most
    2 x max |int8 - fp32| of xiaoa over the golden features (0.4055; the factor allows for another weight set,
    not for kernel error, which is zero)."""
    import wakeword
    from wakeword.train import default_init
    xiaoa_err = float(np.abs(R.forward_int8(g24, xiaoa_sd, R.DEFAULT) - O.kws_forward(g24, xiaoa_sd)[:, 0]).max())
    feats = wakeword.mfcc(O.synth_clips(5, 0, 64)).cpu().numpy()
    labels = (np.arange(64) % 2).astype(np.float32)          # odd synthetic clips carry the 440 Hz tone
    tr = wakeword.Trainer(default_init(0))
    for _ in range(20):
        tr.step(feats, labels)
    sd = tr.state_dict()
    m8 = tr.to_model("int8", calib=feats)
    spec = m8.quant
    assert spec == wakeword.calibrate(sd, feats) and spec.e_in == -4
    got = m8(feats).reshape(-1).cpu().numpy()
    np.testing.assert_array_equal(got, R.forward_int8(feats, sd, spec))
    err = float(np.abs(got - O.kws_forward(feats, sd)[:, 0]).max())
    print(f"trained: max|int8 - fp32| = {err:.4f}; xiaoa at the default spec = {xiaoa_err:.4f}; spec {spec}")
    assert err <= 2.0 * xiaoa_err
    np.testing.assert_array_equal(wakeword.int8_weights(sd, spec)["conv_layers.6.weight"],
                                  R.quantize_weights(sd, spec)["conv_layers.6.weight"])


def test_quantize_model_and_accuracy(fp32_model, xiaoa_sd, g24):
    import wakeword
    labels = (O.kws_forward(g24, xiaoa_sd)[:, 0] > 0).astype(np.float32)
    labels[::5] = 1.0 - labels[::5]                          # some wrong on purpose: accuracy below 100
    loader = [(g24[i:i + 6], labels[i:i + 6]) for i in range(0, 24, 6)]
    m8, spec = wakeword.quantize_model(fp32_model, loader, calib_steps=2)
    assert spec == wakeword.calibrate(fp32_model, g24[:12]) and m8.quant == spec and m8.precision == "int8"
    m8_all, spec_all = wakeword.quantize_model(fp32_model, (f for f, _ in loader))   # batches without labels
    assert spec_all == wakeword.calibrate(fp32_model, g24)
    for model in (fp32_model, m8):
        logits = model(g24).reshape(-1).cpu().numpy()
        want = 100.0 * float(((logits > 0) == (labels > 0.5)).mean())
        assert wakeword.accuracy(model, loader) == pytest.approx(want, abs=1e-9)
    assert 0.0 < wakeword.accuracy(fp32_model, loader) < 100.0


def test_device_detector_refuses_another_input_exponent(gpu, xiaoa_sd):
    import wakeword
    ok = wakeword.KWSModel(xiaoa_sd, precision="int8")
    wakeword.DeviceDetector(ok)
    other = wakeword.KWSModel(xiaoa_sd, precision="int8",
                              quant=wakeword.QuantSpec(-5, (-8, -9, -9, -9, -9), (-5, -5, -4, -5, -4, -3)))
    with pytest.raises(ValueError, match="input exponent"):
        wakeword.DeviceDetector(other)
