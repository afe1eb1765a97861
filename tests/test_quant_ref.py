"""CPU tests of the post-training quantisation pieces that need no GPU: the
generalised int8 reference against the pinned oracle, the weight-exponent rule
against xiaoa.info, the bit-pattern bin rule against exact arithmetic, and the
argument checks of the C entry points."""
import ctypes as C
import os

import numpy as np
import pytest

import quant_ref as R
from oracle import wk_oracle as O


@pytest.fixture(scope="module")
def golden_feats(golden_dir):
    w = np.load(os.path.join(golden_dir, "wavs.npz"))
    s = np.load(os.path.join(golden_dir, "synth.npz"))
    return np.concatenate([w["feat_zero"], s["feats"]]).astype(np.float32)   # 8 + 16 = 24 feature sets


@pytest.fixture(scope="module")
def L():
    from wakeword import _lib
    return _lib.lib()


def test_generalised_reference_equals_the_oracle_at_the_default_spec(golden_feats, golden_dir, xiaoa_sd):
    assert golden_feats.shape == (24, 13, 63)
    qw = R.quantize_weights(xiaoa_sd, R.DEFAULT)
    for k, v in O.quantize_int8(xiaoa_sd).items():
        np.testing.assert_array_equal(qw[k], v)
    q_in = R.quantize_input(golden_feats, R.DEFAULT)
    np.testing.assert_array_equal(q_in, O.quantize_input(golden_feats))
    np.testing.assert_array_equal(R.forward_int8_q(q_in, qw, R.DEFAULT), O.kws_forward_int8(q_in, qw))
    k = np.load(os.path.join(golden_dir, "kat.npz"))
    kat_in = k["kat_in_int8"].transpose(0, 2, 1).astype(np.int64)
    assert R.forward_int8_q(kat_in, qw, R.DEFAULT)[0] == -40 == int(k["kat_out_int8"][0, 0])
    assert R.shifts(R.DEFAULT) == [7, 9, 10, 10, 10]


def test_weight_rule_gives_xiaoa_info_exponents(xiaoa_sd, golden_dir):
    assert R.weight_exponents(xiaoa_sd) == [-8, -9, -9, -9, -9]
    k = np.load(os.path.join(golden_dir, "kat.npz"))
    pinned = [int(k["qexp_" + n]) for n in ("conv_layers_0_weight", "conv_layers_3_weight", "conv_layers_6_weight",
                                            "onnx__MatMul_23", "onnx__MatMul_24")]
    assert R.weight_exponents(xiaoa_sd) == pinned


def test_wk_quant_weights_reproduces_the_kat_weights(L, xiaoa_sd, golden_dir):
    import wakeword
    from wakeword import quant
    spec = wakeword.QuantSpec.default()
    assert spec.to_dict() == R.DEFAULT and wakeword.QuantSpec.from_dict(R.DEFAULT) == spec
    k = np.load(os.path.join(golden_dir, "kat.npz"))
    # kat.npz keeps xiaoa.info's values in esp-dl's (N/16)WC16 order (tests/test_oracle.py); the library's export
    # is the logical conv [k][ci][co], matmul [in][out]
    want = []
    for n, (co, ci) in (("conv_layers_0_weight", (32, 13)), ("conv_layers_3_weight", (64, 32)),
                        ("conv_layers_6_weight", (128, 64))):
        want.append(k["q_" + n].reshape(co // 16, 3, ci, 16).transpose(1, 2, 0, 3).reshape(-1))
    want.append(k["q_onnx__MatMul_23"].reshape(64 // 16, 128, 16).transpose(1, 0, 2).reshape(-1))
    want.append(k["q_onnx__MatMul_24"].reshape(-1))
    want = np.concatenate(want)
    np.testing.assert_array_equal(quant.int8_blob(xiaoa_sd, spec), want)
    shaped = wakeword.int8_weights(xiaoa_sd, spec)
    for key, v in R.quantize_weights(xiaoa_sd, R.DEFAULT).items():
        assert shaped[key].dtype == np.int8 and shaped[key].shape == v.shape
        np.testing.assert_array_equal(shaped[key], v)
    # another set of exponents, saturation included (max |w| 0.496 * 2^10 > 127)
    other = wakeword.QuantSpec(-4, (-10, -7, -9, -6, -9), spec.e_act)
    shaped = wakeword.int8_weights(xiaoa_sd, other)
    for key, v in R.quantize_weights(xiaoa_sd, other).items():
        np.testing.assert_array_equal(shaped[key], v)
    assert np.abs(shaped["conv_layers.0.weight"].astype(int)).max() >= 127


def test_bit_pattern_bin_rule_is_exact_at_every_threshold():
    """b(a) = min{e : a <= 127 * 2^e} from the float's bits equals ceil(log2(a / 127))
    in exact rational arithmetic on both sides of every threshold."""
    for e in range(-30, 12):
        thr = np.float32(127.0 * 2.0 ** e)
        below, above = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(np.inf))
        for a, want in ((thr, e), (below, e), (above, e + 1)):
            assert R.hold_exp_exact(a) == want, (e, a)
            assert R.hold_exp_bits(a) == want, (e, a)
            assert int(R.hold_exp(a)) == min(max(want, R.E_MIN), R.E_MAX)
    rng = np.random.default_rng(3)
    for a in np.exp(rng.uniform(-20, 6, 300)).astype(np.float32):
        assert R.hold_exp_bits(a) == R.hold_exp_exact(a)
    assert int(R.hold_exp(0.0)) == R.E_MIN


def test_gap_rounding_of_the_reference():
    # d >= 0 never ties; d < 0 ties go to even: 7 / 14 = 0.5 -> 0, 21 / 14 = 1.5 -> 2
    np.testing.assert_array_equal(R._rne_div(np.array([7, 21, 8, 6, 35]), 14), [0, 2, 1, 0, 2])
    s = np.arange(0, 890)
    np.testing.assert_array_equal(R._rne_div(s << 1, 7), np.round(s * 2.0 / 7.0).astype(np.int64))


def _spec(e_in=-4, e_w=(-8, -9, -9, -9, -9), e_act=(-5, -5, -4, -5, -4, -3)):
    from wakeword import _lib
    return _lib.WkQuantSpec(e_in, (C.c_int32 * 5)(*e_w), (C.c_int32 * 6)(*e_act))


def test_set_quant_rejects_bad_arguments_without_gpu(L):
    """The spec is checked before the handle is touched, so the checks run without a device."""
    def err(spec):
        assert L.wk_set_quant(None, C.byref(spec) if spec is not None else None) == 1
        return L.wk_last_error().decode()

    assert "null handle" in err(_spec())                                    # a valid spec reaches the handle check
    assert "null spec" in err(None)
    assert "shift" in err(_spec(e_act=(-13, -5, -4, -5, -4, -3)))           # conv1: s = -13 + 4 + 8 = -1
    assert "shift" in err(_spec(e_w=(-8, -9, -9, -9, -30)))                 # classifier.2: s = -3 + 4 + 30 = 31
    assert "shift" in err(_spec(e_act=(-5, -5, -4, -5, -4, 13)))            # s = 13 + 4 + 9 = 26 > 24
    assert "null handle" in err(_spec(e_act=(-5, -5, -4, -5, -4, 11)))      # s = 24 is allowed
    assert "null handle" in err(_spec(e_act=(-12, -5, -4, -5, -4, -3), e_w=(-8, -2, -9, -9, -9)))   # s = 0 is allowed
    assert "gap" in err(_spec(e_act=(-5, -5, 0, -5, -4, -3), e_w=(-8, -9, -5, -9, -9)))    # d = 5
    assert "gap" in err(_spec(e_act=(-5, -5, -10, -5, -4, -3), e_w=(-8, -9, -15, -9, -9)))  # d = -5
    assert "exponent" in err(_spec(e_in=40))
    out = _spec()
    assert L.wk_get_quant(None, C.byref(out)) == 1
    assert L.wk_quant_spec_default(None) == 1
    assert L.wk_quant_weights(None, C.byref(out), None) == 1
    n = C.c_size_t(7)
    assert L.wk_calibrate_workspace_bytes(0, C.byref(n)) == 1 and n.value == 0
    assert L.wk_calibrate_workspace_bytes(640, C.byref(n)) == 0 and n.value > 0
    assert L.wk_calibrate(None, None, 1, 99.9, -4, None, 0, C.byref(out), None, None) == 1


def test_quant_spec_summary_follows_xiaoa_info_order():
    import wakeword
    lines = wakeword.QuantSpec.default().summary().splitlines()
    assert [ln.split()[0] for ln in lines] == [
        "input", "conv_layers.0.weight", "conv_layers.0", "conv_layers.3.weight", "conv_layers.3",
        "conv_layers.6.weight", "conv_layers.6", "global_avg_pool", "classifier.0.weight", "classifier.0",
        "classifier.2.weight", "classifier.2"]
    assert [int(ln.split()[-1]) for ln in lines] == [-4, -8, -5, -9, -5, -9, -4, -5, -9, -4, -9, -3]
