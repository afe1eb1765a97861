"""The run-time-exponent check of tests/test_gpu_quant.py, importable and runnable.

``check_entry_points`` runs in the test process (the int8 matrix-core kernel)
and, through ``python quant_gpu_checks.py`` with WAKEWORD_INT8_VALU set, in a
child process (the one-block-per-clip VALU kernel: the library reads the
variable once per process).  Exit status 0 = every comparison held.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (HERE, REPO, os.path.join(REPO, "esp32-wake-word_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import quant_ref as R  # noqa: E402
from oracle import wk_oracle as O  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")

# Hand-made specs: a shift of 0 (classifier.2: -3 = 0 + -3, saturate only), GAP with d = -1 (ties to even on the
# even divisor 14) and with d = 3 (conv3's output at a coarse exponent); the other shifts stay in [0, 24].
HAND_MADE = {
    "s0": {"e_in": -4, "e_w": [-8, -9, -9, -9, -3], "e_act": [-5, -5, -4, -5, 0, -3]},
    "d-1": {"e_in": -4, "e_w": [-8, -9, -9, -9, -9], "e_act": [-5, -5, -4, -3, -4, -3]},
    "d3": {"e_in": -4, "e_w": [-8, -9, -9, -9, -9], "e_act": [-5, -5, -2, -5, -4, -3]},
}
assert R.shifts(HAND_MADE["s0"])[4] == 0
assert HAND_MADE["d-1"]["e_act"][2] - HAND_MADE["d-1"]["e_act"][3] == -1
assert HAND_MADE["d3"]["e_act"][2] - HAND_MADE["d3"]["e_act"][3] == 3


def xiaoa_sd():
    from wakeword.onnx_reader import read_onnx, xiaoa_state_dict
    return xiaoa_state_dict(read_onnx(os.path.join(GOLDEN, "xiaoa.onnx"))[0])


def golden_feats():
    w = np.load(os.path.join(GOLDEN, "wavs.npz"))
    s = np.load(os.path.join(GOLDEN, "synth.npz"))
    return np.concatenate([w["feat_zero"], s["feats"]]).astype(np.float32)


def check_entry_points(sd, calibrated, batches=(1, 9, 300)):
    """wk_cnn, wk_forward and wk_scan of an int8 model at the default spec, `calibrated` and the hand-made specs
    against the numpy int8 network, bit for bit, on the features the device itself computed."""
    import wakeword
    x = O.synth_clips(99, 0, max(batches), 16000)
    rec = np.concatenate([x[0], x[1][:8 * 256]])          # 9 windows at hop 256: the shared-frame scan path
    specs = {"default": R.DEFAULT, "calibrated": R.as_dict(calibrated), **HAND_MADE}
    for name, spec in specs.items():
        m = wakeword.KWSModel(sd, precision="int8", quant=wakeword.QuantSpec.from_dict(spec))
        assert m.quant.to_dict() == spec, name
        for B in batches:
            fwd, feats = m.detect(x[:B], return_features=True)                  # wk_forward
            feats = feats.cpu().numpy()
            want = R.forward_int8(feats, sd, spec)
            np.testing.assert_array_equal(fwd.cpu().numpy(), want, err_msg=f"wk_forward {name} B={B}")
            np.testing.assert_array_equal(m(feats).reshape(-1).cpu().numpy(), want, err_msg=f"wk_cnn {name} B={B}")
        sc, sf = m.scan(rec, hop=256, return_features=True)                     # wk_scan
        assert sc.shape == (9,)
        np.testing.assert_array_equal(sc.cpu().numpy(), R.forward_int8(sf.cpu().numpy(), sd, spec),
                                      err_msg=f"wk_scan {name}")
        assert len(np.unique(want)) > 8, (name, "the check needs logits that vary")
    default = wakeword.KWSModel(sd, precision="int8")                            # a handle that never sets a spec
    np.testing.assert_array_equal(default(feats).reshape(-1).cpu().numpy(), R.forward_int8(feats, sd, R.DEFAULT))


if __name__ == "__main__":
    import wakeword
    sd_ = xiaoa_sd()
    check_entry_points(sd_, wakeword.calibrate(sd_, golden_feats()))
    print("quant_gpu_checks: ok", "VALU" if os.environ.get("WAKEWORD_INT8_VALU") else "MFMA")
