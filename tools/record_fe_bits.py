"""Recorder of tests/golden/fe_bits.npz, the bit-identity fixture of
tests/test_gpu_fe_bits.py, and the one definition of what both compute.

    WAKEWORD_LIB=<library of the commit to record> python tools/record_fe_bits.py out.npz

The fixture holds, from seeded synthetic clips, every output the MFCC
front-end's device code (csrc/wk_fe_dev.h) feeds:

  fused_{prec}_B{n}_logits / _feats   the fused kernel (wk_forward) on the first
                                      n = 1, 3, 5 clips, prec = fp32 (packed
                                      unit), bf16 and bf16x3 (scalar unit)
  mfcc_b                              the standalone front-end, mode B, 2 clips
  mfcc_a_full / mfcc_a_short          the same in mode A: 2 clips of 1 s, and
                                      2 clips of 5,000 samples (a last chunk
                                      with fewer frames than slots)
  scan_logits / scan_feats            wk_scan of one recording of 5 windows at
                                      hop 256 (shared interior frames + the
                                      per-window edge frames)

It was recorded at the commit before the LDS tables of the front-end became
lane-major; a change that moves no arithmetic must reproduce it exactly.
Re-record it only from a build whose front-end arithmetic is known good."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "esp32-wake-word_amd")]

SEED = 97
FUSED_B = (1, 3, 5)
PRECISIONS = ("fp32", "bf16", "bf16x3")
SHORT = 5000
SCAN_WINDOWS, SCAN_HOP = 5, 256


def clips() -> np.ndarray:
    from oracle import wk_oracle as O
    return O.synth_clips(SEED, 0, max(FUSED_B)).astype(np.float32)


def recording() -> np.ndarray:
    from oracle import wk_oracle as O
    x = O.synth_clips(SEED + 1, 0, 2).astype(np.float32).reshape(-1)
    return np.ascontiguousarray(x[:16000 + SCAN_HOP * (SCAN_WINDOWS - 1)])


def record() -> dict:
    import wakeword
    onnx = os.path.join(REPO, "tests", "golden", "xiaoa.onnx")
    x = clips()
    out = {}
    for prec in PRECISIONS:
        model = wakeword.load_onnx(onnx, precision=prec)
        for n in FUSED_B:
            logits, feats = model.detect(x[:n], return_features=True)
            out[f"fused_{prec}_B{n}_logits"] = logits.cpu().numpy()
            out[f"fused_{prec}_B{n}_feats"] = feats.cpu().numpy()
        model.check_device_errors()
        if prec == "fp32":
            logits, feats = model.scan(recording(), hop=SCAN_HOP, return_features=True)
            out["scan_logits"] = logits.cpu().numpy()
            out["scan_feats"] = feats.cpu().numpy()
    out["mfcc_b"] = wakeword.mfcc(x[:2], mode="torchaudio").cpu().numpy()
    out["mfcc_a_full"] = wakeword.mfcc(x[:2], mode="esp").cpu().numpy()
    out["mfcc_a_short"] = wakeword.mfcc(np.ascontiguousarray(x[1:3, 300:300 + SHORT]), mode="esp").cpu().numpy()
    return out


if __name__ == "__main__":
    res = record()
    for k, v in res.items():
        assert np.isfinite(v).all(), k
    np.savez(sys.argv[1], **res)
    print("wrote", sys.argv[1], {k: v.shape for k, v in res.items()})
