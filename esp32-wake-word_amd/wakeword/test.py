"""Config 1 (BASELINE.json configs[0]): score WAV files end to end.

    python -m wakeword.test file.wav [file2.wav ...] [--onnx xiaoa.onnx]
        [--pad noise|zero] [--seed S] [--threshold 0.5] [--precision fp32|bf16|bf16x3|int8] [--json]
        [--cpu]
    python -m wakeword.test --scan HOP file.wav [...] [--threshold 0.8] [--refractory 5.0] [--json]

The reference's single-file path is WAV -> ``pad_audio`` -> torchaudio MFCC +
CMVN -> ``LightweightKWS`` -> sigmoid > 0.5 (ml_models/src/extract_mfcc.py:7-23,
123-182; ml_models/src/wakeModel.py:29-34; ml_models/main.py:52-53).  Here the
WAV header walk and the pad run on the host (wakeword.wav, the esp_wav.cpp
restatement in libwakeword.so) and everything from pre-emphasis to the logit
runs in the fused HIP kernel on cuda:0.

``--cpu`` runs the same path on the host instead (libwakeword_host.so,
wakeword.host: the C++ host implementation of the WAV loader, mode B and the
CNN, fp32) -- the reference's own config-1 setting, "on CPU, no GPU".  It is
a separate library chosen by this flag, not a fallback: without ``--cpu`` a
missing GPU is an error.

``--scan HOP`` reads each file whole (not its first second) and scores every
window [w*HOP, w*HOP + 16000) of it on the GPU (wk_scan; HOP in samples, a
multiple of 256 shares the MFCC frames between windows), then applies the
firmware's decision rule (probability >= --threshold, default 0.8 in this
mode, then deaf for --refractory seconds) and prints one line per event.

``--pad noise`` (the reference default, add_noise_to_pad=True) draws the pad
from N(0, 0.005^2) with the loader's seeded generator, so a run is
repeatable; ``--pad zero`` pads with zeros.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from typing import List, Optional, Sequence

import numpy as np

_REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEFAULT_ONNX = os.path.join(_REPO, "tests", "golden", "xiaoa.onnx")


def default_onnx() -> str:
    """$WAKEWORD_ONNX, else the xiaoa.onnx kept with the test fixtures."""
    return os.environ.get("WAKEWORD_ONNX", DEFAULT_ONNX)


def prepare(paths: Sequence[str], pad: str = "noise", seed: int = 0, cpu: bool = False) -> np.ndarray:
    """WAV files -> (B, 16000) float32 windows: x/32768, trimmed or right-padded
    as pad_audio does (native loader: wakeword.wav.load_batch, or the host
    library's copy of it with cpu=True)."""
    if cpu:
        from .host import load_batch
    else:
        from .wav import load_batch
    if not paths:
        return np.zeros((0, 16000), np.float32)
    x, _ = load_batch(list(paths), 16000, 0.005 if pad == "noise" else 0.0, seed)
    return x


def score(paths: Sequence[str], onnx: Optional[str] = None, pad: str = "noise", seed: int = 0,
          threshold: float = 0.5, precision: str = "fp32", device: int = 0, cpu: bool = False) -> List[dict]:
    """One result dict per file: logit, probability = sigmoid(logit), decision."""
    x = prepare(paths, pad, seed, cpu)
    if cpu:
        if precision != "fp32":
            raise ValueError("--cpu runs the fp32 path only")
        from . import host
        model = host.load_onnx(onnx or default_onnx())
        logits = model.detect(x) if len(paths) else np.zeros((0,), np.float32)
    else:
        from .api import load_onnx
        model = load_onnx(onnx or default_onnx(), device=device, precision=precision)
        logits = model.detect(x).cpu().numpy() if len(paths) else np.zeros((0,), np.float32)
    out = []
    for p, z in zip(paths, logits):
        prob = 1.0 / (1.0 + math.exp(-float(z)))
        out.append({"file": p, "logit": float(z), "probability": prob, "wake": bool(prob > threshold)})
    return out


def scan_files(paths: Sequence[str], hop: int, onnx: Optional[str] = None, threshold: float = 0.8,
               refractory_s: float = 5.0, precision: str = "fp32", device: int = 0) -> List[dict]:
    """--scan: one result dict per event (a window that fired) of each file."""
    from .api import load_onnx, load_wav
    from .scan import scan_events
    model = load_onnx(onnx or default_onnx(), device=device, precision=precision)
    out = []
    for p in paths:
        for w in scan_events(model, load_wav(p), hop, threshold, refractory_s):
            if w.detected:
                out.append({"file": p, "start_s": (w.end - 16000) / 16000.0, "end_s": w.end / 16000.0,
                            "logit": w.logit, "probability": w.prob})
    return out


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m wakeword.test", description=__doc__.split("\n\n")[0])
    ap.add_argument("wav", nargs="+")
    ap.add_argument("--onnx", default=None, help="xiaoa.onnx (default: $WAKEWORD_ONNX or tests/golden/xiaoa.onnx)")
    ap.add_argument("--pad", choices=("noise", "zero"), default="noise")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threshold", type=float, default=None, help="default 0.5 (0.8 with --scan)")
    ap.add_argument("--precision", choices=("fp32", "bf16", "bf16x3", "int8"), default="fp32")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", action="store_true", help="one JSON object per file")
    ap.add_argument("--cpu", action="store_true",
                    help="run on the host CPU (libwakeword_host.so) instead of the GPU: config 1's setting")
    ap.add_argument("--scan", type=int, default=None, metavar="HOP",
                    help="score every window of the whole file at this hop (samples) and print the events")
    ap.add_argument("--refractory", type=float, default=5.0, help="--scan: seconds the detector is deaf after an event")
    a = ap.parse_args(argv)
    if a.scan is not None:
        if a.cpu:
            ap.error("--scan runs on the GPU only")
        thr = 0.8 if a.threshold is None else a.threshold
        for r in scan_files(a.wav, a.scan, a.onnx, thr, a.refractory, a.precision, a.device):
            if a.json:
                print(json.dumps(r))
            else:
                print(f"{r['file']}: {r['start_s']:.3f}-{r['end_s']:.3f} s  logit {r['logit']:+.6f}  "
                      f"p {r['probability']:.4f}  WAKE")
        return 0
    res = score(a.wav, a.onnx, a.pad, a.seed, 0.5 if a.threshold is None else a.threshold, a.precision, a.device,
                a.cpu)
    for r in res:
        if a.json:
            print(json.dumps(r))
        else:
            print(f"{r['file']}: logit {r['logit']:+.6f}  p {r['probability']:.4f}  "
                  f"{'WAKE' if r['wake'] else '-'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
