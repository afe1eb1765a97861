#!/usr/bin/env python
"""Measurements of the post-training quantisation feature.

1. int8 wk_cnn throughput at 65,536 clips, A/B against another build of the
   library (``--parent-lib``, normally the parent commit's libwakeword.so):
   both libraries are loaded into this process under private symbol scopes and
   timed in alternating passes on the same features -- parent (exponents
   compiled in), this build at the default spec, this build at the spec
   calibrated on the golden features (both through run-time shifts).  The
   default-spec logits of the two builds are compared bit for bit first.
2. wk_calibrate wall time (launch to counters on the host) at 640 clips (the
   reference's 32 x 20) and at 65,536.

Prints one JSON line; ``--out`` also writes it to a file.  Needs a HIP device.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
for _p in (REPO, os.path.join(REPO, "esp32-wake-word_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="another libwakeword.so to compare against (omit: no A/B)")
    ap.add_argument("--clips", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=400, help="timed wk_cnn launches per pass and variant")
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import wakeword
    from wakeword import _lib
    from wakeword.api import pack_weights
    if not torch.cuda.is_available():
        raise SystemExit("bench_quant.py needs a HIP device")

    golden = os.path.join(REPO, "tests", "golden")
    sd = wakeword.xiaoa_state_dict(wakeword.read_onnx(os.path.join(golden, "xiaoa.onnx"))[0])
    blob = pack_weights(sd)
    g = np.concatenate([np.load(os.path.join(golden, "wavs.npz"))["feat_zero"],
                        np.load(os.path.join(golden, "synth.npz"))["feats"]]).astype(np.float32)
    gen = torch.Generator().manual_seed(11)
    feats = torch.randn((args.clips, 13, 63), generator=gen).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    calibrated = wakeword.calibrate(sd, g)
    result = {"bench": "quant", "clips": args.clips, "launches_per_pass": args.launches, "passes": args.passes,
              "device": torch.cuda.get_device_name(0), "calibrated_spec": calibrated.to_dict()}

    def handle(L, spec=None):
        cfg = _lib.WkConfig(_lib.WK_MODE_TORCHAUDIO_CMVN, _lib.WK_PREC_INT8, 1, 0, 1)
        h = C.c_void_p()
        assert L.wk_create(C.byref(cfg), blob.ctypes.data_as(C.c_void_p), C.byref(h)) == 0
        if spec is not None:
            c = spec._to_c()
            assert L.wk_set_quant(h, C.byref(c)) == 0
        return h

    def run(L, h, out, n):
        for _ in range(n):
            assert L.wk_cnn(h, C.c_void_p(feats.data_ptr()), args.clips, C.c_void_p(out.data_ptr()), stream) == 0

    def timed(L, h, out):
        run(L, h, out, 3)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        run(L, h, out, args.launches)
        t1.record()
        t1.synchronize()
        return args.clips * args.launches / (t0.elapsed_time(t1) * 1e-3) / 1e6     # M clips/s

    new = _lib.lib()
    variants = {"default": (new, handle(new)), "calibrated": (new, handle(new, calibrated))}
    if args.parent_lib:
        # private scope, its own definitions first: no symbol of one build resolves into the other
        parent = C.CDLL(os.path.abspath(args.parent_lib), mode=C.RTLD_LOCAL | os.RTLD_DEEPBIND)
        _lib._declare(parent)
        variants = {"parent": (parent, handle(parent)), **variants}
    outs = {k: torch.empty((args.clips,), dtype=torch.float32, device="cuda") for k in variants}
    for k, (L, h) in variants.items():
        run(L, h, outs[k], 1)
    torch.cuda.synchronize()
    if args.parent_lib:
        result["default_logits_differing_from_parent"] = int((outs["parent"] != outs["default"]).sum())
    rates = {k: [] for k in variants}
    for _ in range(args.passes):
        for k, (L, h) in variants.items():
            rates[k].append(round(timed(L, h, outs[k]), 3))
    ab = {"M_clips_per_s": rates, "mean": {k: round(statistics.mean(v), 3) for k, v in rates.items()},
          "spread_pct": {k: round(100.0 * (max(v) - min(v)) / statistics.mean(v), 2) for k, v in rates.items()}}
    base = "parent" if args.parent_lib else "default"
    for k in variants:
        if k != base:
            ab[f"{k}_vs_{base}_pct"] = round(100.0 * (ab["mean"][k] / ab["mean"][base] - 1.0), 2)
            ab[f"{k}_ahead_of_{base}_passes"] = sum(a > b for a, b in zip(rates[k], rates[base]))
    result["int8_cnn_ab"] = ab

    m = wakeword.KWSModel(sd)
    calib = {}
    for B in (640, args.clips):
        x = feats[:B]
        times = []
        for i in range(12):
            torch.cuda.synchronize()
            t = time.perf_counter()
            wakeword.calibrate(m, x)
            if i >= 2:
                times.append((time.perf_counter() - t) * 1e3)
        calib[str(B)] = {"ms_median": round(statistics.median(times), 4), "ms_min": round(min(times), 4),
                         "M_clips_per_s": round(B / statistics.median(times) / 1e3, 3)}
    result["calibrate"] = calib
    for L, h in variants.values():
        L.wk_destroy(h)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
