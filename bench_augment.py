"""bench_augment.py -- rows/s of the waveform augmentation stage (wk_augment_batch).

    python bench_augment.py [--passes P] [--warmup W] [--clips N] [--host-clips H] [--device D]

Three measurements, written to profiles/augment_bench.json and printed as ONE
JSON line:

  (a) wk_augment_batch at N clips x 5 reference variants x 16000 samples, with
      the SNR stage off and on: rows/s, and bytes/s (every clip read once, every
      row written once) against the 6.29 TB/s copy rate measured on this chip.
      With SNR on, the issue-bound estimate: the loop's vector instructions per
      Philox block (counted from the ISA) at one wave-instruction
      per 4 cycles per SIMD (16 for the quarter-rate ones).
  (b) the alternatives, same stage, same variants: the host path it replaces
      (wk_augment per row on 16 threads into pinned memory, then the H2D copy)
      on H clips, and a torch-ROCm statement on the same GPU (F.interpolate,
      randn noise) on N clips.
  (c) end to end: Trainer.step_augmented on 3277 clips (16385 rows) against
      Trainer.step on ready features of as many rows.

All legs of a group run in one process and alternate pass by pass; device legs
are timed with device events, the host leg with a wall clock around work that
ends in a synchronise.  Every leg reports its median and its own spread.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "esp32-wake-word_amd"))
sys.path.insert(0, REPO)

COPY_RATE = 6.29e12          # bytes/s, the measured device copy rate (DESIGN)
CLOCK_HZ = 2.4e9             # the chip's peak engine clock
OUT_LEN = 16000
SNR = (0.01, 5.0, 20.0)
# Vector instructions of one wave for one Philox block of four samples per lane in the SNR-on loop at speed 1,
# counted from the ISA: the ten rounds' 32-bit multiplies, the transcendentals (2 log, 2 sqrt), and
# the rest (xor / add of the rounds, the log and sincospi polynomials, selects, loop, load, LDS, the two sums).
# A plain instruction issues in 4 cycles and a transcendental in 16; the estimate is given with the multiplies at
# 16 cycles (quarter rate) and at 8 (half rate).
ISSUE_MULS, ISSUE_TRANS, ISSUE_PLAIN = 80, 4, 240


def stats(ms):
    s = sorted(ms)
    return {"ms": round(s[len(s) // 2], 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4),
            "spread_pct": round(100.0 * (s[-1] - s[0]) / s[len(s) // 2], 2), "passes": len(s)}


def alternate(torch, legs, passes, warmup):
    """legs: {name: (fn, 'event' | 'wall')}.  One call of every leg per pass, in turn."""
    ms = {k: [] for k in legs}
    for p in range(warmup + passes):
        for name, (fn, how) in legs.items():
            if how == "event":
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                t = a.elapsed_time(b)
            else:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t = (time.perf_counter() - t0) * 1e3
            if p >= warmup:
                ms[name].append(t)
    return {k: stats(v) for k, v in ms.items()}


def torch_stage(torch, F, x, snr):
    """The same stage in torch ops on the device (full-length clips: pad_audio is the identity)."""
    n = x.shape[0]
    outs = [x]
    for speed in (0.8, 1.2):
        y = F.interpolate(x[:, None], size=int(OUT_LEN * speed), mode="linear", align_corners=False)[:, 0]
        if y.shape[1] < OUT_LEN:
            y = torch.cat([y, torch.randn(n, OUT_LEN - y.shape[1], device=x.device) * 0.005], dim=1)
        outs.append(y[:, :OUT_LEN])
    for volume in (0.7, 1.3):
        outs.append(torch.clamp(x * volume, -1.0, 1.0))
    out = torch.stack(outs, 1).reshape(n * 5, OUT_LEN)
    if snr:
        noise = torch.randn_like(out) * SNR[0]
        snr_db = torch.rand(n * 5, 1, device=x.device) * (SNR[2] - SNR[1]) + SNR[1]
        ratio = 10 ** (snr_db / 20)
        scale = torch.sqrt(torch.mean(out ** 2, 1, keepdim=True) / (torch.mean(noise ** 2, 1, keepdim=True) * ratio))
        out = torch.clamp(out + noise * scale, -1.0, 1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", type=int, default=13107)
    ap.add_argument("--host-clips", type=int, default=656)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    import wakeword
    from wakeword import _lib

    torch.cuda.set_device(a.device)
    dev = f"cuda:{a.device}"
    variants = wakeword.REFERENCE_VARIANTS
    K = len(variants)
    res = {"metric": "rows/s of the waveform augmentation stage (5 variants x 16000 samples) on one MI355X",
           "unit": "rows/s", "higher_is_better": True, "copy_rate_bytes_per_s": COPY_RATE,
           "config": {"clips": a.clips, "variants": variants, "out_len": OUT_LEN, "pad_noise": 0.005, "snr": SNR,
                      "passes": a.passes, "warmup": a.warmup}}

    # ---- (a) the kernel, (b) the torch statement ------------------------------------------
    x = wakeword.synth_clips(1234, 0, a.clips, OUT_LEN, device=a.device)
    epoch = [0]

    def wk(snr):
        def fn():
            epoch[0] += 1
            return wakeword.augment_batch(x, None, variants, 0.005, snr, seed=1, epoch=epoch[0], device=a.device)
        return fn

    legs = {"wk_snr_off": (wk(None), "event"), "wk_snr_on": (wk(SNR), "event"),
            "torch_rocm_snr_off": (lambda: torch_stage(torch, F, x, False), "event"),
            "torch_rocm_snr_on": (lambda: torch_stage(torch, F, x, True), "event")}
    r = alternate(torch, legs, a.passes, a.warmup)
    rows = a.clips * K
    nbytes = rows * OUT_LEN * 4 + a.clips * OUT_LEN * 4
    for name, s in r.items():
        s["rows_per_s"] = round(rows / (s["ms"] * 1e-3), 1)
        if name.startswith("wk"):
            s["bytes_per_s"] = round(nbytes / (s["ms"] * 1e-3), 1)
            s["of_copy_rate"] = round(s["bytes_per_s"] / COPY_RATE, 4)
    simds = torch.cuda.get_device_properties(a.device).multi_processor_count * 4
    wave_blocks = rows * (OUT_LEN / 4) / 64                       # a wave makes 64 Philox blocks per pass of its loop
    for name, mul_cycles in (("quarter", 16), ("half", 8)):
        cycles = ISSUE_MULS * mul_cycles + ISSUE_TRANS * 16 + ISSUE_PLAIN * 4
        r["wk_snr_on"][f"issue_bound_ms_mul_{name}_rate"] = round(wave_blocks * cycles / (simds * CLOCK_HZ) * 1e3, 4)
    r["wk_snr_on"]["hbm_bound_ms"] = round(nbytes / COPY_RATE * 1e3, 4)
    res["kernel"] = r
    del legs

    # ---- (b) the host path: wk_augment per row on 16 threads, then the H2D copy --------------
    L = _lib.lib()
    H = a.host_clips
    xh = x[:H].cpu().numpy()
    pinned = torch.empty((H * K, OUT_LEN), dtype=torch.float32).pin_memory()
    ph = pinned.numpy()
    d_rows = torch.empty((H * K, OUT_LEN), dtype=torch.float32, device=dev)
    threads = 16

    def host_rows(t):
        for row in range(t, H * K, threads):
            i, v = divmod(row, K)
            L.wk_augment(xh[i].ctypes.data_as(C.c_void_p), OUT_LEN, variants[v][0], variants[v][1], 0.005, row,
                         ph[row].ctypes.data_as(C.c_void_p), OUT_LEN)

    pool = cf.ThreadPoolExecutor(threads)

    def host():
        list(pool.map(host_rows, range(threads)))
        d_rows.copy_(pinned, non_blocking=True)

    hs = alternate(torch, {"host_16_threads_plus_h2d": (host, "wall")}, max(3, a.passes // 2), 1)["host_16_threads_plus_h2d"]
    hs["clips"] = H
    hs["rows_per_s"] = round(H * K / (hs["ms"] * 1e-3), 1)
    hs["note"] = "SNR stage absent on the host (wk_augment has none)"
    res["host"] = hs
    pool.shutdown()
    res["wk_vs_host"] = round(r["wk_snr_off"]["rows_per_s"] / hs["rows_per_s"], 1)
    res["wk_vs_torch_rocm"] = {k: round(r[f"wk_snr_{k}"]["rows_per_s"] / r[f"torch_rocm_snr_{k}"]["rows_per_s"], 2)
                               for k in ("off", "on")}
    del x, d_rows

    # ---- (c) end to end ------------------------------------------------------------------------
    n = 3277
    xa = wakeword.synth_clips(99, 0, n, OUT_LEN, device=a.device)
    y = (torch.rand(n, device=dev) < 0.5).float()
    feats, _ = wakeword.extract_features(xa, None, is_noise=True)
    y5 = y.repeat_interleave(K)
    t_plain, t_aug = wakeword.Trainer(seed=0, device=a.device), wakeword.Trainer(seed=0, device=a.device)
    ep = [0]

    def aug_step():
        ep[0] += 1
        return t_aug.step_augmented(xa, None, y, ep[0], is_noise=True)

    e = alternate(torch, {"step_on_ready_features": (lambda: t_plain.step(feats, y5), "event"),
                          "step_augmented": (aug_step, "event")}, a.passes, a.warmup)
    e["rows"] = n * K
    e["added_ms"] = round(e["step_augmented"]["ms"] - e["step_on_ready_features"]["ms"], 4)
    loss = float(aug_step())
    e["final_loss"] = loss
    res["end_to_end"] = e

    res["value"] = r["wk_snr_on"]["rows_per_s"]
    res["ok"] = bool(loss == loss and abs(loss) != float("inf"))
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "augment_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    if not res["ok"]:
        sys.exit(3)


if __name__ == "__main__":
    main()
