"""Prefix-beam-search benchmark (not the driver's bench.py line): wk_ctc_beam
(W = 16, K = 16, n_best = 1) against the greedy floor (wk_ctc_frame_argmax and
the collapse of repeats and blanks), against wk_ctc_align on the same shape (a
lattice of the same size, one wave per utterance as well), against a device
copy of the same log-probs (the candidate stage reads them once: the copy rate
is its yardstick) and against the numpy reference (tests/ctc_beam_ref.py) on
the CPU.

Two shapes: the reference's batch (ctc.py:21-40: B = 8, T = 801, V = 4000) and
a large batch (B = 256).  Gaussian logits of scale 4 with the blank column
raised by 12, full-length inputs.  GPU passes alternate in one process; medians
over the timed passes (HIP events on the current stream):

  wk_beam    one wk_ctc_beam call into preallocated outputs (both kernels);
  wk_align   one wk_ctc_align call, S = 40 random labels, all outputs;
  greedy     wk_ctc_frame_argmax of a GRU-CTC model's last decode at the same
             (B, T, V), then the collapse in torch ops on the device;
  copy       dst.copy_(log_probs): the same bytes read once and written once.

Each kernel alone: the two kernels' durations from the device activity records
of torch.profiler over separate, untimed-otherwise calls (`kernel_ms`; null
with the reason where the profiler gives no device records).  The candidate
stage's rate is its bytes read over its duration; `cand_share_of_copy` is that
over the copy's bytes moved (read + written) per second.

The device's best hypothesis is compared with the float64 reference on the
first utterances (reported, with the utterance's margin: random logits at
T = 801 are rarely decisive).  Prints one JSON line and writes it to --out
(profiles/ctc_beam_bench.json).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [REPO, os.path.join(REPO, "esp32-wake-word_amd"), os.path.join(REPO, "tests")]

SHAPES = {"reference": (8, 801, 4000), "large": (256, 801, 4000)}
W, K, S = 16, 16, 40


def kernel_split(fn, calls):
    """Mean device duration (ms) of the two kernels over `calls` profiled calls of fn."""
    import torch
    from torch.profiler import ProfilerActivity, profile, supported_activities
    if ProfilerActivity.CUDA not in supported_activities():
        return None, "torch.profiler has no device activity on this build"
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            for key in ("ctc_beam_cand_kernel", "ctc_beam_recur_kernel"):
                if key in ev.name:
                    us = getattr(ev, "device_time", 0) or getattr(ev, "cuda_time", 0)
                    if us:
                        out.setdefault(key, []).append(us / 1e3)
        if set(out) != {"ctc_beam_cand_kernel", "ctc_beam_recur_kernel"}:
            return None, f"no device records for the kernels (saw {sorted(out)})"
        return {k.replace("ctc_beam_", "").replace("_kernel", ""): statistics.median(v) for k, v in out.items()}, None
    except Exception as e:      # the profiler is an optional measurement; the timed passes do not depend on it
        return None, f"{type(e).__name__}: {e}"


def bench_shape(name, B, T, V, iters, warmup, cpu_utts, profile_calls, greedy):
    import numpy as np
    import torch
    import torch.nn.functional as F
    import ctc_beam_ref as R
    import wakeword
    from wakeword import _lib
    from wakeword.ctc import random_state_dict
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(17)
    z = 4.0 * torch.randn((B, T, V), generator=g, device=dev)
    z[:, :, 0] += 12.0
    lp = F.log_softmax(z, -1)
    del z
    labels = torch.randint(1, V, (B, S), generator=g, device=dev, dtype=torch.int32)
    il32 = torch.full((B,), T, dtype=torch.int32, device=dev)
    tl32 = torch.full((B,), S, dtype=torch.int32, device=dev)

    L = _lib.lib()
    ws_b = torch.empty(L.wk_ctc_beam_workspace_bytes(B, T, W, K), dtype=torch.uint8, device=dev)
    ws_a = torch.empty(L.wk_ctc_align_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    tokens = torch.empty((B, 1, T), dtype=torch.int32, device=dev)
    lengths = torch.empty((B, 1), dtype=torch.int32, device=dev)
    scores = torch.empty((B, 1), device=dev)
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    a_tokens, a_lp = torch.empty_like(states), torch.empty((B, T), device=dev)
    spans, a_scores = torch.empty((B, S, 2), dtype=torch.int32, device=dev), torch.empty(B, device=dev)
    dst = torch.empty_like(lp)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def stream():
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def wk_beam():
        _lib.check(L.wk_ctc_beam(p(lp), B, T, V, None, W, K, 1, T, p(ws_b), p(tokens), p(lengths), p(scores), None, 0, stream()),
                   "wk_ctc_beam")

    def wk_align():
        _lib.check(L.wk_ctc_align(p(lp), B, T, V, p(labels), S, p(il32), p(tl32), S, p(ws_a), p(states), p(a_tokens), p(a_lp),
                                  p(spans), p(a_scores), 0, stream()), "wk_ctc_align")

    def copy():
        dst.copy_(lp)

    fns = {"wk_beam": wk_beam, "wk_align": wk_align, "copy": copy}
    res = {"shape": {"B": B, "T": T, "V": V, "W": W, "K": K, "n_best": 1, "S_align": S}, "iters": iters}
    if greedy:      # the greedy floor needs a model: its frame argmax reads the logits of the model's last decode
        try:
            model = wakeword.CTCModel(random_state_dict(V, seed=3), V)
            model.decode(torch.randn((B, T, 80), generator=g, device=dev))
            pred = torch.empty((B, T), dtype=torch.int32, device=dev)
            g_tok = torch.empty((B, T + 1), dtype=torch.int32, device=dev)      # column T takes the dropped frames
            first = torch.zeros((B, 1), dtype=torch.int32, device=dev)

            def greedy_fn():
                _lib.check(L.wk_ctc_frame_argmax(model._h, B, T, p(pred), stream()), "wk_ctc_frame_argmax")
                keep = (pred != 0) & (pred != torch.cat([first, pred[:, :-1]], 1))
                g_tok.fill_(-1)
                g_tok.scatter_(1, torch.where(keep, keep.cumsum(1) - 1, T), pred)
                g_tok[:, T] = -1
                return keep.sum(1)
            greedy_fn()
            torch.cuda.synchronize()
            fns["greedy"] = greedy_fn
        except Exception as e:      # (a batch the model's workspace does not take: the floor is left out, with the reason)
            res["greedy_unavailable"] = f"{type(e).__name__}: {e}"
            greedy = False

    times = {k: [] for k in fns}
    for i in range(warmup + iters):
        for k, fn in fns.items():            # alternating passes
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[k].append(e0.elapsed_time(e1))
    res["ms_median"] = {k: statistics.median(v) for k, v in times.items()}
    res["ms_min"] = {k: min(v) for k, v in times.items()}
    res["ms_max"] = {k: max(v) for k, v in times.items()}
    res["workspace_bytes"] = {"wk_beam": ws_b.numel(), "wk_align": ws_a.numel()}

    res["kernel_ms"], why = kernel_split(wk_beam, profile_calls)
    if why:
        res["kernel_ms_unavailable"] = why
    m, nbytes = res["ms_median"], lp.numel() * 4
    res["log_prob_bytes"] = nbytes
    res["copy_GBps_read_plus_write"] = 2 * nbytes / m["copy"] / 1e6
    if res["kernel_ms"]:
        res["cand_GBps_read"] = nbytes / res["kernel_ms"]["cand"] / 1e6
        res["cand_share_of_copy"] = res["cand_GBps_read"] / res["copy_GBps_read_plus_write"]
        res["recur_us_per_frame"] = res["kernel_ms"]["recur"] * 1e3 / T
    res["beam_over_align"] = m["wk_beam"] / m["wk_align"]
    if greedy:
        res["beam_over_greedy"] = m["wk_beam"] / m["greedy"]

    # the numpy reference on the first utterances: its time, and what the device's best hypothesis is against it
    wk_beam()
    torch.cuda.synchronize()
    n = min(cpu_utts, B)
    lp_h = lp[:n].cpu().numpy()
    t0 = time.perf_counter()
    ref = R.beam_batch(lp_h, None, W, K, 1, T, np.float64)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    m["numpy_cpu_per_utterance"] = cpu_ms / n
    m["numpy_cpu_batch_extrapolated"] = cpu_ms / n * B
    res["speedup_vs_numpy_cpu"] = m["numpy_cpu_batch_extrapolated"] / m["wk_beam"]
    tok_h, len_h, sc_h = tokens[:n].cpu().numpy(), lengths[:n].cpu().numpy(), scores[:n].cpu().numpy()
    res["against_reference"] = [
        {"same_best_hypothesis": bool(len_h[b, 0] == ref["lengths"][b, 0] and np.array_equal(tok_h[b, 0], ref["tokens"][b, 0])),
         "score_device": float(sc_h[b, 0]), "score_float64": float(ref["scores"][b, 0]), "length": int(len_h[b, 0]),
         "margin": float(R.margin(lp_h[b], W, K)), "tau": R.TAU} for b in range(n)]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-utts", type=int, default=2)
    ap.add_argument("--profile-calls", type=int, default=5)
    ap.add_argument("--no-greedy", action="store_true", help="leave out the greedy floor (it builds a GRU-CTC model)")
    ap.add_argument("--shapes", default="reference,large")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ctc_beam_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ctc_beam.py needs a HIP device")
    out = {"bench": "ctc_beam", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "shapes": {n: bench_shape(n, *SHAPES[n], a.iters, a.warmup, a.cpu_utts, a.profile_calls, not a.no_greedy)
                      for n in a.shapes.split(",")}}
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
