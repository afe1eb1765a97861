"""Forced-alignment benchmark (not the driver's bench.py line): wk_ctc_align
against wk_ctc_loss without gradient on the same inputs (the same lattice with
lse in place of max), against a torch-ROCm statement of the same Viterbi on the
same GPU, and against the numpy reference (tests/ctc_align_ref.py) on the CPU.

Two shapes: the reference's training batch (ctc.py:21-40: B = 8, T = 801,
V = 4000; S = 40) and a large batch (B = 256).  Random logits, full-length
inputs and labels.  GPU passes alternate in one process; medians over the timed
passes (HIP events on the current stream):

  wk_align   one wk_ctc_align call into preallocated outputs, all five of them;
  wk_loss    one wk_ctc_loss call, d_grad = NULL (prep, gather, both recursions, finish);
  torch_gpu  the recurrence as T steps of batched torch ops with back-pointers,
             then a T-step gather chase (what the HIP kernels replace; few passes).

The alignment is checked against the numpy reference on the timed inputs (bit
equality, first utterances).  Prints one JSON line and writes it to --out
(profiles/ctc_align_bench.json).
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

SHAPES = {"reference": (8, 801, 4000, 40), "large": (256, 801, 4000, 40)}
NEG = float("-inf")


def torch_viterbi(lp, labels):
    """The recurrence and tie rule of wk_ctc_align in torch ops, full lengths:
    lp (B, T, V), labels (B, S) int64 -> (states (B, T) int64, scores (B,))."""
    import torch
    B, T, V = lp.shape
    S = labels.shape[1]
    L = 2 * S + 1
    ext = torch.zeros((B, L), dtype=torch.int64, device=lp.device)
    ext[:, 1::2] = labels
    skip = torch.zeros((B, L), dtype=torch.bool, device=lp.device)
    skip[:, 3::2] = labels[:, 1:] != labels[:, :-1]
    x = lp.gather(2, ext.unsqueeze(1).expand(B, T, L))              # (B, T, L)
    a = torch.full((B, L), NEG, device=lp.device)
    a[:, :2] = x[:, 0, :2]
    bp = torch.zeros((T, B, L), dtype=torch.int64, device=lp.device)
    pad = torch.full((B, 2), NEG, device=lp.device)
    for t in range(1, T):
        ext_a = torch.cat([pad, a], 1)
        n1, n2 = ext_a[:, 1:L + 1], ext_a[:, :L]
        m1 = n1 > a
        best = torch.where(m1, n1, a)
        m2 = skip & (n2 > best)
        best = torch.where(m2, n2, best)
        bp[t] = m1.long().masked_fill(m2, 2)
        a = x[:, t] + best
    last = a[:, L - 1] >= a[:, L - 2]
    scores = torch.where(last, a[:, L - 1], a[:, L - 2])
    s = torch.where(last, L - 1, L - 2).unsqueeze(1)
    states = torch.empty((B, T), dtype=torch.int64, device=lp.device)
    for t in range(T - 1, -1, -1):
        states[:, t] = s[:, 0]
        s = s - bp[t].gather(1, s)
    return states, scores


def bench_shape(name, B, T, V, S, iters, warmup, torch_iters, cpu_utts):
    import numpy as np
    import torch
    import torch.nn.functional as F
    import ctc_align_ref as A
    from wakeword import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(17)
    lp = F.log_softmax(torch.randn((B, T, V), generator=g, device=dev), -1)
    labels = torch.randint(1, V, (B, S), generator=g, device=dev, dtype=torch.int64)
    lab32 = labels.to(torch.int32)
    il32 = torch.full((B,), T, dtype=torch.int32, device=dev)
    tl32 = torch.full((B,), S, dtype=torch.int32, device=dev)

    L = _lib.lib()
    ws_a = torch.empty(L.wk_ctc_align_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    ws_l = torch.empty(L.wk_ctc_loss_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    tokens = torch.empty_like(states)
    frame_lp = torch.empty((B, T), device=dev)
    spans = torch.empty((B, S, 2), dtype=torch.int32, device=dev)
    scores = torch.empty(B, device=dev)
    nll = torch.empty(B, device=dev)
    loss = torch.empty(1, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def stream():
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def wk_align():
        _lib.check(L.wk_ctc_align(p(lp), B, T, V, p(lab32), S, p(il32), p(tl32), S, p(ws_a), p(states), p(tokens), p(frame_lp),
                                  p(spans), p(scores), 0, stream()), "wk_ctc_align")

    def wk_loss():
        _lib.check(L.wk_ctc_loss(p(lp), B, T, V, p(lab32), S, p(il32), p(tl32), S, 1, 0, 1.0, p(ws_l), p(nll), p(loss), None, 0,
                                 stream()), "wk_ctc_loss")

    tv = {}

    def torch_gpu():
        tv["states"], tv["scores"] = torch_viterbi(lp, labels)

    fns = {"wk_align": wk_align, "wk_loss": wk_loss, "torch_gpu": torch_gpu}
    times = {k: [] for k in fns}
    for i in range(warmup + iters):
        for k, fn in fns.items():            # alternating passes
            if k == "torch_gpu" and i >= 1 + torch_iters:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= (1 if k == "torch_gpu" else warmup):
                times[k].append(e0.elapsed_time(e1))
    res = {"shape": {"B": B, "T": T, "V": V, "S": S}, "iters": iters, "torch_iters": len(times["torch_gpu"]),
           "ms_median": {k: statistics.median(v) for k, v in times.items()},
           "ms_min": {k: min(v) for k, v in times.items()}, "ms_max": {k: max(v) for k, v in times.items()},
           "workspace_bytes": {"wk_align": ws_a.numel(), "wk_loss": ws_l.numel()}}

    # the numpy reference on the first utterances: the time, and bit equality of the device's result
    lp_h, lab_h = lp[:cpu_utts].cpu().numpy(), labels[:cpu_utts].cpu().numpy()
    n = lp_h.shape[0]
    t0 = time.perf_counter()
    ref = A.align_batch(lp_h, lab_h, [T] * n, [S] * n)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    res["ms_median"]["numpy_cpu_per_utterance"] = cpu_ms / n
    res["ms_median"]["numpy_cpu_batch_extrapolated"] = cpu_ms / n * B
    same = (np.array_equal(states[:n].cpu().numpy(), ref["states"]) and np.array_equal(spans[:n].cpu().numpy(), ref["spans"])
            and np.array_equal(scores[:n].cpu().numpy().view(np.int32), ref["scores"].view(np.int32)))
    res["bit_equal_to_numpy_reference"] = bool(same)
    res["torch_gpu_same_path"] = bool(torch.equal(tv["states"].to(torch.int32), states))
    res["score_mean"] = float(scores.mean())
    m = res["ms_median"]
    res["align_over_loss"] = m["wk_align"] / m["wk_loss"]
    res["speedup_vs_torch_gpu"] = m["torch_gpu"] / m["wk_align"]
    res["speedup_vs_numpy_cpu"] = m["numpy_cpu_batch_extrapolated"] / m["wk_align"]
    if not same:
        sys.exit(f"bench_ctc_align.py: {name}: the device alignment differs from the numpy reference")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--cpu-utts", type=int, default=4)
    ap.add_argument("--shapes", default="reference,large")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ctc_align_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ctc_align.py needs a HIP device")
    out = {"bench": "ctc_align", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "shapes": {n: bench_shape(n, *SHAPES[n], a.iters, a.warmup, a.torch_iters, a.cpu_utts) for n in a.shapes.split(",")}}
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
