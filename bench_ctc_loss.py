"""CTC-loss benchmark (not the driver's bench.py line): loss + gradient of
wk_ctc_loss against torch-ROCm's F.ctc_loss forward + backward on the same GPU
in the same process, passes alternating, and against torch-CPU on 16 threads.

Two shapes: the reference's training batch (ctc.py:21-40: B = 8, T = 801,
V = 4000; S = 40) and a large batch (B = 256).  Random logits, full-length
inputs and labels, reduction "mean".  Each implementation gets the layout it
reads: (B, T, V) for wk_ctc_loss, (T, B, V) for torch.  Three timings each on
the GPU, medians over the timed passes (HIP events on the current stream):

  wk_call      one wk_ctc_loss call into preallocated outputs (loss + gradient);
  wk_autograd  wakeword.ctc_loss(...).backward() (allocations and the
               grad_output scaling included) -- what replaces the line below;
  torch_gpu    F.ctc_loss(...).backward() on a (T, B, V) leaf.

Prints one JSON line and writes it to --out (profiles/ctc_loss_bench.json).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [REPO, os.path.join(REPO, "esp32-wake-word_amd")]

SHAPES = {"reference": (8, 801, 4000, 40), "large": (256, 801, 4000, 40)}


def bench_shape(name, B, T, V, S, iters, warmup, cpu_iters):
    import torch
    import torch.nn.functional as F
    import wakeword
    from wakeword import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(17)
    lp_btv = F.log_softmax(torch.randn((B, T, V), generator=g, device=dev), -1)
    lp_tbv = lp_btv.transpose(0, 1).contiguous()
    labels = torch.randint(1, V, (B, S), generator=g, device=dev, dtype=torch.int64)
    il = torch.full((B,), T, dtype=torch.int64)
    tl = torch.full((B,), S, dtype=torch.int64)
    il_d, tl_d = il.to(dev), tl.to(dev)

    L = _lib.lib()
    lab32, il32, tl32 = labels.to(torch.int32), il_d.to(torch.int32), tl_d.to(torch.int32)
    ws = torch.empty(L.wk_ctc_loss_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    nll = torch.empty(B, device=dev)
    loss = torch.empty(1, device=dev)
    grad = torch.empty_like(lp_btv)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def wk_call():
        _lib.check(L.wk_ctc_loss(p(lp_btv), B, T, V, p(lab32), S, p(il32), p(tl32), S, 2, 0, 1.0, p(ws), p(nll), p(loss),
                                 p(grad), 0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "wk_ctc_loss")
        return loss

    def wk_autograd():
        x = lp_btv.detach().requires_grad_(True)
        out = wakeword.ctc_loss(x, lab32, il32, tl32, batch_first=True)
        out.backward()
        return out.detach()

    def torch_gpu():
        x = lp_tbv.detach().requires_grad_(True)
        out = F.ctc_loss(x, labels, il_d, tl_d, blank=0, reduction="mean")
        out.backward()
        return out.detach()

    fns = {"wk_call": wk_call, "wk_autograd": wk_autograd, "torch_gpu": torch_gpu}
    times = {k: [] for k in fns}
    values = {}
    for i in range(warmup + iters):
        for k, fn in fns.items():            # alternating passes
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[k].append(e0.elapsed_time(e1))
            values[k] = float(out.reshape(-1)[0])
    res = {"shape": {"B": B, "T": T, "V": V, "S": S}, "iters": iters,
           "loss": values, "ms_median": {k: statistics.median(v) for k, v in times.items()},
           "ms_min": {k: min(v) for k, v in times.items()}, "ms_max": {k: max(v) for k, v in times.items()}}
    # bytes the gradient pass cannot avoid: one read of lp, one write of g
    res["wk_call_lp_plus_grad_GBs"] = 2 * B * T * V * 4 / (res["ms_median"]["wk_call"] * 1e-3) / 1e9

    torch.set_num_threads(16)
    lp_cpu, lab_cpu = lp_tbv.cpu(), labels.cpu()
    cpu = []
    for i in range(1 + cpu_iters):
        x = lp_cpu.detach().requires_grad_(True)
        t0 = time.perf_counter()
        out = F.ctc_loss(x, lab_cpu, il, tl, blank=0, reduction="mean")
        out.backward()
        if i:
            cpu.append((time.perf_counter() - t0) * 1e3)
    res["ms_median"]["torch_cpu_16t"] = statistics.median(cpu)
    res["loss"]["torch_cpu_16t"] = float(out)
    m = res["ms_median"]
    res["speedup_vs_torch_gpu"] = {"wk_call": m["torch_gpu"] / m["wk_call"], "wk_autograd": m["torch_gpu"] / m["wk_autograd"]}
    res["speedup_vs_torch_cpu_16t"] = {"wk_call": m["torch_cpu_16t"] / m["wk_call"],
                                       "wk_autograd": m["torch_cpu_16t"] / m["wk_autograd"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-iters", type=int, default=3)
    ap.add_argument("--shapes", default="reference,large")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ctc_loss_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ctc_loss.py needs a HIP device")
    out = {"bench": "ctc_loss", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "shapes": {n: bench_shape(n, *SHAPES[n], a.iters, a.warmup, a.cpu_iters) for n in a.shapes.split(",")}}
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
