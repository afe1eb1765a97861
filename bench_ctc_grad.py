"""GRU-CTC gradient benchmark (not the driver's bench.py line): forward_train +
wk_ctc_loss + wk_ctc_backward (CTCModel.loss_and_grad: loss, every parameter's
gradient, the gradient norm) against torch-ROCm autograd of the same module on
the same GPU in the same process, passes alternating, and against torch-CPU on
16 threads.

Two shapes: the reference's training batch (ctc.py:21-40: B = 8, T = 801,
V = 4000; S = 40) and B = 64.  Seeded default-initialised weights, random
z-score-like features, full-length inputs, reduction "mean".  The torch module
runs in train mode with both dropouts at p = 0 (its RNN backward needs train
mode; the function is then the eval-mode one both sides differentiate) and
ends with clip_grad_norm_ at a bound that never clips, for the norm.  Timings
are medians over the timed passes (HIP events on the current stream):

  wk_step            CTCModel.loss_and_grad, allocations included;
  wk_forward_train, wk_loss, wk_backward   its three calls, timed apart;
  torch_gpu          zero_grad, module forward, F.ctc_loss, backward, norm.

Prints one JSON line and writes it to --out (profiles/ctc_grad_bench.json).
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

SHAPES = {"reference": (8, 801, 4000, 40), "b64": (64, 801, 4000, 40)}


def torch_module(vocab, seed):
    import torch
    from torch import nn

    class GRUCTC(nn.Module):     # GRU_CTC_Model (ctc.py:119-152), dropouts at 0
        def __init__(self):
            super().__init__()
            self.audio_encoder = nn.Sequential(nn.Linear(80, 128), nn.LayerNorm(128), nn.ReLU(), nn.Dropout(0.0))
            self.gru = nn.GRU(input_size=128, hidden_size=128, num_layers=2, batch_first=True, dropout=0.0, bidirectional=True)
            self.output_layer = nn.Linear(256, vocab)

        def forward(self, x):
            y, _ = self.gru(self.audio_encoder(x))
            return torch.nn.functional.log_softmax(self.output_layer(y), dim=-1)

    from wakeword.ctc import random_state_dict
    m = GRUCTC()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in random_state_dict(vocab, seed).items()})
    return m.train()


def torch_step(m, feats, labels, il, tl):
    import torch
    import torch.nn.functional as F
    m.zero_grad(set_to_none=True)
    lp = m(feats)
    loss = F.ctc_loss(lp.transpose(0, 1), labels, il, tl, blank=0, reduction="mean")
    loss.backward()
    norm = torch.nn.utils.clip_grad_norm_(m.parameters(), 1e30)
    return loss.detach(), norm


def bench_shape(name, B, T, V, S, iters, warmup, cpu_iters):
    import torch
    import wakeword
    from wakeword import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(23)
    feats_c = torch.randn((B, T, 80), generator=g)
    labels_c = torch.randint(1, V, (B, S), generator=g, dtype=torch.int64)
    il_c = torch.full((B,), T, dtype=torch.int64)
    tl_c = torch.full((B,), S, dtype=torch.int64)
    feats, labels, il, tl = (t.to(dev) for t in (feats_c, labels_c, il_c, tl_c))
    m_cpu = torch_module(V, 5)
    m_gpu = torch_module(V, 5).to(dev)
    wk = wakeword.CTCModel(m_cpu.state_dict(), V)
    lab32, il32, tl32 = labels.to(torch.int32), il.to(torch.int32), tl.to(torch.int32)
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    ws = torch.empty(L.wk_ctc_loss_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    nll, loss1 = torch.empty(B, device=dev), torch.empty(1, device=dev)
    grad = torch.empty((B, T, V), device=dev)
    state = {}

    def wk_step():
        loss, _, norm = wk.loss_and_grad(feats, lab32, il32, tl32)
        return loss, norm

    def wk_forward_train():
        state["lp"] = wk.forward_train(feats)
        return state["lp"], None

    def wk_loss():
        _lib.check(L.wk_ctc_loss(p(state["lp"]), B, T, V, p(lab32), S, p(il32), p(tl32), S, 2, 0, 1.0, p(ws), p(nll), p(loss1),
                                 p(grad), 0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "wk_ctc_loss")
        return loss1, None

    def wk_backward():
        flat, norm = wk.backward(grad, return_norm=True)
        return loss1, norm

    def torch_gpu():
        return torch_step(m_gpu, feats, labels, il, tl)

    fns = {"wk_step": wk_step, "wk_forward_train": wk_forward_train, "wk_loss": wk_loss, "wk_backward": wk_backward,
           "torch_gpu": torch_gpu}
    times = {k: [] for k in fns}
    values = {}
    for i in range(warmup + iters):
        for k, fn in fns.items():            # alternating passes
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out, norm = fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[k].append(e0.elapsed_time(e1))
            if norm is not None:
                values[k] = {"loss": float(out.reshape(-1)[0]), "grad_norm": float(norm)}
    res = {"shape": {"B": B, "T": T, "V": V, "S": S}, "iters": iters, "values": values,
           "ms_median": {k: statistics.median(v) for k, v in times.items()},
           "ms_min": {k: min(v) for k, v in times.items()}, "ms_max": {k: max(v) for k, v in times.items()}}

    torch.set_num_threads(16)
    cpu = []
    for i in range(1 + cpu_iters):
        t0 = time.perf_counter()
        out, norm = torch_step(m_cpu, feats_c, labels_c, il_c, tl_c)
        if i:
            cpu.append((time.perf_counter() - t0) * 1e3)
    res["ms_median"]["torch_cpu_16t"] = statistics.median(cpu)
    res["values"]["torch_cpu_16t"] = {"loss": float(out), "grad_norm": float(norm)}
    m = res["ms_median"]
    res["speedup_wk_step"] = {"vs_torch_gpu": m["torch_gpu"] / m["wk_step"], "vs_torch_cpu_16t": m["torch_cpu_16t"] / m["wk_step"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-iters", type=int, default=2)
    ap.add_argument("--shapes", default="reference,b64")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ctc_grad_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ctc_grad.py needs a HIP device")
    out = {"bench": "ctc_grad", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "shapes": {n: bench_shape(n, *SHAPES[n], a.iters, a.warmup, a.cpu_iters) for n in a.shapes.split(",")}}
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
