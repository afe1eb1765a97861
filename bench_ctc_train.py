"""GRU-CTC training-step benchmark (not the driver's bench.py line): one full
step of the loop of ctc.py:390-402 -- forward, CTC loss, backward,
clip_grad_norm_(5.0), Adam(lr=1e-3) -- as CTCTrainer.step, against the same
step in torch-ROCm on the same GPU in the same process, passes alternating, and
against torch-CPU on 16 threads.

Shapes, weights and inputs follow bench_ctc_grad.py: the reference's training
batch (B = 8, T = 801, V = 4000, S = 40) and B = 64; the torch module runs in
train mode with both dropouts at p = 0.  wk_step and torch_gpu really train,
each on its own copy of the same initial weights, one step per pass, so their
last losses are comparable; the optimiser-alone legs step a second handle.
Timings are medians over the timed passes (HIP events on the current stream):

  wk_step            CTCTrainer.step: loss_and_grad, then wk_ctc_adam_step with its norm;
  wk_loss_and_grad   CTCModel.loss_and_grad alone, on the trainer's handle: the yardstick --
                     wk_step minus this should lie within this leg's own min..max spread;
  wk_adam_step       wk_ctc_adam_step alone (Adam + the W_hh layouts), the norm passed;
  wk_adam_step_norm  the same with the norm computed by the call (one more launch);
  torch_gpu          zero_grad, forward, F.ctc_loss, backward, clip_grad_norm_, Adam.step.

Prints one JSON line and writes it to --out (profiles/ctc_train_bench.json).

--dropout P runs another measurement instead and leaves the one above alone:
CTCTrainer.step with both dropouts at P and with dropout off, on one handle
(the trainer's dropout switched between passes), passes alternating, both
really training; plus the no-dropout step's own min..max spread, which is
what the difference has to be read against.  It writes
profiles/ctc_dropout_bench.json (or --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [REPO, os.path.join(REPO, "esp32-wake-word_amd")]

from bench_ctc_grad import SHAPES, torch_module  # noqa: E402

MAX_NORM = 5.0


def torch_train_step(m, opt, feats, labels, il, tl):
    import torch
    import torch.nn.functional as F
    opt.zero_grad(set_to_none=True)
    lp = m(feats)
    loss = F.ctc_loss(lp.transpose(0, 1), labels, il, tl, blank=0, reduction="mean")
    loss.backward()
    norm = torch.nn.utils.clip_grad_norm_(m.parameters(), MAX_NORM)
    opt.step()
    return loss.detach(), norm


def bench_shape(name, B, T, V, S, iters, warmup, cpu_iters):
    import torch
    import wakeword
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(23)
    feats_c = torch.randn((B, T, 80), generator=g)
    labels_c = torch.randint(1, V, (B, S), generator=g, dtype=torch.int64)
    il_c = torch.full((B,), T, dtype=torch.int64)
    tl_c = torch.full((B,), S, dtype=torch.int64)
    feats, labels, il, tl = (t.to(dev) for t in (feats_c, labels_c, il_c, tl_c))
    m_cpu = torch_module(V, 5)
    m_gpu = torch_module(V, 5).to(dev)
    opt_cpu = torch.optim.Adam(m_cpu.parameters(), lr=1e-3)
    opt_gpu = torch.optim.Adam(m_gpu.parameters(), lr=1e-3)
    trainer = wakeword.CTCTrainer(m_cpu.state_dict(), V, max_norm=MAX_NORM)
    lab32, il32, tl32 = labels.to(torch.int32), il.to(torch.int32), tl.to(torch.int32)
    opt_only = wakeword.CTCTrainer(m_cpu.state_dict(), V, max_norm=MAX_NORM)   # the optimiser-alone legs: a handle of
    _, flat, norm0 = opt_only.grad(feats, lab32, il32, tl32)                   # their own, one gradient reused
    flat, norm0 = flat.clone(), norm0.clone()

    def wk_step():
        return trainer.step(feats, lab32, il32, tl32), trainer._last[1]

    def wk_loss_and_grad():
        loss, _, norm = trainer.model.loss_and_grad(feats, lab32, il32, tl32)
        return loss, norm

    def wk_adam_step():
        opt_only.apply(flat, norm0)
        return None, None

    def wk_adam_step_norm():
        opt_only.apply(flat, None)
        return None, None

    def torch_gpu():
        return torch_train_step(m_gpu, opt_gpu, feats, labels, il, tl)

    fns = {"wk_step": wk_step, "wk_loss_and_grad": wk_loss_and_grad, "wk_adam_step": wk_adam_step,
           "wk_adam_step_norm": wk_adam_step_norm, "torch_gpu": torch_gpu}
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
                values[k] = {"last_loss": float(out.reshape(-1)[0]), "last_grad_norm": float(norm)}
    res = {"shape": {"B": B, "T": T, "V": V, "S": S}, "iters": iters, "weights": trainer.model.num_weights(), "values": values,
           "ms_median": {k: statistics.median(v) for k, v in times.items()},
           "ms_min": {k: min(v) for k, v in times.items()}, "ms_max": {k: max(v) for k, v in times.items()}}

    torch.set_num_threads(16)
    cpu = []
    for i in range(1 + cpu_iters):
        t0 = time.perf_counter()
        out, norm = torch_train_step(m_cpu, opt_cpu, feats_c, labels_c, il_c, tl_c)
        if i:
            cpu.append((time.perf_counter() - t0) * 1e3)
    res["ms_median"]["torch_cpu_16t"] = statistics.median(cpu)
    m = res["ms_median"]
    res["step_minus_loss_and_grad_ms"] = m["wk_step"] - m["wk_loss_and_grad"]
    res["loss_and_grad_spread_ms"] = res["ms_max"]["wk_loss_and_grad"] - res["ms_min"]["wk_loss_and_grad"]
    res["speedup_wk_step"] = {"vs_torch_gpu": m["torch_gpu"] / m["wk_step"], "vs_torch_cpu_16t": m["torch_cpu_16t"] / m["wk_step"]}
    return res


def bench_dropout_shape(name, B, T, V, S, p, iters, warmup):
    import torch
    import wakeword
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(23)
    feats = torch.randn((B, T, 80), generator=g).to(dev)
    lab32 = torch.randint(1, V, (B, S), generator=g, dtype=torch.int64).to(dev, torch.int32)
    il32 = torch.full((B,), T, dtype=torch.int32, device=dev)
    tl32 = torch.full((B,), S, dtype=torch.int32, device=dev)
    trainer = wakeword.CTCTrainer(torch_module(V, 5).state_dict(), V, max_norm=MAX_NORM, seed=23)
    legs = {"wk_step": (0.0, 0.0), "wk_step_dropout": (p, p)}
    times = {k: [] for k in legs}
    values = {}
    for i in range(warmup + iters):
        for k, pair in legs.items():         # alternating passes on the one handle
            trainer.dropout = pair
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = trainer.step(feats, lab32, il32, tl32)
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[k].append(e0.elapsed_time(e1))
            values[k] = {"last_loss": float(loss), "last_grad_norm": float(trainer._last[1])}
    m0, m1 = trainer.model.dropout_masks()   # (of the last pass: the dropout leg's)
    rows = B * T
    res = {"shape": {"B": B, "T": T, "V": V, "S": S}, "iters": iters, "dropout": p, "values": values,
           "kept_share": {"enc": float(m0.float().mean()), "gru": float(m1.float().mean())},
           # forward: x0 read + written, y0 read, its dropped copy written; backward: both gradients read + written
           "mask_traffic_bytes": 4 * rows * (2 * 128 + 2 * 256) * 2,
           "ms_median": {k: statistics.median(v) for k, v in times.items()},
           "ms_min": {k: min(v) for k, v in times.items()}, "ms_max": {k: max(v) for k, v in times.items()}}
    res["dropout_minus_plain_ms"] = res["ms_median"]["wk_step_dropout"] - res["ms_median"]["wk_step"]
    res["plain_spread_ms"] = res["ms_max"]["wk_step"] - res["ms_min"]["wk_step"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-iters", type=int, default=2)
    ap.add_argument("--shapes", default="reference,b64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dropout", type=float, default=None, metavar="P",
                    help="time CTCTrainer.step with both dropouts at P against dropout off, on one handle")
    a = ap.parse_args()
    if a.dropout is not None and not 0.0 < a.dropout < 1.0:
        ap.error("--dropout takes a probability in (0, 1)")
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "ctc_dropout_bench.json" if a.dropout is not None else "ctc_train_bench.json")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ctc_train.py needs a HIP device")
    if a.dropout is not None:
        out = {"bench": "ctc_dropout", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
               "shapes": {n: bench_dropout_shape(n, *SHAPES[n], a.dropout, a.iters, a.warmup) for n in a.shapes.split(",")}}
    else:
        out = {"bench": "ctc_train", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
               "shapes": {n: bench_shape(n, *SHAPES[n], a.iters, a.warmup, a.cpu_iters) for n in a.shapes.split(",")}}
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
