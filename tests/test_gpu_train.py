"""GPU tests of the training step (wk_trainer_*, wakeword.train) against torch
autograd on the CPU.

The reference is a restatement of LightweightKWS(num_classes=1)
(ml_models/src/wakeModel.py:4-34) from torch.nn.functional ops, run in float64;
the same restatement in float32 is the yardstick of every tolerance: per tensor
e = max|g - g64| / max|g64| must satisfy e_gpu <= max(8 e_torch32, 16 * 2^-23)
(the factor 8 allows for another summation order of the same arithmetic; a
wrong tap, pool index or tail clip gives >= 1e-3).

ReLU and max-pool decisions are discrete, so clips whose reference
pre-activations sit within rounding of a tie or of zero are removed first,
by the reference alone (kept_clips)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KEYS = ("conv_layers.0.weight", "conv_layers.3.weight", "conv_layers.6.weight", "classifier.0.weight",
        "classifier.2.weight")
N_CAND = 2048
FLOOR = 16 * 2.0 ** -23
HYPER = dict(lr=5e-4, betas=(0.9, 0.99), eps=1e-7, weight_decay=1e-3)   # ml_models/main.py:16-22


def kws(x, W, pres=None):
    """LightweightKWS.forward -> logits (B,); appends the four decision layers'
    pre-activations to `pres` when given."""
    h = x
    for k in KEYS[:3]:
        pre = F.conv1d(h, W[k], padding=1)
        if pres is not None:
            pres.append(pre)
        h = F.max_pool1d(F.relu(pre), 2)
    pre = F.linear(h.mean(dim=2), W[KEYS[3]])
    if pres is not None:
        pres.append(pre)
    return F.linear(F.relu(pre), W[KEYS[4]])[:, 0]


def grads_of(x, y, W, dtype):
    """(loss, logits, {key: grad}) by torch-CPU autograd in `dtype`."""
    Wd = {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in W.items()}
    z = kws(x.to(dtype), Wd)
    loss = F.binary_cross_entropy_with_logits(z, y.to(dtype))
    g = torch.autograd.grad(loss, [Wd[k] for k in KEYS])
    return loss.detach(), z.detach(), dict(zip(KEYS, g))


def rel_err(a, ref):
    a, ref = torch.as_tensor(a).double().cpu(), ref.double()
    return float((a - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def weight_set(name):
    if name == "xiaoa":
        import os
        from wakeword.onnx_reader import read_onnx, xiaoa_state_dict
        inits, _, _ = read_onnx(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xiaoa.onnx"))
        sd = xiaoa_state_dict(inits)
    else:
        from wakeword.train import default_init
        sd = default_init(seed=11)
    return {k: np.ascontiguousarray(sd[k], np.float32) for k in KEYS}


@functools.lru_cache(maxsize=None)
def kept_clips(name):
    """Candidates whose every ReLU / pool decision has a margin of >= 64 x the
    largest fp32-vs-fp64 pre-activation difference of its layer."""
    gen = torch.Generator().manual_seed(2024)
    x = torch.randn(N_CAND, 13, 63, generator=gen)
    y = (torch.rand(N_CAND, generator=gen) < 0.5).float()
    W = weight_set(name)
    p32, p64 = [], []
    with torch.no_grad():
        kws(x, {k: torch.from_numpy(v) for k, v in W.items()}, p32)
        kws(x.double(), {k: torch.from_numpy(v).double() for k, v in W.items()}, p64)
    keep = torch.ones(N_CAND, dtype=torch.bool)
    for layer, (a32, a64) in enumerate(zip(p32, p64)):
        d = float((a32.double() - a64).abs().max())
        if layer < 3:
            n = a64.shape[2] // 2
            a, b = a64[:, :, 0:2 * n:2], a64[:, :, 1:2 * n:2]
            m = torch.maximum(a, b)
            margin = torch.where(m <= 0, m.abs(), torch.minimum(m, (a - b).abs())).flatten(1).min(dim=1).values
        else:
            margin = a64.abs().min(dim=1).values
        keep &= margin >= 64 * d
    idx = torch.nonzero(keep).flatten()
    print(f"near-tie filter [{name}]: kept {idx.numel()} of {N_CAND}")
    return x[idx].contiguous(), y[idx].contiguous()


@pytest.mark.parametrize("name", ["xiaoa", "default"])
def test_filter_keeps_at_least_half(gpu, name):
    x, _ = kept_clips(name)
    assert x.shape[0] >= N_CAND // 2, x.shape[0]


def check_against(tag, gpu_vals, ref, e32s):
    """gpu_vals / ref / e32s: name -> value; prints every figure, then asserts the bound."""
    bad = []
    for k in gpu_vals:
        e_gpu, bound = rel_err(gpu_vals[k], ref[k]), max(8 * e32s[k], FLOOR)
        print(f"{tag} {k}: e_gpu={e_gpu:.3e} e_torch32={e32s[k]:.3e} bound={bound:.3e}")
        if not e_gpu <= bound:
            bad.append((k, e_gpu, bound))
    assert not bad, bad


@pytest.mark.parametrize("B", [1, 5, 200, 1037])
@pytest.mark.parametrize("name", ["xiaoa", "default"])
def test_gradient_parity(gpu, name, B):
    from wakeword.train import Trainer
    x, y = kept_clips(name)
    assert x.shape[0] >= B
    x, y, W = x[:B], y[:B], weight_set(name)
    l64, z64, g64 = grads_of(x, y, W, torch.float64)
    l32, z32, g32 = grads_of(x, y, W, torch.float32)
    loss, logits, grads = Trainer(W).grad(x, y)
    ref = dict(g64, loss=l64, logits=z64)
    e32 = {k: rel_err(g32[k], g64[k]) for k in KEYS}
    e32.update(loss=rel_err(l32, l64), logits=rel_err(z32, z64))
    check_against(f"[{name} B={B}]", dict(grads, loss=loss, logits=logits), ref, e32)


def tie_case():
    """Integer features that are constant over runs of frames and weights that
    are multiples of 1/8: every conv sum is exact in fp32, neighbouring
    pre-activations tie exactly (also at positive values), and zeroed output
    channels give pre-activations of exactly 0."""
    gen = torch.Generator().manual_seed(7)
    runs = torch.randint(-2, 3, (6, 13, 16), generator=gen).float()
    x = runs.repeat_interleave(4, dim=2)[:, :, :63].contiguous()
    y = (torch.rand(6, generator=gen) < 0.5).float()
    W = {}
    for k, shape in zip(KEYS, ((32, 13, 3), (64, 32, 3), (128, 64, 3), (64, 128), (1, 64))):
        W[k] = (torch.randint(-2, 3, shape, generator=gen).float() / 8).numpy()
    for k in KEYS[:3]:
        W[k][::5] = 0.0
    return x, y, W


def test_tie_convention(gpu):
    from wakeword.train import Trainer
    x, y, W = tie_case()
    pres = []
    with torch.no_grad():
        kws(x, {k: torch.from_numpy(v) for k, v in W.items()}, pres)
    for pre in pres[:3]:   # the construction does what it says
        n = pre.shape[2] // 2
        a, b = pre[:, :, 0:2 * n:2], pre[:, :, 1:2 * n:2]
        assert int(((a == b) & (a > 0)).sum()) > 0 and int((pre == 0).sum()) > 0
    assert float(pres[3].abs().min()) > 1e-3   # classifier.0 is away from its own ReLU threshold
    l64, z64, g64 = grads_of(x, y, W, torch.float64)
    l32, z32, g32 = grads_of(x, y, W, torch.float32)
    loss, logits, grads = Trainer(W).grad(x, y)
    e32 = {k: rel_err(g32[k], g64[k]) for k in KEYS}
    check_against("[tie]", grads, g32, e32)


def test_determinism(gpu):
    from wakeword.train import Trainer
    x, y = kept_clips("default")
    x, y = x[:1037].cuda(), y[:1037].cuda()
    t = Trainer(weight_set("default"))
    l1, z1, g1 = t.grad(x, y)
    l2, z2, g2 = t.grad(x, y)
    assert torch.equal(l1, l2) and torch.equal(z1, z2)
    assert all(torch.equal(g1[k], g2[k]) for k in KEYS)


def test_adamw(gpu):
    from wakeword.train import Trainer
    from wakeword.api import pack_weights
    W = weight_set("xiaoa")
    w0 = torch.from_numpy(pack_weights(W))
    gen = torch.Generator().manual_seed(5)
    gs = [torch.randn(w0.numel(), generator=gen) * 10.0 ** -k for k in range(3)]
    lr, (b1, b2), eps, wd = HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"]
    # float64 restatement of the four formulas
    p, m, v = w0.double().clone(), torch.zeros_like(w0, dtype=torch.float64), torch.zeros_like(w0, dtype=torch.float64)
    p32 = w0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([p32], **HYPER)
    t = Trainer(W, **HYPER)
    for step, g in enumerate(gs, 1):
        g64 = g.double()
        p *= 1 - lr * wd
        m = b1 * m + (1 - b1) * g64
        v = b2 * v + (1 - b2) * g64 * g64
        p -= (lr / (1 - b1 ** step)) * m / (v.sqrt() / math.sqrt(1 - b2 ** step) + eps)
        p32.grad = g.clone()
        opt.step()
        t.apply(g)
        e_gpu = float((t.weights().cpu().double() - p).abs().max())
        e32 = float((p32.detach().double() - p).abs().max())
        bound = max(8 * e32, FLOOR * float(p.abs().max()))
        print(f"[adamw step {step}] e_gpu={e_gpu:.3e} e_torch32={e32:.3e} bound={bound:.3e}")
        assert e_gpu <= bound, (step, e_gpu, bound)


def torch_curve(x, y, W, dtype, steps):
    P = {k: torch.from_numpy(v).to(dtype).clone().requires_grad_(True) for k, v in W.items()}   # (a copy: the optimizer updates in place)
    opt = torch.optim.AdamW([P[k] for k in KEYS], **HYPER)
    out = []
    for _ in range(steps):
        loss = F.binary_cross_entropy_with_logits(kws(x.to(dtype), P), y.to(dtype))
        opt.zero_grad()
        loss.backward()
        opt.step()
        out.append(float(loss.detach()))
    return np.array(out)


def test_training_run(gpu):
    from wakeword.train import Trainer
    x, y = kept_clips("default")
    x, y, W = x[:64], y[:64], weight_set("default")
    c64, c32 = torch_curve(x, y, W, torch.float64, 20), torch_curve(x, y, W, torch.float32, 20)
    t = Trainer(W, **HYPER)
    xd, yd = x.cuda(), y.cuda()
    curve = np.array([float(t.step(xd, yd)) for _ in range(20)])
    c, gap = float(np.abs(c32 - c64).max()), float(np.abs(curve - c64).max())
    print(f"[train] loss {curve[0]:.6f} -> {curve[-1]:.6f}; c={c:.3e} gpu gap={gap:.3e} bound={max(8 * c, 1e-5):.3e}")
    assert curve[-1] < curve[0]
    assert gap <= max(8 * c, 1e-5), (gap, c)
    _, logits, _ = t.grad(xd, yd)
    fwd = t.to_model().forward(xd)[:, 0]
    d = float((fwd - logits).abs().max())
    print(f"[train] max|to_model().forward - trainer logits| = {d:.3e}")
    assert d < 1e-3


def test_train_model_surface(gpu):
    from wakeword import KWSModel, train_model
    x, y = kept_clips("default")
    loader = [(x[i * 16:(i + 1) * 16], y[i * 16:(i + 1) * 16]) for i in range(3)]
    losses, accuracies, model = train_model(loader, loader[:1], 2)
    assert len(losses) == 2 and len(accuracies) == 2 and isinstance(model, KWSModel)
    assert all(math.isfinite(v) and v > 0 for v in losses) and all(0 <= a <= 100 for a in accuracies)
    assert tuple(model.forward(x[:4]).shape) == (4, 1)
