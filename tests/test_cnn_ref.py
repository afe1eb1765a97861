"""CPU tests of tests/cnn_ref.py, the references of tests/test_gpu_cnn_parity.py:
forward64 against the oracle and the golden logits, the bf16 grid rounding
against torch's bf16 bit for bit, the caps of the bf16 bound from the reference
alone, the mutations each bound must see, and the exact probe's construction."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_ref as R
from oracle import wk_oracle as O

C_MI355X = 256                       # CUs: the GPU test's largest batch is 15 C clips
N_MAX = R.sizes_cnn(C_MI355X)[-1]
N_MUT = 1024


def test_sizes_reach_the_tails_they_are_chosen_for():
    """The launch arithmetic of launch_fused / launch_cnn_fused restated: which
    (batch index, nv) pairs a size produces."""
    C = C_MI355X

    def tails(n_mine):
        return {(b, min(4, n - 4 * b)) for n in n_mine for b in range((n + 3) // 4)}

    def fused(B):
        grid = min(B, C)
        return tails([(B - 1 - w) // grid + 1 for w in range(grid)])

    def cnn(B):
        roles = (B + 3) // 4
        grid = min((roles + 1) // 2, C)
        return [(B - 1 - r) // (2 * grid) + 1 if B > r else 0 for r in range(2 * grid)]

    f = [fused(B) for B in R.sizes_fused(C)]
    assert (1, 1) in f[0] and {(1, 1), (1, 2)} <= f[1] and {(1, 2), (1, 3)} <= f[2] and {(2, 1), (2, 2)} <= f[3]
    assert all((0, 4) in s for s in f)
    c = {B: cnn(B) for B in R.sizes_cnn(C)}
    assert c[1] == [1, 0] and c[4] == [2, 2] and c[9] == [3, 2, 2, 2]
    assert all(max(c[B]) <= 4 for B in (1, 2, 3, 4, 5, 7, 8, 9))
    second = set()
    for B in R.sizes_cnn(C)[-3:]:
        second |= {nv for b, nv in tails(c[B]) if b == 1}
    assert second == {1, 2, 3, 4}


def test_forward64_is_the_oracle_and_the_golden_logits(golden_dir):
    W = R.weight_set("xiaoa")
    x = R.features("normal", 64)
    sd = {k: v.numpy() for k, v in W.items()}
    want = torch.from_numpy(np.asarray(O.kws_forward(x.double().numpy(), sd), np.float64)[:, 0])
    assert float((R.forward64(x, W) - want).abs().max()) < 1e-12
    g = np.load(os.path.join(golden_dir, "synth.npz"))
    feats, logits = torch.from_numpy(g["feats"]), torch.from_numpy(g["logits"]).double().reshape(-1)
    r = R.Ref(W, feats)
    e = float((r.z64 - logits).abs().max())
    print(f"golden synth.npz: max|z64 - logits| = {e:.3e}, unit32 = {r.unit32():.3e}")
    assert e <= R.K_ORDER * r.unit32()      # the golden logits are another fp32 evaluation (the torch module's)


def test_the_three_convolutions_agree_in_float64():
    x = R.features("wide", 16).double()
    for name in R.WEIGHT_SETS:
        W = {k: v.double() for k, v in R.weight_set(name).items()}
        a = R.network(x, W, R.conv_conv1d)
        for conv in (R.conv_taps, R.conv_wino):
            assert float((R.network(x, W, conv) - a).abs().max()) <= 1e-13 * max(1.0, float(a.abs().max()))


def test_bf16_grid_is_torchs_bf16_bit_for_bit():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-30, 30, (1 << 16,), generator=g).float())
    bits = torch.randint(0x1000, 0x7000, (4096,), generator=g, dtype=torch.int32)
    ties = ((bits << 16) | 0x8000).view(torch.float32)          # exactly half way between two bf16 values
    edge = torch.tensor([0.0, -0.0, 1.0, -1.0, 255.5, 1.99609375, 1.998046875, 3.3895314e38 / 2])
    for v in (x, ties, -ties, edge):
        want = v.bfloat16().float()
        assert torch.equal(R.bf16_grid(v.double()).float().view(torch.int32), want.view(torch.int32))
        assert torch.equal(R.bf16_grid(v).view(torch.int32), want.view(torch.int32))
        h, lo = R.split_bf16(v, R.bf16_torch)
        h64, lo64 = R.split_bf16(v.double(), R.bf16_grid)
        assert torch.equal(h64.float(), h) and torch.equal(lo64.float(), lo)
    # the mutant rounding differs, and only downward in magnitude
    t = R.bf16_trunc(x.double())
    assert bool((t.abs() <= x.double().abs()).all()) and not torch.equal(t, R.bf16_grid(x.double()))


@pytest.mark.parametrize("kind", ["normal", "wide"])
@pytest.mark.parametrize("name", R.WEIGHT_SETS)
def test_reference_alone_stays_inside_the_bf16_caps(name, kind):
    """At the GPU test's largest batch, every summation order of the fp32
    emulation against the float64 emulation: at most 5 % of the clips above
    8 unit32, none above 0.25 Q.  (Measured with other seeds: <= 1.8 %, <= 0.10 Q.)"""
    n = N_MAX if kind == "normal" else R.sizes_cnn(C_MI355X)[-2]
    r = R.ref(name, kind, n)
    u, Q = r.unit32(), r.q()
    for conv, e in r.eb32.items():
        share, ratio = float((e > R.K_ORDER * u).double().mean()), float(e.max()) / Q
        print(f"[{name} {kind} n={r.n}] bf16 fp32-emulation ({conv}): share(>8u)={share:.4f} max/Q={ratio:.3f} "
              f"median={float(e.median()):.2e} u={u:.3e} Q={Q:.3e}")
        assert share <= R.SHARE_CAP and ratio <= R.Q_CAP
    e3 = max(float(v.max()) for v in r.e3_32.values())
    print(f"[{name} {kind}] bf16x3 fp32-emulation vs float64 emulation: max {e3:.3e} = {e3 / u:.2f} u; "
          f"split vs float64: {float((r.z3_64 - r.z64).abs().max()):.3e}")
    # the 1024-clip prefix too (Q of the small batches)
    assert all(float(e[:R.Q_SET].max()) <= R.Q_CAP * r.q(1) for e in r.eb32.values())


# ---- mutants ---------------------------------------------------------------------
def _swap(layer):
    def conv(h, w):
        w = w.clone()
        w[17, [5, 6], 2] = w[17, [6, 5], 2]
        return R.conv_conv1d(h, w)
    return conv if layer == 2 else R.conv_conv1d


def _stale_pad(layer):
    def conv(h, w):     # the left pad row holds the last row of another clip
        hp = torch.cat([h.roll(1, 0)[:, :, -1:], h, torch.zeros_like(h[:, :, :1])], 2)
        return F.conv1d(hp, w)
    return conv if layer == 1 else R.conv_conv1d


def _no_frame_62(layer):
    def conv(h, w):
        h = h.clone()
        h[:, :, 62] = 0
        return R.conv_conv1d(h, w)
    return conv if layer == 0 else R.conv_conv1d


def _gap_to_14(y):
    """t <= 14 of the even columns instead of t <= 12: an eighth window (14, the pad)."""
    return (F.max_pool1d(y, 2).sum(dim=2) + y[:, :, 14]) / 7.0


FP32_MUTANTS = {"one-channel tap swap": dict(conv_of=_swap), "stale left pad in conv2": dict(conv_of=_stale_pad),
                "frame 62 ignored": dict(conv_of=_no_frame_62), "pooling over t <= 14": dict(gap_fn=_gap_to_14)}


@pytest.mark.parametrize("name", R.WEIGHT_SETS)
def test_mutants_break_their_bounds_tenfold(name):
    W = R.weight_set(name)
    x = R.features("normal", N_MUT)
    r = R.ref(name, "normal", N_MUT)
    assert r.n == N_MUT
    u, u3, Q = r.unit32(), r.unit3(), r.q()
    x64 = x.double()
    with torch.no_grad():
        for tag, kw in FP32_MUTANTS.items():
            e = (R.network(x64, W, **kw) - r.z64).abs()
            eb = (R.network(x64, W, rnd=R.bf16_grid, **kw) - r.zb64).abs()
            e3 = (R.network(x64, W, rnd=R.bf16_grid, split=True, **kw) - r.z3_64).abs()
            share = float((eb > R.K_ORDER * u).double().mean())
            print(f"[{name}] {tag}: fp32 max={float(e.max()):.3e} median={float(e.median()):.3e} = "
                  f"{float(e.max()) / (R.K_ORDER * u):.0f} x bound; bf16x3 {float(e3.max()) / (R.K_ORDER * u3):.0f} x bound; "
                  f"bf16 share(>8u)={share:.3f} max/Q={float(eb.max()) / Q:.2f}")
            x32, x3 = float(e.max()) / (R.K_ORDER * u), float(e3.max()) / (R.K_ORDER * u3)
            xb = max(share / R.SHARE_CAP, float(eb.max()) / (R.Q_CAP * Q))
            assert x32 > 1 and x3 > 1 and xb > 1               # seen in every precision
            assert max(x32, xb) >= 10 and max(x3, xb) >= 10, (tag, x32, x3, xb)
            if tag == "one-channel tap swap" and name == "xiaoa":
                assert 0.5e-3 <= float(e.max()) <= 2e-3     # at the old absolute tolerance of 1e-3
        e = (R.network(x64, W, rnd=R.bf16_trunc) - r.zb64).abs()
        share = float((e > R.K_ORDER * u).double().mean())
        print(f"[{name}] bf16 truncation: max/Q={float(e.max()) / Q:.2f} share(>8u)={share:.3f}")
        assert share >= 10 * R.SHARE_CAP and float(e.max()) >= 10 * R.Q_CAP * Q
        for layer in range(3):
            e = (R.network(x64, W, rnd=R.bf16_grid, split=True, drop=layer) - r.z3_64).abs()
            print(f"[{name}] bf16x3 without xl wh in conv{layer + 1}: max={float(e.max()):.3e} = "
                  f"{float(e.max()) / (R.K_ORDER * u3):.0f} x bound")
            assert float(e.max()) >= 10 * R.K_ORDER * u3


# ---- the exact probe ---------------------------------------------------------------
def test_probe_sets_cover_every_ci_tap_and_co():
    for layer, (cout, cin) in enumerate(R.PROBE_SHAPES):
        used_ci, used_tap = set(), set()
        for j in range(4):
            w = R.probe_set(j)[R.KEYS[layer]]
            assert tuple(w.shape) == (cout, cin, 3)
            nz = torch.nonzero(w)
            assert nz.shape[0] == cout and sorted(nz[:, 0].tolist()) == list(range(cout))   # one-hot per co
            assert set(w[w != 0].abs().tolist()) <= {1.0, 0.5}
            used_ci |= set(nz[:, 1].tolist())
            used_tap |= set(nz[:, 2].tolist())
            if layer:
                assert set(nz[:, 1].tolist()) == set(range(cin))
        assert used_ci == set(range(cin)) and used_tap == {0, 1, 2}
    sel = set()
    for j in range(4):
        W = R.probe_set(j)
        f1, f2 = W[R.KEYS[3]], W[R.KEYS[4]]
        assert bool((f1.sum(dim=1) == 1).all()) and set(f1.unique().tolist()) == {0.0, 1.0}
        assert bool((torch.frexp(f2.abs())[0] == 0.5).all()) and bool((f2 < 0).any()) and bool((f2 > 0).any())
        sel |= set(torch.nonzero(f1)[:, 1].tolist())
    assert sel == set(range(128))


@pytest.mark.parametrize("j", range(4))
def test_probe_is_exact_in_every_arithmetic(j):
    """The construction does what it says: the pooled sums of the fp32 direct
    form, the fp32 Winograd restatement and both bf16 emulations equal the
    float64 ones bit for bit, xl = 0, and most pooled channels are alive."""
    W, x = R.probe_set(j), R.probe_features(12)
    s = R.probe_pooled(x, W)

    def pooled(**kw):
        seen = []

        def tap(y):
            seen.append(F.max_pool1d(y, 2).sum(dim=2))
            return seen[0]
        with torch.no_grad():
            R.network(x, W, gap_fn=tap, **kw)
        return seen[0].double()
    for kw in (dict(conv=R.conv_conv1d), dict(conv=R.conv_wino), dict(rnd=R.bf16_torch),
               dict(rnd=R.bf16_torch, split=True), dict(rnd=R.bf16_torch, split=True, drop=1)):
        assert torch.equal(pooled(**kw), s), kw
    assert float((s != 0).double().mean()) > 0.25
    h, z, bound = R.probe_expect(x, W)
    assert bool((z.abs() > 0).all()) and bool((bound < 1e-3 * z.abs().max()).all())
    # watch mode: the logit is the watched channel's relu(h) itself
    ch = int(torch.nonzero(s[0])[0])
    h, z, _ = R.probe_expect(x, R.probe_set(j, watch=ch))
    assert torch.equal(z, torch.relu(h[:, ch]).double())


def test_probe_points_reach_one_pooled_channel():
    for c, t in R.PROBE_POINTS:
        got = R.probe_reach(c, t)
        assert got is not None, (c, t)
        j, ch = got
        s = R.probe_pooled(R.impulse_clip(c, t)[None], R.probe_set(j))[0]
        print(f"impulse at (c={c}, t={t}): probe set {j}, pooled channel {ch}, s={float(s[ch])}")
        assert float(s[ch]) > 0
