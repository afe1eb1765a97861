"""The inference CNN -- the CNN role of wk_fused_kernel and wk_cnn_fused_kernel in
fp32 (Winograd F(2,3)), bf16 and split bf16 -- against float64 (tests/cnn_ref.py),
on two weight sets and on batch sizes whose workgroups run ragged second and
third batches.

* wk_cnn (KWSModel.forward) at every cnn_ref.sizes_cnn(C) on N(0,1) features, and
  on wide and impulse features at 10C + 3 and 5: every clip compared;
* the fused wk_forward at every cnn_ref.sizes_fused(C), with and without the
  feature output (two kernel instantiations), against the reference applied to
  the features the device returned (the front-end has its own parity tests);
* bounds in units of the reference's own fp32 error (cnn_ref.check).  Measured
  on an MI355X (profiles/cnn_parity_bounds.md): fp32 <= 0.17 u (bound 8),
  bf16x3 <= 1.06 (bound 8), bf16 <= 0.9 % of clips above 8 u (cap 5 %) and
  <= 0.11 Q (cap 0.25);
* one-hot probe weights with which all three precisions are exact;
* bit-identity of a clip's logit across ragged multi-batch launches.
The int8 network (bit-exact against numpy, test_gpu_int8.py / test_gpu_quant.py),
wk_scan and the streaming path are not covered here."""
import functools
import hashlib

import pytest
import torch

import cnn_ref as R

pytestmark = pytest.mark.gpu

CNN_IDS = ("1", "2", "3", "4", "5", "7", "8", "9", "8C+1", "10C+3", "15C")
FUSED_IDS = ("4C+1", "5C+3", "6C+C/2", "9C+7")
SYNTH_SEED = 4242


@functools.lru_cache(maxsize=None)
def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def model(name, precision):
    from wakeword import KWSModel
    return KWSModel({k: v.numpy() for k, v in R.weight_set(name).items()}, precision=precision)


def probe_model(W, precision):
    from wakeword import KWSModel
    return KWSModel({k: v.numpy() for k, v in W.items()}, precision=precision)


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for f in (model, cnn_run, fused_big):
        f.cache_clear()
    _FEATS_REF.clear()


@functools.lru_cache(maxsize=None)
def cnn_run(name, precision, kind, B):
    n = R.sizes_cnn(n_cu())[-1] if kind == "normal" else R.sizes_cnn(n_cu())[-2]
    r = R.ref(name, kind, n)
    z = model(name, precision)(R.features(kind, r.n)[:B])
    assert tuple(z.shape) == (B, 1)
    return z[:, 0].cpu(), r


# ---- 1. wk_cnn against float64 ------------------------------------------------------
@pytest.mark.parametrize("size", range(len(CNN_IDS)), ids=CNN_IDS)
@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("name", R.WEIGHT_SETS)
def test_wk_cnn_normal_features(gpu, name, precision, size):
    B = R.sizes_cnn(n_cu())[size]
    z, r = cnn_run(name, precision, "normal", B)
    R.check(f"CNNPAR| wk_cnn {name} normal {CNN_IDS[size]}", precision, z, r, B)


@pytest.mark.parametrize("size", [9, 4], ids=["10C+3", "5"])
@pytest.mark.parametrize("kind", ["wide", "impulse"])
@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("name", R.WEIGHT_SETS)
def test_wk_cnn_wide_and_impulse_features(gpu, name, precision, kind, size):
    B = R.sizes_cnn(n_cu())[size]
    z, r = cnn_run(name, precision, kind, B)
    R.check(f"CNNPAR| wk_cnn {name} {kind} {CNN_IDS[size]}", precision, z, r, B)


# ---- 2. the fused kernel against float64 -----------------------------------------------
_FEATS_REF = {}


def feats_ref(name, feats):
    """The Ref of (weights, device features), computed once per content."""
    f = feats.cpu().contiguous()
    key = (name, hashlib.sha1(f.numpy().tobytes()).hexdigest())
    if key not in _FEATS_REF:
        _FEATS_REF[key] = R.Ref(R.weight_set(name), f)
    return _FEATS_REF[key]


@functools.lru_cache(maxsize=None)
def fused_big(name, precision):
    """The largest fused launch: (audio, logits with features, features, logits without)."""
    import wakeword
    B = R.sizes_fused(n_cu())[-1]
    x = wakeword.synth_clips(SYNTH_SEED, 0, B)
    m = model(name, precision)
    z, feats = m.detect(x, return_features=True)
    z2 = m.detect(x)
    m.check_device_errors()
    return x, z.cpu(), feats.cpu(), z2.cpu()


@pytest.mark.parametrize("size", range(len(FUSED_IDS)), ids=FUSED_IDS)
@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("name", R.WEIGHT_SETS)
def test_fused_against_float64_on_device_features(gpu, name, precision, size):
    B = R.sizes_fused(n_cu())[size]
    x, z, feats, z2 = fused_big(name, precision)
    if size < len(FUSED_IDS) - 1:
        m = model(name, precision)
        big_feats = feats
        z, feats = m.detect(x[:B], return_features=True)
        z2 = m.detect(x[:B])
        m.check_device_errors()
        z, feats, z2 = z.cpu(), feats.cpu(), z2.cpu()
        # a clip's features do not depend on the launch: the largest launch's reference serves
        r = feats_ref(name, big_feats) if torch.equal(feats, big_feats[:B]) else feats_ref(name, feats)
    else:
        r = feats_ref(name, feats)
    assert bool(torch.isfinite(feats).all()) and float(feats.abs().max()) <= 62 ** 0.5 + 1e-3
    tag = f"CNNPAR| fused {name} synth {FUSED_IDS[size]}"
    R.check(tag + " +feats", precision, z, r, B)
    R.check(tag + " product", precision, z2, r, B)


# ---- 4. the exact probe ---------------------------------------------------------------------
def probe_sizes():
    return (6, 4 * n_cu() + 5)


@pytest.mark.parametrize("j", range(4))
def test_probe_logits_are_the_same_in_every_precision(gpu, j):
    W = R.probe_set(j)
    models = {p: probe_model(W, p) for p in R.PRECISIONS}
    for B in probe_sizes():
        x = R.probe_features(B)
        h, z64, bound = R.probe_expect(x, W)
        got = {p: m(x)[:, 0].cpu() for p, m in models.items()}
        for p, z in got.items():
            e = (z.double() - z64).abs()
            print(f"probe {j} B={B} {p}: max e/bound = {float((e / bound).max()):.3f} (max|z|={float(z64.abs().max()):.1f})")
            assert bool((e <= bound).all()), (p, B, int((e > bound).sum()), float(e.max()))
        assert torch.equal(got["fp32"], got["bf16"]) and torch.equal(got["fp32"], got["bf16x3"])


@pytest.mark.parametrize("point", R.PROBE_POINTS, ids=[f"c{c}-t{t}" for c, t in R.PROBE_POINTS])
def test_probe_localises_one_input_element(gpu, point):
    """Clip 1 is zero but for a single 1 at (c, t); clip 2 is clip 3 with that 1
    added.  With classifier.0 / classifier.2 passing pooled channel ch through,
    the logits are relu(fp32(s fp32(1/7))) of the exact pooled sums s: equal bit
    for bit in every precision, and clip 1's is the impulse's own path."""
    c, t = point
    j, ch = R.probe_reach(c, t)
    W = R.probe_set(j, watch=ch)
    models = {p: probe_model(W, p) for p in R.PRECISIONS}
    for B in probe_sizes():
        x = R.probe_features(B)
        x[1] = R.impulse_clip(c, t)
        x[2] = x[3]
        x[2, c, t] += 1.0
        h, z64, _ = R.probe_expect(x, W)
        want = torch.relu(h[:, ch])
        assert torch.equal(want.double(), z64) and float(want[1]) > 0
        for p, m in models.items():
            z = m(x)[:, 0].cpu()
            bad = torch.nonzero(z != want).flatten()
            assert bad.numel() == 0, (p, B, (j, ch), bad[:8].tolist(), z[bad[:8]].tolist(), want[bad[:8]].tolist())


# ---- 5. bit-identity on ragged multi-batch launches -------------------------------------------
def sampled(C):
    """Eight clips of the 5C + 3 launch: first batches, the second batch's clips
    (fused: clips >= 4C), the tail."""
    return (0, 3, C - 1, C, 4 * C, 4 * C + 2, 5 * C, 5 * C + 2)


@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("name", R.WEIGHT_SETS)
def test_wk_cnn_logits_do_not_depend_on_the_launch(gpu, name, precision):
    C = n_cu()
    mid, big = R.sizes_fused(C)[1], R.sizes_fused(C)[3]
    x = R.features("normal", big).cuda()
    m = model(name, precision)
    z_big, z_mid = m(x)[:, 0], m(x[:mid])[:, 0]
    assert torch.equal(z_mid, z_big[:mid])
    for i in sampled(C):
        assert torch.equal(m(x[i:i + 1])[0, 0], z_mid[i]), i


@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("name", R.WEIGHT_SETS)
def test_fused_logits_do_not_depend_on_the_launch(gpu, name, precision):
    C = n_cu()
    mid = R.sizes_fused(C)[1]
    x, _, _, z2_big = fused_big(name, precision)
    m = model(name, precision)
    z_mid = m.detect(x[:mid]).cpu()
    assert torch.equal(z_mid, z2_big[:mid])
    for i in sampled(C):
        assert torch.equal(m.detect(x[i:i + 1]).cpu()[0], z_mid[i]), i
    m.check_device_errors()
