"""The mode-B front-end, CMVN and the CNN behind them on degenerate audio --
digital silence, DC, full scale, a few LSBs, half-silent clips, an impulse
(tests/fe_cases.py) -- against float64, and wk_normalize against float64.

Bounds (fe_cases.Ref; none is fitted to the device's output):
  raw MFCC        max|dev - raw64| <= eps_raw = max(8 e_host, 16 2^-23 max|raw64|)
  CMVN'd          |df| <= eps_raw (2 + |f64|) / (s_k + 1e-8) + 2^-22 |f64| on rows with s_k >= eps_raw
  constant rows   exactly 0.0 (the reference's value in exact arithmetic: std == 0 -> 1, x - mean = 0)
  CNN             8 u, u = cnn_ref.Ref.unit32 (tests/test_gpu_cnn_parity.py)
  mode A          test_gpu_mode_a._tol
  wk_normalize    max|dev - ref64| <= max(8 e32, 16 2^-23) max|ref64| per tensor, e32 the same lines in numpy float32
  scan            test_gpu_scan.SAME_CODE_ATOL against wk_forward, the CMVN bound against the oracle
  bf16 logits     test_gpu_bf16.BF16_LOGIT_ATOL against fp32
Measured on an MI355X (profiles/fe_degenerate_bounds.md): raw <= 0.25 eps_raw,
CMVN'd <= 0.14 of its bound on every path, CNN 0.11 u, wk_normalize <= 0.31 of
its bound; before the kernels took rows of equal values as rows of zeros
(cmvn_row_is_flat, wk_fe_dev.h) silence scored logit -4.04 and 42 of the 106
constant rows of wk_normalize came out +-0.99.  Every test prints each figure
beside its bound before it asserts."""
import functools
import os

import numpy as np
import pytest

import cnn_ref as R
import fe_cases as F
from oracle import build_oracle as B
from oracle import wk_oracle as O
from test_gpu_bf16 import BF16_LOGIT_ATOL
from test_gpu_mode_a import _tol as mode_a_tol
from test_gpu_parity import _unfused_model
from test_gpu_scan import SAME_CODE_ATOL, WIN, _forward_strided, _windows

pytestmark = pytest.mark.gpu

SILENCE = F.NAMES.index("silence")
PATHS = ("fused", "unfused", "bf16")


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def models(gpu, golden_dir):
    import wakeword
    onnx = os.path.join(golden_dir, "xiaoa.onnx")
    m = {"fused": wakeword.load_onnx(onnx), "unfused": _unfused_model(golden_dir),
         "bf16": wakeword.load_onnx(onnx, precision="bf16")}
    yield m
    for v in m.values():
        v.check_device_errors()


class _Sub:
    """A Ref's per-clip figures at some indices (for _report)."""

    def __init__(self, r, idx):
        self.e_host, self.eps = r.e_host[idx], r.eps[idx]


def _report(tag, names, err, ratio, ref):
    """One line per clip: the measured error beside e_host, eps_raw and the ratio to the bound."""
    for i, name in enumerate(names):
        print(f"FEDEG| {tag} {name}: e_dev={err[i]:.3e} e_host={ref.e_host[i]:.3e} eps_raw={ref.eps[i]:.3e} "
              f"e_dev/bound={ratio[i]:.3f}")


# ---- 1. raw MFCC -------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f32", "i16"])
def test_raw_mfcc(gpu, form):
    import wakeword
    r = F.ref()
    names = F.NAMES if form == "f32" else F.INT16_NAMES
    idx = [F.NAMES.index(n) for n in names]
    x = np.stack([F.CASES[n] if form == "f32" else F.int16_form(n) for n in names])
    got = _np(wakeword.mfcc(x, cmvn=False))
    assert got.shape == (len(names), 13, 63) and np.isfinite(got).all()
    err = np.abs(got - r.raw64[idx]).max(axis=(1, 2))
    for j, i in enumerate(idx):
        print(f"FEDEG| raw {form} {F.NAMES[i]}: e_dev={err[j]:.3e} e_host={r.e_host[i]:.3e} eps_raw={r.eps[i]:.3e} "
              f"e_dev/bound={err[j] / r.eps[i]:.3f}")
    s = names.index("silence")
    print(f"FEDEG| raw {form} silence: device c0 = {got[s, 0, 0]!r} (host library {r.host_raw[SILENCE, 0, 0]!r})")
    bad = [(names[j], err[j], r.eps[i]) for j, i in enumerate(idx) if not err[j] <= r.eps[i]]
    assert not bad, bad
    # the reflected edge frames 0 and 62 run the same arithmetic as the interior
    assert np.array_equal(got[s], np.repeat(got[s][:, :1], 63, axis=1)), np.nonzero(got[s] != got[s][:, :1])
    if form == "i16":
        assert np.array_equal(got, _np(wakeword.mfcc(np.stack([F.CASES[n] for n in names]), cmvn=False)))


# ---- 2. CMVN'd features of the standalone front-end ----------------------------------
@pytest.mark.parametrize("form", ["f32", "i16"])
def test_cmvn_features(gpu, form):
    import wakeword
    r = F.ref()
    names = F.NAMES if form == "f32" else F.INT16_NAMES
    idx = [F.NAMES.index(n) for n in names]
    x = np.stack([F.CASES[n] if form == "f32" else F.int16_form(n) for n in names])
    got = np.zeros((len(F.NAMES), 13, 63), np.float32)
    got[idx] = _np(wakeword.mfcc(x))
    assert np.isfinite(got).all()
    err, ratio = r.cmvn_err(got), r.cmvn_ratio(got)
    _report(f"cmvn mfcc {form}", names, err[idx], ratio[idx], _Sub(r, idx))
    assert ratio[idx].max() <= 1.0, [(F.NAMES[i], ratio[i]) for i in idx if ratio[i] > 1.0]


# ---- 3. constant rows normalise to exactly 0.0 ---------------------------------------
def test_silence_gives_zero_features_and_zero_logit(models):
    import wakeword
    x = F.CASES["silence"]
    f = _np(wakeword.mfcc(x))
    print(f"FEDEG| zero mfcc(silence): max|f| = {np.abs(f).max():.3e}, rows not 0: "
          f"{sorted(set(np.nonzero(f)[1].tolist()))}")
    lg, ft = models["fused"].detect(x, return_features=True)
    lg, ft = _np(lg), _np(ft)
    print(f"FEDEG| zero detect(silence): max|f| = {np.abs(ft).max():.3e}, rows not 0: "
          f"{sorted(set(np.nonzero(ft)[1].tolist()))}, logit = {lg[0]!r}")
    assert not f.any()
    assert not ft.any()
    assert lg[0] == 0.0          # the network has no bias


CONST_VALUES = (1.0, 0.1, 1e-6, 3e4, 0.0)


@pytest.mark.parametrize("method", ["standardization", "cmvn"])
def test_wk_normalize_constant_rows_are_zero(gpu, method):
    import wakeword
    vals = np.concatenate([F.neighbours32(np.float32(-87.376984)), np.array(CONST_VALUES, np.float32)])
    assert vals.shape == (106,)
    x = np.repeat(vals[:, None], 63, axis=1)[None]
    got = _np(wakeword.normalize_mfcc(x, method))[0]
    bad = np.nonzero(got.any(axis=1))[0]
    print(f"FEDEG| zero wk_normalize {method}: {bad.size} of 106 constant rows are not 0"
          + (f" (max|f| = {np.abs(got).max():.3f}, first values {vals[bad[:4]].tolist()})" if bad.size else ""))
    assert bad.size == 0


# ---- 4. the three paths of wk_forward, one mixed batch -------------------------------
N_SYNTH = 5
SYNTH_AT = (1, 4, 8, 11, 15)        # where the ordinary clips sit among the 12 cases (B = 17)


@functools.lru_cache(maxsize=None)
def mixed():
    """(x [17][16000], names, Ref): the 12 cases with 5 synthetic clips between them."""
    synth = O.synth_clips(2718, 0, N_SYNTH)
    clips, names, c, s = [], [], 0, 0
    for i in range(len(F.NAMES) + N_SYNTH):
        if i in SYNTH_AT:
            clips.append(synth[s])
            names.append(f"synth{s}")
            s += 1
        else:
            clips.append(F.CASES[F.NAMES[c]])
            names.append(F.NAMES[c])
            c += 1
    x = np.stack(clips)
    assert x.shape == (17, F.N)
    return x, tuple(names), F.Ref(x)


_RUNS = {}


def _run_mixed(models, path):
    """(logits [17], features [17][13][63]) of the mixed batch through one path, run once."""
    if path not in _RUNS:
        x, _, _ = mixed()
        lg, ft = models[path].detect(x, return_features=True)
        _RUNS[path] = (_np(lg), _np(ft))
    return _RUNS[path]


@pytest.mark.parametrize("path", PATHS)
def test_paths_meet_the_cmvn_bound(models, path):
    x, names, r = mixed()
    lg, ft = _run_mixed(models, path)
    assert lg.shape == (17,) and ft.shape == (17, 13, 63)
    assert np.isfinite(lg).all() and np.isfinite(ft).all()
    err, ratio = r.cmvn_err(ft), r.cmvn_ratio(ft)
    _report(f"cmvn {path} B=17", names, err, ratio, r)
    left_out = [(names[i], k) for i, k in zip(*np.nonzero(~r.kept))]
    assert left_out == [("silence", k) for k in range(13)]
    assert ratio.max() <= 1.0, [(names[i], ratio[i]) for i in range(17) if ratio[i] > 1.0]
    s = names.index("silence")
    print(f"FEDEG| zero {path} B=17 silence: max|f| = {np.abs(ft[s]).max():.3e} logit = {lg[s]!r}")
    assert not ft[s].any() and lg[s] == 0.0
    if path == "bf16":
        l32, _ = _run_mixed(models, "fused")
        d = np.abs(lg - l32)
        print(f"FEDEG| bf16 logits vs fp32: max {d.max():.3e} (bound {BF16_LOGIT_ATOL})")
        assert d.max() <= BF16_LOGIT_ATOL
    else:
        ref_l = O.kws_forward(r.f64, models[path].state_dict())[:, 0]
        d = np.abs(lg - ref_l)
        print(f"FEDEG| {path} logits vs oracle end to end: max {d.max():.3e} at {names[int(d.argmax())]} (printed only: "
              f"the CNN is bounded on the device's own features)")


@pytest.mark.parametrize("path", PATHS)
def test_a_clip_does_not_depend_on_its_neighbours(models, path):
    """Each clip alone (B = 1) gives the bits it gave between a silent and a
    saturated neighbour: nothing leaks through the shared LDS rows."""
    x, names, _ = mixed()
    lg, ft = _run_mixed(models, path)
    for i, name in enumerate(names):
        l1, f1 = models[path].detect(x[i], return_features=True)
        assert np.array_equal(_np(f1)[0], ft[i]), (path, name)
        assert np.array_equal(_np(l1)[0], lg[i]), (path, name, _np(l1)[0], lg[i])


# ---- 5. the CNN on the features these inputs give --------------------------------------
def test_cnn_on_extreme_features(models):
    """|f| reaches 62 / sqrt(63) = 7.81 and a whole map is 0: the fp32 logit
    against float64 on the device's own features, in cnn_ref's units."""
    x, names, _ = mixed()
    lg, ft = _run_mixed(models, "fused")
    print(f"FEDEG| cnn features: max|f| = {np.abs(ft).max():.4f}, all-zero maps: {[names[i] for i in range(17) if not ft[i].any()]}")
    assert np.abs(ft).max() > 7.8
    import torch
    r = R.Ref(R.weight_set("xiaoa"), torch.from_numpy(ft))
    z64 = O.kws_forward(ft.astype(np.float64), models["fused"].state_dict())[:, 0]
    assert np.abs(z64 - r.z64.numpy()).max() <= 1e-9 * max(1.0, np.abs(z64).max())     # two float64 restatements agree
    R.check("FEDEG| cnn fused extreme", "fp32", lg, r)
    R.check("FEDEG| cnn wk_cnn extreme", "fp32", _np(models["fused"](ft))[:, 0], r)


# ---- 6. scan ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recording():
    rng = np.random.default_rng(1)
    a = 0.1 * rng.standard_normal(20000)
    b = 0.1 * rng.standard_normal(8000)
    return np.concatenate([a, np.zeros(20000), b]).astype(np.float32)


@pytest.mark.parametrize("hop", [256, 480])
def test_scan_over_a_silent_stretch(models, hop):
    model = models["fused"]
    x = recording()
    W = (x.size - WIN) // hop + 1
    lg, ft = model.scan(x, hop=hop, return_features=True)
    lg, ft = _np(lg), _np(ft)
    assert lg.shape == (W,) and ft.shape == (W, 13, 63) and np.isfinite(lg).all() and np.isfinite(ft).all()
    start = np.arange(W) * hop
    silent = (start >= 20000) & (start + WIN <= 40000)
    assert silent.sum() == (15 if hop == 256 else 9)
    print(f"FEDEG| scan hop {hop}: {int(silent.sum())} silent windows, max|f| = {np.abs(ft[silent]).max():.3e}, "
          f"max|logit| = {np.abs(lg[silent]).max():.3e}")
    assert not ft[silent].any() and not lg[silent].any()
    lf, ff = _forward_strided(model, x, hop, W)
    sf, sl = np.abs(ft - ff).max(axis=(1, 2)), np.abs(lg - lf)
    print(f"FEDEG| scan hop {hop} vs wk_forward: feat {sf.max():.3e} (window {int(sf.argmax())}) logit {sl.max():.3e} "
          f"(bound {SAME_CODE_ATOL})")
    assert sf.max() < SAME_CODE_ATOL and sl.max() < SAME_CODE_ATOL
    r = F.Ref(_windows(x, hop, W))
    # no row is left out but those of the silent windows
    assert np.array_equal(~r.kept.all(axis=1), silent) and not r.kept[silent].any()
    ratio, err = r.cmvn_ratio(ft), r.cmvn_err(ft)
    partly = ~silent & np.array([not w.all() for w in _windows(x, hop, W)])
    i = int(ratio.argmax())
    print(f"FEDEG| scan hop {hop} cmvn: {int(partly.sum())} partly silent windows, worst window {i} (start {start[i]}): "
          f"e_dev={err[i]:.3e} e_host={r.e_host[i]:.3e} eps_raw={r.eps[i]:.3e} e_dev/bound={ratio[i]:.3f}")
    assert partly.sum() > 40 and ratio.max() <= 1.0, (i, ratio[i])


# ---- 7. mode A ---------------------------------------------------------------------------
@pytest.mark.parametrize("pack", [True, False])
def test_mode_a_degenerate(gpu, pack):
    import wakeword
    names = ("silence", "dc1", "fullscale_sq", "int16_min")
    xf = np.stack([F.CASES[n] for n in names[:3]])
    got = list(_np(wakeword.mfcc(xf, mode="esp", esp_dsp_packing=pack)))
    got.append(_np(wakeword.mfcc(F.int16_form("int16_min")[None], mode="esp", esp_dsp_packing=pack))[0])
    for name, g in zip(names, got):
        ref = B.esp_mfcc(F.CASES[name], pack)
        assert g.shape == ref.shape == (62, 13) and np.isfinite(g).all(), name
        e = np.abs(g - ref).max()
        print(f"FEDEG| mode A pack={int(pack)} {name}: e_dev={e:.3e} tol={mode_a_tol(ref):.3e} max|ref|={np.abs(ref).max():.2f}")
        assert e <= mode_a_tol(ref), name
    assert np.array_equal(got[0], np.repeat(got[0][:1], 62, axis=0))      # silence: every frame the same bits


# ---- 8. wk_normalize against float64 -------------------------------------------------------
NORM_SHAPES = ((1, 13, 63), (1, 1, 2), (2, 3, 64), (1, 5, 65), (3, 2, 200), (1, 7, 63))   # 7 rows: not a multiple of 4
NORM_INPUTS = ((1.0, 0.0), (1.0, 100.0), (1e-3, -87.0))


def _norm32(m, method):
    """O.normalize_mfcc's lines in numpy float32."""
    m = np.asarray(m, np.float32)
    if method in ("standardization", "cmvn"):
        mean = m.mean(axis=-1, keepdims=True, dtype=np.float32)
        std = m.std(axis=-1, ddof=1, keepdims=True, dtype=np.float32)
        std = np.where(std == 0, np.float32(1.0), std)
        return (m - mean) / (std + np.float32(1e-8))
    if method == "minmax":
        mn, mx = m.min(axis=-1, keepdims=True), m.max(axis=-1, keepdims=True)
        return (m - mn) / (mx - mn + np.float32(1e-8))
    return m


@pytest.mark.parametrize("method", ["standardization", "cmvn", "minmax", "no_such_method"])
def test_wk_normalize_parity(gpu, method):
    """Every shape and input at once per method.  A tensor's last row is
    constant (the only row of (1, 1, 2) in a second tensor): it must come out
    exactly 0 (bit-equal to the input for the pass-through), and stays out of
    the yardstick, where numpy's own fp32 mean would make it +-0.99."""
    import wakeword
    bad = []
    for si, shape in enumerate(NORM_SHAPES):
        rows = shape[0] * shape[1]
        for ii, (scale, offset) in enumerate(NORM_INPUTS):
            rng = np.random.default_rng(1000 + 10 * si + ii)
            x = (rng.standard_normal(shape) * scale + offset).astype(np.float32)
            tensors = [x]
            if rows > 1:
                x.reshape(rows, -1)[-1] = x.reshape(rows, -1)[-1, 0]
            else:
                tensors.append(np.full(shape, np.float32(offset + scale), np.float32))
            for t, xt in enumerate(tensors):
                got = _np(wakeword.normalize_mfcc(xt, method))
                assert got.shape == shape and np.isfinite(got).all()
                if method == "no_such_method":
                    assert np.array_equal(got.view(np.uint32), xt.view(np.uint32)), (shape, scale, offset)
                    continue
                const = got.reshape(rows, -1)[-1] if (rows > 1 or t == 1) else None
                if const is not None and const.any():
                    bad.append((shape, scale, offset, "constant row", float(np.abs(const).max())))
                if rows == 1 and t == 1:
                    continue
                keep = slice(0, rows - 1) if rows > 1 else slice(0, 1)
                ref = O.normalize_mfcc(xt, method).reshape(rows, -1)[keep]
                scale_ref = np.abs(ref).max()
                e_dev = np.abs(got.reshape(rows, -1)[keep] - ref).max() / scale_ref
                e32 = np.abs(_norm32(xt, method).reshape(rows, -1)[keep] - ref).max() / scale_ref
                bound = max(F.K_ORDER * e32, F.FLOOR)
                print(f"FEDEG| wk_normalize {method} {shape} scale={scale} offset={offset}: e_dev={e_dev:.3e} "
                      f"e32={e32:.3e} bound={bound:.3e} e_dev/bound={e_dev / bound:.3f}")
                if not e_dev <= bound:
                    bad.append((shape, scale, offset, e_dev, bound))
    assert not bad, bad
