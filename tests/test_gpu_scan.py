"""GPU tests of wk_scan / KWSModel.scan: every window of a recording scored as
wk_forward scores the clip starting there, with the interior MFCC frames
computed once per recording when hop is a multiple of 256.

Tolerances are the project's own: features 5e-4 and logits 1e-3 against the
float64 oracle (test_gpu_parity.py), 5e-5 between two compilations of the same
device front-end code (test_fused_matches_unfused_and_oracle), bf16 0.05 and
split bf16 1e-3 against fp32 (test_gpu_bf16.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import wk_oracle as O

pytestmark = pytest.mark.gpu

FEAT_ATOL = 5e-4
LOGIT_ATOL = 1e-3
SAME_CODE_ATOL = 5e-5
WIN = 16000

INVALID, UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def model(gpu, golden_dir):
    import wakeword
    return wakeword.load_onnx(os.path.join(golden_dir, "xiaoa.onnx"))


def _noise(n, seed):
    return (np.random.default_rng(seed).standard_normal(n) * 0.1).astype(np.float32)


def _windows(x, hop, W):
    return np.stack([x[w * hop:w * hop + WIN] for w in range(W)])


def _oracle(model, x, hop, W):
    f = O.features_mode_b(_windows(x, hop, W))
    return f, O.kws_forward(f, model.state_dict())[:, 0]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def _forward_strided(model, x, hop, W):
    """wk_forward with clip_stride = hop over one recording: what the library offered before wk_scan."""
    import torch
    from wakeword import _lib
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    lg = torch.empty((W,), dtype=torch.float32, device="cuda")
    ft = torch.empty((W, 13, 63), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wk_forward(model._h.h, _ptr(xd), _lib.WK_DTYPE_F32, W, WIN, hop, _ptr(lg), _ptr(ft),
                                     _stream(torch)), "wk_forward")
    return lg.cpu().numpy(), ft.cpu().numpy()


def _workspace_bytes(n_rec, n, hop, wpc=0):
    from wakeword import _lib
    b = C.c_size_t(0)
    _lib.check(_lib.lib().wk_scan_workspace_bytes(n_rec, n, hop, wpc, C.byref(b)), "wk_scan_workspace_bytes")
    return b.value


def _scan_raw(model, buf, n_rec, n, rec_stride, hop, ws_bytes, want_feats=True, dtype=None):
    """wk_scan through the C ABI on a flat device buffer; returns (status, logits, feats)."""
    import torch
    from wakeword import _lib
    W = (n - WIN) // hop + 1 if n >= WIN else 0
    lg = torch.full((n_rec, W), float("nan"), dtype=torch.float32, device="cuda")
    ft = torch.full((n_rec, W, 13, 63), float("nan"), dtype=torch.float32, device="cuda") if want_feats else None
    ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device="cuda")
    if dtype is None:
        dtype = _lib.WK_DTYPE_I16 if buf.dtype == torch.int16 else _lib.WK_DTYPE_F32
    st = _lib.lib().wk_scan(model._h.h, _ptr(buf), dtype, n_rec, n, rec_stride, hop, _ptr(lg), _ptr(ft),
                            _ptr(ws) if ws_bytes else None, ws_bytes, _stream(torch))
    torch.cuda.synchronize()
    return st, lg.cpu().numpy(), (ft.cpu().numpy() if ft is not None else None)


def test_single_window(model):
    x = _noise(WIN, 1)
    lg, ft = model.scan(x, hop=256, return_features=True)
    assert tuple(lg.shape) == (1,) and tuple(ft.shape) == (1, 13, 63)
    lg, ft = lg.cpu().numpy(), ft.cpu().numpy()
    ld, fd = model.detect(x, return_features=True)
    ef, el = np.abs(ft - fd.cpu().numpy()).max(), np.abs(lg - ld.cpu().numpy()).max()
    rf, rl = _oracle(model, x, 256, 1)
    of, ol = np.abs(ft - rf).max(), np.abs(lg - rl).max()
    print(f"single window: vs detect feat {ef:.2e} logit {el:.2e}; vs oracle feat {of:.2e} logit {ol:.2e}")
    assert ef < SAME_CODE_ATOL and el < SAME_CODE_ATOL
    assert of < FEAT_ATOL and ol < LOGIT_ATOL


# G = k (W - 1) + 61 = 62, 63, 64, 130, 69, 157: below, at and above the 63-frame work unit
@pytest.mark.parametrize("hop,W", [(256, 2), (256, 3), (256, 4), (256, 70), (512, 5), (768, 33)])
def test_geometry(model, hop, W):
    n = WIN + hop * (W - 1) + 100          # 100 trailing samples complete no window
    x = _noise(n, 100 + W)
    lg, ft = model.scan(x, hop=hop, return_features=True)
    assert tuple(lg.shape) == (W,) and tuple(ft.shape) == (W, 13, 63)
    lg, ft = lg.cpu().numpy(), ft.cpu().numpy()
    rf, rl = _oracle(model, x, hop, W)
    lf, ff = _forward_strided(model, x, hop, W)
    of, ol = np.abs(ft - rf).max(axis=(1, 2)), np.abs(lg - rl)
    sf, sl = np.abs(ft - ff).max(axis=(1, 2)), np.abs(lg - lf)
    print(f"hop {hop} W {W}: vs oracle feat {of.max():.2e} logit {ol.max():.2e}; "
          f"vs wk_forward feat {sf.max():.2e} logit {sl.max():.2e}")
    assert np.isfinite(lg).all() and np.isfinite(ft).all()
    assert of.max() < FEAT_ATOL, (int(of.argmax()), of.max())
    assert ol.max() < LOGIT_ATOL, (int(ol.argmax()), ol.max())
    assert sf.max() < SAME_CODE_ATOL, (int(sf.argmax()), sf.max())
    assert sl.max() < SAME_CODE_ATOL, (int(sl.argmax()), sl.max())


def test_batch_isolation(model, gpu):
    """Three recordings 777 samples apart with 1e3 between them: nothing may read the padding."""
    torch = gpu
    hop, W, R = 256, 6, 3
    n = WIN + hop * (W - 1)                # the last window ends on the recording's last sample
    stride = n + 777
    recs = [_noise(n, 200 + r) for r in range(R)]
    host = np.full(R * stride, 1e3, np.float32)
    for r in range(R):
        host[r * stride:r * stride + n] = recs[r]
    buf = torch.from_numpy(host).cuda()
    st, lg, ft = _scan_raw(model, buf, R, n, stride, hop, _workspace_bytes(R, n, hop))
    assert st == 0
    for r in range(R):
        l1, f1 = model.scan(recs[r], hop=hop, return_features=True)
        assert np.array_equal(lg[r], l1.cpu().numpy()), r
        assert np.array_equal(ft[r], f1.cpu().numpy()), r
    # the (R, n) form of the Python call is the same batch, densely packed
    l2 = model.scan(np.stack(recs), hop=hop)
    assert tuple(l2.shape) == (R, W) and np.array_equal(l2.cpu().numpy(), lg)


def test_batch_isolation_int16_odd_stride(model, gpu):
    """The same with int16 audio and an odd stride: recording 1 starts on a 2-byte boundary."""
    torch = gpu
    hop, W, R = 256, 6, 3
    n = WIN + hop * (W - 1)
    stride = n + 777
    rng = np.random.default_rng(210)
    recs = [(rng.standard_normal(n) * 3000).clip(-32768, 32767).astype(np.int16) for _ in range(R)]
    host = np.full(R * stride, 32767, np.int16)
    for r in range(R):
        host[r * stride:r * stride + n] = recs[r]
    buf = torch.from_numpy(host).cuda()
    st, lg, ft = _scan_raw(model, buf, R, n, stride, hop, _workspace_bytes(R, n, hop))
    assert st == 0
    for r in range(R):
        l1, f1 = model.scan(recs[r], hop=hop, return_features=True)
        assert np.array_equal(lg[r], l1.cpu().numpy()), r
        assert np.array_equal(ft[r], f1.cpu().numpy()), r
    rf, rl = _oracle(model, recs[1].astype(np.float64) / 32768.0, hop, W)
    assert np.abs(ft[1] - rf).max() < FEAT_ATOL and np.abs(lg[1] - rl).max() < LOGIT_ATOL


def test_golden_pin(model, golden_dir):
    """The reference's own LightweightKWS logits of the eight golden windows, found
    again inside a long recording at every hop that lands on them."""
    g = np.load(os.path.join(golden_dir, "wavs.npz"))
    xs, ref = g["x_noise"], g["logit_noise"]
    gap = 17 * 1024
    offs = [1024 + i * gap for i in range(len(xs))]
    rec = _noise(offs[-1] + WIN + 2048, 7)
    for o, x in zip(offs, xs):
        rec[o:o + WIN] = x
    for hop in (256, 512, 1024):
        lg = model.scan(rec, hop=hop).cpu().numpy()
        got = np.array([lg[o // hop] for o in offs])
        err = np.abs(got - ref)
        print(f"golden pin hop {hop}: max err {err.max():.2e}")
        assert err.max() < LOGIT_ATOL, (hop, err)


def test_int16_equals_scaled_float(model):
    n = WIN + 256 * 9 + 31
    xi = (np.random.default_rng(5).standard_normal(n) * 3000).clip(-32768, 32767).astype(np.int16)
    a, fa = model.scan(xi, hop=256, return_features=True)
    b, fb = model.scan(xi.astype(np.float32) / 32768.0, hop=256, return_features=True)
    assert tuple(a.shape) == (10,)
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(fa.cpu().numpy(), fb.cpu().numpy())


def test_hop_480_is_the_forward_path(model):
    hop, W = 480, 9
    x = _noise(WIN + hop * (W - 1) + 100, 8)
    assert _workspace_bytes(1, x.size, hop) == 0
    lg, ft = model.scan(x, hop=hop, return_features=True)
    ld, fd = model.detect(_windows(x, hop, W), return_features=True)
    assert np.array_equal(lg.cpu().numpy(), ld.cpu().numpy())
    assert np.array_equal(ft.cpu().numpy(), fd.cpu().numpy())


def test_deterministic_and_prefix_invariant(model):
    x = _noise(WIN + 256 * 40, 9)
    a, fa = model.scan(x, hop=256, return_features=True)
    b, fb = model.scan(x, hop=256, return_features=True)
    a, fa = a.cpu().numpy(), fa.cpu().numpy()
    assert a.shape == (41,)
    assert np.array_equal(a, b.cpu().numpy()) and np.array_equal(fa, fb.cpu().numpy())
    c, fc = model.scan(x[:WIN + 256 * 10], hop=256, return_features=True)
    assert tuple(c.shape) == (11,)
    assert np.array_equal(a[:11], c.cpu().numpy())
    assert np.array_equal(fa[:11], fc.cpu().numpy())


def test_chunking(model, gpu):
    torch = gpu
    hop, W = 256, 70
    n = WIN + hop * (W - 1)
    buf = torch.from_numpy(_noise(n, 10)).cuda()
    full, small, one = _workspace_bytes(1, n, hop), _workspace_bytes(1, n, hop, 7), _workspace_bytes(1, n, hop, 1)
    assert full - small == (W - 7) * 13 * 63 * 4 and small - one == 6 * 13 * 63 * 4
    st0, l0, f0 = _scan_raw(model, buf, 1, n, n, hop, full)
    st1, l1, f1 = _scan_raw(model, buf, 1, n, n, hop, small)
    st2, l2, _ = _scan_raw(model, buf, 1, n, n, hop, small, want_feats=False)   # features staged in the workspace
    st3, l3, _ = _scan_raw(model, buf, 1, n, n, hop, one, want_feats=False)
    assert (st0, st1, st2, st3) == (0, 0, 0, 0)
    assert np.isfinite(l0).all()
    assert np.array_equal(l0, l1) and np.array_equal(f0, f1)
    assert np.array_equal(l0, l2) and np.array_equal(l0, l3)
    # one byte short of one window per chunk: refused, nothing written
    st4, l4, _ = _scan_raw(model, buf, 1, n, n, hop, one - 1, want_feats=False)
    assert st4 == INVALID and np.isnan(l4).all()


def test_precisions(model, golden_dir):
    import wakeword
    x = _noise(WIN + 512 * 20, 11)
    ref = model.scan(x, hop=512).cpu().numpy()
    onnx = os.path.join(golden_dir, "xiaoa.onnx")
    for prec, tol in (("bf16", 0.05), ("bf16x3", 1e-3)):
        m = wakeword.load_onnx(onnx, precision=prec)
        got = m.scan(x, hop=512).cpu().numpy()
        err = np.abs(got - ref).max()
        print(f"{prec}: max |dlogit| vs fp32 scan {err:.2e}")
        assert got.shape == ref.shape and err < tol, (prec, err)
        m.check_device_errors()
    m = wakeword.load_onnx(onnx, precision="int8")
    got = m.scan(x, hop=512).cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert np.array_equal(got * 8.0, np.round(got * 8.0))       # the int8 network's output grid, 2^-3


def test_errors(model, gpu, xiaoa_sd):
    torch = gpu
    from wakeword import _lib
    from wakeword.api import _Handle, pack_weights
    L = _lib.lib()
    hop = 256
    n = WIN + hop * 3
    buf = torch.from_numpy(_noise(2 * n, 12)).cuda()
    ws = _workspace_bytes(2, n, hop)
    assert _scan_raw(model, buf, 1, n, n, hop, ws)[0] == 0
    assert _scan_raw(model, buf, 2, n, n, hop, ws)[0] == 0
    assert _scan_raw(model, buf, 2, n, n - 1, hop, ws)[0] == INVALID      # n_rec > 1, rec_stride < n_samples
    assert _scan_raw(model, buf, 1, n, n, hop, ws, dtype=7)[0] == INVALID
    lg = torch.zeros((4,), dtype=torch.float32, device="cuda")
    wsb = torch.empty((ws,), dtype=torch.uint8, device="cuda")
    st = _stream(torch)

    def call(h, audio, n_rec, n_samples, logits, workspace, nbytes, hop_=hop):
        return L.wk_scan(h, audio, _lib.WK_DTYPE_F32, n_rec, n_samples, n_samples, hop_, logits, None, workspace,
                         nbytes, st)

    h = model._h.h
    assert call(h, _ptr(buf), -1, n, _ptr(lg), _ptr(wsb), ws) == INVALID
    assert call(h, None, 1, n, _ptr(lg), _ptr(wsb), ws) == INVALID         # null audio with W > 0
    assert call(h, _ptr(buf), 1, n, None, _ptr(wsb), ws) == INVALID        # null logits with W > 0
    assert call(h, _ptr(buf), 1, n, _ptr(lg), None, ws) == INVALID         # null workspace on the shared path
    assert call(h, _ptr(buf), 1, (1 << 30) + 1, _ptr(lg), _ptr(wsb), ws) == INVALID
    assert call(None, _ptr(buf), 1, n, _ptr(lg), _ptr(wsb), ws) == INVALID
    assert call(h, _ptr(buf), 1, n, _ptr(lg), _ptr(wsb), ws, hop_=0) == INVALID      # hop < 1
    assert call(h, _ptr(buf), 1, n, _ptr(lg), _ptr(wsb), ws, hop_=-256) == INVALID
    # W = 0: nothing to do, whatever the pointers
    assert call(h, None, 1, WIN - 1, None, None, 0) == 0
    assert call(h, None, 0, n, None, None, 0) == 0
    assert _workspace_bytes(1, WIN - 1, hop) == 0
    nb = C.c_size_t(0)
    assert L.wk_scan_workspace_bytes(1, n, 0, 0, C.byref(nb)) == INVALID
    assert L.wk_scan_workspace_bytes(-1, n, hop, 0, C.byref(nb)) == INVALID
    assert L.wk_scan_workspace_bytes(1, (1 << 30) + 1, hop, 0, C.byref(nb)) == INVALID
    assert L.wk_scan_workspace_bytes(1, n, hop, 0, None) == INVALID
    torch.cuda.synchronize()
    assert float(lg.abs().max()) == 0.0                                     # no refused call launched anything
    # wrong handles: mode A (esp_mfcc) is unsupported, as in wk_forward; no weights is an argument error
    mode_a = _Handle(_lib.WK_MODE_ESP_MFCC, pack_weights(xiaoa_sd), 0)
    assert call(mode_a.h, _ptr(buf), 1, n, _ptr(lg), _ptr(wsb), ws) == UNSUPPORTED
    bare = _Handle(_lib.WK_MODE_TORCHAUDIO_CMVN, None, 0)
    assert call(bare.h, _ptr(buf), 1, n, _ptr(lg), _ptr(wsb), ws) == INVALID
    with pytest.raises(ValueError):
        model.scan(np.zeros(WIN, np.float32), hop=0)


def test_no_device_errors_after_the_suite(model):
    model.check_device_errors()
