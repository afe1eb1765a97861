"""The fused kernel's two reflect-padded frames (0 and 62 of every clip).

Their rounds issue the common round's loads and take the reflected rows from
the frame's other rows in registers (csrc/wk_fe_dev.h fe_stage0_rows; the row
geometry is tests/test_edge_frame_rows.py).  Checked here, in both compilation
units (fp32 and bf16 precision) and for float32 and int16 audio:

  - features of frames 0, 1, 61, 62 and of all frames, and the logits, against
    the oracle, for batches of 1, 2, n_cu + 1 and 2 n_cu + 3 clips (the
    prefetch past a workgroup's last clip; workgroups with two and three clips,
    i.e. the prefetch from a clip's last round into the next clip's edge
    round), with clip_stride 16,000, 16,384 and 480 (overlapping windows);
  - on the CPU first, that the check can fail: the oracle with a wrong padding
    ('symmetric' for 'reflect'; y[0] = x[0] - 0.97 x[1]) moves the edge frames
    of this input by more than 100 x the feature tolerance;
  - bit identity (fp32 precision) of frames 0 and 62 and the logits of 8 clips
    with tests/golden/edge_frames_parent.npz, recorded by
    tools/record_edge_frames.py from the commit that still loaded the edge
    frames through per-lane reflected indices: the arithmetic is the same
    operations in the same forms."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from oracle import wk_oracle as O
from test_gpu_bf16 import BF16_LOGIT_ATOL
from test_gpu_parity import FEAT_ATOL, LOGIT_ATOL

WIN = 16000
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_edge_frames", os.path.join(REPO, "tools", "record_edge_frames.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)

LOGIT_TOL = {"fp32": LOGIT_ATOL, "bf16": BF16_LOGIT_ATOL}
EDGE = [0, 62]


def _features(x, pad_mode="reflect", y0_minus_x1=False):
    """O.features_mode_b from the oracle's own parts, with the padding (and the first pre-emphasis sample) to choose."""
    y = O.preemphasis(x)
    if y0_minus_x1:
        y[..., 0] = x[..., 0] - 0.97 * x[..., 1]
    pad = O.N_FFT // 2
    yp = np.pad(y, [(0, 0)] * (y.ndim - 1) + [(pad, pad)], mode=pad_mode)
    win = np.zeros(O.N_FFT)
    left = (O.N_FFT - O.WIN_LENGTH) // 2
    win[left:left + O.WIN_LENGTH] = O.hamming_periodic(O.WIN_LENGTH)
    idx = np.arange(O.N_FRAMES)[:, None] * O.HOP + np.arange(O.N_FFT)[None, :]
    spec = np.fft.rfft(yp[..., idx] * win, n=O.N_FFT, axis=-1)
    p = spec.real ** 2 + spec.imag ** 2
    mf = np.log(p @ O.melscale_fbanks() + 1e-6) @ O.create_dct()
    return O.normalize_mfcc(np.swapaxes(mf, -1, -2), "cmvn")


def test_wrong_padding_is_visible_in_this_input():
    """Not a GPU test: the edge-frame check can fail for the input used below."""
    x = REC.edge_clips(REC.EDGE_FIXTURE_CLIPS).astype(np.float64)
    right = _features(x)
    assert np.array_equal(right, O.features_mode_b(x))
    sym = np.abs(_features(x, pad_mode="symmetric") - right).max(axis=1)       # [clip][frame]
    assert sym[:, 0].min() >= 100 * FEAT_ATOL and sym[:, 62].min() >= 100 * FEAT_ATOL, (sym[:, 0].min(), sym[:, 62].min())
    # y[0] belongs to frame 0 alone (frame 62 only moves through CMVN's statistics)
    y0 = np.abs(_features(x, y0_minus_x1=True) - right).max(axis=1)
    assert y0[:, 0].min() >= 100 * FEAT_ATOL, y0[:, 0].min()


# --------------------------------------------------------------------------- GPU
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _forward(model, buf, B, stride, want_feats):
    """wk_forward on a flat device buffer: clip i starts at element i * stride."""
    import torch
    from wakeword import _lib
    lg = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
    ft = torch.full((B, 13, 63), float("nan"), dtype=torch.float32, device="cuda") if want_feats else None
    dt = _lib.WK_DTYPE_I16 if buf.dtype == torch.int16 else _lib.WK_DTYPE_F32
    _lib.check(_lib.lib().wk_forward(model._h.h, _ptr(buf), dt, B, WIN, stride, _ptr(lg), _ptr(ft),
                                     C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "wk_forward")
    return lg.cpu().numpy(), (ft.cpu().numpy() if want_feats else None)


@pytest.fixture(scope="module")
def n_cu(gpu):
    return gpu.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def models(gpu, golden_dir):
    import wakeword
    return {p: wakeword.load_onnx(os.path.join(golden_dir, "xiaoa.onnx"), precision=p) for p in ("fp32", "bf16")}


def _reference(x, sd):
    """Oracle features and logits, in chunks (float64 frames of a few hundred clips at a time)."""
    f = np.concatenate([O.features_mode_b(x[i:i + 128]) for i in range(0, len(x), 128)])
    return f, O.kws_forward(f, sd)[:, 0]


@pytest.fixture(scope="module")
def batch(n_cu, xiaoa_sd):
    """2 n_cu + 3 clips, float32 and int16, with their oracle results (computed once, never modified)."""
    x = REC.edge_clips(2 * n_cu + 3)
    xi = REC.to_i16(x)
    out = {"f32": (x,) + _reference(x, xiaoa_sd), "i16": (xi,) + _reference(xi.astype(np.float32) / 32768.0, xiaoa_sd)}
    for a in out.values():
        for v in a:
            v.setflags(write=False)
    return out


def _check(tag, lg, ft, lg_nofeat, ref_f, ref_l, logit_tol):
    per_frame = np.abs(ft - ref_f).max(axis=(0, 1))
    print(f"{tag}: max|dfeat| frames 0,1,61,62 = {per_frame[[0, 1, 61, 62]]}, all = {per_frame.max():.2e}; "
          f"max|dlogit| = {np.abs(lg - ref_l).max():.2e}")
    assert np.isfinite(ft).all() and np.isfinite(lg).all(), tag
    for t in (0, 1, 61, 62):
        assert per_frame[t] < FEAT_ATOL, (tag, t, per_frame[t])
    assert per_frame.max() < FEAT_ATOL, (tag, int(per_frame.argmax()), per_frame.max())
    assert np.abs(lg - ref_l).max() < logit_tol, tag
    assert np.array_equal(lg, lg_nofeat), tag        # the launch without a feature buffer gives the same logits


@pytest.mark.gpu
@pytest.mark.parametrize("audio", ["f32", "i16"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_edge_frames_batches(gpu, models, batch, n_cu, prec, audio):
    x, ref_f, ref_l = batch[audio]
    xd = gpu.from_numpy(x).cuda()
    for B in (1, 2, n_cu + 1, 2 * n_cu + 3):
        lg, ft = _forward(models[prec], xd, B, WIN, True)
        lg0, _ = _forward(models[prec], xd, B, WIN, False)
        _check(f"{prec} {audio} B={B}", lg, ft, lg0, ref_f[:B], ref_l[:B], LOGIT_TOL[prec])


@pytest.mark.gpu
@pytest.mark.parametrize("audio", ["f32", "i16"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_edge_frames_padded_stride(gpu, models, batch, n_cu, prec, audio):
    """clip_stride = 16,384: the clips of the batch above, 384 samples apart (filled with a large value that must not leak in)."""
    B = n_cu + 1
    x, ref_f, ref_l = batch[audio]
    buf = np.full((B, 16384), 0.9 if audio == "f32" else 29000, x.dtype)
    buf[:, :WIN] = x[:B]
    lg, ft = _forward(models[prec], gpu.from_numpy(buf).cuda(), B, 16384, True)
    lg0, _ = _forward(models[prec], gpu.from_numpy(buf).cuda(), B, 16384, False)
    _check(f"{prec} {audio} stride=16384", lg, ft, lg0, ref_f[:B], ref_l[:B], LOGIT_TOL[prec])


@pytest.fixture(scope="module")
def stream(n_cu, xiaoa_sd):
    """One recording scored as n_cu + 1 overlapping windows 480 samples apart (the streaming shape; an even
    stride keeps the pair loads' alignment parity)."""
    B, hop = n_cu + 1, 480
    rec = np.concatenate([c[:4000] for c in REC.edge_clips((B - 1) * hop // 4000 + 5, seed=7)])[:(B - 1) * hop + WIN]
    out = {}
    for audio, r in (("f32", rec), ("i16", REC.to_i16(rec))):
        w = np.lib.stride_tricks.sliding_window_view(r, WIN)[::hop][:B]
        wf = w.astype(np.float32) / 32768.0 if audio == "i16" else w
        out[audio] = (np.ascontiguousarray(r),) + _reference(wf, xiaoa_sd)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("audio", ["f32", "i16"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_edge_frames_overlapping_windows(gpu, models, stream, n_cu, prec, audio):
    rec, ref_f, ref_l = stream[audio]
    B = n_cu + 1
    lg, ft = _forward(models[prec], gpu.from_numpy(rec).cuda(), B, 480, True)
    lg0, _ = _forward(models[prec], gpu.from_numpy(rec).cuda(), B, 480, False)
    _check(f"{prec} {audio} stride=480", lg, ft, lg0, ref_f, ref_l, LOGIT_TOL[prec])


@pytest.mark.gpu
@pytest.mark.parametrize("audio", ["f32", "i16"])
def test_edge_frames_bit_identical_to_parent(gpu, models, golden_dir, audio):
    g = np.load(os.path.join(golden_dir, "edge_frames_parent.npz"))
    x = REC.edge_clips(REC.EDGE_FIXTURE_CLIPS)
    if audio == "i16":
        x = REC.to_i16(x)
    lg, ft = _forward(models["fp32"], gpu.from_numpy(x).cuda(), len(x), WIN, True)
    lg0, _ = _forward(models["fp32"], gpu.from_numpy(x).cuda(), len(x), WIN, False)
    edge = np.ascontiguousarray(ft[:, :, EDGE])
    assert np.array_equal(edge.view(np.uint32), g[f"feats_edge_{audio}"].view(np.uint32))
    assert np.array_equal(lg.view(np.uint32), g[f"logits_{audio}"].view(np.uint32))
    assert np.array_equal(lg0.view(np.uint32), lg.view(np.uint32))
