"""GPU checks that go with the even power-row pitch and the 16-byte weight
fragment loads, on small clips.

  - The fused kernel at B = 2, 4, 8, 9 in fp32, bf16 and bf16x3: every clip's
    logit and features are bit-equal to the same clip run alone (B = 1).  The
    invariant holds across launches; these batch sizes run full
    CNN batches of 4 (every fragment of conv1-3 and classifier.0 feeds real
    clips), a ragged tail and two workgroups' worth of batches, which the
    B = 1, 3, 5 of test_gpu_fe_bits.py do not.
  - wk_scan of a 3-window recording (frame store + edge frames through the
    power rows) against the standalone front-end and wk_forward on the same
    windows, at test_gpu_scan.py's tolerance between two compilations of the
    same device code.
  - Mode A on 5,000-sample clips (19 frames: a chunk with fewer frames than
    frame slots) against the standalone front-end on a 1 s clip holding the
    same samples 768 samples in: frame t of the short clip is frame t + 3 of
    the long one, in another frame slot and power row, and must come out
    bit-equal (t >= 1: frame 0 differs in its pre-emphasis predecessor)."""
import os

import numpy as np
import pytest

from oracle import wk_oracle as O

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "bf16", "bf16x3")
BATCHES = (2, 4, 8, 9)
SAME_CODE_ATOL = 5e-5   # test_gpu_scan.py: two compilations of the same device front-end code
WIN = 16000


@pytest.fixture(scope="module")
def clips():
    return O.synth_clips(131, 0, max(BATCHES)).astype(np.float32)


@pytest.fixture(scope="module")
def models(gpu, golden_dir):
    import wakeword
    onnx = os.path.join(golden_dir, "xiaoa.onnx")
    return {p: wakeword.load_onnx(onnx, precision=p) for p in PRECISIONS}


@pytest.fixture(scope="module")
def alone(models, clips):
    """Per precision: every clip run alone, computed once."""
    out = {}
    for p, m in models.items():
        lg, ft = [], []
        for i in range(len(clips)):
            l1, f1 = m.detect(clips[i:i + 1], return_features=True)
            lg.append(l1.cpu().numpy())
            ft.append(f1.cpu().numpy())
        out[p] = (np.concatenate(lg), np.concatenate(ft))
    return out


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_batch_equals_clips_alone(models, alone, clips, prec, B):
    lg, ft = models[prec].detect(clips[:B], return_features=True)
    lg, ft = lg.cpu().numpy(), ft.cpu().numpy()
    want_l, want_f = alone[prec][0][:B], alone[prec][1][:B]
    assert lg.shape == (B,) and ft.shape == (B, 13, 63) and np.isfinite(lg).all() and np.isfinite(ft).all()
    dl = lg.view(np.uint32) != want_l.view(np.uint32)
    df = ft.view(np.uint32) != want_f.view(np.uint32)
    print(f"{prec} B={B}: {int(dl.sum())} of {B} logits, {int(df.sum())} of {df.size} features differ from B = 1")
    assert not dl.any() and not df.any(), (prec, B, np.argwhere(dl).ravel().tolist(), np.argwhere(df)[:4].tolist())
    models[prec].check_device_errors()


def test_scan_three_windows_matches_the_standalone_front_end(models):
    import wakeword
    hop, W = 256, 3
    x = O.synth_clips(132, 0, 2).astype(np.float32).reshape(-1)[:WIN + hop * (W - 1)]
    x = np.ascontiguousarray(x)
    lg, ft = models["fp32"].scan(x, hop=hop, return_features=True)
    lg, ft = lg.cpu().numpy(), ft.cpu().numpy()
    wins = np.stack([x[w * hop:w * hop + WIN] for w in range(W)])
    fe = wakeword.mfcc(wins, mode="torchaudio").cpu().numpy()
    ld, fd = models["fp32"].detect(wins, return_features=True)
    ef, el = np.abs(ft - fe).max(), np.abs(lg - ld.cpu().numpy()).max()
    efd = np.abs(ft - fd.cpu().numpy()).max()
    print(f"scan W=3: features vs standalone front-end {ef:.2e}, vs wk_forward {efd:.2e}; logits vs wk_forward {el:.2e}")
    assert ft.shape == (W, 13, 63) and np.isfinite(ft).all() and np.isfinite(lg).all()
    assert ef < SAME_CODE_ATOL and efd < SAME_CODE_ATOL and el < SAME_CODE_ATOL


def test_mode_a_short_clip_matches_the_same_samples_in_a_long_clip(gpu):
    import wakeword
    short, shift = 5000, 3
    x = O.synth_clips(133, 0, 2).astype(np.float32)
    long_ = wakeword.mfcc(x, mode="esp").cpu().numpy()                     # [2][62][13]
    cut = np.ascontiguousarray(x[:, 256 * shift:256 * shift + short])
    got = wakeword.mfcc(cut, mode="esp").cpu().numpy()                     # [2][19][13]
    nf = (short - 320) // 256 + 1
    assert got.shape == (2, nf, 13) and long_.shape == (2, 62, 13) and np.isfinite(got).all()
    want = long_[:, shift + 1:shift + nf]
    diff = got[:, 1:].view(np.uint32) != want.view(np.uint32)
    print(f"mode A, {short} samples: {int(diff.sum())} of {diff.size} values of frames 1..{nf - 1} differ from the "
          f"long clip's frames {shift + 1}..{shift + nf - 1}; max |d| {np.abs(got[:, 1:] - want).max():.2e}")
    assert not diff.any(), np.argwhere(diff)[:4].tolist()
