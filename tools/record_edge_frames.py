"""Input of tests/test_gpu_edge_frames.py and the recorder of its bit-identity
fixture, tests/golden/edge_frames_parent.npz.

    WAKEWORD_LIB=<library of the commit to record> python tools/record_edge_frames.py out.npz

The fixture holds what the fused kernel (fp32 precision) gave for the two
reflect-padded frames (0 and 62) and the logits of EDGE_FIXTURE_CLIPS clips,
for float32 and int16 audio, at the commit before the edge rounds took their
reflected rows from registers (per-lane reflected loads then).  Re-record it
only from a build whose edge-frame arithmetic is known good."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "esp32-wake-word_amd")]

EDGE_FIXTURE_CLIPS = 8


def edge_clips(count: int, seed: int = 2024) -> np.ndarray:
    """(count, 16000) float32: the synthetic clips with strongly asymmetric
    content where the centre padding reflects (samples 0-3 and 158-162 for
    frame 0, 15,964-15,999 for frame 62), different in every clip."""
    from oracle import wk_oracle as O
    x = O.synth_clips(seed, 0, count).copy()
    c = np.arange(count, dtype=np.float32)[:, None]
    s = 1.0 - 0.05 * (c % 7)                                    # per-clip scale, 0.7 .. 1.0
    x[:, 0:4] = s * np.array([0.9, -0.7, 0.45, -0.2], np.float32)
    x[:, 158:163] = s * np.array([0.8, -0.6, 0.35, -0.9, 0.65], np.float32)
    k = np.arange(36, dtype=np.float32)
    tail = (0.15 + 0.02 * k) * np.where(k % 3 == 0, 1.0, -0.6)   # growing, no symmetry about any sample
    x[:, 15964:16000] = s * tail.astype(np.float32)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def to_i16(x: np.ndarray) -> np.ndarray:
    return np.round(x * 32767.0).clip(-32768, 32767).astype(np.int16)


def record() -> dict:
    import wakeword
    model = wakeword.load_onnx(os.path.join(REPO, "tests", "golden", "xiaoa.onnx"), precision="fp32")
    x = edge_clips(EDGE_FIXTURE_CLIPS)
    out = {}
    for name, audio in (("f32", x), ("i16", to_i16(x))):
        logits, feats = model.detect(audio, return_features=True)
        out[f"logits_{name}"] = logits.cpu().numpy()
        out[f"feats_edge_{name}"] = np.ascontiguousarray(feats.cpu().numpy()[:, :, [0, 62]])
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **record())
    print("wrote", sys.argv[1])
