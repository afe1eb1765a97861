"""CPU tests of the scan geometry (wakeword.scan): window / global-frame
arithmetic, the frame-sharing argument checked in float64 against the oracle,
and the event walk over a scan's logits."""
import numpy as np
import pytest

from oracle import wk_oracle as O
from wakeword.scan import events_from_logits, plan, scan_events
from wakeword.stream import DecisionRule


def test_plan_counts():
    p = plan(15999, 256)
    assert p.W == 0 and not p.shared and p.G == 0
    p = plan(16000, 256)
    assert (p.W, p.shared, p.k, p.G) == (1, True, 1, 61)
    p = plan(16000 + 256 * 3 + 100, 256)
    assert (p.W, p.shared, p.k, p.G) == (4, True, 1, 64)
    p = plan(16000 + 512 * 4 + 100, 512)
    assert (p.W, p.shared, p.k, p.G) == (5, True, 2, 2 * 4 + 61)
    p = plan(16000 + 480 * 7, 480)
    assert p.W == 8 and not p.shared and p.k == 0 and p.G == 0


def test_plan_frame_index():
    p = plan(16000 + 768 * 2, 768)
    assert p.frame_index(0, 0) == ("edge", 0, 0)
    assert p.frame_index(2, 62) == ("edge", 2, 62)
    assert p.frame_index(0, 1) == ("global", 1)
    assert p.frame_index(2, 61) == ("global", 3 * 2 + 61) and p.G == 3 * 2 + 61
    # windows one hop apart share frames: frame t + k of window w is frame t of window w + 1
    assert p.frame_index(0, 1 + 3) == p.frame_index(1, 1)
    q = plan(16000 + 480 * 2, 480)
    assert q.frame_index(1, 30) == ("edge", 1, 30)
    with pytest.raises(IndexError):
        p.frame_index(3, 0)
    with pytest.raises(IndexError):
        p.frame_index(0, 63)
    with pytest.raises(ValueError):
        plan(16000, 0)


def test_hops_without_a_common_frame_are_not_shared():
    # hop = 256 * 62: frames 1..61 of consecutive windows do not overlap
    assert plan(16000 * 4, 256 * 61).shared
    assert not plan(16000 * 4, 256 * 62).shared


def _global_frame(x, g):
    """Raw MFCC (13,) of global frame g of recording x, float64, computed
    directly: samples [256 g - 160, 256 g + 160) with their predecessor for the
    pre-emphasis, periodic Hamming 320 centred in 512, rFFT, HTK mel, log, DCT."""
    lo = 256 * g - 160
    seg = np.asarray(x[lo - 1:lo + 320], np.float64)
    y = seg[1:] - 0.97 * seg[:-1]
    fr = np.zeros(512)
    fr[96:96 + 320] = y * O.hamming_periodic(320)
    s = np.fft.rfft(fr, n=512)
    mel = (s.real ** 2 + s.imag ** 2) @ O.melscale_fbanks()
    return np.log(mel + 1e-6) @ O.create_dct()


def test_shared_frames_reproduce_the_per_window_front_end():
    hop = 256
    x = np.random.default_rng(11).standard_normal(16000 + 256 * 5) * 0.1
    p = plan(x.size, hop)
    assert p.W == 6 and p.shared
    store = {g: _global_frame(x, g) for g in range(1, p.G + 1)}
    for w in range(p.W):
        win = x[w * hop:w * hop + 16000]
        own = O.mfcc_torchaudio(win)            # (13, 63): only its frames 0 and 62 are used
        m = np.empty((13, 63))
        for t in range(63):
            src = p.frame_index(w, t)
            if src[0] == "global":
                m[:, t] = store[src[1]]
            else:
                assert src == ("edge", w, t) and t in (0, 62)
                m[:, t] = own[:, t]
        got = O.normalize_mfcc(m, "cmvn")
        assert np.abs(got - O.features_mode_b(win)).max() < 1e-9, w
    # ... and the edge frames are the window's own: the recording's frame there differs
    w = 1
    edge = O.mfcc_torchaudio(x[w * hop:w * hop + 16000])[:, 0]
    assert np.abs(edge - _global_frame(x, w)).max() > 0.1


class _FakeModel:
    def __init__(self, logits):
        self.logits = np.asarray(logits, np.float32)
        self.calls = []

    def scan(self, audio, hop=256):
        self.calls.append((len(audio), hop))
        return self.logits


def test_scan_events_walks_the_decision_rule():
    hop = 512
    logits = np.full(400, -6.0, np.float32)
    logits[[3, 4, 5, 100, 170, 171, 399]] = [2.0, 5.0, 1.0, 1.3, 4.0, 4.0, 9.0]   # 1.3 -> p 0.786 < 0.8
    audio = np.zeros(16000 + hop * 399, np.float32)
    m = _FakeModel(logits)
    got = scan_events(m, audio, hop=hop, threshold=0.8, refractory_s=5.0)
    assert m.calls == [(audio.size, hop)]
    rule = DecisionRule(0.8, 5 * 16000)
    ref = [rule(w * hop + 16000, float(z)) for w, z in enumerate(logits)]
    assert got == ref
    assert events_from_logits(logits, hop, 0.8, 5.0) == ref
    assert events_from_logits([], hop) == []
    # a shorter refractory lets window 170 fire: its start, 87040, is past 17536 + 16000
    assert [i for i, e in enumerate(events_from_logits(logits, hop, 0.8, 1.0)) if e.detected] == [3, 170, 399]
    fired = [i for i, e in enumerate(got) if e.detected]
    # 3 fires (p 0.88); 4 and 5 are inside its 5 s; 100 is below threshold; 170 starts
    # before 3's suppression ends (window 3 ends at 17536, + 80000 = 97536 > 170*512), 399 fires
    assert fired == [3, 399]
    assert got[3].end == 3 * hop + 16000
