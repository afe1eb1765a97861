"""Dense sliding-window scoring of long recordings (wk_scan).

Window ``w`` of a recording covers samples ``[w*hop, w*hop + 16000)``.  In the
mode-B front-end (centre padding 256 with reflection, 320-sample Hamming
window, frame hop 256) frame ``t`` of a window reads window samples
``[256t - 160, 256t + 160)`` and the one sample before them (pre-emphasis).
For ``t = 1..61`` all of those lie inside the window, so when ``hop = 256 k``
the frame is *global frame* ``g = k*w + t`` of the recording -- the same frame
for every window that contains it -- and is computed once.  Frames 0 and 62
reflect at the window's own edges (and frame 0 starts the pre-emphasis with
``y[0] = x[0]``), so they are computed per window.

``plan`` is that geometry as host arithmetic (no GPU); ``scan_events`` walks a
scan's logits through the firmware's decision rule (``stream.DecisionRule``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np

from .stream import DecisionRule, Window

WIN = 16000
FRAME_HOP = 256
N_FRAMES = 63
MAX_K = 61          # hop = 256 k shares frames for k <= 61; beyond it consecutive windows have none in common


@dataclass(frozen=True)
class ScanPlan:
    n_samples: int
    hop: int
    W: int            # windows: (n_samples - 16000) // hop + 1, 0 if n_samples < 16000
    shared: bool      # interior frames are computed once per recording
    k: int            # hop // 256 when shared, else 0
    G: int            # global frames 1..G = k (W - 1) + 61 when shared, else 0

    def frame_index(self, w: int, t: int):
        """Where frame t (0..62) of window w comes from: ``("global", g)`` for an
        interior frame of a shared plan, ``("edge", w, t)`` for a frame computed
        for that window alone."""
        if not 0 <= w < self.W or not 0 <= t < N_FRAMES:
            raise IndexError((w, t))
        if self.shared and 1 <= t <= N_FRAMES - 2:
            return ("global", self.k * w + t)
        return ("edge", w, t)


def plan(n_samples: int, hop: int) -> ScanPlan:
    if hop < 1:
        raise ValueError("hop must be >= 1")
    W = (n_samples - WIN) // hop + 1 if n_samples >= WIN else 0
    shared = W > 0 and hop % FRAME_HOP == 0 and hop // FRAME_HOP <= MAX_K
    k = hop // FRAME_HOP if shared else 0
    return ScanPlan(n_samples, hop, W, shared, k, k * (W - 1) + (N_FRAMES - 2) if shared else 0)


def events_from_logits(logits, hop: int, threshold: float = 0.8, refractory_s: float = 5.0,
                       sample_rate: int = 16000) -> List[Window]:
    """One ``Window`` per logit (window w ends at ``w*hop + 16000``), through a
    fresh ``DecisionRule``."""
    rule = DecisionRule(threshold, int(round(refractory_s * sample_rate)))
    return [rule(w * hop + WIN, float(z)) for w, z in enumerate(np.asarray(logits, np.float32).reshape(-1))]


def scan_events(model, audio, hop: int = 256, threshold: float = 0.8, refractory_s: float = 5.0) -> List[Window]:
    """Scan one recording with ``model.scan`` and apply the firmware's threshold
    + refractory rule to its windows in order -> ``list[Window]`` (every
    window; ``detected`` marks the events)."""
    z = model.scan(audio, hop=hop)
    if hasattr(z, "cpu"):
        z = z.cpu().numpy()
    z = np.asarray(z)
    if z.ndim != 1:
        raise ValueError("scan_events takes one recording (1-D audio)")
    return events_from_logits(z, hop, threshold, refractory_s)
