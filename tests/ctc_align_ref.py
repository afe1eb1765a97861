"""Reference for wk_ctc_align (numpy only): the Viterbi recurrence and tie rule
of include/wakeword.h in float32 (the exact oracle: one exact max and one IEEE
add per state define every output bit for bit) and in float64 (the independent
check), the validity rules of a CTC path, and the case table.

    a_0(0) = lp_0(0),  a_0(1) = lp_0(l'_1),  a_0(s >= 2) = -inf
    a_t(s) = lp_t(l'_s) + max(a_{t-1}(s), a_{t-1}(s-1), [a_{t-1}(s-2)])
Ties: s, then s-1, then s-2 (replace only if strictly greater); exit L-1 when
a(L-1) >= a(L-2).  No alignment: score -inf, states None.
"""
import functools

import numpy as np

EPS32 = 2.0 ** -24
NEG = -np.inf


def extended(labels):
    """l': the labels interleaved with blanks, L = 2S+1."""
    ext = np.zeros(2 * len(labels) + 1, dtype=np.int64)
    ext[1::2] = labels
    return ext


def skip_mask(labels):
    """skip[s]: state s may be entered from s-2 (a label state whose label
    differs from the one two states back)."""
    lab = np.asarray(labels, dtype=np.int64)
    skip = np.zeros(2 * len(lab) + 1, dtype=bool)
    if len(lab) > 1:
        skip[3::2] = lab[1:] != lab[:-1]
    return skip


def viterbi(lp, labels, dtype=np.float32):
    """lp (Tb, V) log-probs, labels a sequence of S ids in [1, V) -> (score,
    states (Tb,) int32), or (-inf, None) without an alignment.  All arithmetic
    in `dtype`."""
    lp = np.asarray(lp)
    Tb = lp.shape[0]
    if Tb == 0:
        return dtype(NEG), None
    ext, skip = extended(labels), skip_mask(labels)
    L = len(ext)
    x = lp[:, ext].astype(dtype)                       # (Tb, L)
    a = np.full(L, NEG, dtype=dtype)
    a[0] = x[0, 0]
    if L > 1:
        a[1] = x[0, 1]
    bp = np.zeros((Tb, L), dtype=np.int8)
    ninf1, ninf2 = np.full(1, NEG, dtype=dtype), np.full(2, NEG, dtype=dtype)
    for t in range(1, Tb):
        n1 = np.concatenate([ninf1, a[:-1]])
        n2 = np.concatenate([ninf2, a[:-2]])[:L]
        best, k = a.copy(), np.zeros(L, dtype=np.int8)
        m = n1 > best
        best[m], k[m] = n1[m], 1
        m = skip & (n2 > best)
        best[m], k[m] = n2[m], 2
        a = x[t] + best
        assert a.dtype == dtype
        bp[t] = k
    e1 = a[L - 1]
    e2 = a[L - 2] if L >= 2 else dtype(NEG)
    s = L - 1 if e1 >= e2 else L - 2
    score = e1 if e1 >= e2 else e2
    if score == NEG:
        return dtype(NEG), None
    states = np.empty(Tb, dtype=np.int32)
    for t in range(Tb - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    return score, states


def valid_alignment(states, labels, Tb):
    """A CTC path of `labels` over Tb frames: starts in state 0 or 1, steps in
    {0, 1, 2}, a step of 2 only onto a label state whose label differs from
    the one two back, ends in L-1 or L-2."""
    states = np.asarray(states)
    L, skip = 2 * len(labels) + 1, skip_mask(labels)
    if len(states) != Tb or Tb == 0:
        return False
    if states[0] not in (0, 1) or states[-1] not in (L - 1, L - 2) or states.min() < 0 or states.max() >= L:
        return False
    for t in range(1, Tb):
        d = int(states[t]) - int(states[t - 1])
        if d not in (0, 1, 2) or (d == 2 and not skip[states[t]]):
            return False
    return True


def path_score64(lp, labels, states):
    """The log-probability of a path, summed in float64."""
    ext = extended(labels)
    lp = np.asarray(lp)
    return float(np.sum(lp[np.arange(len(states)), ext[np.asarray(states)]].astype(np.float64)))


def all_paths(labels, Tb):
    """Every valid path, by enumeration (tiny problems only)."""
    L, skip = 2 * len(labels) + 1, skip_mask(labels)
    out = []

    def grow(p):
        if len(p) == Tb:
            if p[-1] in (L - 1, L - 2):
                out.append(tuple(p))
            return
        for d in (0, 1, 2):
            s = p[-1] + d
            if s < L and (d < 2 or skip[s]):
                grow(p + [s])

    for s0 in (0, 1):
        if s0 < L and Tb > 0:
            grow([s0])
    assert all(valid_alignment(np.array(p), labels, Tb) for p in out)
    return out


def spans_of(states, S):
    """(S, 2) [start, end) of each label's run of frames."""
    sp = np.full((S, 2), -1, dtype=np.int32)
    for i in range(S):
        t = np.nonzero(np.asarray(states) == 2 * i + 1)[0]
        if len(t):
            assert t[-1] - t[0] + 1 == len(t)           # one contiguous run
            sp[i] = (t[0], t[-1] + 1)
    return sp


def align_batch(lp, labels, in_len, lab_len, max_label_len=None, dtype=np.float32):
    """wk_ctc_align's outputs on the host: lp (B, T, V) float32, labels (B,
    stride) -> dict of states, tokens, frame_lp, spans, scores with the -1 /
    0 / -inf conventions of the header."""
    lp = np.asarray(lp, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    B, T, V = lp.shape
    smax = labels.shape[1] if max_label_len is None else max_label_len
    out = dict(states=np.full((B, T), -1, np.int32), tokens=np.full((B, T), -1, np.int32),
               frame_lp=np.zeros((B, T), np.float32), spans=np.full((B, smax, 2), -1, np.int32),
               scores=np.full(B, NEG, dtype))
    for b in range(B):
        Tb, S = min(max(int(in_len[b]), 0), T), min(max(int(lab_len[b]), 0), smax)
        lab = labels[b, :S]
        if S and (lab.min() < 1 or lab.max() >= V):
            continue
        score, st = viterbi(lp[b, :Tb], lab, dtype)
        if st is None:
            continue
        tok = extended(lab)[st]
        out["scores"][b] = score
        out["states"][b, :Tb] = st
        out["tokens"][b, :Tb] = tok
        out["frame_lp"][b, :Tb] = lp[b, np.arange(Tb), tok]
        out["spans"][b, :S] = spans_of(st, S)
    return out


def log_softmax(z):
    z = np.asarray(z, dtype=np.float32)
    m = z.max(-1, keepdims=True)
    return (z - m - np.log(np.exp(z - m).sum(-1, keepdims=True, dtype=np.float32))).astype(np.float32)


def planted_path(rng, labels, T):
    """A random valid path of `labels` over T frames (T >= the shortest path):
    every state of the shortest route, each held a random number of frames."""
    ext = extended(labels)
    route = [s for s in range(len(ext)) if (s & 1) or (0 < s < len(ext) - 1 and ext[s - 1] == ext[s + 1])]
    if not route:
        route = [0]
    assert T >= len(route)
    cuts = np.sort(rng.choice(np.arange(1, T), size=len(route) - 1, replace=False)) if len(route) > 1 else np.array([], int)
    bounds = np.concatenate([[0], cuts, [T]]).astype(int)
    st = np.empty(T, dtype=np.int32)
    for r, s in enumerate(route):
        st[bounds[r]:bounds[r + 1]] = s
    return st


# ---- the case table: (T, V, S) x kind ---------------------------------------------
SHAPES = [(50, 32, 10), (64, 8, 20), (130, 5, 64), (300, 50, 127), (801, 4000, 40), (801, 4000, 255)]
KINDS = ("plain", "planted", "same")          # seeded normal logits; +12 along a planted path; all labels equal
CASES = [(shape, kind) for shape in SHAPES for kind in KINDS] + [(shape, "same-planted") for shape in SHAPES[:3]]
CASE_IDS = [f"T{t}-V{v}-S{s}-{kind}" for (t, v, s), kind in CASES]


@functools.lru_cache(maxsize=4)
def case(shape, kind):
    """-> (lp (T, V) float32 log_softmax rows, labels (S,) int64, planted states or None)."""
    T, V, S = shape
    rng = np.random.default_rng(1000 * T + 10 * S + V + KINDS.index(kind.split("-")[0]))
    z = rng.standard_normal((T, V)).astype(np.float32)
    labels = np.full(S, 1 + rng.integers(V - 1), dtype=np.int64) if kind.startswith("same") else rng.integers(1, V, size=S)
    planted = None
    if kind.endswith("planted"):
        planted = planted_path(rng, labels, T)
        z[np.arange(T), extended(labels)[planted]] += 12.0
    return log_softmax(z), labels, planted
