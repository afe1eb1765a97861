"""Reference for wk_ctc_spot (numpy only): the keyword-spotting recurrence and
tie rules of include/wakeword.h in float32 (the exact oracle: one exact max and
one IEEE add -- with normalize one IEEE subtract -- per state define every
output bit for bit) and in float64 (the independent check), the float64 score
of one given segment, and the brute force over all segments.

    L = 2S-1 states: even j emits w_{j/2}, odd j the blank
    x_t(j) = lp_t(l_j), or lp_t(l_j) - max_v lp_t(v) with normalize (-inf stays -inf)
    a_t(0) = x_t(0) + max(a_{t-1}(0), 0)
    a_t(j) = x_t(j) + max(a_{t-1}(j), a_{t-1}(j-1), [a_{t-1}(j-2)])
    score  = max_t a_t(L-1), the first t that attains it
Ties: stay, then j-1 (at state 0: enter), then j-2; replace only if strictly
greater.  Every state carries the frame its path entered state 0 (-1 at -inf).
"""
import numpy as np

EPS32 = 2.0 ** -24
NEG = -np.inf


def lattice(kw):
    """(l_j, skip_j) of a keyword: the labels interleaved with inner blanks, and
    whether state j may be entered from j-2."""
    kw = np.asarray(kw, dtype=np.int64)
    S = len(kw)
    ext = np.zeros(2 * S - 1, dtype=np.int64)
    ext[0::2] = kw
    skip = np.zeros(2 * S - 1, dtype=bool)
    if S > 1:
        skip[2::2] = kw[1:] != kw[:-1]
    return ext, skip


def emissions(lp, kw, normalize, dtype):
    """x (Tb, L) in `dtype`: the subtraction is done in `dtype` on the float32
    inputs (exact in float64)."""
    lp = np.asarray(lp, dtype=np.float32)
    ext, _ = lattice(kw)
    x = lp[:, ext].astype(dtype)
    if normalize and lp.shape[0]:
        g = lp.max(axis=1).astype(dtype)[:, None]
        with np.errstate(invalid="ignore"):
            x = np.where(x == NEG, dtype(NEG), x - g).astype(dtype)
    return x


def _advance(a, st, x_t, skip, enter, t):
    """One frame.  enter: state 0 may be entered at this frame (value 0, start t)."""
    L = len(a)
    dtype = a.dtype.type
    n1 = np.concatenate([[dtype(0.0) if enter else dtype(NEG)], a[:-1]]).astype(a.dtype)
    s1 = np.concatenate([[t if enter else -1], st[:-1]])
    n2 = np.concatenate([[dtype(NEG), dtype(NEG)], a[:-2]])[:L].astype(a.dtype)
    s2 = np.concatenate([[-1, -1], st[:-2]])[:L]
    best, bs = a.copy(), st.copy()
    m = n1 > best
    best[m], bs[m] = n1[m], s1[m]
    m = skip & (n2 > best)
    best[m], bs[m] = n2[m], s2[m]
    a = x_t + best
    assert a.dtype == best.dtype
    return a, np.where(a == NEG, -1, bs)


def spot(lp, kw, normalize, dtype=np.float32):
    """lp (Tb, V) float32, kw S labels in [1, V), S >= 1 -> (score, (start, end),
    e (Tb,)), all arithmetic in `dtype`; (-inf, (-1, -1), e) without an occurrence."""
    lp = np.asarray(lp, dtype=np.float32)
    Tb = lp.shape[0]
    _, skip = lattice(kw)
    L = len(skip)
    x = emissions(lp, kw, normalize, dtype)
    a, st = np.full(L, NEG, dtype=dtype), np.full(L, -1, dtype=np.int64)
    e = np.full(Tb, NEG, dtype=dtype)
    score, span = dtype(NEG), (-1, -1)
    for t in range(Tb):
        a, st = _advance(a, st, x[t], skip, True, t)
        e[t] = a[L - 1]
        if e[t] > score:
            score, span = e[t], (int(st[L - 1]), t + 1)
    return score, span, e


def seg64(lp, kw, normalize, start, end):
    """The float64 best score of a path that enters state 0 exactly at frame
    `start` and is in state L-1 at frame end - 1 (-inf if there is none)."""
    _, skip = lattice(kw)
    L = len(skip)
    x = emissions(lp, kw, normalize, np.float64)
    a, st = np.full(L, NEG, dtype=np.float64), np.full(L, -1, dtype=np.int64)
    for t in range(start, end):
        a, st = _advance(a, st, x[t], skip, t == start, t)
        if t == start:
            a[1:], st[1:] = NEG, -1          # (L = 1: nothing; else only state 0 is live after the entry)
    return float(a[L - 1]) if end > start else NEG


def brute64(lp, kw, normalize):
    """(Tb + 1, Tb + 1) float64 table of seg64 over all segments 0 <= t0 < t1 <= Tb (-inf elsewhere)."""
    Tb = np.asarray(lp).shape[0]
    tab = np.full((Tb + 1, Tb + 1), NEG)
    for t0 in range(Tb):
        for t1 in range(t0 + 1, Tb + 1):
            tab[t0, t1] = seg64(lp, kw, normalize, t0, t1)
    return tab


def spot_batch(lp, keywords, kw_len, in_len=None, max_len=None, normalize=True, dtype=np.float32):
    """wk_ctc_spot's outputs on the host: lp (B, T, V) float32, keywords (K,
    stride) -> dict of scores (B, K), spans (B, K, 2), trace (B, K, T) with the
    -inf / -1 conventions of the header."""
    lp = np.asarray(lp, dtype=np.float32)
    keywords = np.asarray(keywords, dtype=np.int64)
    B, T, V = lp.shape
    K = keywords.shape[0]
    max_len = keywords.shape[1] if max_len is None else max_len
    out = dict(scores=np.full((B, K), NEG, dtype), spans=np.full((B, K, 2), -1, np.int32), trace=np.full((B, K, T), NEG, dtype))
    for b in range(B):
        Tb = T if in_len is None else min(max(int(in_len[b]), 0), T)
        for k in range(K):
            S = min(max(int(kw_len[k]), 0), max_len)
            kw = keywords[k, :S]
            if S == 0 or Tb == 0 or kw.min() < 1 or kw.max() >= V:
                continue
            score, span, e = spot(lp[b, :Tb], kw, normalize, dtype)
            out["scores"][b, k], out["spans"][b, k], out["trace"][b, k, :Tb] = score, span, e
    return out


def log_softmax(z):
    z = np.asarray(z, dtype=np.float32)
    m = z.max(-1, keepdims=True)
    return (z - m - np.log(np.exp(z - m).sum(-1, keepdims=True, dtype=np.float32))).astype(np.float32)


def planted(T, V, kw, start, hold=2, gap=0):
    """(T, V) one-hot log-probs (0 on one token per frame, -inf elsewhere) whose
    greedy path spells `kw` from frame `start`: each label held `hold` frames,
    `gap` blanks between labels (one at least between equal labels), blanks
    elsewhere.  -> (lp, (start, first frame of the last label + 1))."""
    tok = np.zeros(T, dtype=np.int64)
    t, last_first = start, start
    for i, w in enumerate(kw):
        if i:
            t += max(gap, 1 if kw[i - 1] == w else 0)
        last_first = t
        tok[t:t + hold] = w
        t += hold
    assert t <= T
    lp = np.full((T, V), NEG, dtype=np.float32)
    lp[np.arange(T), tok] = 0.0
    return lp, (start, last_first + 1)
