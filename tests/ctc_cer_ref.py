"""numpy reference of wk_ctc_cer (include/wakeword.h): the row recurrence on
int64 keys d * 2^16 + s, the greedy CTC collapse, the oracle choice and the
corpus totals.  Everything is integer, so the device outputs must be equal."""
import numpy as np

INS = DEL = 1 << 16
SUB = (1 << 16) + 1

_CACHE = {}


def collapse(labels):
    """The labels of the frames with label_t != 0 and label_t != label_{t-1}, label_{-1} = 0."""
    x = np.asarray(labels, dtype=np.int64).reshape(-1)
    keep = (x != 0) & (x != np.concatenate([[0], x[:-1]]))
    return x[keep]


def edit_key(h, r):
    """min over alignments of the additive cost (match 0, insertion / deletion
    2^16, substitution 2^16 + 1) = d * 2^16 + s, one row at a time: the
    deletion chain cur_j = min(tmp_j, cur_{j-1} + DEL) as a prefix minimum of
    tmp_j - j DEL."""
    h, r = np.asarray(h, dtype=np.int64).reshape(-1), np.asarray(r, dtype=np.int64).reshape(-1)
    at = (h.tobytes(), r.tobytes())
    if at not in _CACHE:
        jd = np.arange(len(r) + 1, dtype=np.int64) * DEL
        prev = jd.copy()
        tmp = np.empty_like(prev)
        for i, tok in enumerate(h, 1):
            tmp[0] = i * INS
            tmp[1:] = np.minimum(prev[1:] + INS, prev[:-1] + np.where(r == tok, 0, SUB))
            prev = np.minimum.accumulate(tmp - jd) + jd
        _CACHE[at] = int(prev[-1])
    return _CACHE[at]


def edit_stats(h, r):
    """(d, s, del, ins) of hypothesis h against reference r."""
    key = edit_key(h, r)
    d, s = key >> 16, key & 0xFFFF
    dele = (d - s - (len(h) - len(r))) // 2
    return d, s, dele, d - s - dele


def cer_batch(hyp, hyp_len, ref, ref_len, max_ref_len=None, collapse_frames=False):
    """wk_ctc_cer on host arrays: hyp (B, H, stride) or (B, stride), hyp_len
    (B * H,) or None (collapse only), ref (B, ref_stride), ref_len (B,).
    Returns stats (B, H, 4) int32, best (B,) int32, totals (2, 8) int64, and the
    hypothesis lengths n (B, H)."""
    hyp = np.asarray(hyp)
    if hyp.ndim == 2:
        hyp = hyp[:, None, :]
    ref = np.asarray(ref)
    B, H, stride = hyp.shape
    max_ref_len = ref.shape[1] if max_ref_len is None else max_ref_len
    hl = None if hyp_len is None else np.asarray(hyp_len).reshape(B, H)
    stats = np.zeros((B, H, 4), dtype=np.int32)
    n = np.zeros((B, H), dtype=np.int64)
    m = np.zeros((B,), dtype=np.int64)
    for b in range(B):
        m[b] = min(max(int(ref_len[b]), 0), max_ref_len)
        r = ref[b, :m[b]]
        for k in range(H):
            ln = stride if hl is None else min(max(int(hl[b, k]), 0), stride)
            h = collapse(hyp[b, k, :ln]) if collapse_frames else hyp[b, k, :ln]
            n[b, k] = len(h)
            stats[b, k] = edit_stats(h, r)
    best = np.zeros((B,), dtype=np.int32)
    totals = np.zeros((2, 8), dtype=np.int64)
    for b in range(B):
        best[b] = min(range(H), key=lambda k: (stats[b, k, 0], stats[b, k, 1], k))
        for row, k in ((0, 0), (1, best[b])):
            totals[row, :4] += stats[b, k]
            totals[row, 4] += m[b]
            totals[row, 5] += n[b, k]
            totals[row, 6] += stats[b, k, 0] > 0
            totals[row, 7] += 1
    return dict(stats=stats, best=best, totals=totals, n=n)


def tuple_dp(h, r):
    """(d, s) by a plain lexicographic DP on (non-match moves, substitutions) tuples."""
    N, M = len(h), len(r)
    D = [[None] * (M + 1) for _ in range(N + 1)]
    for i in range(N + 1):
        for j in range(M + 1):
            if i == 0 or j == 0:
                D[i][j] = (i + j, 0)
                continue
            a, b, c = D[i - 1][j], D[i][j - 1], D[i - 1][j - 1]
            diag = c if h[i - 1] == r[j - 1] else (c[0] + 1, c[1] + 1)
            D[i][j] = min((a[0] + 1, a[1]), (b[0] + 1, b[1]), diag)
    return D[N][M]


def exhaustive(h, r):
    """(d, s): the smallest (non-match moves, substitutions) over every monotone alignment, enumerated."""
    N, M = len(h), len(r)

    def walk(i, j, cost, subs):
        if i == N and j == M:
            yield cost, subs
            return
        if i < N:
            yield from walk(i + 1, j, cost + 1, subs)                     # insertion
        if j < M:
            yield from walk(i, j + 1, cost + 1, subs)                     # deletion
        if i < N and j < M:
            hit = h[i] == r[j]
            yield from walk(i + 1, j + 1, cost + (not hit), subs + (not hit))
    return min(walk(0, 0, 0, 0))
