"""Reference for wk_ctc_beam (numpy only): CTC prefix beam search as
include/wakeword.h states it, parametrised by dtype -- float64 is the yardstick,
float32 shows the arithmetic's own error -- with a brute-force scorer (the
float64 CTC forward over every label sequence up to a length), the margin of
an utterance's pruning decisions and the case table.

Blank is 0; W the beam width, K the per-frame candidate count.  A hypothesis
is a label prefix l with log-masses pb (paths ending in blank) and pnb (paths
ending in its last label e), total p = lse(pb, pnb).  Start: () with pb = 0,
pnb = -inf.  Per frame t < Tb, row lp:
  C_t     the min(K, V-1) non-blank ids of largest lp, ties to the lower id
          (compares only);
  stay    every live (l, pb, pnb) in slot order gives l:  pb' (+)= lp[0] + p,
          and if l is non-empty  pnb' (+)= lp[e] + pnb  (lp[e] whether or not
          e is in C_t);
  extend  every live hypothesis in slot order, c in C_t in ascending id, gives
          l + c:  pnb' (+)= lp[c] + (pb if c == e else p);
  merge   (+) is log-add-exp; an extension that is a live prefix adds to that
          prefix's stay (identity is by prefix);
  prune   totals of -inf are dropped; the W largest survive in descending
          order, equal totals in candidate order (stays by slot, then
          extensions by parent slot, then token id).
"""
import functools
import itertools

import numpy as np

NEG = -np.inf

# The largest score error of the float32 run against the float64 run over the
# whole case table (test_ctc_beam_ref.py asserts it; the measured value and the
# device's ratios are in profiles/ctc_beam_bounds.md).  TAU = 16 E32 is the
# margin above which an utterance is decisive; scores are held to TAU / 2.
E32 = 2.75e-6
TAU = 16.0 * E32


def lse(a, b, dtype):
    """log(exp(a) + exp(b)) in `dtype`: max + log1p(exp(min - max)); -inf for two -inf."""
    m, n = (a, b) if a >= b else (b, a)
    if m == NEG:
        return dtype(NEG)
    return dtype(m + np.log1p(np.exp(dtype(n - m))))


def candidates(row, K):
    """C_t in selection order: the min(K, V-1) non-blank ids by descending lp, ties to the lower id."""
    order = np.argsort(-np.asarray(row)[1:], kind="stable") + 1
    return order[:min(K, len(row) - 1)]


def step(hyps, row, W, K, dtype):
    """One frame: hyps, a list of (prefix, pb, pnb, p), and the row in `dtype`
    -> (the pruned list, C_t in selection order, every finite candidate total
    in pruning order)."""
    C = candidates(row, K)
    slot = {h[0]: j for j, h in enumerate(hyps)}
    stays = [[l, dtype(row[0] + p), dtype(row[l[-1]] + pnb) if l else dtype(NEG)] for l, pb, pnb, p in hyps]
    exts = []
    for l, pb, pnb, p in hyps:
        for c in sorted(int(c) for c in C):
            v = dtype(row[c] + (pb if (l and c == l[-1]) else p))
            j = slot.get(l + (c,))
            if j is not None:
                stays[j][2] = lse(stays[j][2], v, dtype)
            else:
                exts.append([l + (c,), dtype(NEG), v])
    allc = [(l, pb, pnb, lse(pb, pnb, dtype)) for l, pb, pnb in stays + exts]
    allc = [c for c in allc if c[3] > NEG]
    order = sorted(range(len(allc)), key=lambda i: -allc[i][3])      # stable: equal totals keep candidate order
    return [allc[i] for i in order[:W]], C, np.array([allc[i][3] for i in order], dtype=dtype)


def start(dtype):
    return [((), dtype(0.0), dtype(NEG), dtype(0.0))]


def beam_search(lp, W, K, dtype=np.float64):
    """lp (Tb, V) log-probs -> (hyps, cand): hyps the live hypotheses after the
    last frame in order, each (prefix tuple, pb, pnb, p); cand (Tb, K) int32,
    C_t in selection order, -1 beyond V-1 entries.  All arithmetic in `dtype`."""
    lp = np.asarray(lp)
    cand = np.full((lp.shape[0], K), -1, dtype=np.int32)
    hyps = start(dtype)
    for t in range(lp.shape[0]):
        hyps, C, _ = step(hyps, lp[t].astype(dtype), W, K, dtype)
        cand[t, :len(C)] = C
    return hyps, cand


def margin(lp, W, K):
    """The smallest gap, over all frames of the float64 run, at the two pruning
    boundaries: the K-th against the (K+1)-th non-blank lp, and the W-th
    against the (W+1)-th finite candidate total.  inf where neither ever binds."""
    lp = np.asarray(lp)
    hyps, g = start(np.float64), np.inf
    for t in range(lp.shape[0]):
        row = lp[t].astype(np.float64)
        hyps, _, tot = step(hyps, row, W, K, np.float64)
        v = np.sort(row[1:])[::-1]
        if len(v) > K:
            g = min(g, 0.0 if v[K - 1] == v[K] else float(v[K - 1] - v[K]))
        if len(tot) > W:
            g = min(g, float(tot[W - 1] - tot[W]))
    return g


def recreated_merges(lp, W, K):
    """How often (float64 run) an extension merges into a live prefix l + c
    whose parent l left the beam after l + c was made and has come back since:
    the prefix is the same, the search-tree node of l is not.  A case with a
    count > 0 exercises an implementation's identity check beyond 'the same
    parent node'."""
    lp = np.asarray(lp)
    hyps, born, n = start(np.float64), {(): -1}, 0      # born: the frame at which a live prefix last entered the beam
    for t in range(lp.shape[0]):
        row = lp[t].astype(np.float64)
        live = {h[0] for h in hyps}
        C = set(int(c) for c in candidates(row, K))
        n += sum(1 for l in live if l and l[-1] in C and l[:-1] in live and born[l[:-1]] > born[l])
        hyps, _, _ = step(hyps, row, W, K, np.float64)
        born = {h[0]: born.get(h[0], t) if h[0] in live else t for h in hyps}
    return n


def beam_batch(lp, in_len, W, K, n_best, max_len, dtype=np.float64):
    """wk_ctc_beam's outputs on the host: lp (B, T, V), in_len (B,) or None ->
    dict of tokens (B, n_best, max_len) int32, lengths (B, n_best) int32,
    scores (B, n_best) `dtype`, cand (B, T, K) int32, with the -1 / -inf fill
    of the header, and hyps, the full hypothesis list per utterance."""
    lp = np.asarray(lp)
    B, T, V = lp.shape
    out = dict(tokens=np.full((B, n_best, max_len), -1, np.int32), lengths=np.full((B, n_best), -1, np.int32),
               scores=np.full((B, n_best), NEG, dtype), cand=np.full((B, T, K), -1, np.int32), hyps=[])
    for b in range(B):
        Tb = T if in_len is None else min(max(int(in_len[b]), 0), T)
        hyps, cand = beam_search(lp[b, :Tb], W, K, dtype)
        out["cand"][b, :Tb] = cand
        out["hyps"].append(hyps)
        for i, (l, _, _, p) in enumerate(hyps[:n_best]):
            out["lengths"][b, i] = len(l)
            out["scores"][b, i] = p
            out["tokens"][b, i, :min(len(l), max_len)] = l[:max_len]
    return out


# ---- brute force ------------------------------------------------------------------
def ctc_loglik(lp, labels):
    """The float64 CTC log-likelihood of `labels` (the forward recursion over
    the blank-interleaved states); -inf when no path exists."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0]
    ext = np.zeros(2 * len(labels) + 1, dtype=np.int64)
    ext[1::2] = labels
    L = len(ext)
    if T == 0:
        return 0.0 if L == 1 else NEG
    skip = np.zeros(L, dtype=bool)
    if len(labels) > 1:
        lab = np.asarray(labels)
        skip[3::2] = lab[1:] != lab[:-1]
    a = np.full(L, NEG)
    a[0] = lp[0, 0]
    if L > 1:
        a[1] = lp[0, ext[1]]
    for t in range(1, T):
        n1 = np.concatenate([[NEG], a[:-1]])
        n2 = np.where(skip, np.concatenate([[NEG, NEG], a[:-2]])[:L], NEG)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.maximum(np.maximum(a, n1), n2)
            s = np.where(m == NEG, NEG, m + np.log(np.exp(a - m) + np.exp(n1 - m) + np.exp(n2 - m)))
        a = lp[t, ext] + np.where(np.isnan(s), NEG, s)
    tail = a[L - 1] if L == 1 else np.logaddexp(a[L - 1], a[L - 2])
    return float(tail)


def brute_force(lp, max_len):
    """{label tuple: float64 CTC log-likelihood} over every label sequence of
    length <= max_len with a path (finite likelihood)."""
    V = np.asarray(lp).shape[1]
    out = {}
    for n in range(max_len + 1):
        for l in itertools.product(range(1, V), repeat=n):
            v = ctc_loglik(lp, l)
            if v > NEG:
                out[l] = v
    return out


# ---- the case table ---------------------------------------------------------------
def log_softmax(z):
    z = np.asarray(z, dtype=np.float32)
    m = z.max(-1, keepdims=True)
    return (z - m - np.log(np.exp(z - m).sum(-1, keepdims=True, dtype=np.float32))).astype(np.float32)


BATCH = 16                       # utterances per case
# (T, V, W, K, logit scale): Gaussian logits of that scale, the blank column raised by the same amount
SHAPES = [(32, 12, 4, 3, 4.0), (32, 12, 8, 11, 4.0), (32, 40, 16, 8, 5.0), (24, 300, 32, 16, 6.0), (24, 300, 64, 8, 6.0),
          (12, 6, 64, 5, 3.0)]
CASE_IDS = [f"T{t}-V{v}-W{w}-K{k}" for t, v, w, k, _ in SHAPES]


@functools.lru_cache(maxsize=None)
def case(shape):
    """-> lp (BATCH, T, V) float32 log_softmax rows."""
    T, V, W, K, scale = shape
    rng = np.random.default_rng(7000 + 100 * T + V + 13 * W + K)
    z = scale * rng.standard_normal((BATCH, T, V))
    z[:, :, 0] += scale
    return log_softmax(z)


@functools.lru_cache(maxsize=None)
def case_reference(shape):
    """-> (float64 beam_batch with n_best = W, max_len = T; margins (BATCH,))."""
    T, V, W, K, _ = shape
    lp = case(shape)
    return beam_batch(lp, None, W, K, W, T, np.float64), np.array([margin(lp[b], W, K) for b in range(BATCH)])


def score_error32(shape):
    """The largest |float32 score - float64 score| over the hypotheses both
    runs hold at the same rank with the same prefix, and the number compared."""
    T, V, W, K, _ = shape
    lp = case(shape)
    ref, _ = case_reference(shape)
    worst, n = 0.0, 0
    for b in range(BATCH):
        h32, _ = beam_search(lp[b], W, K, np.float32)
        for a, r in zip(h32, ref["hyps"][b]):
            if a[0] == r[0]:
                worst, n = max(worst, abs(float(a[3]) - float(r[3]))), n + 1
    return worst, n
