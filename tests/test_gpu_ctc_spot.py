"""wk_ctc_spot / wakeword.ctc_spot / CTCModel.spot / KeywordSpotter on the MI355X.

Exact oracle: scores, spans and frame scores are BIT-EQUAL to the float32
numpy reference (tests/ctc_spot_ref.py) -- no tolerance: the recurrence is one
exact max and one IEEE add per state (with normalize one IEEE subtract more),
so the lane layout cannot change a bit.  The outputs start as a sentinel / NaN,
and every call is made with and without the optional trace.

Independent check against float64, for every pair with a finite score: with
opt64 the float64 optimum over all segments and seg64(span) the float64 optimum
inside the span the device chose,
    opt64 - seg64(span) <= c Tb 2^-24 |opt64|   and   |score - seg64(span)| <= the same
c = 4 without normalize (each of at most Tb adds rounds by at most 2^-24 of a
partial sum no larger than the total, once for the chosen path and once for
the optimum, times 2 for second-order terms; holds for x <= 0), c = 8 with
normalize (the subtract rounds too).  Largest measured ratio to this bound:
profiles/ctc_spot_bounds.md.

Shapes are the smallest that reach each path of the kernels: S with 1, 3, 15,
17, 31, 61 and 63 states (the last lane), T on both sides of the prefetch
group (G = 16 rows) and of the 64-frame trace and row-maximum chunk, vocabularies
with every head / quad / tail split of the row-maximum loads."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_spot_ref as R

SENT = 0x5A5A5A5A
G = 16                 # kSpotGroup: rows in flight
WORST = {False: 0.0, True: 0.0}


def raw(lp, kws, kw_len, in_len=None, max_len=None, normalize=True, trace=True, stream=None):
    """One wk_ctc_spot call through the C ABI on (B, T, V) host log-probs -> dict
    of host arrays.  The outputs start as a sentinel / NaN, so anything the call
    leaves unwritten shows."""
    from wakeword import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    d_lp = torch.as_tensor(lp, dtype=torch.float32).to(dev).contiguous()
    B, T, V = d_lp.shape
    d_kw = torch.as_tensor(np.asarray(kws), dtype=torch.int32).to(dev).contiguous()
    K = d_kw.shape[0]
    smax = d_kw.shape[1] if max_len is None else max_len
    kl = torch.tensor(kw_len, dtype=torch.int32, device=dev)
    il = torch.tensor(in_len, dtype=torch.int32, device=dev) if in_len is not None else None
    nbytes = L.wk_ctc_spot_workspace_bytes(B, T, K, smax)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    scores = torch.full((B, K), float("nan"), device=dev)
    spans = torch.full((B, K, 2), SENT, dtype=torch.int32, device=dev)
    tr = torch.full((B, K, T), float("nan"), device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    _lib.check(L.wk_ctc_spot(p(d_lp), B, T, V, p(il), p(d_kw), d_kw.shape[1], p(kl), K, smax, int(normalize), p(ws), p(scores),
                             p(spans), p(tr) if trace else None, 0, C.c_void_p(s.cuda_stream)), "wk_ctc_spot")
    s.synchronize()
    return dict(scores=scores.cpu().numpy(), spans=spans.cpu().numpy(), trace=tr.cpu().numpy())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(got, want, keys=("scores", "spans", "trace")):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(bits(got[k]), bits(want[k])), (k, got[k], want[k])


def check(lp, kws, kw_len, in_len=None, max_len=None, normalize=True, tag=""):
    """Run with and without the trace, compare bit for bit with the float32
    reference, check each finite pair against float64.  Returns the device outputs."""
    lp = np.asarray(lp, dtype=np.float32)
    kws = np.asarray(kws)
    got = raw(lp, kws, kw_len, in_len, max_len, normalize)
    want = R.spot_batch(lp, kws, kw_len, in_len, max_len, normalize)
    same(got, want)
    bare = raw(lp, kws, kw_len, in_len, max_len, normalize, trace=False)
    same(bare, got, keys=("scores", "spans"))
    assert np.isnan(bare["trace"]).all()                       # the optional output is left alone
    B, T, V = lp.shape
    smax = kws.shape[1] if max_len is None else max_len
    c = 8.0 if normalize else 4.0
    for b in range(B):
        Tb = T if in_len is None else min(max(int(in_len[b]), 0), T)
        assert (got["trace"][b, :, Tb:] == -np.inf).all()
        for k in range(kws.shape[0]):
            score, (t0, t1) = got["scores"][b, k], got["spans"][b, k]
            if score == -np.inf:
                assert (t0, t1) == (-1, -1)
                continue
            kw = kws[k, :min(max(int(kw_len[k]), 0), smax)]
            assert 0 <= t0 < t1 <= Tb and score == got["trace"][b, k, t1 - 1]
            assert not (got["trace"][b, k, :t1 - 1] >= score).any()        # the first frame that attains the maximum
            opt64 = float(R.spot(lp[b, :Tb], kw, normalize, np.float64)[0])
            s64 = R.seg64(lp[b, :Tb], kw, normalize, t0, t1)
            gap, err, bound = opt64 - s64, abs(float(score) - s64), c * Tb * R.EPS32 * abs(opt64)
            ratio = max(gap, err) / bound if bound > 0 else 0.0
            WORST[bool(normalize)] = max(WORST[bool(normalize)], ratio)
            print(f"ctc-spot {tag} norm={int(normalize)} b={b} k={k} Tb={Tb} S={len(kw)} opt64={opt64:.6f} gap={gap:.3e} "
                  f"err={err:.3e} bound={bound:.3e} ratio={ratio:.3f} worst so far={WORST[bool(normalize)]:.3f}")
            assert 0.0 <= gap <= bound and err <= bound
    return got


def rand_lp(rng, B, T, V):
    return R.log_softmax(rng.standard_normal((B, T, V)))


def keywords_of(rng, lens, V, stride=None, repeats=False):
    """(K, stride) padded keywords of the given lengths, labels in [1, V); the
    padding holds a label out of range, which is never read."""
    stride = max(max(lens), 1) if stride is None else stride
    kws = np.full((len(lens), stride), V + 7, dtype=np.int64)
    for k, n in enumerate(lens):
        w = rng.integers(1, V, size=n)
        if not repeats and V > 2:
            for i in range(1, n):
                while w[i] == w[i - 1]:
                    w[i] = rng.integers(1, V)
        kws[k, :n] = w
    return kws


BOTH = pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalized"])


# ---- keyword lengths: 1, 3, 15, 17, 31, 61 and 63 states ------------------------------
@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("S", [1, 2, 8, 9, 16, 31, 32])
def test_keyword_lengths(gpu, S, normalize):
    """K = 3: no adjacent repeats (feasible in S frames), plain random labels
    (repeats need blanks), and a single label; T = 2 S + 3, the second
    utterance one frame short."""
    rng = np.random.default_rng(S)
    T, V = 2 * S + 3, 11
    kws = np.concatenate([keywords_of(rng, [S], V), keywords_of(rng, [S], V, repeats=True), keywords_of(rng, [1], V, stride=S)])
    got = check(rand_lp(rng, 2, T, V), kws, [S, S, 1], [T, T - 1], normalize=normalize, tag=f"S{S}")
    assert np.isfinite(got["scores"][:, 0]).all() and np.isfinite(got["scores"][:, 2]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 8, 9, 16, 31, 32])
def test_all_labels_equal_exactly_feasible(gpu, S):
    """All labels equal: no skip, Tb = 2S-1 has the single path 0, 1, ..., 2S-2 and Tb = 2S-2 none."""
    rng = np.random.default_rng(100 + S)
    T, V = 2 * S - 1, 7
    kws = np.full((1, S), 1 + S % 6, dtype=np.int64)
    got = check(rand_lp(rng, 2, T, V), kws, [S], [T, T - 1], normalize=False, tag=f"equal-S{S}")
    assert got["spans"][0, 0].tolist() == [0, T] and np.isfinite(got["scores"][0, 0])
    assert got["scores"][1, 0] == -np.inf and got["spans"][1, 0].tolist() == [-1, -1]


# ---- the prefetch group (16 rows) and the 64-frame trace / row-maximum chunks ----------
@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("T", [1, 2, G - 1, G, G + 1, 63, 64, 65, 130])
def test_group_and_chunk_boundaries(gpu, T, normalize):
    rng = np.random.default_rng(1000 + T)
    V = 9
    lens = [min(5, T), 1, min(12, T)]
    kws = keywords_of(rng, lens, V, stride=14)
    check(rand_lp(rng, 3, T, V), kws, lens, [T, T - 1, T // 2], max_len=12, normalize=normalize, tag=f"T{T}")
    check(rand_lp(rng, 1, T, V), kws, lens, None, max_len=12, normalize=normalize, tag=f"T{T}-nolen")


# ---- vocabulary: every head / quad / tail split of the row-maximum loads ---------------
@pytest.mark.gpu
@pytest.mark.parametrize("V", [2, 5, 63, 65, 257, 4000])
def test_vocabulary(gpu, V):
    """B = 3, T = 5: with an odd V the rows start at every alignment.  The frame
    maximum is planted at the first, the last and a middle column of some rows."""
    rng = np.random.default_rng(V)
    B, T = 3, 5
    lp = rand_lp(rng, B, T, V)
    lp[0, 1, 0] = lp[1, 2, V - 1] = lp[2, 3, V // 2] = 0.0
    kws = np.array([[1, V - 1], [V - 1, 1], [V - 1, V - 1]], dtype=np.int64)       # V = 2: equal labels, the blank between them
    for normalize in (True, False):
        check(lp, kws, [2, 2, 1], [T, T, T - 1], normalize=normalize, tag=f"V{V}")


# ---- several keywords of mixed lengths, ragged inputs ----------------------------------
def _mixed_case(B, seed=0):
    rng = np.random.default_rng(seed)
    T, V = 40, 13
    lens = [3, 1, 9, 2, 5, 9, 4]
    kws = keywords_of(rng, lens, V, stride=11, repeats=True)
    in_len = [T] if B == 1 else [-2, T + 9, 17]          # beyond the range: clamped to 0 and T
    return rand_lp(rng, B, T, V), kws, lens, in_len


@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("B", [1, 3])
def test_mixed_keywords_ragged_lengths(gpu, B, normalize):
    lp, kws, lens, in_len = _mixed_case(B)
    got = check(lp, kws, lens, in_len, max_len=9, normalize=normalize, tag=f"mixed-B{B}")
    if B == 3:
        assert (got["scores"][0] == -np.inf).all() and (got["spans"][0] == -1).all()       # Tb = 0
        assert np.isfinite(got["scores"][1]).all()
    # one keyword alone gives the bits it has among the seven
    for k in (0, 2, 6):
        alone = raw(lp, kws[k:k + 1], lens[k:k + 1], in_len, 9, normalize)
        for key in ("scores", "spans", "trace"):
            assert np.array_equal(bits(alone[key][:, 0]), bits(got[key][:, k])), (key, k)


# ---- edge cases ------------------------------------------------------------------------
@pytest.mark.gpu
@BOTH
def test_no_occurrence_next_to_valid_keywords(gpu, normalize):
    """A keyword longer than Tb, invalid labels, empty and negative lengths: score
    -inf, span (-1, -1), a trace of -inf -- and the neighbours keep their bits."""
    rng = np.random.default_rng(11)
    B, T, V = 2, 12, 13
    lp = rand_lp(rng, B, T, V)
    good = keywords_of(rng, [4, 2, 6], V, stride=16)
    clean = raw(lp, good, [4, 2, 6], [T, 5], 16, normalize)
    kws = np.full((9, 16), 3, dtype=np.int64)
    kws[[0, 4, 8]] = good
    kws[1, :13] = np.arange(1, 14) % 12 + 1                      # 13 distinct-neighbour labels: longer than both inputs
    kws[2, :3] = [2, 0, 5]                                       # the blank as a label
    kws[3, :3] = [2, V, 5]                                       # V
    kws[5, :3] = [-5, 2, 5]                                      # negative
    kws[6, :3] = [2, 5, 1 << 30]                                 # huge
    lens = [4, 13, 3, 3, 2, 3, 3, 0, 6]
    lens[7] = -3                                                 # clamped to 0; row 7 is otherwise a valid keyword
    got = check(lp, kws, lens, [T, 5], max_len=16, normalize=normalize, tag="no-occurrence")
    for k in (1, 2, 3, 5, 6, 7):
        assert (got["scores"][:, k] == -np.inf).all() and (got["spans"][:, k] == -1).all() and (got["trace"][:, k] == -np.inf).all()
    for k, j in ((0, 0), (4, 1), (8, 2)):
        for key in ("scores", "spans", "trace"):
            assert np.array_equal(bits(got[key][:, k]), bits(clean[key][:, j]))
    assert got["scores"][1, 8] == -np.inf and np.isfinite(got["scores"][0, 8])     # 6 labels, Tb = 5


@pytest.mark.gpu
@BOTH
def test_repeated_labels(gpu, normalize):
    rng = np.random.default_rng(5)
    V, T = 6, 20
    kws = np.array([[2, 2, 2, 0], [1, 1, 3, 3], [4, 5, 5, 4], [3, 0, 0, 0]], dtype=np.int64)
    got = check(rand_lp(rng, 2, T, V), kws, [3, 4, 4, 1], [T, 5], normalize=normalize, tag="repeats")
    assert got["scores"][1, 1] == -np.inf and np.isfinite(got["scores"][1, [0, 2, 3]]).all()     # Tb = 5: 2+2 labels need 6


@pytest.mark.gpu
@BOTH
def test_minus_infinity_entries(gpu, normalize):
    """-inf entries: scattered, at the column that is another frame's maximum, a
    keyword's own column, and a whole row (no path may cross it)."""
    rng = np.random.default_rng(17)
    B, T, V = 3, 30, 7
    lp = rand_lp(rng, B, T, V)
    lp[rng.random(lp.shape) < 0.15] = -np.inf
    top = lp.argmax(axis=2)
    lp[0, 5, top[0, 6]] = -np.inf                    # frame 6's maximum column, at frame 5
    lp[1, :, 3] = -np.inf                            # label 3 never occurs in utterance 1
    lp[2, 14, :] = -np.inf                           # nothing at all at one frame
    kws = keywords_of(rng, [2, 4, 1], V, stride=4)
    kws[1, 1] = 3
    got = check(lp, kws, [2, 4, 1], [T, T, T], normalize=normalize, tag="minus-inf")
    assert got["scores"][1, 1] == -np.inf and got["spans"][1, 1].tolist() == [-1, -1]
    assert got["trace"][2, :, 14].tolist() == [-np.inf] * 3
    for k in range(3):                               # no span of utterance 2 crosses frame 14
        t0, t1 = got["spans"][2, k]
        assert t1 <= 14 or t0 > 14 or t0 == -1


@pytest.mark.gpu
def test_planted_keyword_scores_zero(gpu):
    """One-hot rows along a planted keyword: normalized score exactly 0, the
    span from the first label's first frame to the last label's first frame + 1;
    one frame of it broken: a lower or no score, the neighbour unaffected."""
    kw = [3, 1, 1, 4, 2]
    lp0, want = R.planted(70, 6, kw, start=9, hold=3, gap=2)
    lp1 = lp0.copy()
    lp1[want[0] + 1:want[0] + 3, :] = -np.inf         # the first label is left one frame, then nothing
    kws = np.array([kw, [4, 2, 0, 0, 0], [5, 0, 0, 0, 0]], dtype=np.int64)
    for normalize in (True, False):
        got = check(np.stack([lp0, lp1]), kws, [5, 2, 1], None, normalize=normalize, tag="planted")
        assert got["scores"][0, 0] == 0.0 and got["spans"][0, 0].tolist() == list(want)
        assert got["scores"][:, 1].tolist() == [0.0, 0.0] and got["spans"][0, 1].tolist() == got["spans"][1, 1].tolist()
        assert got["scores"][1, 0] == -np.inf and (got["scores"][:, 2] == -np.inf).all()


@pytest.mark.gpu
def test_tie_rule_uniform_rows(gpu):
    """lp = -ln V everywhere: without normalize the shortest segment wins and the
    first end among the equal ones; with it every path ties at exactly 0 and
    stay is preferred, so the start stays at frame 0."""
    V, T = 7, 70
    lp = np.full((1, T, V), -np.log(np.float32(V)), dtype=np.float32)
    kws = np.array([[2, 2, 5], [1, 2, 3], [4, 0, 0]], dtype=np.int64)
    got = check(lp, kws, [3, 3, 1], None, normalize=False, tag="ties-raw")
    assert got["spans"][0].tolist() == [[0, 4], [0, 3], [0, 1]]
    got = check(lp, kws, [3, 3, 1], None, normalize=True, tag="ties-normalized")
    assert (got["scores"] == 0.0).all() and got["spans"][0].tolist() == [[0, 4], [0, 3], [0, 1]]


@pytest.mark.gpu
def test_reference_shape(gpu):
    """T = 801, V = 4000, S = 4: a keyword boosted along a planted stretch of an
    otherwise random utterance is found there; ragged second utterance."""
    rng = np.random.default_rng(801)
    T, V = 801, 4000
    z = rng.standard_normal((2, T, V)).astype(np.float32)
    kw = [17, 3999, 256, 1]
    tok = np.zeros(T, dtype=np.int64)
    for i, w in enumerate(kw):
        tok[300 + 12 * i:308 + 12 * i] = w
    z[0, np.arange(T), tok] += 14.0
    kws = np.array([kw, [5, 5, 9, 0]], dtype=np.int64)
    lp = R.log_softmax(z)
    got = check(lp, kws, [4, 3], [T, 700], normalize=True, tag="T801-V4000")
    assert got["spans"][0, 0].tolist() == [300, 337] and got["scores"][0, 0] == 0.0
    check(lp, kws, [4, 3], [T, 700], normalize=False, tag="T801-V4000")


@pytest.mark.gpu
def test_offsets_past_2_31_elements(gpu):
    """B = 5, T = 8200, V = 65536: utterance 4 starts 2.15e9 elements into the
    log-probs, past what a 32-bit element index reaches.  Only its first 40
    rows are filled and used (the other utterances have length 0; the rest of
    the tensor is uninitialised and never used)."""
    B, T, V, Tb = 5, 8200, 65536, 40
    assert (B - 1) * T * V > 2 ** 31
    rows = R.log_softmax(np.random.default_rng(31).standard_normal((Tb, V)))
    d = torch.empty((B, T, V), dtype=torch.float32, device="cuda:0")
    d[B - 1, :Tb] = torch.from_numpy(rows).to("cuda:0")
    kws, lens = np.array([[7, 65535, 40000], [1, 0, 0]], dtype=np.int64), [3, 1]
    for normalize in (False, True):
        got = raw(d, kws, lens, [0] * (B - 1) + [Tb], normalize=normalize)
        assert (got["scores"][:B - 1] == -np.inf).all() and (got["spans"][:B - 1] == -1).all()
        assert (got["trace"][:B - 1] == -np.inf).all() and (got["trace"][B - 1, :, Tb:] == -np.inf).all()
        for k in range(2):
            score, span, e = R.spot(rows, kws[k, :lens[k]], normalize)
            assert np.isfinite(score) and bits(got["scores"])[B - 1, k] == bits(np.float32(score).reshape(1))[0]
            assert tuple(got["spans"][B - 1, k]) == span
            assert np.array_equal(bits(got["trace"][B - 1, k, :Tb]), bits(e))
    del d
    torch.cuda.empty_cache()


# ---- call conditions -------------------------------------------------------------------
@pytest.mark.gpu
def test_two_calls_and_non_default_stream(gpu):
    lp, kws, lens, in_len = _mixed_case(3, seed=2)
    for normalize in (True, False):
        got = raw(lp, kws, lens, in_len, 9, normalize)
        same(raw(lp, kws, lens, in_len, 9, normalize), got)                       # two calls: the same bits
        same(raw(lp, kws, lens, in_len, 9, normalize, stream=torch.cuda.Stream()), got)


# ---- the Python surface ----------------------------------------------------------------
def _host(spot):
    return dict(scores=spot.scores.cpu().numpy(), spans=spot.spans.cpu().numpy(),
                trace=spot.frame_scores.cpu().numpy() if spot.frame_scores is not None else None)


@pytest.mark.gpu
def test_ctc_spot_python_forms(gpu):
    """(T, B, V) with a list of label lists == batch-first with a padded tensor and lengths == the raw call."""
    import wakeword
    lp, kws, lens, in_len = _mixed_case(3, seed=3)
    kws = np.where(kws > 12, 0, kws)[:, :9]
    want = raw(lp, kws, lens, in_len, 9, True)
    d = torch.from_numpy(lp).to("cuda:0")
    a = wakeword.ctc_spot(d, torch.from_numpy(kws), lens, in_len, frame_scores=True, batch_first=True)
    b = wakeword.ctc_spot(d.transpose(0, 1).contiguous(), [kws[k, :n].tolist() for k, n in enumerate(lens)],
                          input_lengths=torch.tensor(in_len), frame_scores=True)
    for sp in (a, b):
        assert isinstance(sp, wakeword.Spot) and sp.scores.is_cuda
        same(_host(sp), want)
    c = wakeword.ctc_spot(d, kws, lens, in_len, normalize=False, batch_first=True)
    assert c.frame_scores is None
    same(_host(c), raw(lp, kws, lens, in_len, 9, False), keys=("scores", "spans"))
    sec = wakeword.span_seconds(a.spans)
    assert sec.is_cuda and torch.equal(sec, torch.where(a.spans < 0, -1.0, a.spans.double() * 0.01))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_through_the_model(gpu, precision):
    """CTCModel.spot on a random-weight model (B = 2, T = 40, V = 50) equals
    ctc_spot of its own forward(..., return_log_probs=True), and the reference."""
    import wakeword
    from wakeword.ctc import random_state_dict
    V = 50
    model = wakeword.CTCModel(random_state_dict(V, seed=4), V, precision=precision)
    feats = torch.randn((2, 40, 80), generator=torch.Generator().manual_seed(9))
    kws, lens = [[3, 3, 17], [8], [49, 2, 5, 1]], [3, 1, 4]
    _, lp = model.forward(feats, return_log_probs=True)
    assert lp.dtype == torch.float32
    for il in (None, [40, 33]):
        got = model.spot(feats, kws, input_lengths=il, frame_scores=True)
        want = wakeword.ctc_spot(lp, kws, input_lengths=il, frame_scores=True, batch_first=True)
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        assert bool(torch.isfinite(got.scores).all()) and bool((got.scores <= 0).all())
    padded = np.array([w + [0] * (4 - len(w)) for w in kws])
    same(_host(got), R.spot_batch(lp.cpu().numpy(), padded, lens, [40, 33]))


class _PlantedModel:
    """CTCModel's spot_audio on fixed log-probs: what KeywordSpotter.detect calls."""

    def __init__(self, lp):
        self.lp = lp

    def spot_audio(self, audio, keywords, keyword_lengths=None, n_samples=0, normalize=True, frame_scores=False):
        import wakeword
        return wakeword.ctc_spot(self.lp, keywords, keyword_lengths, normalize=normalize, frame_scores=frame_scores,
                                 batch_first=True)


@pytest.mark.gpu
def test_keyword_spotter_detects_the_planted_keyword(gpu):
    import wakeword
    c2i = {"x": 1, "i": 2, "a": 3, "o": 4, "b": 5}
    lp0, (t0, t1) = R.planted(120, 6, [1, 2, 3, 4], start=31, hold=4, gap=1)       # "xiao" from frame 31
    lp1 = R.planted(120, 6, [5, 3], start=80, hold=2)[0]                           # "ba": holds "a", not "xiao"
    spotter = wakeword.KeywordSpotter(_PlantedModel(torch.from_numpy(np.stack([lp0, lp1])).to("cuda:0")), c2i,
                                      ["xiao", "a", "ob"], threshold=0.8)
    got = spotter.detect(np.zeros((2, 19200), dtype=np.float32))
    assert [(d.utterance, d.keyword, d.confidence) for d in got] == [(0, "xiao", 1.0), (0, "a", 1.0), (1, "a", 1.0)]
    assert (t0, t1) == (31, 47) and (got[0].start_s, got[0].end_s) == (0.31, 0.47)
    assert (got[1].start_s, got[1].end_s) == (0.41, 0.42) and (got[2].start_s, got[2].end_s) == (0.82, 0.83)


@pytest.mark.gpu
def test_spot_audio(gpu):
    """0.5 s of synthetic audio through features, the GRU-CTC forward and the
    spotter: confidences in (0, 1], spans inside [0, T]."""
    import wakeword
    from wakeword.ctc import random_state_dict
    V, n = 50, 8000
    model = wakeword.CTCModel(random_state_dict(V, seed=4), V)
    t = np.arange(n, dtype=np.float32) / 16000.0
    audio = np.stack([0.3 * np.sin(2 * np.pi * f * t) * np.sin(2 * np.pi * 3.0 * t) ** 2 for f in (440.0, 1250.0)]).astype(np.float32)
    sp = model.spot_audio(audio, [[3, 7, 7, 12], [20, 5]], n_samples=n, frame_scores=True)
    T = 1 + n // 160
    assert sp.scores.shape == (2, 2) and sp.spans.shape == (2, 2, 2) and sp.frame_scores.shape == (2, 2, T)
    conf, spans = torch.exp(sp.scores).cpu().numpy(), sp.spans.cpu().numpy()
    assert ((conf > 0) & (conf <= 1)).all()
    assert (spans[..., 0] >= 0).all() and (spans[..., 0] < spans[..., 1]).all() and (spans[..., 1] <= T).all()
    assert torch.equal(sp.frame_scores.max(dim=2).values, sp.scores)
