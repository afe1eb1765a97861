"""wk_ctc_beam / wakeword.ctc_beam_search / CTCModel.beam_decode on the MI355X.

The candidate stage is compares only, so d_cand is BIT-EQUAL to the reference's
C_t (tests/ctc_beam_ref.py).  The recurrence sums in fp32 with the device's exp
and log, so it is held to the float64 reference through the margin rule: with
E32 the float32 reference's own score error over the case table (pinned in
ctc_beam_ref.py) and tau = 16 E32, an utterance whose smallest pruning gap
exceeds tau is decisive, and on it the device makes every decision of the
reference -- the same hypotheses, in the same order wherever adjacent
reference scores are more than tau apart, the same tokens and lengths -- with
every score within tau / 2.  On every utterance, decisive or not, a score is at
most the hypothesis's full float64 CTC log-likelihood + tau / 2 (a beam sums a
subset of its paths).  Largest measured score error against tau / 2:
profiles/ctc_beam_bounds.md.

Shapes are the smallest that reach each path: rows at every 16-byte
misalignment with head, quads and tail, more than one 256-element chunk, beam
slots and candidate counts at both ends of their ranges, every KMAX
instantiation (K <= 8, <= 16, <= 32)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_beam_ref as R

SENT = 0x5A5A5A5A
HALF_TAU = R.TAU / 2


def raw(lp, in_len, W, K, n_best=None, max_len=None, cand=True, stream=None, offset=0):
    """One wk_ctc_beam call through the C ABI on (B, T, V) host log-probs -> dict
    of host arrays.  The outputs start as a sentinel / NaN, so anything the call
    leaves unwritten shows.  `offset` floats in front of the log-probs move
    their base off a 16-byte boundary."""
    from wakeword import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    lp = np.ascontiguousarray(lp, dtype=np.float32)
    B, T, V = lp.shape
    n_best = W if n_best is None else n_best
    max_len = T if max_len is None else max_len
    flat = torch.empty(offset + lp.size, dtype=torch.float32, device=dev)
    flat[offset:] = torch.from_numpy(lp).reshape(-1).to(dev)
    d_lp = flat[offset:]
    il = torch.tensor(in_len, dtype=torch.int32, device=dev) if in_len is not None else None
    nbytes = L.wk_ctc_beam_workspace_bytes(B, T, W, K)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tokens = torch.full((B, n_best, max_len), SENT, dtype=torch.int32, device=dev)
    lengths = torch.full((B, n_best), SENT, dtype=torch.int32, device=dev)
    scores = torch.full((B, n_best), float("nan"), device=dev)
    d_cand = torch.full((B, T, K), SENT, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    _lib.check(L.wk_ctc_beam(p(d_lp), B, T, V, p(il), W, K, n_best, max_len, p(ws), p(tokens), p(lengths), p(scores),
                             p(d_cand) if cand else None, 0, C.c_void_p(s.cuda_stream)), "wk_ctc_beam")
    s.synchronize()
    return dict(tokens=tokens.cpu().numpy(), lengths=lengths.cpu().numpy(), scores=scores.cpu().numpy(),
                cand=d_cand.cpu().numpy())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(got, want, keys=("tokens", "lengths", "scores", "cand")):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(bits(got[k]), bits(want[k])), (k, got[k], want[k])


def hyps_of(got, b):
    """Utterance b's hypotheses as (prefix tuple, score), with the fill checked."""
    out = []
    n_best, max_len = got["tokens"].shape[1:]
    seen_empty = False
    for i in range(n_best):
        n = int(got["lengths"][b, i])
        row = got["tokens"][b, i]
        if n < 0:
            seen_empty = True
            assert n == -1 and got["scores"][b, i] == -np.inf and (row == -1).all()
            continue
        assert not seen_empty                                   # the empty slots are the last ones
        assert (row[min(n, max_len):] == -1).all() and (row[:min(n, max_len)] >= 1).all()
        assert np.isfinite(got["scores"][b, i])
        out.append((tuple(int(x) for x in row[:min(n, max_len)]), float(got["scores"][b, i]), n))
    return out


WORST = {"ratio": 0.0}


def check(lp, in_len, W, K, tag="", need_decisive=True, **kw):
    """Run with n_best = W and max_len = T, check the candidate stage bit for
    bit and every utterance against the float64 reference by the margin rule.
    Returns (device outputs, reference, decisive mask)."""
    lp = np.asarray(lp, dtype=np.float32)
    B, T, V = lp.shape
    got = raw(lp, in_len, W, K, **kw)
    ref = R.beam_batch(lp, in_len, W, K, W, T, np.float64)
    assert np.array_equal(got["cand"], ref["cand"])
    decisive = np.zeros(B, dtype=bool)
    for b in range(B):
        Tb = T if in_len is None else min(max(int(in_len[b]), 0), T)
        dev = hyps_of(got, b)
        assert len({h[0] for h in dev}) == len(dev)             # no prefix twice: identity is exact
        for l, s, n in dev:
            assert n == len(l)
            full = R.ctc_loglik(lp[b, :Tb], l)
            assert s <= full + HALF_TAU, (b, l, s, full)
        want = [(h[0], float(h[3])) for h in ref["hyps"][b]]
        decisive[b] = R.margin(lp[b, :Tb], W, K) > R.TAU
        if not decisive[b]:
            continue
        assert {h[0] for h in dev} == {h[0] for h in want}, (b, dev, want)
        pos = {h[0]: i for i, h in enumerate(dev)}
        err = 0.0
        for i, (l, s) in enumerate(want):
            err = max(err, abs(dev[pos[l]][1] - s))
            if i + 1 < len(want) and s - want[i + 1][1] > R.TAU:
                assert pos[l] < pos[want[i + 1][0]], (b, l, want[i + 1][0])
        WORST["ratio"] = max(WORST["ratio"], err / HALF_TAU)
        print(f"ctc-beam {tag} b={b} Tb={Tb} W={W} K={K} hyps={len(dev)} score err={err:.3e} tau/2={HALF_TAU:.3e} "
              f"ratio={err / HALF_TAU:.3f} worst so far={WORST['ratio']:.3f}")
        assert err <= HALF_TAU
    if need_decisive:
        assert decisive.any()
    return got, ref, decisive


def logits(rng, B, T, V, scale=4.0):
    z = scale * rng.standard_normal((B, T, V))
    z[:, :, 0] += scale
    return R.log_softmax(z)


# ---- the candidate stage: bit-exact ---------------------------------------------------
def cand_only(lp, in_len, K, **kw):
    got = raw(lp, in_len, 1, K, **kw)
    ref = R.beam_batch(np.asarray(lp, np.float32), in_len, 1, K, 1, lp.shape[1], np.float32)
    assert np.array_equal(got["cand"], ref["cand"]), (got["cand"], ref["cand"])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("V", [2, 3, 65, 300, 4000])
def test_candidates_vocabulary(gpu, V):
    """Head, quads and tail at every row misalignment (V odd or even, the base
    on and off a 16-byte boundary), one chunk and several, K below and at or
    above V - 1."""
    rng = np.random.default_rng(V)
    lp = R.log_softmax(3.0 * rng.standard_normal((2, 5, V)))
    for K, offset in ((1, 0), (5, 1), (16, 2), (32, 3)):
        got = cand_only(lp, None, K, offset=offset)
        assert (got["cand"][:, :, min(K, V - 1):] == -1).all() and (got["cand"][:, :, :min(K, V - 1)] >= 1).all()


@pytest.mark.gpu
def test_candidates_ties_and_infinities(gpu):
    rng = np.random.default_rng(11)
    V = 300
    lp = np.round(2.0 * rng.standard_normal((3, 6, V))) / 2           # a few distinct values: ties everywhere
    lp[1][rng.random((6, V)) < 0.5] = -np.inf
    lp[2, 0] = -np.inf                                                # nothing finite: ids 1 .. K
    lp[2, 1, 5:] = -np.inf                                            # fewer finite entries than K
    lp[2, 2] = 0.25                                                   # one value
    lp[2, 3, ::2] = 0.0
    lp[2, 3, 1::2] = -0.0                                             # equal under compares
    lp = lp.astype(np.float32)
    for K in (1, 7, 32):
        got = cand_only(lp, None, K)
        assert got["cand"][2, 0, :K].tolist() == list(range(1, K + 1))
        assert got["cand"][2, 2, :K].tolist() == list(range(1, K + 1))
        assert got["cand"][2, 3, :K].tolist() == list(range(1, K + 1))
    # ascending, descending and constant rows: every element enters, none does, ties keep the first
    ramp = np.stack([np.linspace(-9, 0, 700), np.linspace(0, -9, 700), np.zeros(700)])[None].astype(np.float32)
    got = cand_only(ramp, None, 16)
    assert got["cand"][0, 0].tolist() == list(range(699, 683, -1)) and got["cand"][0, 1].tolist() == list(range(1, 17))


@pytest.mark.gpu
def test_candidates_ragged(gpu):
    rng = np.random.default_rng(12)
    lp = logits(rng, 4, 7, 65)
    got = cand_only(lp, [7, 0, 3, 99], 9)
    assert (got["cand"][1] == -1).all() and (got["cand"][2, 3:] == -1).all() and (got["cand"][3] >= 1).all()


# ---- exactness ------------------------------------------------------------------------
@pytest.mark.gpu
def test_exhaustive_against_brute_force(gpu):
    """T = 5, V = 3, W = 64, K = 2: nothing is pruned; the hypotheses are the
    label sequences with a path and the scores their CTC log-likelihoods."""
    lp = np.stack([R.log_softmax(2.0 * np.random.default_rng(seed).standard_normal((5, 3))) for seed in range(4)])
    got = raw(lp, None, 64, 2)
    for b in range(4):
        exact = R.brute_force(lp[b], 5)
        dev = hyps_of(got, b)
        assert {h[0] for h in dev} == set(exact) and len(dev) == len(exact) == 25
        err = max(abs(s - exact[l]) for l, s, _ in dev)
        print(f"ctc-beam exhaustive b={b}: score err {err:.3e} (tau/2 {HALF_TAU:.3e})")
        assert err <= HALF_TAU
        assert dev[0][0] == max(exact, key=exact.get) or exact[max(exact, key=exact.get)] - exact[dev[0][0]] <= R.TAU


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.CASE_IDS)
def test_case_table(gpu, shape):
    T, V, W, K, _ = shape
    lp = R.case(shape)
    _, margins = R.case_reference(shape)
    got, ref, decisive = check(lp, None, W, K, tag=R.CASE_IDS[R.SHAPES.index(shape)])
    assert np.array_equal(decisive, margins > R.TAU)
    assert decisive.sum() >= R.BATCH - R.BATCH // 4
    if shape == R.SHAPES[-1]:       # a decisive utterance merges into a prefix whose parent left the beam and came back
        assert any(decisive[b] and R.recreated_merges(lp[b], W, K) > 0 for b in range(R.BATCH))


# ---- shape coverage -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,K", [(1, 1), (1, 32), (2, 31), (63, 32), (64, 1), (64, 31), (16, 8), (16, 9), (16, 16), (16, 17)])
def test_beam_and_candidate_limits(gpu, W, K):
    rng = np.random.default_rng(100 * W + K)
    check(logits(rng, 3, 10, 40, 5.0), [10, 7, 10], W, K, tag=f"W{W}-K{K}")


@pytest.mark.gpu
def test_n_best_and_fill(gpu):
    rng = np.random.default_rng(21)
    lp = logits(rng, 2, 12, 20)
    full, _, dec = check(lp, None, 8, 4, tag="n-best")
    part = raw(lp, None, 8, 4, n_best=3)
    assert np.array_equal(part["tokens"], full["tokens"][:, :3]) and np.array_equal(part["lengths"], full["lengths"][:, :3])
    assert np.array_equal(bits(part["scores"]), bits(full["scores"][:, :3]))
    # one frame of V = 3 has three hypotheses: (), (1), (2); the other five slots are empty
    one = raw(R.log_softmax(np.array([[[0.5, 1.5, -0.5]]])), None, 8, 2)
    assert one["lengths"][0].tolist() == [1, 0, 1, -1, -1, -1, -1, -1]
    assert one["tokens"][0, :, 0].tolist() == [1, -1, 2, -1, -1, -1, -1, -1]
    assert np.isneginf(one["scores"][0, 3:]).all() and np.isfinite(one["scores"][0, :3]).all()


def planted(rng, T, V, seq, gain=9.0):
    """Rows that spell `seq` with a blank after each label (T = 2 len(seq)), noise elsewhere."""
    z = rng.standard_normal((T, V))
    for i, c in enumerate(seq):
        z[2 * i, c] += gain
        z[2 * i + 1, 0] += gain
    return R.log_softmax(z)


@pytest.mark.gpu
def test_max_len_truncates(gpu):
    rng = np.random.default_rng(22)
    seq = (3, 3, 7, 1, 5)
    lp = planted(rng, 10, 9, seq)[None]
    full, _, _ = check(lp, None, 4, 3, tag="max-len")
    assert full["lengths"][0, 0] == 5 and tuple(full["tokens"][0, 0, :5]) == seq
    cut = raw(lp, None, 4, 3, max_len=2)
    assert np.array_equal(cut["lengths"], full["lengths"]) and np.array_equal(bits(cut["scores"]), bits(full["scores"]))
    assert np.array_equal(cut["tokens"], full["tokens"][:, :, :2])
    one = raw(lp, None, 4, 3, max_len=1, n_best=1)
    assert one["tokens"].tolist() == [[[3]]] and one["lengths"].tolist() == [[5]]


@pytest.mark.gpu
def test_last_label_outside_the_candidates(gpu):
    """K = 1: a hypothesis ending in a label that is not the frame's candidate
    still takes lp[e] from the row."""
    rng = np.random.default_rng(23)
    lp = planted(rng, 8, 6, (1, 2, 3, 4), gain=3.0)
    lp = np.stack([lp, planted(rng, 8, 6, (5, 5, 1, 5), gain=2.5)])
    got, ref, _ = check(lp, None, 4, 1, tag="gather")
    # (the reference confirms the situation arises: a live last label differs from the only candidate)
    hyps, hit = R.start(np.float64), 0
    for t in range(8):
        c = int(R.candidates(lp[0, t], 1)[0])
        hit += sum(1 for h in hyps if h[0] and h[0][-1] != c and np.isfinite(h[2]))
        hyps, _, _ = R.step(hyps, lp[0, t].astype(np.float64), 4, 1, np.float64)
    assert hit > 0


# ---- degenerate inputs ----------------------------------------------------------------
@pytest.mark.gpu
def test_zero_frames_and_mixed_lengths(gpu):
    rng = np.random.default_rng(31)
    lp = logits(rng, 5, 9, 12)
    in_len = [9, 0, 4, -3, 1]
    got, ref, _ = check(lp, in_len, 6, 4, tag="mixed")
    for b in (1, 3):
        assert got["lengths"][b].tolist() == [0, -1, -1, -1, -1, -1] and got["scores"][b, 0] == 0.0
        assert np.isneginf(got["scores"][b, 1:]).all() and (got["tokens"][b] == -1).all() and (got["cand"][b] == -1).all()
    # utterance 2 stops at its length: the frames after it change nothing
    short = raw(lp[:, :4], [4, 0, 4, 0, 1], 6, 4)
    assert np.array_equal(short["tokens"][2], got["tokens"][2, :, :4]) and (got["tokens"][2, :, 4:] == -1).all()
    assert np.array_equal(short["lengths"][2], got["lengths"][2]) and np.array_equal(bits(short["scores"][2]), bits(got["scores"][2]))


@pytest.mark.gpu
def test_one_hot_rows(gpu):
    """Rows with one 0 and -inf elsewhere: the one path's hypothesis survives, with score 0."""
    V = 7
    path = [0, 3, 3, 0, 3, 5, 5, 0, 0, 2]
    lp = np.full((2, len(path), V), -np.inf, dtype=np.float32)
    lp[0, np.arange(len(path)), path] = 0.0
    lp[1] = lp[0]
    lp[1, 4, 3], lp[1, 4, 0] = -np.inf, 0.0                       # the second 3 becomes a blank: (3, 5, 2)
    got = raw(lp, None, 8, 4)
    for b, seq in ((0, (3, 3, 5, 2)), (1, (3, 5, 2))):
        assert hyps_of(got, b) == [(seq, 0.0, len(seq))]
        assert got["lengths"][b, 1:].tolist() == [-1] * 7
    ref = R.beam_batch(lp, None, 8, 4, 8, len(path), np.float64)
    assert np.array_equal(got["cand"], ref["cand"]) and np.array_equal(got["tokens"], ref["tokens"])
    # half the mass on a second label in one frame: two hypotheses of log(1/2)
    lp[0, 5, 6] = lp[0, 5, 5] = np.log(0.5)
    got = raw(lp, None, 8, 4)
    assert [h[0] for h in hyps_of(got, 0)] == [(3, 3, 5, 2), (3, 3, 6, 5, 2)]
    assert np.allclose(got["scores"][0, :2], np.log(0.5), rtol=0, atol=1e-6)


@pytest.mark.gpu
def test_nan_input_stays_in_bounds(gpu):
    rng = np.random.default_rng(33)
    V = 30
    lp = logits(rng, 3, 12, V)
    lp[0][rng.random((12, V)) < 0.3] = np.nan
    lp[1, 5] = np.nan
    got = raw(lp, None, 8, 8)
    assert ((got["tokens"] >= -1) & (got["tokens"] < V)).all() and ((got["cand"] >= -1) & (got["cand"] < V)).all()
    assert ((got["lengths"] >= -1) & (got["lengths"] <= 12)).all()
    clean = raw(lp[2:], None, 8, 8)                               # the clean utterance is not affected
    assert np.array_equal(got["tokens"][2:], clean["tokens"]) and np.array_equal(bits(got["scores"][2:]), bits(clean["scores"]))


# ---- batch, stream, surfaces ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 65])
def test_batch_sizes(gpu, B):
    rng = np.random.default_rng(40 + B)
    lp = logits(rng, B, 8, 17)
    in_len = [int(x) for x in rng.integers(0, 9, size=B)]
    in_len[0] = 8
    got, _, _ = check(lp, in_len, 5, 6, tag=f"B{B}")
    same(raw(lp, in_len, 5, 6), got)                                  # two calls: the same bits
    for b in range(0, B, 7):                                          # every utterance is independent of its batch
        alone = raw(lp[b:b + 1], in_len[b:b + 1], 5, 6)
        same(alone, {k: v[b:b + 1] for k, v in got.items()})


@pytest.mark.gpu
def test_stream_null_candidates_null_lengths(gpu):
    rng = np.random.default_rng(50)
    lp = logits(rng, 4, 11, 23)
    got = raw(lp, [11] * 4, 7, 5)
    same(raw(lp, None, 7, 5), got)                                    # null input_lengths: all T
    same(raw(lp, [11] * 4, 7, 5, stream=torch.cuda.Stream()), got)
    bare = raw(lp, None, 7, 5, cand=False)
    same(bare, got, keys=("tokens", "lengths", "scores"))
    assert (bare["cand"] == SENT).all()


def _result(res):
    out = dict(tokens=res.tokens.cpu().numpy(), lengths=res.lengths.cpu().numpy(), scores=res.scores.cpu().numpy())
    if res.candidates is not None:
        out["cand"] = res.candidates.cpu().numpy()
    return out


@pytest.mark.gpu
def test_ctc_beam_search_python_forms(gpu):
    """(T, B, V) == batch-first == the raw call; max_len defaults to T."""
    import wakeword
    rng = np.random.default_rng(60)
    lp = logits(rng, 3, 9, 14)
    in_len = [9, 5, 0]
    want = raw(lp, in_len, 6, 4, n_best=3)
    d = torch.from_numpy(lp).to("cuda:0")
    a = wakeword.ctc_beam_search(d, in_len, beam=6, top_k=4, n_best=3, batch_first=True, return_candidates=True)
    b = wakeword.ctc_beam_search(d.transpose(0, 1).contiguous(), torch.tensor(in_len), beam=6, top_k=4, n_best=3,
                                 return_candidates=True)
    for res in (a, b):
        assert isinstance(res, wakeword.BeamResult) and res.tokens.is_cuda and res.tokens.shape == (3, 3, 9)
        same(_result(res), want)
    c = wakeword.ctc_beam_search(d, None, beam=6, top_k=4, n_best=2, max_len=3, batch_first=True)
    assert c.candidates is None
    same(_result(c), raw(lp, None, 6, 4, n_best=2, max_len=3), keys=("tokens", "lengths", "scores"))
    texts = wakeword.beam_texts(a, {i: chr(96 + i) for i in range(1, 14)})
    assert len(texts) == 3 and texts[2] == [""] and all(len(t) == 3 for t in texts[:2])
    assert texts[0][0] == "".join(chr(96 + int(x)) for x in want["tokens"][0, 0, :want["lengths"][0, 0]])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_through_the_model(gpu, precision):
    """CTCModel.beam_decode on a random-weight model (B = 2, T = 40, V = 50)
    equals the raw call on its own forward(..., return_log_probs=True)."""
    import wakeword
    from wakeword.ctc import random_state_dict
    V = 50
    model = wakeword.CTCModel(random_state_dict(V, seed=4), V, precision=precision)
    feats = torch.randn((2, 40, 80), generator=torch.Generator().manual_seed(9))
    _, lp = model.forward(feats, return_log_probs=True)
    assert lp.dtype == torch.float32
    got = model.beam_decode(feats, beam=8, top_k=6, n_best=4)
    same(_result(got), raw(lp.cpu().numpy(), None, 8, 6, n_best=4), keys=("tokens", "lengths", "scores"))
    assert bool(torch.isfinite(got.scores).all())
    one = model.beam_decode(feats)
    assert one.tokens.shape == (2, 1, 40)
    same(_result(one), raw(lp.cpu().numpy(), None, 16, 16, n_best=1), keys=("tokens", "lengths", "scores"))


@pytest.mark.gpu
def test_audio_and_transcribe(gpu):
    """beam_decode_audio == the raw call on the model's log-probs of the same
    audio; transcribe(beam=None) is the greedy path, bit for bit, and
    transcribe(beam=W) the beam's best hypothesis."""
    import wakeword
    from wakeword.ctc import random_state_dict
    V, n = 50, 8000
    chars = {i: chr(64 + i) for i in range(1, V)}
    model = wakeword.CTCModel(random_state_dict(V, seed=4), V, idx_to_char=chars)
    t = np.arange(n, dtype=np.float32) / 16000.0
    rng = np.random.default_rng(1)
    audio = np.stack([0.3 * np.sin(2 * np.pi * f * t) * np.sin(2 * np.pi * 3.0 * t) ** 2 for f in (440.0, 1250.0)])
    audio = (audio + 0.01 * rng.standard_normal(audio.shape)).astype(np.float32)
    res = model.beam_decode_audio(audio, n_samples=n, beam=8, top_k=6, n_best=2)
    _, lp = model.forward(model.features(audio, n), return_log_probs=True)
    want = raw(lp.cpu().numpy(), None, 8, 6, n_best=2)
    same(_result(res), want, keys=("tokens", "lengths", "scores"))
    # greedy, as before this surface existed: wk_ctc_transcribe's tokens cut at their lengths
    tok, ln = model.decode_audio(audio, n)
    tok, ln = tok.cpu().numpy(), ln.cpu().numpy()
    greedy = [tok[b, :ln[b]].tolist() for b in range(2)]
    assert model.transcribe(audio, n) == greedy and model.transcribe(audio, n, beam=None) == greedy
    assert model.transcribe_text(audio, n) == model.transcribe_text(audio, n, beam=None) == wakeword.tokens_to_text(greedy, chars)
    best = raw(lp.cpu().numpy(), None, 8, 16, n_best=1)
    beam = [best["tokens"][b, 0, :best["lengths"][b, 0]].tolist() for b in range(2)]
    assert model.transcribe(audio, n, beam=8) == beam
    assert model.transcribe_text(audio, n, beam=8) == wakeword.tokens_to_text(beam, chars)
