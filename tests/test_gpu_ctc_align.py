"""wk_ctc_align / wakeword.ctc_align / CTCModel.align on the MI355X.

Exact oracle: states, tokens, spans and scores are BIT-EQUAL to the float32
numpy reference (tests/ctc_align_ref.py) and frame_log_probs to the gathered
input -- no tolerance: the recurrence is one exact max and one IEEE add per
state, so the lane layout cannot change a bit.

Independent check against float64, for every utterance with an alignment: the
path passes valid_alignment, and
    opt64 - path_score64(path) <= 4 Tb 2^-24 |opt64|
(each of the Tb adds rounds by at most 2^-24 of a partial sum no larger than the
total, once for the chosen path and once for the optimum, times 2 for second-
order terms; holds for lp <= 0).  Largest measured ratio to this bound:
profiles/ctc_align_bounds.md.

Shapes are the smallest that reach each path of the kernels: every register
layout R (S on both sides of 31|32, 63|64, 127|128), the prefetch groups (16
rows for R <= 2, 8 above) and the backtrace's 64-frame chunks."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_align_ref as A

SENT = 0x5A5A5A5A


def raw(lp, labels, in_len, lab_len, max_label_len=None, optional=True, stream=None):
    """One wk_ctc_align call through the C ABI on (B, T, V) host log-probs -> dict
    of host arrays.  The outputs start as a sentinel / NaN, so anything the call
    leaves unwritten shows."""
    from wakeword import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    d_lp = torch.as_tensor(lp, dtype=torch.float32).to(dev).contiguous()
    B, T, V = d_lp.shape
    d_lab = torch.as_tensor(np.asarray(labels), dtype=torch.int32).to(dev).contiguous()
    smax = d_lab.shape[1] if max_label_len is None else max_label_len
    il = torch.tensor(in_len, dtype=torch.int32, device=dev)
    tl = torch.tensor(lab_len, dtype=torch.int32, device=dev)
    nbytes = L.wk_ctc_align_workspace_bytes(B, T, smax)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    states = torch.full((B, T), SENT, dtype=torch.int32, device=dev)
    tokens = torch.full((B, T), SENT, dtype=torch.int32, device=dev)
    frame_lp = torch.full((B, T), float("nan"), device=dev)
    spans = torch.full((B, max(smax, 1), 2), SENT, dtype=torch.int32, device=dev)
    scores = torch.full((B,), float("nan"), device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    _lib.check(L.wk_ctc_align(p(d_lp), B, T, V, p(d_lab), d_lab.shape[1], p(il), p(tl), smax, p(ws), p(states),
                              p(tokens) if optional else None, p(frame_lp) if optional else None,
                              p(spans) if optional else None, p(scores), 0, C.c_void_p(s.cuda_stream)), "wk_ctc_align")
    s.synchronize()
    return dict(states=states.cpu().numpy(), tokens=tokens.cpu().numpy(), frame_lp=frame_lp.cpu().numpy(),
                spans=spans.cpu().numpy()[:, :smax], scores=scores.cpu().numpy())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(got, want, keys=("states", "tokens", "frame_lp", "spans", "scores")):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(bits(got[k]), bits(want[k])), (k, got[k], want[k])


WORST = {"ratio": 0.0}


def check(lp, labels, in_len, lab_len, max_label_len=None, tag=""):
    """Run, compare bit for bit with the float32 reference, check each path
    against float64.  Returns (device outputs, reference outputs)."""
    lp = np.asarray(lp, dtype=np.float32)
    labels = np.asarray(labels)
    got = raw(lp, labels, in_len, lab_len, max_label_len)
    want = A.align_batch(lp, labels, in_len, lab_len, max_label_len)
    same(got, want)
    B, T, V = lp.shape
    smax = labels.shape[1] if max_label_len is None else max_label_len
    for b in range(B):
        Tb, S = min(max(int(in_len[b]), 0), T), min(max(int(lab_len[b]), 0), smax)
        if got["scores"][b] == -np.inf:
            assert (got["states"][b] == -1).all() and (got["tokens"][b] == -1).all() and (got["spans"][b] == -1).all()
            assert not got["frame_lp"][b].any()
            continue
        lab, path = labels[b, :S], got["states"][b, :Tb]
        assert A.valid_alignment(path, lab, Tb)
        assert (got["states"][b, Tb:] == -1).all() and (got["spans"][b, S:] == -1).all()
        opt64, _ = A.viterbi(lp[b, :Tb], lab, np.float64)
        gap, bound = opt64 - A.path_score64(lp[b, :Tb], lab, path), 4.0 * Tb * A.EPS32 * abs(opt64)
        ratio = gap / bound if bound > 0 else 0.0
        WORST["ratio"] = max(WORST["ratio"], ratio)
        print(f"ctc-align {tag} b={b} Tb={Tb} S={S} opt64={opt64:.6f} gap={gap:.3e} bound={bound:.3e} ratio={ratio:.3f} "
              f"worst so far={WORST['ratio']:.3f}")
        assert 0.0 <= gap + 1e-12 * abs(opt64) and gap <= bound
    return got, want


def rand_lp(rng, B, T, V):
    return A.log_softmax(rng.standard_normal((B, T, V)))


def labels_no_repeat(rng, S, V):
    """S labels in [1, V), no two adjacent equal: feasible in S frames."""
    lab = np.empty(S, dtype=np.int64)
    prev = 0
    for i in range(S):
        v = int(rng.integers(1, V))
        while v == prev and V > 2:
            v = int(rng.integers(1, V))
        lab[i] = prev = v
    return lab


# ---- register layouts -------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 31, 32, 63, 64, 127, 128, 255])
def test_register_layouts(gpu, S):
    """Every R with L on both sides of each boundary, T = S + 5, V = 11:
    utterance 0 has no adjacent repeats (feasible), utterance 1 plain random
    labels and a shorter input (often infeasible at large S: then no
    alignment, like the reference)."""
    rng = np.random.default_rng(S)
    T, V = S + 5, 11
    labels = np.stack([labels_no_repeat(rng, S, V), rng.integers(1, V, size=S)])
    got, _ = check(rand_lp(rng, 2, T, V), labels, [T, T - 1], [S, S], tag=f"layout-S{S}")
    assert got["scores"][0] > -np.inf


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 31, 32, 63, 64, 127, 128, 255])
def test_all_labels_equal_exactly_feasible(gpu, S):
    """All labels equal: no skip, Tb = 2S-1 has the single path 1, 2, ..., 2S-1
    and Tb = 2S-2 none."""
    rng = np.random.default_rng(100 + S)
    T, V = 2 * S - 1, 11
    labels = np.full((2, S), 1 + S % 10, dtype=np.int64)
    got, _ = check(rand_lp(rng, 2, T, V), labels, [T, T - 1], [S, S], tag=f"equal-S{S}")
    assert got["states"][0].tolist() == list(range(1, 2 * S))
    assert got["scores"][1] == -np.inf and got["scores"][0] > -np.inf
    assert got["spans"][0].tolist() == [[2 * i, 2 * i + 1] for i in range(S)]


# ---- prefetch groups (8 and 16 rows) and backtrace chunks (64 frames) ----
BOUNDARY_T = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]


@pytest.mark.gpu
@pytest.mark.parametrize("smax", [3, 64], ids=["R1-prefetch16", "R4-prefetch8"])
@pytest.mark.parametrize("T", BOUNDARY_T)
def test_group_boundaries(gpu, T, smax):
    rng = np.random.default_rng(1000 * smax + T)
    V, stride = 9, smax + 6
    lens = [min(smax, max(T // 2, 1)), 1, 0, min(smax, T)]
    labels = np.zeros((4, stride), dtype=np.int64)
    for b, n in enumerate(lens):
        labels[b, :n] = labels_no_repeat(rng, n, V)
    labels[:, smax:] = 99                                   # past max_label_len: never read as labels
    check(rand_lp(rng, 4, T, V), labels, [T, T - 1, T // 2, T], lens, max_label_len=smax, tag=f"T{T}-smax{smax}")


@pytest.mark.gpu
def test_reference_shape(gpu):
    """T = 801, V = 4000, S = 40, B = 2: the table's plain and planted cases."""
    (lp0, lab0, _), (lp1, lab1, planted) = A.case((801, 4000, 40), "plain"), A.case((801, 4000, 40), "planted")
    got, _ = check(np.stack([lp0, lp1]), np.stack([lab0, lab1]), [801, 801], [40, 40], tag="T801-V4000-S40")
    assert np.array_equal(got["states"][1], planted)


# ---- ragged lengths ---------------------------------------------------------------
@pytest.mark.gpu
def test_ragged_lengths(gpu):
    rng = np.random.default_rng(7)
    B, T, V, smax, stride = 6, 40, 13, 9, 12
    in_len, lab_len = [0, 40, 17, 40, 5, 33], [3, 0, 9, 4, 5, 9]
    labels = np.full((B, stride), 12, dtype=np.int64)
    for b, n in enumerate(lab_len):
        labels[b, :n] = labels_no_repeat(rng, n, V)
    lp = rand_lp(rng, B, T, V)
    got, _ = check(lp, labels, in_len, lab_len, max_label_len=smax, tag="ragged")
    assert got["scores"][0] == -np.inf                                       # Tb = 0
    assert (got["states"][1] == 0).all() and (got["tokens"][1] == 0).all()   # S = 0: all blanks
    assert np.isfinite(got["scores"][1:]).all()
    for b in range(1, B):
        assert (got["states"][b, in_len[b]:] == -1).all() and (got["tokens"][b, in_len[b]:] == -1).all()
        assert not got["frame_lp"][b, in_len[b]:].any()
        assert (got["spans"][b, lab_len[b]:] == -1).all() and (got["spans"][b, :lab_len[b]] >= 0).all()
    # lengths outside their range are clamped: T + 9 frames means T, -3 labels means 0
    got2 = raw(lp, labels, [0, T + 9, 17, 40, 5, 33], [3, -3, 9, 4, 5, 9], smax)
    same(got2, got)


# ---- invalid labels ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("value", [0, 13, -5, 1 << 30], ids=["blank", "V", "negative", "huge"])
def test_invalid_label_is_no_alignment(gpu, value):
    rng = np.random.default_rng(11)
    B, T, V, S = 3, 20, 13, 6
    lp = rand_lp(rng, B, T, V)
    labels = np.stack([labels_no_repeat(rng, S, V) for _ in range(B)])
    clean = raw(lp, labels, [T] * B, [S] * B)
    labels[1, 2] = value
    got = raw(lp, labels, [T] * B, [S] * B)
    assert got["scores"][1] == -np.inf and (got["states"][1] == -1).all() and (got["tokens"][1] == -1).all()
    assert (got["spans"][1] == -1).all() and not got["frame_lp"][1].any()
    for b in (0, 2):
        for k in clean:
            assert np.array_equal(bits(got[k][b]), bits(clean[k][b]))
    same(got, A.align_batch(lp, labels, [T] * B, [S] * B))


# ---- vocabulary -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("V,T", [(2, 9), (7, 9), (65536, 3)])
def test_vocabulary(gpu, V, T):
    rng = np.random.default_rng(V)
    labels = np.array([[1, V - 1], [V - 1, 1]], dtype=np.int64)       # V = 2: equal labels, the blank between them
    check(rand_lp(rng, 2, T, V), labels, [T, T], [2, 2], tag=f"V{V}")


# ---- tie rule ---------------------------------------------------------------------
@pytest.mark.gpu
def test_tie_rule_uniform_rows(gpu):
    """lp = -ln V everywhere: every path ties exactly, the tie rule alone decides."""
    V, T = 7, 12
    lp = np.full((3, T, V), -np.log(np.float32(V)), dtype=np.float32)
    labels = np.array([[2, 2, 5], [1, 2, 3], [4, 4, 4]], dtype=np.int64)
    got, _ = check(lp, labels, [T, T, 7], [3, 3, 3], tag="ties")
    assert got["states"][0].tolist() == [1, 2, 3, 5] + [6] * 8
    assert got["spans"][0].tolist() == [[0, 1], [2, 3], [3, 4]]
    # a wider lattice: R = 4 and ties across lanes
    S = 70
    labels = np.random.default_rng(3).integers(1, 4, size=(1, S))
    check(np.full((1, 150, 4), -np.log(np.float32(4)), dtype=np.float32), labels, [150], [S], tag="ties-R4")


# ---- -inf input -------------------------------------------------------------------
@pytest.mark.gpu
def test_one_hot_rows(gpu):
    """Rows 0 on one token and -inf elsewhere along a planted path: score 0
    exactly and the planted path; one frame broken: no alignment."""
    rng = np.random.default_rng(5)
    T, V, S = 37, 6, 9
    labels = np.array([[1, 1, 2, 3, 3, 3, 4, 5, 1]], dtype=np.int64)
    planted = A.planted_path(rng, labels[0], T)
    lp = np.full((2, T, V), -np.inf, dtype=np.float32)
    lp[:, np.arange(T), A.extended(labels[0])[planted]] = 0.0
    lp[1, 20, :] = -np.inf                                              # no token at all at one frame
    got, _ = check(lp, np.repeat(labels, 2, 0), [T, T], [S, S], tag="one-hot")
    assert got["scores"][0] == 0.0 and np.array_equal(got["states"][0], planted)
    assert not got["frame_lp"][0].any()
    assert got["scores"][1] == -np.inf and (got["states"][1] == -1).all()


# ---- batch, stream, optional outputs ----------------------------------------------
def _batch_case(B, seed=0):
    rng = np.random.default_rng(seed)
    T, V, S = 21, 10, 6
    labels = np.stack([labels_no_repeat(rng, S, V) for _ in range(B)])
    in_len = [T - (b % 5) for b in range(B)]
    lab_len = [S - (b % 3) for b in range(B)]
    return rand_lp(rng, B, T, V), labels, in_len, lab_len


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 257])
def test_batch_sizes(gpu, B):
    lp, labels, in_len, lab_len = _batch_case(B)
    got = raw(lp, labels, in_len, lab_len)
    same(got, A.align_batch(lp, labels, in_len, lab_len))
    same(raw(lp, labels, in_len, lab_len), got)                       # two calls: the same bits


@pytest.mark.gpu
def test_non_default_stream_and_optional_outputs(gpu):
    lp, labels, in_len, lab_len = _batch_case(5, seed=2)
    got = raw(lp, labels, in_len, lab_len)
    same(raw(lp, labels, in_len, lab_len, stream=torch.cuda.Stream()), got)
    bare = raw(lp, labels, in_len, lab_len, optional=False)
    same(bare, got, keys=("states", "scores"))
    assert (bare["tokens"] == SENT).all() and (bare["spans"] == SENT).all() and np.isnan(bare["frame_lp"]).all()


# ---- the Python surface -----------------------------------------------------------
@pytest.mark.gpu
def test_ctc_align_python_forms(gpu):
    """(T, B, V) with concatenated targets == batch-first with padded ones == the raw call."""
    import wakeword
    lp, labels, in_len, lab_len = _batch_case(4, seed=3)
    want = raw(lp, labels, in_len, lab_len)
    d = torch.from_numpy(lp).to("cuda:0")
    a = wakeword.ctc_align(d, torch.from_numpy(labels), in_len, lab_len, batch_first=True)
    concat = torch.cat([torch.from_numpy(labels[b, :n]) for b, n in enumerate(lab_len)])
    b = wakeword.ctc_align(d.transpose(0, 1).contiguous(), concat, torch.tensor(in_len), torch.tensor(lab_len))
    for al in (a, b):
        assert isinstance(al, wakeword.Alignment)
        got = dict(states=al.states.cpu().numpy(), tokens=al.tokens.cpu().numpy(), frame_lp=al.frame_log_probs.cpu().numpy(),
                   spans=al.spans.cpu().numpy(), scores=al.scores.cpu().numpy())
        same(got, want)
    sec = wakeword.span_seconds(a.spans)
    assert sec.is_cuda and sec.dtype == torch.float64
    assert torch.equal(sec, torch.where(a.spans < 0, -1.0, a.spans.double() * 0.01))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_through_the_model(gpu, precision):
    """CTCModel.align on a random-weight model (B = 2, T = 40, V = 50) equals
    ctc_align of its own forward(..., return_log_probs=True)."""
    import wakeword
    from wakeword.ctc import random_state_dict
    V = 50
    model = wakeword.CTCModel(random_state_dict(V, seed=4), V, precision=precision)
    feats = torch.randn((2, 40, 80), generator=torch.Generator().manual_seed(9))
    targets = torch.tensor([[3, 3, 17, 49, 2], [8, 1, 0, 0, 0]])
    tl = [5, 2]
    _, lp = model.forward(feats, return_log_probs=True)
    assert lp.dtype == torch.float32
    for il in (None, [40, 33]):
        got = model.align(feats, targets, tl, input_lengths=il)
        want = wakeword.ctc_align(lp, targets, il if il is not None else [40, 40], tl, batch_first=True)
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        assert bool(torch.isfinite(got.scores).all())
    ref = A.align_batch(lp.cpu().numpy(), targets.numpy(), [40, 33], tl)
    same(dict(states=got.states.cpu().numpy(), tokens=got.tokens.cpu().numpy(), frame_lp=got.frame_log_probs.cpu().numpy(),
              spans=got.spans.cpu().numpy(), scores=got.scores.cpu().numpy()), ref)


@pytest.mark.gpu
def test_align_audio(gpu):
    """0.5 s of synthetic audio: spans inside [0, T], start < end, ordered by label."""
    import wakeword
    from wakeword.ctc import random_state_dict
    V, n = 50, 8000
    model = wakeword.CTCModel(random_state_dict(V, seed=4), V)
    t = np.arange(n, dtype=np.float32) / 16000.0
    rng = np.random.default_rng(1)
    audio = np.stack([0.3 * np.sin(2 * np.pi * f * t) * np.sin(2 * np.pi * 3.0 * t) ** 2 for f in (440.0, 1250.0)])
    audio = (audio + 0.01 * rng.standard_normal(audio.shape)).astype(np.float32)
    targets, tl = torch.tensor([[3, 7, 7, 12], [20, 5, 0, 0]]), [4, 2]
    al = model.align_audio(audio, targets, tl, n_samples=n)
    T = 1 + n // 160
    assert al.states.shape == (2, T) and al.spans.shape == (2, 4, 2)
    spans, sec = al.spans.cpu().numpy(), wakeword.span_seconds(al.spans).cpu().numpy()
    assert bool(torch.isfinite(al.scores).all())
    for b, S in enumerate(tl):
        sp = spans[b, :S]
        assert (sp[:, 0] >= 0).all() and (sp[:, 1] <= T).all() and (sp[:, 0] < sp[:, 1]).all()
        assert (sp[1:, 0] >= sp[:-1, 1]).all()                        # in label order, not overlapping
        assert (spans[b, S:] == -1).all() and (sec[b, S:] == -1).all()
        assert np.allclose(sec[b, :S], sp * 0.01, rtol=0, atol=1e-12)
        tok = al.tokens[b].cpu().numpy()
        for i in range(S):
            assert (tok[sp[i, 0]:sp[i, 1]] == int(targets[b, i])).all()
