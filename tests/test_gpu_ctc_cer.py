"""wk_ctc_cer / wakeword.edit_distance / CTCModel.cer / CTCTrainer.val_cer on the MI355X.

Exact oracle: every output is integer, so stats, best and totals are EQUAL to
the numpy reference (tests/ctc_cer_ref.py, itself checked against a tuple DP
and exhaustive enumeration in test_ctc_cer_ref.py) -- no tolerance anywhere.
Every call goes through `raw`, whose outputs start as a sentinel and are
followed by canary words that must survive the call; the buffers hold random
tokens beyond every length.

Shapes are the smallest that reach each path of the kernels: hypothesis
lengths on both sides of the 64-word chunk, reference lengths on both sides of
every lane and register edge of the five template instances (1, 2, 4, 8 and 16
columns per lane: max_ref_len up to 64, 128, 256, 512, 1024)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_cer_ref as R

SENT = 0x5A5A5A5A
CANARY = 16
N_GRID = (0, 1, 2, 63, 64, 65, 127, 128, 129, 801)
M_GRID = (0, 1, 63, 64, 65, 128, 129, 255, 256, 257, 1023, 1024)


def _with_canary(shape, dtype, dev):
    n = int(np.prod(shape))
    return torch.full((n + CANARY,), SENT, dtype=dtype, device=dev)


def raw(hyp, hyp_len, ref, ref_len, max_ref_len=None, collapse=False, want_best=True, want_totals=True, stream=None):
    """One wk_ctc_cer call through the C ABI on host arrays -> dict of host
    arrays.  Outputs start as a sentinel; the canary words after each must be
    untouched, and an output not asked for stays a sentinel."""
    from wakeword import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    d_hyp = torch.as_tensor(np.asarray(hyp), dtype=torch.int32).to(dev).contiguous()
    if d_hyp.dim() == 2:
        d_hyp = d_hyp.unsqueeze(1)
    B, H, stride = d_hyp.shape
    d_ref = torch.as_tensor(np.asarray(ref), dtype=torch.int32).to(dev).contiguous()
    mrl = d_ref.shape[1] if max_ref_len is None else max_ref_len
    hl = torch.as_tensor(np.asarray(hyp_len).reshape(-1), dtype=torch.int32).to(dev) if hyp_len is not None else None
    rl = torch.as_tensor(np.asarray(ref_len), dtype=torch.int32).to(dev)
    nbytes = L.wk_ctc_cer_workspace_bytes(B, H, stride, mrl)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stats = _with_canary((B, H, 4), torch.int32, dev)
    best = _with_canary((B,), torch.int32, dev)
    totals = _with_canary((2, 8), torch.int64, dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    _lib.check(L.wk_ctc_cer(p(d_hyp), p(hl), B, H, stride, p(d_ref), d_ref.shape[1], p(rl), mrl, int(collapse), p(ws), p(stats),
                            p(best) if want_best else None, p(totals) if want_totals else None, 0, C.c_void_p(s.cuda_stream)),
               "wk_ctc_cer")
    s.synchronize()
    stats, best, totals = stats.cpu().numpy(), best.cpu().numpy(), totals.cpu().numpy()
    for name, a, n in (("stats", stats, B * H * 4), ("best", best, B), ("totals", totals, 16)):
        assert (a[n:] == SENT).all(), f"canary after {name} overwritten"
    if not want_best:
        assert (best == SENT).all()
    if not want_totals:
        assert (totals == SENT).all()
    return dict(stats=stats[:B * H * 4].reshape(B, H, 4), best=best[:B], totals=totals[:16].reshape(2, 8))


def same(got, want, keys=("stats", "best", "totals")):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])


def check(hyp, hyp_len, ref, ref_len, max_ref_len=None, collapse=False):
    got = raw(hyp, hyp_len, ref, ref_len, max_ref_len, collapse)
    want = R.cer_batch(hyp, hyp_len, ref, ref_len, max_ref_len, collapse)
    same(got, want)
    st = got["stats"].astype(np.int64)
    assert (st[..., 0] == st[..., 1] + st[..., 2] + st[..., 3]).all() and (st >= 0).all()
    return got


def fill(rng, B, H, stride, ref_stride, alphabet):
    """Buffers of random tokens of the alphabet: whatever lies beyond a length equals real tokens."""
    return rng.integers(1, alphabet + 1, size=(B, H, stride)), rng.integers(1, alphabet + 1, size=(B, ref_stride))


# ---- the (N, M) grid: every lane and register edge of every template instance ----------
@pytest.mark.gpu
@pytest.mark.parametrize("cap", [64, 128, 256, 512, 1024])
def test_length_grid(gpu, cap):
    """One ragged batch per instance: every N of the grid against every M of the
    grid the instance takes, alphabet 3 (ties), rows 801 and cap + 3 wide."""
    ms = [m for m in M_GRID if m <= cap]
    cases = [(n, m) for m in ms for n in N_GRID]
    rng = np.random.default_rng(cap)
    hyp, ref = fill(rng, len(cases), 1, 801, cap + 3, 3)
    for b, (n, m) in enumerate(cases):                     # the same pair in every instance: its reference is computed once
        pr = np.random.default_rng(1000 * n + m)
        hyp[b, 0, :n], ref[b, :m] = pr.integers(1, 4, size=n), pr.integers(1, 4, size=m)
    got = check(hyp, [n for n, _ in cases], ref, [m for _, m in cases], max_ref_len=cap)
    for b, (n, m) in enumerate(cases):
        d = got["stats"][b, 0, 0]
        assert abs(n - m) <= d <= max(n, m)


@pytest.mark.gpu
@pytest.mark.parametrize("n_hyp", [1, 3, 64])
@pytest.mark.parametrize("batch", [1, 5, 257])
def test_batch_and_hypotheses(gpu, batch, n_hyp):
    """Short ragged pairs (N <= 7, M <= 9, alphabet 2: the oracle has ties to break) at every batch and n_hyp."""
    rng = np.random.default_rng(batch * 100 + n_hyp)
    hyp, ref = fill(rng, batch, n_hyp, 7, 9, 2)
    check(hyp, rng.integers(0, 8, size=batch * n_hyp), ref, rng.integers(0, 10, size=batch))


# ---- data ------------------------------------------------------------------------------
def edited(rng, r, k, alphabet):
    h = list(r)
    for _ in range(k):
        op, at = rng.integers(0, 3), rng.integers(0, len(h) + 1)
        if op == 0 and h:
            h[min(at, len(h) - 1)] = int(rng.integers(1, alphabet + 1))
        elif op == 1 and h:
            del h[min(at, len(h) - 1)]
        else:
            h.insert(at, int(rng.integers(1, alphabet + 1)))
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("alphabet", [2, 3, 4000])
def test_alphabets_and_edits(gpu, alphabet):
    """Per utterance three hypotheses: the reference itself, the reference with
    k random edits, an unrelated sequence.  M on both sides of 64, 128 and 192."""
    rng = np.random.default_rng(alphabet)
    ms = [5, 63, 70, 127, 130, 200]
    hyp, ref = fill(rng, len(ms), 3, 230, 203, alphabet)
    hl = np.zeros((len(ms), 3), dtype=np.int64)
    for b, m in enumerate(ms):
        r = ref[b, :m]
        for k, h in enumerate((r, edited(rng, r, 1 + b, alphabet), rng.integers(1, alphabet + 1, size=m + 7))):
            hyp[b, k, :len(h)], hl[b, k] = h, len(h)
    got = check(hyp, hl, ref, ms, max_ref_len=200)
    assert (got["stats"][:, 0] == 0).all() and (got["best"] == 0).all()
    assert (got["stats"][:, 1, 0] <= 1 + np.arange(len(ms))).all()
    assert got["totals"][0].tolist() == [0, 0, 0, 0, sum(ms), sum(ms), 0, len(ms)]


@pytest.mark.gpu
def test_disjoint_alphabets_and_long_runs(gpu):
    """Disjoint alphabets: d = max(N, M), all substitutions but |N - M|.  One
    long run of a repeated token against a reference that holds it once, never
    and throughout."""
    rng = np.random.default_rng(9)
    lens = [(3, 9), (64, 64), (130, 65), (65, 130), (257, 300)]
    hyp, ref = fill(rng, len(lens) + 3, 1, 300, 300, 5)
    hyp[:len(lens)] += 10
    hl, rl = [n for n, _ in lens], [m for _, m in lens]
    hyp[len(lens):, 0, :] = 4                                # the run
    ref[len(lens)] = 1
    ref[len(lens), 77] = 4                                   # once
    ref[len(lens) + 1] = 2                                   # never
    ref[len(lens) + 2] = 4                                   # throughout
    hl, rl = hl + [200, 200, 200], rl + [150, 150, 150]
    got = check(hyp, hl, ref, rl)
    for b, (n, m) in enumerate(lens):
        assert got["stats"][b, 0].tolist() == [max(n, m), min(n, m), max(m - n, 0), max(n - m, 0)]
    assert got["stats"][len(lens):, 0].tolist() == [[199, 149, 0, 50], [200, 150, 0, 50], [50, 0, 0, 50]]


# ---- lengths and what lies beyond them -------------------------------------------------
@pytest.mark.gpu
def test_lengths_are_clamped(gpu):
    rng = np.random.default_rng(21)
    hyp, ref = fill(rng, 4, 2, 70, 40, 3)
    hl = [-1, 0, 70, 71, 1 << 30, -(1 << 31), 5, 69]
    rl = [-3, 33, 1 << 30, 32]
    got = check(hyp, hl, ref, rl, max_ref_len=32)                    # ref_stride 40 > max_ref_len: clamped to 32, not 40
    assert got["stats"][0].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]]  # -1 and 0 against M = 0 (from -3)
    assert got["totals"][0, 4] == 0 + 32 + 32 + 32 and got["totals"][0, 5] == 0 + 70 + 70 + 5
    same(got, raw(hyp, np.clip(hl, 0, 70), ref[:, :32], np.clip(rl, 0, 32)))


@pytest.mark.gpu
@pytest.mark.parametrize("collapse", [False, True], ids=["tokens", "frames"])
def test_nothing_beyond_a_length_is_used(gpu, collapse):
    """The same real tokens with two different fillings beyond every length --
    tokens of the same alphabet, so equal to real ones -- give the same bytes."""
    rng = np.random.default_rng(33)
    B, H, stride, rs = 6, 3, 150, 140
    hl, rl = rng.integers(0, stride + 1, size=B * H), rng.integers(0, 131, size=B)
    hl[:3], rl[0] = [0, 64, 128], 0
    lo = 0 if collapse else 1
    hyp, ref = rng.integers(lo, 4, size=(B, H, stride)), rng.integers(1, 4, size=(B, rs))
    got = check(hyp, hl, ref, rl, max_ref_len=130, collapse=collapse)
    hyp2, ref2 = rng.integers(lo, 4, size=(B, H, stride)), rng.integers(1, 4, size=(B, rs))
    for b in range(B):
        ref2[b, :rl[b]] = ref[b, :rl[b]]
        for k in range(H):
            hyp2[b, k, :hl[b * H + k]] = hyp[b, k, :hl[b * H + k]]
    same(raw(hyp2, hl, ref2, rl, 130, collapse), got)


# ---- collapse --------------------------------------------------------------------------
@pytest.mark.gpu
def test_collapse_chunk_edges(gpu):
    """Frame labels with a run of one label across frames 63|64 and 127|128, a
    blank exactly at frame 64, the same label on both sides of a blank (there
    and elsewhere), a label starting exactly at 64 and at 128."""
    T = 200
    rows = np.zeros((6, T), dtype=np.int64)
    rows[0, 60:70], rows[0, 120:140] = 3, 5                       # runs across both edges
    rows[1, 60:64], rows[1, 65:70] = 3, 3                         # blank exactly at 64, the same label after it
    rows[2, 63], rows[2, 64], rows[2, 127], rows[2, 128] = 2, 2, 2, 2
    rows[3, 64:80], rows[3, 128:130] = 7, 7                       # starts exactly at the chunk edges
    rows[4, :] = np.arange(T) % 2 * 4                             # 0 4 0 4 ...: the same label on both sides of every blank
    rows[5, :] = 6                                                # one run over every chunk
    for b, want in enumerate(([3, 5], [3, 3], [2, 2], [7, 7], [4] * (T // 2), [6])):
        assert R.collapse(rows[b]).tolist() == want
    ref = np.array([[3, 5, 0], [3, 3, 0], [2, 2, 0], [7, 7, 0], [4, 4, 4], [6, 0, 0]])
    got = check(rows, None, ref, [2, 2, 2, 2, 3, 1], collapse=True)                 # null lengths: all T frames
    assert got["stats"][:, 0, 0].tolist() == [0, 0, 0, 0, T // 2 - 3, 0]
    rng = np.random.default_rng(4)
    noisy = rng.integers(0, 3, size=(8, 3, T))                    # short runs of 1, 2 and blanks everywhere
    check(noisy, None, rng.integers(1, 3, size=(8, 90)), rng.integers(0, 91, size=8), collapse=True)


@pytest.mark.gpu
def test_collapse_frame_counts(gpu):
    """Tb in {0, 1, 64, 65, 801} with Tb < hyp_stride = 900, and out-of-range counts."""
    rng = np.random.default_rng(8)
    tb = [0, 1, 64, 65, 801, -4, 5000]
    frames = rng.integers(0, 4, size=(len(tb), 900))
    frames[:, 0] = 2                                              # Tb = 1 keeps a label
    got = check(frames, tb, rng.integers(1, 4, size=(len(tb), 300)), [3, 3, 20, 64, 300, 2, 256], collapse=True)
    assert got["stats"][0, 0].tolist() == [3, 0, 3, 0] and got["stats"][5, 0].tolist() == [2, 0, 2, 0]


@pytest.mark.gpu
def test_collapse_equals_the_decoder(gpu):
    """On the device: wk_ctc_frame_argmax's labels with collapse = 1 give the
    stats of wk_ctc_forward's own tokens and lengths with collapse = 0
    (random small model, B = 3, T = 70, V = 6: repeats and blanks)."""
    import wakeword
    from wakeword.ctc import random_state_dict
    V, B, T = 6, 3, 70
    model = wakeword.CTCModel(random_state_dict(V, seed=2), V)
    feats = torch.randn((B, T, 80), generator=torch.Generator().manual_seed(5))
    tok, ln, _ = model.decode(feats)
    pred = model.frame_argmax(B, T)
    rng = np.random.default_rng(6)
    ref, rl = rng.integers(1, V, size=(B, 30)), [30, 11, 0]
    a = wakeword.edit_distance(pred, None, ref, rl, collapse=True)
    b = wakeword.edit_distance(tok, ln, ref, rl)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a.distance.shape == (B,) and a.totals.shape == (2, 8) and a.totals.dtype == torch.int64
    assert int(a.totals[0, 5]) == int(ln.sum()) and int(ln.sum()) > 0
    same(dict(stats=torch.stack(a[:4], dim=-1).unsqueeze(1).cpu().numpy(), best=a.best.cpu().numpy(), totals=a.totals.cpu().numpy()),
         R.cer_batch(pred.cpu().numpy(), None, ref, rl, collapse_frames=True))


# ---- oracle and totals -----------------------------------------------------------------
@pytest.mark.gpu
def test_oracle_ties_and_totals(gpu):
    """d_best: the smallest d, then the smallest s, then the lowest index; an
    utterance with M = 0; null d_best / d_totals are accepted and leave the rest alone."""
    ref = np.array([[1, 2, 3, 4], [1, 2, 0, 0], [9, 9, 9, 9], [5, 6, 7, 0]])
    rl = [4, 2, 0, 3]
    hyp = np.zeros((4, 4, 5), dtype=np.int64)
    hl = np.zeros((4, 4), dtype=np.int64)
    rows = {(0, 0): [1, 2, 9, 9], (0, 1): [1, 2, 9, 4], (0, 2): [1, 2, 4], (0, 3): [1, 2, 3, 4, 4],      # d = 2, 1, 1, 1; s = 2, 1, 0, 0
            (1, 0): [2, 1], (1, 1): [1], (1, 2): [1], (1, 3): [1, 2, 3],                                # d = 2 (s 0), 1, 1, 1: index breaks the tie
            (2, 0): [4, 4], (2, 1): [4], (2, 2): [], (2, 3): [],                                          # M = 0
            (3, 0): [5, 6, 7], (3, 1): [5, 6, 7], (3, 2): [5, 6], (3, 3): [7]}                            # hypothesis 0 is already exact
    for (b, k), h in rows.items():
        hyp[b, k, :len(h)], hl[b, k] = h, len(h)
    got = check(hyp, hl, ref, rl)
    assert got["stats"][0].tolist() == [[2, 2, 0, 0], [1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 1]]
    assert got["best"].tolist() == [2, 1, 2, 0]
    assert got["totals"].tolist() == [[6, 2, 1, 3, 9, 11, 3, 4], [2, 0, 2, 0, 9, 7, 2, 4]]
    for wb, wt in ((False, True), (True, False), (False, False)):
        part = raw(hyp, hl, ref, rl, want_best=wb, want_totals=wt)
        same(part, got, keys=("stats",) + (("best",) if wb else ()) + (("totals",) if wt else ()))


@pytest.mark.gpu
def test_two_calls_and_non_default_stream(gpu):
    rng = np.random.default_rng(77)
    hyp, ref = fill(rng, 9, 5, 140, 70, 3)
    hl, rl = rng.integers(0, 141, size=45), rng.integers(0, 71, size=9)
    got = raw(hyp, hl, ref, rl)
    again = raw(hyp, hl, ref, rl)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes()                                 # two calls: the same bytes
    same(raw(hyp, hl, ref, rl, stream=torch.cuda.Stream()), got)


# ---- the Python surface ----------------------------------------------------------------
def _host(st):
    stats = torch.stack([st.distance, st.substitutions, st.deletions, st.insertions], dim=-1)
    if stats.dim() == 2:
        stats = stats.unsqueeze(1)
    return dict(stats=stats.cpu().numpy(), best=st.best.cpu().numpy(), totals=st.totals.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_model_cer(gpu, precision):
    """CTCModel.cer equals the reference on host copies of the model's own
    tokens: greedy, and beam = 4 with n_best = 4; error_rate is sum d / sum M."""
    import wakeword
    from wakeword.ctc import random_state_dict
    V, B, T = 12, 4, 40
    model = wakeword.CTCModel(random_state_dict(V, seed=3), V, precision=precision)
    feats = torch.randn((B, T, 80), generator=torch.Generator().manual_seed(1))
    rng = np.random.default_rng(2)
    targets, tl = rng.integers(1, V, size=(B, 9)), [9, 4, 0, 7]
    seqs = model.forward(feats)
    st = model.cer(feats, targets, tl)
    assert isinstance(st, wakeword.EditStats) and st.distance.is_cuda and st.distance.shape == (B,)
    hyp = np.zeros((B, 1, T), dtype=np.int64)
    for b, s in enumerate(seqs):
        hyp[b, 0, :len(s)] = s
    want = R.cer_batch(hyp, [len(s) for s in seqs], targets, tl)
    same(_host(st), want)
    assert wakeword.error_rate(st) == want["totals"][0, 0] / want["totals"][0, 4] == st.error_rate()
    assert st.sentence_error_rate() == want["totals"][0, 6] / B
    cut = model.cer(feats, targets, tl, input_lengths=[T, 17, 0, 33])
    same(_host(cut), R.cer_batch(model.frame_argmax(B, T).cpu().numpy(), [T, 17, 0, 33], targets, tl, collapse_frames=True))
    # 1-D concatenated targets are the same references
    flat = np.concatenate([targets[b, :n] for b, n in enumerate(tl)])
    same(_host(model.cer(feats, flat, tl)), want)
    res = model.beam_decode(feats, beam=4, top_k=8, n_best=4)
    st = model.cer(feats, targets, tl, beam=4, top_k=8, n_best=4)
    assert st.distance.shape == (B, 4)
    want = R.cer_batch(res.tokens.cpu().numpy(), res.lengths.cpu().numpy().reshape(-1), targets, tl)
    same(_host(st), want)
    assert wakeword.error_rate(st, oracle=True) == want["totals"][1, 0] / want["totals"][1, 4] <= wakeword.error_rate(st)
    with pytest.raises(ValueError, match="n_best"):
        model.cer(feats, targets, tl, n_best=2)


@pytest.mark.gpu
def test_cer_audio(gpu):
    import wakeword
    from wakeword.ctc import random_state_dict
    V, n = 12, 8000
    model = wakeword.CTCModel(random_state_dict(V, seed=4), V)
    t = np.arange(n, dtype=np.float32) / 16000.0
    audio = np.stack([0.3 * np.sin(2 * np.pi * f * t) * np.sin(2 * np.pi * 3.0 * t) ** 2 for f in (440.0, 1250.0)]).astype(np.float32)
    targets, tl = np.array([[3, 7, 7, 1], [2, 5, 0, 0]]), [4, 2]
    tok, ln = model.decode_audio(audio, n)
    st = model.cer_audio(audio, targets, tl, n_samples=n)
    same(_host(st), R.cer_batch(tok.cpu().numpy(), ln.cpu().numpy(), targets, tl))


@pytest.mark.gpu
def test_val_cer_and_train_history(gpu):
    """Two tiny epochs (V = 12, T = 40, B = 4, two validation batches):
    history["val_cer"] has one entry per epoch, each the reference's sum d / sum M
    on the frame labels the model decoded at that epoch's weights."""
    import wakeword
    from wakeword.ctc import random_state_dict
    V, T, B = 12, 40, 4
    rng = np.random.default_rng(12)
    gen = torch.Generator().manual_seed(12)

    def batch():
        return (torch.randn((B, T, 80), generator=gen), torch.from_numpy(rng.integers(1, V, size=(B, 6))), torch.tensor([T, 31, T, 9]),
                torch.tensor([6, 3, 0, 2]))
    train, val = [batch(), batch()], [batch(), batch()]

    class Recording(wakeword.CTCTrainer):
        seen = []

        def val_cer(self, feats, targets, input_lengths, target_lengths):
            row = super().val_cer(feats, targets, input_lengths, target_lengths)
            want = R.cer_batch(self.model.frame_argmax(B, T).cpu().numpy(), input_lengths.numpy(), targets.numpy(),
                               target_lengths.numpy(), collapse_frames=True)
            assert row.is_cuda and row.dtype == torch.int64 and row.shape == (8,)
            assert row.cpu().numpy().tolist() == want["totals"][0].tolist()
            self.seen.append(want["totals"][0])
            return row

    trainer = Recording(random_state_dict(V, seed=1, out_scale=1.0), V, zero_infinity=True)
    hist = {}
    out = wakeword.train_ctc(train, val, V, num_epochs=2, trainer=trainer, history=hist)
    assert out[0] is trainer and len(out) == 4 and len(out[1]) == len(out[2]) == 2
    assert list(hist) == ["val_cer"] and len(hist["val_cer"]) == 2 and len(Recording.seen) == 4
    for epoch in range(2):
        tot = Recording.seen[2 * epoch] + Recording.seen[2 * epoch + 1]
        assert tot[4] == 22 and hist["val_cer"][epoch] == tot[0] / tot[4]
    # without history the loop is today's: the same losses from the same start, and no val_cer call
    plain = Recording(random_state_dict(V, seed=1, out_scale=1.0), V, zero_infinity=True)
    out2 = wakeword.train_ctc(train, val, V, num_epochs=2, trainer=plain)
    assert out2[1] == out[1] and out2[2] == out[2] and len(Recording.seen) == 4
