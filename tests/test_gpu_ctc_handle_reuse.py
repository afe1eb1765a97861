"""GPU tests of one wk_ctc handle reused across geometries: what a call returns
must not depend on what the handle did before.

A handle keeps three workspaces that grow on demand (wk_ctc_forward's,
wk_ctc_transcribe's, the training one with its lazily made dropped copy), the
"last call" markers wk_ctc_frame_argmax, wk_ctc_transcribe_stats,
wk_ctc_backward and wk_ctc_dropout_masks check, and the stage-timing ring.
Each sequence below goes small -> large (a regrow) -> small (reuse of a larger
workspace) -> large (reuse at capacity), and every output of every step is
compared bit for bit with a fresh handle that makes only that call.  V = 512:
there the backward's K splits do not depend on the workspace's capacity
(profiles/ctc_handle_refactor.md), so the gradient's bits are a function of
the call alone.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 512
GEOMS = ((3, 5), (17, 13), (2, 7), (17, 13))                      # (B, T)
AUDIO = ((2, 800), (9, 2080), (3, 480), (9, 2080))                # (batch, n_samples): T = 6, 14, 4, 14
TRAIN = (((3, 5), (0.1, 0.2)), ((17, 13), (0.1, 0.2)), ((2, 7), None), ((17, 13), (0.1, 0.2)))
STAGES = ("LOGMEL", "ZSCORE", "ENCODER", "PROJ0", "GRU0", "PROJ1", "GRU1", "OUTPUT", "DECODE")
# wk_ctc_stage_times after 10 wk_ctc_transcribe at (2, 800): one bracket per stage and call;
# the fp16 GRU has its projections fused in (no PROJ stage)
COUNTS = {"fp32": [10] * 9, "fp16": [10, 10, 10, 0, 10, 0, 10, 10, 10]}


@functools.lru_cache(maxsize=None)
def weights():
    from wakeword import ctc
    return ctc.pack_state_dict(ctc.random_state_dict(V, seed=3), V)


def fresh(precision):
    import wakeword
    return wakeword.CTCModel(weights(), V, precision=precision)


@functools.lru_cache(maxsize=None)
def feats(B, T):
    return torch.randn((B, T, 80), generator=torch.Generator().manual_seed(100 * B + T))


@functools.lru_cache(maxsize=None)
def dlogits(B, T):
    return torch.randn((B, T, V), generator=torch.Generator().manual_seed(7 + 100 * B + T)) * 1e-2


@functools.lru_cache(maxsize=None)
def audio(batch, n):
    return (torch.rand((batch, n), generator=torch.Generator().manual_seed(batch + n)) - 0.5).numpy()


def same(tag, got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, i)
        assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)), \
            f"{tag}: output {i} differs from a fresh handle's"


def decode_step(m, B, T):
    tok, ln, lp = m.decode(feats(B, T), return_log_probs=True)
    return [tok, ln, lp, m.frame_argmax(B, T)]


@pytest.mark.parametrize("precision", ("fp32", "fp16"))
def test_decode_sequence(gpu, precision):
    m = fresh(precision)
    for i, (B, T) in enumerate(GEOMS):
        got = decode_step(m, B, T)
        want = decode_step(fresh(precision), B, T)
        torch.cuda.synchronize()
        same(f"decode {precision} step {i} ({B}, {T})", got, want)


def transcribe_step(m, batch, n, fused):
    T = 1 + n // 160
    out = list(m.decode_audio(audio(batch, n), n_samples=n))
    out.append(m.frame_argmax(batch, T))
    if fused:
        out += list(m.transcribe_stats(batch, T, return_raw=True))
    return out


@pytest.mark.parametrize("precision", ("fp32", "fp16"))
def test_transcribe_sequence(gpu, precision):
    import wakeword
    m = fresh(precision)
    for i, (batch, n) in enumerate(AUDIO):
        T = 1 + n // 160
        fused = precision == "fp16" and T >= 6
        got = transcribe_step(m, batch, n, fused)
        want = transcribe_step(fresh(precision), batch, n, fused)
        torch.cuda.synchronize()
        same(f"transcribe {precision} step {i} ({batch}, {n})", got, want)
        if not fused:
            with pytest.raises(wakeword.WakewordError, match=f"batch {batch}, T {T}, not fused"):
                m.transcribe_stats(batch, T)


def train_step(m, B, T, dropout):
    lp = m.forward_train(feats(B, T), dropout=dropout, seed=11, offset=1000 * B + T)
    enc, gru = m.dropout_masks()
    flat, norm = m.backward(dlogits(B, T), return_norm=True)
    return [lp, enc, gru, flat, norm]


def test_training_sequence(gpu):
    """The second step regrows the training workspace, which drops the dropped
    copy of layer 0's output and makes it again; the third runs without
    dropout on the larger workspace; the decodes around the sequence show the
    inference workspace is apart from the training one."""
    m = fresh("fp32")
    dec = decode_step(fresh("fp32"), 17, 13)
    same("decode before training", decode_step(m, 17, 13), dec)
    for i, ((B, T), dropout) in enumerate(TRAIN):
        got = train_step(m, B, T, dropout)
        want = train_step(fresh("fp32"), B, T, dropout)
        torch.cuda.synchronize()
        if dropout:
            assert not bool(got[1].all()) and not bool(got[2].all())
        else:
            assert bool(got[1].all()) and bool(got[2].all())
        same(f"train step {i} ({B}, {T}) dropout {dropout}", got, want)
        same(f"frame_argmax after train step {i}", [m.frame_argmax(17, 13)], dec[3:])
    same("decode after training", decode_step(m, 17, 13), dec)
    torch.cuda.synchronize()


def stage_counts(m):
    from wakeword import _lib
    ms = (C.c_double * len(STAGES))()
    cnt = (C.c_int64 * len(STAGES))()
    _lib.check(_lib.lib().wk_ctc_stage_times(m._h, ms, cnt), "wk_ctc_stage_times")
    assert all(np.isfinite(v) and v >= 0.0 for v in ms)
    return list(cnt)


@pytest.mark.parametrize("precision", ("fp32", "fp16"))
def test_stage_counts(gpu, precision):
    """10 transcribes record 90 (fp16: 70) event pairs, more than the ring of 64
    holds, so it folds once on the way; wk_ctc_stage_times covers features and
    forward only, so the training calls add nothing."""
    from wakeword import _lib
    m = fresh(precision)
    _lib.check(_lib.lib().wk_ctc_profile(m._h, 1), "wk_ctc_profile")
    for _ in range(10):
        m.decode_audio(audio(2, 800), n_samples=800)
    counts = stage_counts(m)
    print(f"stage counts {precision}: {dict(zip(STAGES, counts))}")
    assert counts == COUNTS[precision]
    if precision == "fp32":
        m.forward_train(feats(3, 5))
        m.backward(dlogits(3, 5))
        m.forward_train(feats(3, 5), dropout=(0.1, 0.2), seed=1)
        m.backward(dlogits(3, 5))
    else:
        with pytest.raises(_lib.WakewordError, match="fp32 handles only"):
            m.forward_train(feats(3, 5))
    assert stage_counts(m) == counts
    m.decode(feats(3, 5))                       # no LOGMEL / ZSCORE: wk_ctc_forward alone
    assert stage_counts(m) == [c + (1 if c and i >= 2 else 0) for i, c in enumerate(counts)]
    _lib.check(_lib.lib().wk_ctc_profile(m._h, 0), "wk_ctc_profile")
    assert stage_counts(m) == [0] * len(STAGES)
    torch.cuda.synchronize()
