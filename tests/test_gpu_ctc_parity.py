"""CTC head against float64 on a trained-like model (tests/ctc_ref.py): LayerNorm
parameters off 1 / 0, a saturated GRU, the blank and the last ragged column
winning half and a tenth of the frames; T from 1 to 129 (either side of the
one-call path's switch at 6 and of the decode's 64-frame chunk) and B either
side of the recurrences' 16- and 32-utterance tiles.

* log-probs within K32 e32 (fp32) / K16 e16 (fp16 modes) of ref64, e32 / e16
  being the error of torch-CPU fp32 / of the fp16-operand emulation ref16 on
  the same case (constants and the measurement behind them: ctc_ref.K32, K16;
  profiles/ctc_parity_bounds.md);
* the per-frame argmax equal to ref64's wherever its top-2 margin exceeds
  twice that bound, with the gate's cap and coverage asserted (at most 15 % of
  frames left out; blank and last column among those compared);
* tokens and lengths equal to decode_predictions of the device's own argmax
  map, exactly, and the decode's edge patterns present in that map.
Each (vocab, mode, path, case) is one forward, run once and shared."""
import functools
import os

import numpy as np
import pytest
import torch

import ctc_ref as R

FEAT_ATOL = 2e-3      # tests/test_ctc.py's feature tolerance: here only the conditioning check

# mode -> (precision, environment while the handle is created)
HANDLES = {"fp32": ("fp32", {}), "fp16": ("fp16", {}), "gemm": ("fp16", {"WAKEWORD_CTC_GEMM": "1"}),
           "out16": ("fp32", {"WAKEWORD_CTC_MIX": "out16"})}
LP_MODES = ("fp32", "fp16", "gemm")          # out16 decodes only
CASE_IDS = [f"B{b}-T{t}" for b, t in R.CASES]
# one-call path (wk_ctc_transcribe): T = 1 + n_samples // 160, n_samples > 200
AUDIO_T = {2: 201, 5: 640, 6: 800, 7: 960, 129: 160 * 128}


@functools.lru_cache(maxsize=None)
def handle(vocab, mode):
    import wakeword
    precision, env = HANDLES[mode]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return wakeword.CTCModel(R.model(vocab).state_dict(), vocab, precision=precision)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    yield
    handle.cache_clear()
    run.cache_clear()
    audio_run.cache_clear()


@functools.lru_cache(maxsize=None)
def run(vocab, mode, path, B, T):
    """One forward of the (vocab, B, T) case: path "lp" with log-probs, "tok"
    the argmax-only kernels.  -> (max |log-probs - ref64| or None, frame argmax,
    tokens, lengths)."""
    g, c = handle(vocab, mode), R.case(vocab, B, T)
    tok, ln, lp = g.decode(c.feats, return_log_probs=path == "lp")
    pred = g.frame_argmax(B, T).cpu().numpy()
    err = None
    if lp is not None:
        lp = lp.cpu()
        assert lp.shape == c.lp.shape and bool(torch.isfinite(lp).all())
        err = float((lp.double() - c.lp).abs().max())
    return err, pred, tok.cpu().numpy(), ln.cpu().numpy()


@functools.lru_cache(maxsize=None)
def audio_run(vocab, mode, T):
    """wk_ctc_transcribe on the case's clips cut to T frames.  Its reference is
    ref64 on the handle's own features() of that audio (held to the oracle's by
    the feature tests), so only the head is compared; fp16 mode at T >= 6
    z-scores inside the encoder instead, a rounding of the same features."""
    g = handle(vocab, mode)
    n = AUDIO_T[T]
    x = R.audio_case(35)[:, :n]
    tok, ln = g.decode_audio(x, n_samples=n)
    pred = g.frame_argmax(35, T).cpu().numpy()
    c = R.Case(vocab, g.features(x, n_samples=n).cpu())
    return c, pred, tok.cpu().numpy(), ln.cpu().numpy()


def assert_argmax(c, mode, pred):
    ok = R.gate(c, mode)
    R.check_gate(c, ok)
    bad = (torch.from_numpy(pred).long() != c.argmax) & ok
    assert not bool(bad.any()), (int(bad.sum()), float(c.margin[bad].max()), R.bound(c, mode))


def assert_decode(pred, tok, ln):
    want_tok, want_ln = R.greedy(pred)
    assert np.array_equal(ln, want_ln)
    assert np.array_equal(tok, want_tok)


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
@pytest.mark.parametrize("mode", LP_MODES)
@pytest.mark.parametrize("vocab", R.VOCABS)
def test_log_probs_within_k_reference_errors(gpu, vocab, mode, case):
    """max |device log-probs - ref64| <= K * (the reference arithmetic's own
    error on the case).  Measured ratios: 1.22 to 1.90 (fp32), 0.91 to 1.14 (fp16
    modes); K is twice the worst (ctc_ref.K32, K16)."""
    c = R.case(vocab, *case)
    err, _, _, _ = run(vocab, mode, "lp", *case)
    ref_err = c.err(mode)
    print(f"ctc-parity V={vocab} mode={mode} B={c.B} T={c.T} dev={err:.3e} ref={ref_err:.3e} ratio={err / ref_err:.2f}")
    assert err <= R.bound(c, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
@pytest.mark.parametrize("mode,path", [(m, "lp") for m in LP_MODES] + [(m, "tok") for m in HANDLES])
@pytest.mark.parametrize("vocab", R.VOCABS)
def test_frame_argmax_matches_ref64(gpu, vocab, mode, path, case):
    """frame_argmax after forward, with log-probs and on the argmax-only path,
    on every frame the gate keeps."""
    assert_argmax(R.case(vocab, *case), mode, run(vocab, mode, path, *case)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
@pytest.mark.parametrize("mode,path", [("fp32", "lp"), ("fp32", "tok"), ("fp16", "lp"), ("fp16", "tok"), ("gemm", "tok"),
                                       ("out16", "tok")])
@pytest.mark.parametrize("vocab", R.VOCABS)
def test_decode_is_greedy_of_own_argmax(gpu, vocab, mode, path, case):
    """tokens / lengths == decode_predictions(frame_argmax), ungated: batch-major
    best[] (fp32 handles) and time-major (fp16)."""
    _, pred, tok, ln = run(vocab, mode, path, *case)
    assert_decode(pred, tok, ln)


@pytest.mark.gpu
@pytest.mark.parametrize("T", sorted(AUDIO_T))
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
@pytest.mark.parametrize("vocab", R.VOCABS)
def test_one_call_path(gpu, vocab, mode, T):
    """wk_ctc_transcribe either side of its unfused / fused switch (T = 6) and at
    T = 129: the gated argmax against ref64 and the exact decode."""
    c, pred, tok, ln = audio_run(vocab, mode, T)
    assert_decode(pred, tok, ln)
    ok = R.gate(c, mode)
    bad = (torch.from_numpy(pred).long() != c.argmax) & ok
    assert float(ok.float().mean()) >= 1.0 - R.MAX_EXCLUDED or T < 5
    assert not bool(bad.any()), (int(bad.sum()), float(c.margin[bad].max()), R.bound(c, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
@pytest.mark.parametrize("vocab", R.VOCABS)
def test_decode_edge_patterns_on_device(gpu, vocab, mode):
    """The device's own argmax maps hold the patterns the equality above is
    about: a blank at t = 0, "a, blank, a", a repeat and a blank across frames
    63 / 64 (T = 65, 129, and T = 129 through the one-call path); at T <= 2 an
    all-blank utterance with length 0 and every slot -1."""
    maps = [run(vocab, mode, "tok", 35, T)[1] for T in (65, 129)] + [audio_run(vocab, mode, 129)[1]]
    for pred in maps:
        p = R.patterns(pred)
        assert all(p[k] for k in ("blank_at_0", "a_blank_a", "repeat_63_64", "blank_63_64")), p
    for T in (1, 2):
        _, pred, tok, ln = run(vocab, mode, "tok", 35, T)
        blank = (pred == 0).all(1)
        assert blank.any() and (ln[blank] == 0).all() and (tok[blank] == -1).all()


@pytest.mark.gpu
def test_out16_mix_refuses_log_probs(gpu):
    """WAKEWORD_CTC_MIX=out16 decodes only (as out32): asking it for log-probs
    is an error, not an unwritten buffer."""
    import wakeword
    c = R.case(512, 1, 13)
    with pytest.raises(wakeword.WakewordError, match="out16"):
        handle(512, "out16").decode(c.feats, return_log_probs=True)


# ---- features at other amplitudes --------------------------------------------------
# The existing feature tests use synth_clips' own level (|x| <= 0.5).  The
# z-scored log-mel is scale-free but for the 1e-8 floor; x 1e-3 (a quiet
# recording) and x 32768 (int16-valued floats) are both well-conditioned:
# torch-CPU fp32 stays within 3e-5 of float64 there, far inside FEAT_ATOL.
# Bound: KFEAT times torch-CPU fp32's own error on the same input.  Measured on
# the MI355X (profiles/ctc_parity_bounds.md): device / reference ratios 0.81,
# 2.87, 5.40 and 6.93 (device error 1.6e-5 to 2.0e-5); KFEAT = twice the worst.
KFEAT = 14.0


@pytest.mark.gpu
@pytest.mark.parametrize("n_samples", [1920, 48000], ids=["T13", "T301"])
@pytest.mark.parametrize("amp", [1e-3, 32768.0])
def test_features_at_other_amplitudes(gpu, amp, n_samples):
    from oracle import wk_ctc_oracle as CO
    from oracle import wk_oracle as O
    x = (O.synth_clips(11, 0, 5, n_samples) * np.float32(amp)).astype(np.float32)
    ref = R.features64(x)
    ref_err = float((CO.features(torch.from_numpy(x)).double() - ref).abs().max())
    assert ref_err < FEAT_ATOL          # else the input is ill-conditioned and proves nothing
    got = handle(512, "fp32").features(x, n_samples=n_samples).cpu().double()
    err = float((got - ref).abs().max())
    print(f"ctc-features amp={amp:g} T={1 + n_samples // 160} dev={err:.3e} ref={ref_err:.3e} ratio={err / ref_err:.2f}")
    assert err <= KFEAT * ref_err
