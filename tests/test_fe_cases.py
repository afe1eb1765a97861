"""The conditions tests/test_gpu_fe_degenerate.py relies on, checked with the
references alone (CPU): which rows the CMVN comparison leaves out, what the
oracle makes of silence, and that a constant row is a real hazard for an fp32
mean taken with the device's reduction order."""
import numpy as np

import fe_cases as F
from oracle import wk_oracle as O


def test_cases_are_what_they_say():
    assert tuple(F.CASES) == F.NAMES and len(F.NAMES) == 12
    for name, x in F.CASES.items():
        assert x.shape == (F.N,) and x.dtype == np.float32 and np.abs(x).max() <= 1.0, name
    assert F.INT16_NAMES == ("silence", "dc0.5", "int16_min", "quiet1lsb")
    assert int(F.int16_form("int16_min")[0]) == -32768 and int(F.int16_form("dc0.5")[0]) == 16384
    for name in F.INT16_NAMES:      # the int16 form is the same clip: one reference serves both
        assert np.array_equal(F.int16_form(name).astype(np.float32) / 32768.0, F.CASES[name]), name
    q = F.CASES["quiet1lsb"] * 32768.0
    assert set(np.unique(q)) == {-1.0, 0.0, 1.0}
    sq = F.CASES["fullscale_sq"]
    assert np.all(sq[:20] == 1.0) and np.all(sq[20:40] == -1.0) and np.all(sq[40:60] == 1.0)
    assert not F.CASES["half_silence"][8000:].any() and F.CASES["half_silence"][:8000].std() > 0.09


def test_only_the_rows_of_silence_are_left_out():
    """The cap on the CMVN comparison: rows with s_k < eps_raw are the 13 rows
    of silence and no others."""
    r = F.ref()
    for i, name in enumerate(F.NAMES):
        print(f"{name:17s} e_host={r.e_host[i]:.2e} eps_raw={r.eps[i]:.2e} max|raw64|={np.abs(r.raw64[i]).max():.2f} "
              f"min s_k={r.s[i].min():.3e} max|f64|={np.abs(r.f64[i]).max():.3f}")
    left_out = [(F.NAMES[i], k) for i, k in zip(*np.nonzero(~r.kept))]
    assert left_out == [("silence", k) for k in range(13)], left_out
    assert np.isfinite(r.raw64).all() and np.isfinite(r.f64).all()
    # the CNN sees the CMVN maximum 62 / sqrt(63) on these inputs (synthetic noise stays below about 3.5)
    assert np.abs(r.f64).max() > 7.8


def test_oracle_on_silence():
    r = F.ref()
    i = F.NAMES.index("silence")
    f = O.features_mode_b(F.CASES["silence"])
    print(f"silence: oracle max|f| = {np.abs(f).max():.2e}, raw c0 = {r.raw64[i, 0, 0]:.6f}")
    assert np.abs(f).max() <= 1e-5
    raw = r.raw64[i]
    assert np.array_equal(raw, np.repeat(raw[:, :1], 63, axis=1))       # columns 0..62 identical, edge frames too
    # the host library normalises in double: constant rows come out at the oracle's size, not +-0.99
    from wakeword import host
    assert np.abs(host.mfcc(F.CASES["silence"])).max() <= 1e-5


def test_wave_sum_emulation_is_a_sum():
    rng = np.random.default_rng(3)
    v = rng.standard_normal((50, 64)).astype(np.float32)
    assert np.abs(F.wave_sum32(v) - v.astype(np.float64).sum(axis=1)).max() < 1e-5
    k = np.arange(64, dtype=np.float32)                                  # exact in fp32 whatever the order
    assert float(F.wave_sum32(k)) == 2016.0


def test_fp32_mean_of_a_constant_row_is_a_hazard():
    """63 identical values summed in wave_sum's order do not always give 63 v:
    then mean != v, d = v - mean is an ulp in every lane and the whole row
    comes out +-sqrt(62/63) instead of 0.  Counted over the 101 fp32 neighbours
    of the silent clip's c0; with the kernels' rule (a row of equal values is
    taken as a row of zeros) none remains, and rows that vary keep their bits."""
    from wakeword import host
    c0 = host.mfcc(F.CASES["silence"], cmvn=False)[0, 0, 0]
    rows = np.repeat(F.neighbours32(c0)[:, None], 63, axis=1)
    assert rows.shape == (101, 63)
    bad = int((np.abs(F.cmvn_lane32(rows, flat_rule=False)).max(axis=1) > 0.5).sum())
    bad_rule = int((F.cmvn_lane32(rows) != 0).any(axis=1).sum())
    print(f"host c0 on silence = {c0!r}: {bad} of 101 neighbouring constant rows give |f| > 0.5 without the rule, "
          f"{bad_rule} are not exactly 0 with it")
    assert bad > 0
    assert bad_rule == 0
    v = (np.random.default_rng(4).standard_normal((20, 63)) + c0).astype(np.float32)
    assert np.array_equal(F.cmvn_lane32(v), F.cmvn_lane32(v, flat_rule=False))
    assert np.abs(F.cmvn_lane32(v) - O.normalize_mfcc(v)).max() < 1e-3
