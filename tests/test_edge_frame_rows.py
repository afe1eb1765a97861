"""The row geometry the fused kernel's edge rounds rely on (csrc/wk_fe_dev.h,
fe_stage0_rows), from the constants alone: hop 256, window 320, centre pad 256,
16,000 samples.  Lane j of row n1 of frame t holds the samples
i0 = 256 t - 160 + 32 n1 + 2 j and i0 + 1.

  - the centre padding reflects whole rows: rows 0-4 of frame 0 and row 9 of
    frame 62, and nothing else;
  - the register mapping of the edge rounds (unreflected pair loads only, the
    reflected rows taken from the frame's other rows by DPP row moves, x[160]
    in xb) yields the samples refl_idx gives, for every (n1, j)."""
import numpy as np

HOP, WIN, PAD, N = 256, 320, 256, 16000
N_FFT = 512
N_FRAMES = 1 + N // HOP
BASE0 = -PAD + (N_FFT - WIN) // 2          # -160: first sample of frame 0's window


def refl_idx(i, n=N):
    i = np.abs(i)
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def _i0(t):
    n1, j = np.meshgrid(np.arange(10), np.arange(16), indexing="ij")
    return HOP * t + BASE0 + 32 * n1 + 2 * j


def test_constants_match_the_oracle():
    from oracle import wk_oracle as O
    assert (O.HOP, O.WIN_LENGTH, O.N_FFT, O.WIN_SAMPLES, O.N_FRAMES) == (HOP, WIN, N_FFT, N, N_FRAMES)
    assert BASE0 == -160 and HOP * 62 + BASE0 == 15712
    # refl_idx is numpy's reflect padding
    x = np.arange(N)
    assert np.array_equal(np.pad(x, (PAD, PAD), mode="reflect"), refl_idx(np.arange(-PAD, N + PAD)))


def test_reflection_is_uniform_per_row():
    for t in range(N_FRAMES):
        i0 = _i0(t)
        refl = np.stack([(i0 + d < 0) | (i0 + d > N - 1) for d in (0, 1)], -1)   # [n1][j][sample of the pair]
        whole = refl.all(axis=(1, 2))
        none = ~refl.any(axis=(1, 2))
        assert (whole | none).all(), t            # no mixed row
        want = {0: [0, 1, 2, 3, 4], 62: [9]}.get(t, [])
        assert np.flatnonzero(whole).tolist() == want, t
    assert _i0(0)[5, 0] == 0                      # y[0] = x[0] is row 5, lane 0 of frame 0


# DPP row moves over the 16 lanes of a lane group; `old` fills lanes without a source.
def _mirror(v):
    return v[::-1].copy()


def _shr1(old, v):      # lane j <- lane j - 1
    return np.concatenate([old[:1], v[:-1]])


def _shl1(old, v):      # lane j <- lane j + 1
    return np.concatenate([v[1:], old[-1:]])


def _loaded(t):
    """Sample indices the unreflected pair loads bring in: first/second [n1][j], -1 = outside the clip (reads 0)."""
    i0 = _i0(t)
    ok = (i0 >= 0) & (i0 + 1 <= N - 1)
    return np.where(ok, i0, -1), np.where(ok, i0 + 1, -1)


def _want(t, n1):
    """What a reflected row needs: x[r(i0)], x[r(i0+1)], x[r(i0+2)] (y(i0) = x[r(i0)] + pre x[r(i0+1)],
    y(i0+1) = x[r(i0+1)] + pre x[r(i0+2)])."""
    i0 = _i0(t)[n1]
    return refl_idx(i0), refl_idx(i0 + 1), refl_idx(i0 + 2)


def test_frame0_register_mapping():
    x0, x1 = _loaded(0)
    xb = 160
    assert (x0[:5] == -1).all() and (x0[5:] >= 0).all()       # rows 0-4 load nothing, rows 5-9 hold x[0..159]
    for n1 in range(5):
        p1 = _mirror(x0[9 - n1])                  # x[r0 - 2]
        c1 = _mirror(x1[9 - n1])                  # x[r0 - 1]
        l0 = xb if n1 == 0 else x0[10 - n1][0]
        c0 = _shr1(np.array([l0]), p1)            # x[r0]
        r0, r1, r2 = _want(0, n1)
        assert np.array_equal(c0, r0) and np.array_equal(c1, r1) and np.array_equal(p1, r2), n1
        assert (r0 % 2 == 0).all() and np.array_equal(r0, 160 - 32 * n1 - 2 * np.arange(16))


def test_frame62_register_mapping():
    x0, x1 = _loaded(62)
    assert (x0[:9] >= 0).all() and (x0[9] == -1).all()        # row 9 loads nothing
    assert (x0[8][0], x1[8][15]) == (15968, 15999)
    c0 = _mirror(x0[8])                           # x[r0]
    s1 = _mirror(x1[8])                           # x[r0 + 1]
    p1 = _shl1(x0[7], c0)                         # x[r0 - 2]; lane 15: its own row-7 first, x[15966]
    c1 = _shl1(x1[7], s1)                         # x[r0 - 1]; lane 15: x[15967]
    r0, r1, r2 = _want(62, 9)
    assert np.array_equal(c0, r0) and np.array_equal(c1, r1) and np.array_equal(p1, r2)
    assert np.array_equal(r0, 15998 - 2 * np.arange(16))


def test_every_load_is_pair_aligned():
    """The edge rounds issue only the common round's loads: pairs at even
    sample indices (8-byte aligned for float32 clips with an even clip_stride),
    and one single sample (xb)."""
    for t in (0, 62):
        assert (_i0(t) % 2 == 0).all()
