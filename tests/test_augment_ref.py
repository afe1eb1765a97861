"""CPU tests of tests/augment_ref.py, the reference that wk_augment_batch is held
against on the device: its noise-free rows against the host's wk_augment and
F.interpolate, its generator against the known answers and N(0, 1), its SNR
stage against the reference's own lines in torch float64, and the mutations
against the bounds of the device test."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as A
from ctc_dropout_ref import philox4x32_10


def host_augment(x, speed, volume, out_len):
    from wakeword import _lib
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(out_len, np.float32)
    st = _lib.lib().wk_augment(x.ctypes.data_as(C.c_void_p), x.size, speed, volume, 0.0, 0, out.ctypes.data_as(C.c_void_p),
                               out_len)
    assert st == 0
    return out


@pytest.mark.parametrize("out_len", [16000, 4099, 257, 1])
def test_noise_free_rows_are_the_host_functions_bits(out_len):
    """Zero-padded clips, all five variants, the blend rounded to float32 one operation at a time."""
    rng = np.random.default_rng(out_len)
    x = rng.uniform(-0.9, 0.9, size=(2, out_len)).astype(np.float32)
    lengths = (out_len, out_len // 2)
    x[1, lengths[1]:] = 0.0            # (the host function takes the padded clip)
    variants = A.REFERENCE_VARIANTS if out_len > 1 else A.VARIANTS_LEN1
    ref = A.reference(x, lengths, variants, 0.0, None, 0, 0, out_len, np.float32).out
    for i in range(2):
        for v, (speed, volume) in enumerate(variants):
            host = host_augment(x[i], speed, volume, out_len)
            assert np.array_equal(ref[i * 5 + v].view(np.uint32), host.view(np.uint32)), (i, v)


@pytest.mark.parametrize("speed", [0.8, 1.2, 0.5])
def test_resampling_is_f_interpolate(speed):
    n = 16000
    x = np.random.default_rng(3).uniform(-1, 1, size=(1, n)).astype(np.float32)
    ref = A.reference(x, None, ((speed, 1.0),), 0.0, None, 0, 0, n).out[0]
    m = int(n * speed)
    want = F.interpolate(torch.from_numpy(x)[None], size=m, mode="linear", align_corners=False)[0, 0].double().numpy()
    k = min(m, n)
    assert np.abs(ref[:k] - want[:k]).max() <= 1e-7      # the host test's bound
    assert not ref[k:].any()


def test_philox_known_answers():
    """The three of csrc/wk_philox.h."""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)))
    for ctr, key, want in kat:
        assert tuple(int(w) for w in philox4x32_10(np.array(ctr, np.uint64), key)) == want
    # the addressing: counter = (q, row, epoch, stream)
    w = A.words(0x299F31D0A4093822, 0x13198A2E, 0x03707344, 0x85A308D3, 8)
    direct = philox4x32_10(np.array((5, 0x85A308D3, 0x13198A2E, 0x03707344), np.uint64), (0xA4093822, 0x299F31D0))
    assert np.array_equal(w[5], direct)


def test_gaussians_are_standard_normal():
    n = 10 ** 6
    g = A.gauss(0x9E3779B97F4A7C15, 1, 2, 12345, n)
    assert g.shape == (n,)
    mean, var = g.mean(), g.var()
    kurt = ((g - mean) ** 4).mean() / var ** 2
    # standard errors of the three under N(0, 1): sqrt(1/n), sqrt(2/n), sqrt(24/n)
    assert abs(mean) <= 5 * np.sqrt(1 / n)
    assert abs(var - 1) <= 5 * np.sqrt(2 / n)
    assert abs(kurt - 3) <= 5 * np.sqrt(24 / n)
    assert abs(np.corrcoef(g[0::2], g[1::2])[0, 1]) <= 5 / np.sqrt(n / 2)      # a pair's cos and sin


def test_snr_stage_is_the_references_lines():
    rng = np.random.default_rng(5)
    for amp in (0.9, 0.05, 0.0):
        b = rng.uniform(-amp, amp, size=4099)
        z = 0.01 * rng.standard_normal(4099)
        for u in (0.0, 0.37, 1.0 - 2.0 ** -24):
            got = A.snr_stage(b, z, u, 5.0, 20.0)
            want = A.snr_stage_torch(b, z, u, 5.0, 20.0, torch.float64)
            assert np.abs(got - want).max() <= 1e-15
    assert not A.snr_stage(np.zeros(8), np.ones(8), 0.5, 5.0, 20.0).any()       # Ps = 0: the noise is scaled to 0


def test_snr_is_the_power_ratio():
    """add_random_noise applies the amplitude ratio to powers: mean(b^2) / mean(noise^2) = snr = 10^(dB / 20)."""
    x = np.random.default_rng(6).uniform(-0.1, 0.1, size=(2, 16000)).astype(np.float32)      # nothing clamps
    ref = A.reference(x, (16000, 9000), A.REFERENCE_VARIANTS, A.PAD, A.SNR, 7, 3, 16000)
    for r in range(10):
        snr = 10.0 ** ((5.0 + ref.u[r] * 15.0) / 20.0)
        assert np.abs(ref.out[r]).max() < 1.0
        ratio = np.mean(ref.b[r] ** 2) / np.mean((ref.out[r] - ref.b[r]) ** 2)
        assert abs(ratio / snr - 1.0) <= 1e-4, (r, ratio, snr)
    assert len(set(ref.u)) == 10 and 0.0 <= ref.u.min() and ref.u.max() < 1.0


def test_cases_cover_what_the_issue_names():
    cs = A.CASES
    assert {c.n for c in cs} == {1, 3} and {c.out_len for c in cs} == {16000, 1, 257, 4099}
    assert {c.i16 for c in cs} == {False, True} and {(c.seed, c.epoch) for c in cs} == set(A.SEEDS)
    assert ((0.5, 2.0),) in {c.variants for c in cs}
    for out_len in (16000, 257, 4099):
        seen = {ln for c in cs if c.out_len == out_len for ln in c.lengths}
        assert seen >= {0, 1, out_len - 1, out_len, out_len + 37}


@pytest.mark.parametrize("mutation", A.MUTATIONS)
def test_mutation_falls_outside_the_device_bounds(mutation):
    """A tolerance that admits one of them is too wide: the mutated reference, put in the device's place, must fail
    the device test's checks 2 or 3 (at the final K_SNR) on one of its cases."""
    assert A.K_SNR is not None
    caught = []
    for k, c in enumerate(A.CASES):
        if c.out_len == 16000 and c.n == 3:
            continue                      # (the smaller cases already tell; keeps the test quick)
        _, x = A.case_audio(c)
        pad = A.reference(x, c.lengths, c.variants, A.PAD, None, c.seed, c.epoch, c.out_len, mutation=mutation).out
        full = A.reference(x, c.lengths, c.variants, A.PAD, A.SNR, c.seed, c.epoch, c.out_len, mutation=mutation).out
        bad, _ = A.check_rows(k, None, pad, full, tag=mutation)
        caught += bad
    assert caught, f"{mutation} passes every device check"


def test_unmutated_reference_passes_its_own_checks():
    for k in (3, 6):
        q, p, s, _ = A.case_refs(k)
        assert A.check_rows(k, q, p, s, tag="reference") == ([], 0.0)
