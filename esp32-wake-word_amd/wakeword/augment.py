"""Batched waveform augmentation on the device -- mirrors the stage that
``extract_features`` (ml_models/src/extract_mfcc.py:123-182) puts between the
WAV files and the features: ``pad_audio`` (:7-23), the five variants of
``augment_audio_waveform`` (:90-121) and ``add_random_noise`` (:25-45).

``augment_batch`` is ``wk_augment_batch`` (csrc/wk_augment.hip; the full
statement is in include/wakeword.h): raw clips go to the device once, and every
epoch draws its variants with fresh noise there.  The noise is Philox4x32-10
addressed by (seed, epoch, row, sample): the distribution of ``torch.randn``,
not its bit stream, and the same call gives the same bits.

Row order is the reference's: the K variants of clip 0, then of clip 1, ...
The pad noise of a clip is keyed by the clip, so its K variants see the same
padded clip; the pad behind a sped-up clip, the SNR noise and the SNR draw are
keyed by the output row, so a variant's noise depends on its position in
`variants` (moving a variant in the list gives it other noise, by design).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .api import _as_device, _stream, _torch, mfcc

REFERENCE_VARIANTS = ((1.0, 1.0), (0.8, 1.0), (1.2, 1.0), (1.0, 0.7), (1.0, 1.3))   # extract_mfcc.py:99-119
REFERENCE_SNR = (0.01, 5.0, 20.0)     # add_random_noise's noise_level and snr_range (:25)


def _is_i16(x) -> bool:
    return (isinstance(x, np.ndarray) and x.dtype == np.int16) or (hasattr(x, "dtype") and str(x.dtype) == "torch.int16")


def augment_batch(audio, lengths=None, variants: Sequence[Tuple[float, float]] = REFERENCE_VARIANTS,
                  pad_noise: float = 0.005, snr: Optional[Tuple[float, float, float]] = None, seed: int = 0,
                  epoch: int = 0, out_len: int = 16000, device: int = 0):
    """(n, L) clips -> (n * K, out_len) float32 on cuda:<device>, row i*K + v =
    variant v = (speed, volume) of clip i.

    audio: numpy or torch, float32 or int16 (scaled by 1/32768), as
    ``wakeword.mfcc`` takes it.  lengths: the clips' valid samples (n,), None =
    L for all; values outside [0, L] are clamped on the device.  pad_noise:
    ``pad_audio``'s noise level, 0 = zero pad.  snr: None, or ``(noise_level,
    lo_db, hi_db)`` of ``add_random_noise``.  (seed, epoch) address the noise:
    a new epoch draws all of it afresh."""
    torch = _torch()
    dev = f"cuda:{device}"
    i16 = _is_i16(audio)
    x = _as_device(audio, torch.int16 if i16 else torch.float32, dev)
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() != 2:
        raise ValueError(f"expected (n, L) audio, got {tuple(x.shape)}")
    n, L = x.shape
    ln = None
    if lengths is not None:
        if not hasattr(lengths, "dtype"):
            lengths = np.asarray(lengths, np.int32)
        ln = _as_device(lengths, torch.int32, dev).reshape(-1)
        if ln.numel() != n:
            raise ValueError(f"{ln.numel()} lengths for {n} clips")
    K = len(variants)
    if not 1 <= K <= _lib.WK_AUG_MAX_VARIANTS:
        raise ValueError(f"1 to {_lib.WK_AUG_MAX_VARIANTS} variants, got {K}")
    var = (_lib.WkAugVariant * K)(*[_lib.WkAugVariant(float(s), float(v)) for s, v in variants])
    noise, lo, hi = (0.0, 0.0, 0.0) if snr is None else (float(t) for t in snr)
    spec = _lib.WkAugSpec(float(pad_noise), noise, lo, hi, int(seed) & (2 ** 64 - 1), int(epoch) & 0xFFFFFFFF)
    out = torch.empty((n * K, int(out_len)), dtype=torch.float32, device=x.device)
    if x.numel() == 0:      # (no sample to point at: every row is pad)
        x = torch.zeros((max(n, 1), 1), dtype=x.dtype, device=x.device)
        ln = torch.zeros((max(n, 1),), dtype=torch.int32, device=x.device)
        L = 1
    with torch.cuda.device(x.device):
        check(lib().wk_augment_batch(C.c_void_p(x.data_ptr()), _lib.WK_DTYPE_I16 if i16 else _lib.WK_DTYPE_F32,
                                     C.c_void_p(ln.data_ptr()) if ln is not None else None, n, L, L, var, K,
                                     C.byref(spec), int(out_len), C.c_void_p(out.data_ptr()),
                                     _stream(torch, x.device)), "wk_augment_batch")
    return out


def extract_features(audio, lengths=None, label: int = 0, is_noise: bool = False, add_noise_to_pad: bool = True,
                     augment_audio: bool = True, seed: int = 0, epoch: int = 0, device: int = 0):
    """``extract_features`` (extract_mfcc.py:123-182) without the file walk:
    (n, L) clips -> (features (n*K, 13, 63), labels (n*K,)) on the device, K = 5
    with `augment_audio`, else 1.  ``augment_batch`` to 16000 samples (pad
    noise 0.005 with `add_noise_to_pad`; ``add_random_noise`` at (0.01, 5, 20)
    with `is_noise`), then ``mfcc(mode='torchaudio', cmvn=True)``."""
    torch = _torch()
    variants = REFERENCE_VARIANTS if augment_audio else ((1.0, 1.0),)
    wave = augment_batch(audio, lengths, variants=variants, pad_noise=0.005 if add_noise_to_pad else 0.0,
                         snr=REFERENCE_SNR if is_noise else None, seed=seed, epoch=epoch, out_len=16000, device=device)
    feats = mfcc(wave, mode="torchaudio", cmvn=True, device=device)
    labels = torch.full((wave.shape[0],), label, dtype=torch.int64, device=feats.device)
    return feats, labels
