"""ctypes binding of libwakeword.so (the C ABI declared in include/wakeword.h).

The library is the product: every compute entry point below runs a HIP kernel.
There is no CPU fallback -- if the library is missing, ``lib()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WAKEWORD_LIB", os.path.join(_PKG, "libwakeword.so"))

WK_OK = 0
WK_MODE_TORCHAUDIO_CMVN = 0
WK_MODE_ESP_MFCC = 1
WK_DTYPE_F32 = 0
WK_DTYPE_I16 = 1
WK_DTYPE_I8 = 2
WK_PREC_FP32 = 0
WK_PREC_BF16 = 1
WK_PREC_INT8 = 2
WK_PREC_BF16X3 = 3
WK_NUM_WEIGHTS = 40224

# Every symbol include/wakeword.h declares (checked by tests/test_abi.py).
EXPORTS = ("wk_create", "wk_destroy", "wk_mfcc", "wk_cnn", "wk_forward", "wk_synth_clips", "wk_normalize",
           "wk_status_string", "wk_last_error", "wk_abi_version", "extract_mfcc", "free_mfcc",
           "analyze_mfcc_range", "wk_stream_create", "wk_stream_destroy", "wk_stream_reset", "wk_stream_push",
           "wk_ctc_num_weights", "wk_ctc_create", "wk_ctc_destroy", "wk_ctc_features", "wk_ctc_forward",
           "wk_wav_read", "wk_wav_load_batch", "wk_augment", "flow_extract_mfcc_single_frame", "wk_device_cmvn",
           "wk_check_device_errors", "wk_ctc_frame_argmax", "wk_record_front", "wk_quantize_frames",
           "wk_ctc_profile", "wk_ctc_stage_times", "wk_ctc_transcribe", "wk_esp_mfcc_create", "wk_esp_mfcc_run",
           "wk_esp_mfcc_destroy", "wk_scan", "wk_scan_workspace_bytes", "wk_trainer_create", "wk_trainer_destroy",
           "wk_trainer_grad", "wk_trainer_step", "wk_trainer_weights", "wk_quant_spec_default", "wk_set_quant",
           "wk_get_quant", "wk_quant_weights", "wk_calibrate_workspace_bytes", "wk_calibrate",
           "wk_ctc_loss_workspace_bytes", "wk_ctc_loss", "wk_ctc_forward_train", "wk_ctc_backward", "wk_ctc_weights",
           "wk_ctc_set_weights", "wk_ctc_adam_step", "wk_ctc_optim_state", "wk_ctc_set_optim_state",
           "wk_ctc_forward_train_dropout", "wk_ctc_dropout_masks", "wk_augment_batch",
           "wk_ctc_align_workspace_bytes", "wk_ctc_align", "wk_ctc_beam_workspace_bytes", "wk_ctc_beam",
           "wk_ctc_spot_workspace_bytes", "wk_ctc_spot", "wk_ctc_cer_workspace_bytes", "wk_ctc_cer",
           "wk_ctc_transcribe_stats")
WK_CTC_REDUCTION = {"none": 0, "sum": 1, "mean": 2}
WK_NUM_INT8_WEIGHTS = 3 * 13 * 32 + 3 * 32 * 64 + 3 * 64 * 128 + 128 * 64 + 64
WK_QUANT_TENSORS = 7
WK_QUANT_BINS = 32
WK_QUANT_CALIBRATE_INPUT = -2 ** 31
WK_AUG_MAX_VARIANTS = 16
WK_AUG_MAX_LEN = 16384


class WkConfig(C.Structure):
    _fields_ = [("mode", C.c_int32), ("precision", C.c_int32), ("esp_dsp_packing", C.c_int32),
                ("device", C.c_int32), ("cmvn", C.c_int32)]


class WkCtcConfig(C.Structure):
    _fields_ = [("vocab", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32), ("n_mels", C.c_int32),
                ("device", C.c_int32), ("precision", C.c_int32)]


class WkAdamW(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float)]


class WkCtcAdam(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("max_norm", C.c_float)]


class WkCtcDropout(C.Structure):
    _fields_ = [("p_enc", C.c_float), ("p_gru", C.c_float), ("seed", C.c_uint64), ("offset", C.c_uint64)]


class WkAugVariant(C.Structure):
    _fields_ = [("speed", C.c_float), ("volume", C.c_float)]


class WkAugSpec(C.Structure):
    _fields_ = [("pad_noise", C.c_float), ("snr_noise", C.c_float), ("snr_lo_db", C.c_float), ("snr_hi_db", C.c_float),
                ("seed", C.c_uint64), ("epoch", C.c_uint32)]


class WkQuantSpec(C.Structure):
    _fields_ = [("e_in", C.c_int32), ("e_w", C.c_int32 * 5), ("e_act", C.c_int32 * 6)]


class WkCalibStats(C.Structure):
    _fields_ = [("n_clips", C.c_int64), ("counts", (C.c_int64 * WK_QUANT_BINS) * WK_QUANT_TENSORS),
                ("max_abs", C.c_float * WK_QUANT_TENSORS)]


class WkWavInfo(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("bits_per_sample", C.c_int32),
                ("data_samples", C.c_int32), ("n_samples", C.c_int32)]


class WakewordError(RuntimeError):
    pass


_lock = threading.Lock()
_lib = None


def _declare(L):
    vp, i32, i64, u32, fp = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.POINTER(C.c_float)
    L.wk_create.argtypes = [C.POINTER(WkConfig), vp, C.POINTER(vp)]
    L.wk_destroy.argtypes = [vp]
    L.wk_mfcc.argtypes = [vp, vp, i32, i64, i32, i64, vp, vp]
    L.wk_cnn.argtypes = [vp, vp, i64, vp, vp]
    L.wk_forward.argtypes = [vp, vp, i32, i64, i32, i64, vp, vp, vp]
    L.wk_synth_clips.argtypes = [u32, i64, i64, i32, vp, vp]
    L.wk_normalize.argtypes = [vp, vp, i64, i32, i32, i32, vp]
    L.wk_status_string.argtypes = [i32]
    L.wk_status_string.restype = C.c_char_p
    L.wk_last_error.restype = C.c_char_p
    L.wk_abi_version.restype = i32
    L.extract_mfcc.argtypes = [fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.extract_mfcc.restype = fp
    L.free_mfcc.argtypes = [fp]
    L.analyze_mfcc_range.argtypes = [fp, C.c_int, C.c_char_p]
    L.flow_extract_mfcc_single_frame.argtypes = [fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.flow_extract_mfcc_single_frame.restype = fp
    L.wk_stream_create.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
    L.wk_stream_destroy.argtypes = [vp]
    L.wk_stream_reset.argtypes = [vp]
    L.wk_stream_push.argtypes = [vp, fp, i64, fp, C.POINTER(i64), i32, C.POINTER(i32)]
    L.wk_ctc_num_weights.argtypes = [C.POINTER(WkCtcConfig)]
    L.wk_ctc_num_weights.restype = i64
    L.wk_ctc_create.argtypes = [C.POINTER(WkCtcConfig), vp, C.POINTER(vp)]
    L.wk_ctc_destroy.argtypes = [vp]
    L.wk_ctc_features.argtypes = [vp, vp, i64, i32, i32, i64, vp, vp]
    L.wk_ctc_forward.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp]
    L.wk_ctc_transcribe.argtypes = [vp, vp, i64, i32, i32, i64, vp, vp, vp]
    L.wk_ctc_frame_argmax.argtypes = [vp, i64, i32, vp, vp]
    L.wk_record_front.argtypes = [vp, i64, vp, vp, vp]
    L.wk_quantize_frames.argtypes = [vp, i64, vp, vp]
    L.wk_ctc_profile.argtypes = [vp, i32]
    L.wk_ctc_stage_times.argtypes = [vp, vp, vp]
    L.wk_wav_read.argtypes = [C.c_char_p, vp, i32, C.POINTER(WkWavInfo)]
    L.wk_wav_load_batch.argtypes = [C.POINTER(C.c_char_p), i32, i32, C.c_float, u32, vp, vp]
    L.wk_augment.argtypes = [vp, i32, C.c_float, C.c_float, C.c_float, u32, vp, i32]
    L.wk_device_cmvn.argtypes = [vp, i32, i64, vp, vp, vp]
    L.wk_check_device_errors.argtypes = [vp, C.POINTER(u32)]
    if hasattr(L, "wk_scan"):   # (absent from older libraries loaded for A/B timing)
        L.wk_scan_workspace_bytes.argtypes = [i64, i64, i32, i64, C.POINTER(C.c_size_t)]
        L.wk_scan.argtypes = [vp, vp, i32, i64, i64, i64, i32, vp, vp, vp, C.c_size_t, vp]
    if hasattr(L, "wk_esp_mfcc_create"):   # (absent from pre-round-4 libraries loaded for A/B timing)
        L.wk_esp_mfcc_create.argtypes = [i32, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
        L.wk_esp_mfcc_run.argtypes = [vp, vp, i64, i32, i64, i32, C.c_float, vp, vp]
        L.wk_esp_mfcc_destroy.argtypes = [vp]
    if hasattr(L, "wk_trainer_create"):   # (absent from older libraries loaded for A/B timing)
        L.wk_trainer_create.argtypes = [i32, vp, C.POINTER(vp)]
        L.wk_trainer_destroy.argtypes = [vp]
        L.wk_trainer_grad.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp]
        L.wk_trainer_step.argtypes = [vp, C.POINTER(WkAdamW), vp, vp]
        L.wk_trainer_weights.argtypes = [vp, vp, vp]
    if hasattr(L, "wk_calibrate"):   # (absent from older libraries loaded for A/B timing)
        L.wk_quant_spec_default.argtypes = [C.POINTER(WkQuantSpec)]
        L.wk_set_quant.argtypes = [vp, C.POINTER(WkQuantSpec)]
        L.wk_get_quant.argtypes = [vp, C.POINTER(WkQuantSpec)]
        L.wk_quant_weights.argtypes = [vp, C.POINTER(WkQuantSpec), vp]
        L.wk_calibrate_workspace_bytes.argtypes = [i64, C.POINTER(C.c_size_t)]
        L.wk_calibrate.argtypes = [vp, vp, i64, C.c_double, i32, vp, C.c_size_t, C.POINTER(WkQuantSpec),
                                   C.POINTER(WkCalibStats), vp]
    if hasattr(L, "wk_ctc_loss"):   # (absent from older libraries loaded for A/B timing)
        L.wk_ctc_loss_workspace_bytes.argtypes = [i64, i32, i32]
        L.wk_ctc_loss_workspace_bytes.restype = i64
        L.wk_ctc_loss.argtypes = [vp, i64, i32, i32, vp, i32, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp, vp, i32, vp]
        L.wk_ctc_loss.restype = i32
    if hasattr(L, "wk_ctc_backward"):
        L.wk_ctc_forward_train.argtypes = [vp, vp, i64, i32, vp, vp]
        L.wk_ctc_forward_train.restype = i32
        L.wk_ctc_backward.argtypes = [vp, i64, i32, vp, vp, vp, vp]
        L.wk_ctc_backward.restype = i32
    if hasattr(L, "wk_ctc_adam_step"):
        L.wk_ctc_weights.argtypes = [vp, vp, vp]
        L.wk_ctc_set_weights.argtypes = [vp, vp, vp]
        L.wk_ctc_adam_step.argtypes = [vp, C.POINTER(WkCtcAdam), vp, vp, vp]
        L.wk_ctc_optim_state.argtypes = [vp, vp, vp, C.POINTER(i64), vp]
        L.wk_ctc_set_optim_state.argtypes = [vp, vp, vp, i64, vp]
        for name in ("wk_ctc_weights", "wk_ctc_set_weights", "wk_ctc_adam_step", "wk_ctc_optim_state",
                     "wk_ctc_set_optim_state"):
            getattr(L, name).restype = i32
    if hasattr(L, "wk_ctc_forward_train_dropout"):
        L.wk_ctc_forward_train_dropout.argtypes = [vp, vp, i64, i32, C.POINTER(WkCtcDropout), vp, vp]
        L.wk_ctc_forward_train_dropout.restype = i32
        L.wk_ctc_dropout_masks.argtypes = [vp, vp, vp, vp]
        L.wk_ctc_dropout_masks.restype = i32
    if hasattr(L, "wk_augment_batch"):   # (absent from older libraries loaded for A/B timing)
        L.wk_augment_batch.argtypes = [vp, i32, vp, i64, i32, i64, C.POINTER(WkAugVariant), i32, C.POINTER(WkAugSpec), i32,
                                       vp, vp]
        L.wk_augment_batch.restype = i32
    if hasattr(L, "wk_ctc_align"):   # (absent from older libraries loaded for A/B timing)
        L.wk_ctc_align_workspace_bytes.argtypes = [i64, i32, i32]
        L.wk_ctc_align_workspace_bytes.restype = i64
        L.wk_ctc_align.argtypes = [vp, i64, i32, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp]
        L.wk_ctc_align.restype = i32
    if hasattr(L, "wk_ctc_beam"):
        L.wk_ctc_beam_workspace_bytes.argtypes = [i64, i32, i32, i32]
        L.wk_ctc_beam_workspace_bytes.restype = i64
        L.wk_ctc_beam.argtypes = [vp, i64, i32, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]
        L.wk_ctc_beam.restype = i32
    if hasattr(L, "wk_ctc_spot"):
        L.wk_ctc_spot_workspace_bytes.argtypes = [i64, i32, i32, i32]
        L.wk_ctc_spot_workspace_bytes.restype = i64
        L.wk_ctc_spot.argtypes = [vp, i64, i32, i32, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, i32, vp]
        L.wk_ctc_spot.restype = i32
    if hasattr(L, "wk_ctc_cer"):
        L.wk_ctc_cer_workspace_bytes.argtypes = [i64, i32, i32, i32]
        L.wk_ctc_cer_workspace_bytes.restype = i64
        L.wk_ctc_cer.argtypes = [vp, vp, i64, i32, i32, vp, i32, vp, i32, i32, vp, vp, vp, vp, i32, vp]
        L.wk_ctc_cer.restype = i32
    if hasattr(L, "wk_ctc_transcribe_stats"):
        L.wk_ctc_transcribe_stats.argtypes = [vp, i64, i32, vp, vp, vp]
        L.wk_ctc_transcribe_stats.restype = i32
    for name in ("wk_create", "wk_destroy", "wk_mfcc", "wk_cnn", "wk_forward", "wk_synth_clips", "wk_normalize",
                 "wk_stream_create", "wk_stream_destroy", "wk_stream_reset", "wk_stream_push", "wk_ctc_create",
                 "wk_ctc_destroy", "wk_ctc_features", "wk_ctc_forward", "wk_wav_read", "wk_wav_load_batch",
                 "wk_augment", "wk_device_cmvn", "wk_ctc_frame_argmax", "wk_record_front",
                 "wk_quantize_frames", "wk_ctc_profile", "wk_ctc_stage_times", "wk_ctc_transcribe",
                 "wk_esp_mfcc_create", "wk_esp_mfcc_run", "wk_esp_mfcc_destroy", "wk_scan",
                 "wk_scan_workspace_bytes", "wk_trainer_create", "wk_trainer_destroy", "wk_trainer_grad",
                 "wk_trainer_step", "wk_trainer_weights", "wk_quant_spec_default", "wk_set_quant", "wk_get_quant",
                 "wk_quant_weights", "wk_calibrate_workspace_bytes", "wk_calibrate"):
        if hasattr(L, name):
            getattr(L, name).restype = i32


def lib():
    """Load libwakeword.so once (after torch, so both share one HIP runtime)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise WakewordError(
                    f"{LIB_PATH} not found: build it with `python -m wakeword.build` (no CPU fallback exists)")
            try:
                import torch  # noqa: F401  (load torch's libamdhip64 first)
            except ImportError:
                pass
            L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
            _declare(L)
            _lib = L
    return _lib


def check(status: int, what: str = "") -> None:
    if status != WK_OK:
        L = lib()
        raise WakewordError(f"{what}: {L.wk_status_string(status).decode()} ({L.wk_last_error().decode()})")
