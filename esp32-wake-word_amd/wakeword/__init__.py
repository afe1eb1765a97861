"""wakeword -- MI355X-native wake-word inference (MFCC front-end + xiaoa CNN).

Drop-in for the reference's Python surface (ml_models/src/wakeModel.py,
ml_models/src/extract_mfcc.py, the xiaoa.onnx artefact); every compute call
runs a hand-written gfx950 HIP kernel from libwakeword.so.
"""
from ._lib import WakewordError, lib  # noqa: F401
from .api import (EspMfcc, KWSModel, detect, extract_mfcc, load_onnx, load_wav, mfcc, normalize_mfcc, pack_weights,  # noqa: F401
                  pad_audio, synth_clips)
from .onnx_reader import read_onnx, xiaoa_state_dict  # noqa: F401
from .stream import (DecisionRule, DeviceDetector, FrameDecisionLoop, FrameWindow, StreamingDetector,  # noqa: F401
                     Window, device_cmvn, quantize_frames, record_front)
from .scan import ScanPlan, events_from_logits, plan, scan_events  # noqa: F401
from .ctc import (Alignment, BeamResult, CTCLoss, CTCModel, Detection, EditStats, KeywordSpotter, Spot, beam_texts,  # noqa: F401
                  ctc_align, ctc_beam_search, ctc_loss, ctc_spot, ctc_state_dict_spec, decode_predictions, edit_distance,
                  error_rate, keyword_tokens, pack_state_dict, pad_targets, span_seconds, tokens_to_text, unpack_grads)
from .ctc_train import CTCTrainer, train_ctc  # noqa: F401
from .train import Trainer, train_model  # noqa: F401
from .quant import QuantSpec, accuracy, calibrate, int8_weights, quantize_model  # noqa: F401
from .augment import REFERENCE_VARIANTS, augment_batch, extract_features  # noqa: F401
from . import wav  # noqa: F401

LightweightKWS = KWSModel
