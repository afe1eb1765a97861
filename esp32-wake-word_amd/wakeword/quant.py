"""Post-training int8 quantisation of LightweightKWS -- mirrors ml_models/main.py:71-129.

``quantize_model_esp`` there trains, hands the float model and 32 batches of
20 training clips to esp-ppq (``espdl_quantize_torch``: percentile calibration,
power-of-2 scales), exports the int8 model and reports the "Executor accuracy"
of the quantised network.  esp-ppq is third-party and absent; its arithmetic
for this network is: a per-tensor exponent for the input, the five weights
and six activations (``QuantSpec``), ``sat8(rne(w * 2^-e))`` weights, and the
int8 network ``KWSModel(precision="int8")`` runs.  ``calibrate`` finds the
exponents on the device (wk_calibrate: one fp32 forward with power-of-2
histograms), ``quantize_model`` is the reference's workflow around it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Iterable, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .api import STATE_KEYS, KWSModel, _as_device, _stream, _torch, pack_weights
from .train import SHAPES

# xiaoa.info's tensor order: the input, then per layer its weight and its output
_WEIGHT_NAMES = STATE_KEYS
_ACT_NAMES = ("conv_layers.0 (ReLU, MaxPool)", "conv_layers.3 (ReLU, MaxPool)", "conv_layers.6 (ReLU, MaxPool)",
              "global_avg_pool", "classifier.0 (ReLU)", "classifier.2 (output)")


@dataclass(frozen=True)
class QuantSpec:
    """Power-of-2 exponents of the int8 network (wk_quant_spec): a tensor holds
    q * 2^e.  e_w in state-dict order; e_act = conv1, conv2, conv3 outputs (a
    pool output shares its conv's exponent), GAP, classifier.0 output, logit."""
    e_in: int
    e_w: Tuple[int, int, int, int, int]
    e_act: Tuple[int, int, int, int, int, int]

    @staticmethod
    def default() -> "QuantSpec":
        """ml_models/xiaoa.info's exponents (wk_quant_spec_default)."""
        c = _lib.WkQuantSpec()
        check(lib().wk_quant_spec_default(C.byref(c)), "wk_quant_spec_default")
        return QuantSpec._from_c(c)

    @staticmethod
    def _from_c(c) -> "QuantSpec":
        return QuantSpec(int(c.e_in), tuple(int(v) for v in c.e_w), tuple(int(v) for v in c.e_act))

    def _to_c(self):
        if len(self.e_w) != 5 or len(self.e_act) != 6:
            raise ValueError("QuantSpec needs 5 weight and 6 activation exponents")
        return _lib.WkQuantSpec(int(self.e_in), (C.c_int32 * 5)(*map(int, self.e_w)), (C.c_int32 * 6)(*map(int, self.e_act)))

    @staticmethod
    def from_dict(d) -> "QuantSpec":
        return QuantSpec(int(d["e_in"]), tuple(int(v) for v in d["e_w"]), tuple(int(v) for v in d["e_act"]))

    def to_dict(self) -> Dict[str, object]:
        return {"e_in": self.e_in, "e_w": list(self.e_w), "e_act": list(self.e_act)}

    def shifts(self) -> Tuple[int, int, int, int, int]:
        """Requantisation shifts e_out - e_x - e_w of conv1..3, classifier.0, classifier.2."""
        e_x = (self.e_in, self.e_act[0], self.e_act[1], self.e_act[3], self.e_act[4])
        e_out = (self.e_act[0], self.e_act[1], self.e_act[2], self.e_act[4], self.e_act[5])
        return tuple(o - x - w for o, x, w in zip(e_out, e_x, self.e_w))

    def summary(self) -> str:
        """One line per tensor, in xiaoa.info's order."""
        rows = [("input", self.e_in)]
        for i in range(5):
            rows.append((_WEIGHT_NAMES[i], self.e_w[i]))
            rows.append((_ACT_NAMES[i if i < 3 else i + 1], self.e_act[i if i < 3 else i + 1]))
            if i == 2:
                rows.append((_ACT_NAMES[3], self.e_act[3]))
        return "\n".join(f"{name:<34s} exponent {e:+d}" for name, e in rows)


def _state_dict_of(model_or_state_dict) -> Dict[str, np.ndarray]:
    sd = model_or_state_dict.state_dict() if hasattr(model_or_state_dict, "state_dict") else model_or_state_dict
    return {k: np.ascontiguousarray(np.asarray(sd[k], np.float32)) for k in STATE_KEYS}


def calibrate(model_or_state_dict, feats, percentile: float = 99.9, pin_input_exp: Optional[int] = -4,
              return_stats: bool = False, device: Optional[int] = None):
    """Exponents for `model_or_state_dict` (a KWSModel of any precision, a
    Trainer, or a state dict) from calibration features (B, 13, 63), numpy or
    torch: wk_calibrate on the device.  pin_input_exp = -4 keeps the input at
    the firmware's x16 (main.py:92-93 feeds normalize_mfcc(...) * 16); None
    calibrates it.  With return_stats also the histograms: a dict of ``counts``
    (7, 32) int64 (bins = exponents -24 .. 7), ``max_abs`` (7,) and ``n_clips``."""
    torch = _torch()
    if isinstance(model_or_state_dict, KWSModel):
        model = model_or_state_dict
    else:
        dev = getattr(model_or_state_dict, "device", 0) if device is None else device
        model = KWSModel(_state_dict_of(model_or_state_dict), device=dev)
    x = _as_device(feats, torch.float32, f"cuda:{model.device}")
    if x.dim() != 3 or tuple(x.shape[1:]) != (13, 63) or x.shape[0] < 1:
        raise ValueError(f"expected (B >= 1, 13, 63) features, got {tuple(x.shape)}")
    nbytes = C.c_size_t(0)
    check(lib().wk_calibrate_workspace_bytes(x.shape[0], C.byref(nbytes)), "wk_calibrate_workspace_bytes")
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=x.device)
    spec, stats = _lib.WkQuantSpec(), _lib.WkCalibStats()
    pin = _lib.WK_QUANT_CALIBRATE_INPUT if pin_input_exp is None else int(pin_input_exp)
    check(lib().wk_calibrate(model._h.h, C.c_void_p(x.data_ptr()), x.shape[0], float(percentile), pin,
                             C.c_void_p(ws.data_ptr()), nbytes.value, C.byref(spec), C.byref(stats),
                             _stream(torch, x.device)), "wk_calibrate")
    q = QuantSpec._from_c(spec)
    if not return_stats:
        return q
    return q, {"counts": np.array([list(r) for r in stats.counts], np.int64),
               "max_abs": np.array(list(stats.max_abs), np.float32), "n_clips": int(stats.n_clips)}


def int8_blob(state_dict, spec: QuantSpec) -> np.ndarray:
    """The int8 export of the weights at spec.e_w (wk_quant_weights): one int8
    array in the library's logical layouts, conv [k][ci][co], matmul [in][out]."""
    blob = pack_weights(_state_dict_of(state_dict))
    out = np.empty((_lib.WK_NUM_INT8_WEIGHTS,), np.int8)
    c = spec._to_c()
    check(lib().wk_quant_weights(blob.ctypes.data_as(C.c_void_p), C.byref(c), out.ctypes.data_as(C.c_void_p)),
          "wk_quant_weights")
    return out


def int8_weights(state_dict, spec: QuantSpec) -> Dict[str, np.ndarray]:
    """sat8(rne(w * 2^-e_w)) per tensor, int8 arrays in the state dict's shapes."""
    blob, out, off = int8_blob(state_dict, spec), {}, 0
    for k in STATE_KEYS:
        shape = SHAPES[k]
        n = int(np.prod(shape))
        a = blob[off:off + n]
        off += n
        if len(shape) == 3:     # [k][ci][co] -> (co, ci, k)
            out[k] = np.ascontiguousarray(a.reshape(3, shape[1], shape[0]).transpose(2, 1, 0))
        else:                   # [in][out] -> (out, in)
            out[k] = np.ascontiguousarray(a.reshape(shape[1], shape[0]).T)
    return out


def quantize_model(model, calib_loader: Iterable, calib_steps: int = 32, percentile: float = 99.9,
                   pin_input_exp: Optional[int] = -4):
    """main.py:71-129's quantisation step: take `calib_steps` batches of
    features from `calib_loader` (a batch is the features, or a tuple whose
    first item is: the reference's collate_fn drops the label), calibrate on
    them, and return ``(int8_model, spec)``."""
    torch = _torch()
    dev = f"cuda:{model.device}"
    batches = []
    for i, batch in enumerate(calib_loader):
        if i >= calib_steps:
            break
        x = batch[0] if isinstance(batch, (tuple, list)) else batch
        batches.append(_as_device(x, torch.float32, dev).reshape(-1, 13, 63))
    if not batches:
        raise ValueError("quantize_model: the calibration loader gave no batch")
    spec = calibrate(model, torch.cat(batches), percentile=percentile, pin_input_exp=pin_input_exp)
    return KWSModel(model.state_dict(), device=model.device, precision="int8", quant=spec), spec


def accuracy(model, loader: Iterable) -> float:
    """Percent of clips with (sigmoid(logit) > 0.5) == label over a loader of
    (features, labels) batches -- main.py:101-127's count, for the float model
    ("Test Accuracy") and the int8 one ("Executor Accuracy") alike."""
    torch = _torch()
    correct, seen = 0, 0
    for feature, label in loader:
        pred = (torch.sigmoid(model.forward(feature).reshape(-1)) > 0.5).float()
        lab = _as_device(label, torch.float32, pred.device).reshape(-1)
        correct += int((pred == lab).sum())
        seen += lab.numel()
    return 100.0 * correct / seen if seen else 0.0
