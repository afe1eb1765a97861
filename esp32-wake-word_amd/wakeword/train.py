"""Training step of LightweightKWS on MI355X -- mirrors ml_models/main.py:13-64.

``train_model`` there builds ``LightweightKWS(num_classes=1)``, a
``BCEWithLogitsLoss`` and ``AdamW(lr=5e-4, betas=(0.9, 0.99), weight_decay=1e-3,
eps=1e-7)`` and loops over batches.  ``Trainer`` is that step on the device:
forward, loss, backward to the five weight tensors and the AdamW update are HIP
kernels of libwakeword.so (wk_trainer_*); torch is the device-memory container
and, for ``state_dict=None``, the source of the default initial weights.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .api import STATE_KEYS, KWSModel, _as_device, _stream, _torch, mfcc, pack_weights

SHAPES = {"conv_layers.0.weight": (32, 13, 3), "conv_layers.3.weight": (64, 32, 3),
          "conv_layers.6.weight": (128, 64, 3), "classifier.0.weight": (64, 128), "classifier.2.weight": (1, 64)}


def default_init(seed: int = 0) -> Dict[str, np.ndarray]:
    """torch's default Conv1d / Linear weight init (kaiming_uniform_ with
    a = sqrt(5), i.e. U(-1/sqrt(fan_in), 1/sqrt(fan_in))) from a seeded CPU
    generator, in STATE_KEYS order."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for k in STATE_KEYS:
        shape = SHAPES[k]
        bound = 1.0 / math.sqrt(int(np.prod(shape[1:])))
        sd[k] = ((torch.rand(shape, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound).numpy()
    return sd


def _split(blob) -> Dict[str, object]:
    out, off = {}, 0
    for k in STATE_KEYS:
        n = int(np.prod(SHAPES[k]))
        out[k] = blob[off:off + n].reshape(SHAPES[k])
        off += n
    return out


class Trainer:
    """LightweightKWS(num_classes=1) + BCEWithLogitsLoss + AdamW on one device.

    One trainer's calls go on one stream (it owns its gradient workspace)."""

    def __init__(self, state_dict: Optional[Dict[str, np.ndarray]] = None, device: int = 0, seed: int = 0,
                 lr: float = 5e-4, betas: Tuple[float, float] = (0.9, 0.99), eps: float = 1e-7,
                 weight_decay: float = 1e-3):
        self.device = device
        self.opt = _lib.WkAdamW(lr, betas[0], betas[1], eps, weight_decay)
        sd = default_init(seed) if state_dict is None else state_dict
        blob = pack_weights({k: np.asarray(sd[k], np.float32) for k in STATE_KEYS})
        h = C.c_void_p()
        check(lib().wk_trainer_create(device, blob.ctypes.data_as(C.c_void_p), C.byref(h)), "wk_trainer_create")
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().wk_trainer_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _inputs(self, feats, labels):
        torch = _torch()
        dev = f"cuda:{self.device}"
        x = _as_device(feats, torch.float32, dev)
        if x.dim() != 3 or tuple(x.shape[1:]) != (13, 63):
            raise ValueError(f"expected (B, 13, 63) features, got {tuple(x.shape)}")
        y = _as_device(labels, torch.float32, dev).reshape(-1)
        if y.numel() != x.shape[0]:
            raise ValueError(f"{y.numel()} labels for {x.shape[0]} clips")
        return torch, x, y

    def _grad(self, feats, labels, want_grads: bool):
        torch, x, y = self._inputs(feats, labels)
        B = x.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        logits = torch.empty((B,), dtype=torch.float32, device=x.device)
        grads = torch.empty((_lib.WK_NUM_WEIGHTS,), dtype=torch.float32, device=x.device) if want_grads else None
        check(lib().wk_trainer_grad(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), B,
                                    C.c_void_p(loss.data_ptr()), C.c_void_p(logits.data_ptr()),
                                    C.c_void_p(grads.data_ptr()) if want_grads else None,
                                    _stream(torch, x.device)), "wk_trainer_grad")
        return loss, logits, grads

    def grad(self, feats, labels):
        """(B, 13, 63) features, (B,) 0/1 labels -> (mean BCE-with-logits loss,
        logits (B,), {state-dict key: gradient}), torch tensors on the device."""
        loss, logits, grads = self._grad(feats, labels, True)
        return loss, logits, _split(grads)

    def apply(self, grads=None):
        """One AdamW step with the last gradients, or with `grads` (a flat
        WK_NUM_WEIGHTS tensor in blob order, e.g. averaged over ranks)."""
        torch = _torch()
        dev = torch.device(f"cuda:{self.device}")
        g = None
        if grads is not None:
            g = _as_device(grads, torch.float32, dev).reshape(-1)
            if g.numel() != _lib.WK_NUM_WEIGHTS:
                raise ValueError(f"expected {_lib.WK_NUM_WEIGHTS} gradients, got {g.numel()}")
        check(lib().wk_trainer_step(self._h, C.byref(self.opt), C.c_void_p(g.data_ptr()) if g is not None else None,
                                    _stream(torch, dev)), "wk_trainer_step")

    def step(self, feats, labels):
        """Forward, backward and one AdamW update; returns the loss (before the
        update) as a 0-d device tensor."""
        loss, _, _ = self._grad(feats, labels, False)
        self.apply()
        return loss

    def step_audio(self, audio, labels):
        """(B, 16000) audio -> mode-B front-end (MFCC + CMVN, extract_mfcc.py:137-175) -> step."""
        return self.step(mfcc(audio, mode="torchaudio", cmvn=True, device=self.device), labels)

    def step_augmented(self, audio, lengths, labels, epoch: int = 0, **augment_kwargs):
        """(n, L) raw clips with their `lengths` (None = L) and (n,) labels ->
        ``wakeword.augment.extract_features`` (pad, the K variants, optional SNR
        noise, MFCC + CMVN; `augment_kwargs` are its is_noise, add_noise_to_pad,
        augment_audio and seed) -> step on the n*K rows, clip i's label repeated
        for its K variants.  A new `epoch` draws the noise afresh."""
        from .augment import extract_features
        torch = _torch()
        feats, _ = extract_features(audio, lengths, epoch=epoch, device=self.device, **augment_kwargs)
        y = _as_device(labels, torch.float32, feats.device).reshape(-1)
        if y.numel() == 0 or feats.shape[0] % y.numel():
            raise ValueError(f"{y.numel()} labels for {feats.shape[0]} augmented rows")
        return self.step(feats, y.repeat_interleave(feats.shape[0] // y.numel()))

    def weights(self):
        """Current weights as one flat device tensor in blob order."""
        torch = _torch()
        dev = torch.device(f"cuda:{self.device}")
        out = torch.empty((_lib.WK_NUM_WEIGHTS,), dtype=torch.float32, device=dev)
        check(lib().wk_trainer_weights(self._h, C.c_void_p(out.data_ptr()), _stream(torch, dev)), "wk_trainer_weights")
        return out

    def state_dict(self) -> Dict[str, np.ndarray]:
        blob = self.weights().cpu().numpy()
        return {k: v.copy() for k, v in _split(blob).items()}

    def to_model(self, precision: str = "fp32", calib=None, percentile: float = 99.9,
                 pin_input_exp: Optional[int] = -4) -> KWSModel:
        """A KWSModel of the current weights.  precision 'int8' with `calib`
        ((B, 13, 63) features): the int8 network at exponents calibrated on
        them (wakeword.quant.calibrate); without, at xiaoa.info's."""
        sd = self.state_dict()
        if calib is None:
            return KWSModel(sd, device=self.device, precision=precision)
        if precision != "int8":
            raise ValueError("calib applies to precision='int8' only")
        from .quant import calibrate
        spec = calibrate(sd, calib, percentile=percentile, pin_input_exp=pin_input_exp, device=self.device)
        return KWSModel(sd, device=self.device, precision="int8", quant=spec)


def train_model(train_loader: Iterable, test_loader: Iterable, num_epochs: int, learning_rate: float = 0.001,
                device: int = 0):
    """ml_models/main.py:13-64 on the device: per epoch, one ``Trainer.step`` per
    ``(feature, label)`` batch of `train_loader`, then accuracy over
    `test_loader` through ``KWSModel.forward`` with ``sigmoid > 0.5``.

    Returns ``(losses, accuracies, model)``: the mean training loss and the test
    accuracy (percent) of every epoch, and a ``KWSModel`` of the final weights.
    Like the reference, `learning_rate` is ignored: its optimizer is built with
    lr=5e-4 (main.py:16-22), and so is this one."""
    trainer = Trainer(device=device)
    losses, accuracies = [], []
    model = trainer.to_model()
    for _ in range(num_epochs):
        total, n = None, 0
        for feature, label in train_loader:
            loss = trainer.step(feature, label)
            total = loss if total is None else total + loss
            n += 1
        losses.append(float(total) / n if n else 0.0)
        model = trainer.to_model()
        correct, seen = 0, 0
        for feature, label in test_loader:
            torch = _torch()
            pred = (torch.sigmoid(model.forward(feature).reshape(-1)) > 0.5).float()
            lab = _as_device(label, torch.float32, pred.device).reshape(-1)
            correct += int((pred == lab).sum())
            seen += lab.numel()
        accuracies.append(100.0 * correct / seen if seen else 0.0)
    return losses, accuracies, model
