"""Training of the GRU-CTC head on MI355X -- mirrors the loop of
ml_models/ctc.py:366-447 (THCHS30Trainer.train).

The reference builds ``nn.CTCLoss(blank=0)`` and ``optim.Adam(lr=1e-3)``
(ctc.py:368-369) and per batch runs forward, loss, backward,
``clip_grad_norm_(parameters, 5.0)`` and ``optimizer.step()`` (ctc.py:390-402).
``CTCTrainer`` is that step on the device: the training forward, the CTC loss
with its gradient, BPTT, the clip and Adam are HIP kernels of libwakeword.so
working on one ``wk_ctc`` handle, whose weights the step updates in place, so
the same handle validates (``val_loss``) and decodes with the new weights.
Dropout is off by default (the function trained is then the eval-mode one);
``dropout=0.2`` applies the reference's two train-mode dropouts (ctc.py:131,
:140) as masks drawn from ``(seed, step)``, so a run is reproducible and
resumable from ``rng_state()``.

    trainer = wakeword.CTCTrainer(model_or_state_dict_or_blob, vocab=V)
    loss = trainer.step(feats, labels, feat_lengths, label_lengths)   # 0-d device tensor, no host sync
    model16 = trainer.to_model("fp16")                                 # the trained weights on the fp16 inference path
    trainer, train_losses, val_losses, best = wakeword.train_ctc(train_loader, val_loader, vocab=V)
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Mapping, Optional, Tuple

import numpy as np

from .ctc import CTCModel, _as_f32, dropout_pair, error_rate, pack_state_dict, unpack_grads


def check_hyper(lr, betas, eps, weight_decay, max_norm) -> None:
    """wk_ctc_adam_step's argument rules, raised as ValueError before any device work."""
    def num(x):
        return isinstance(x, (int, float)) and not isinstance(x, bool)
    if not num(lr) or not math.isfinite(lr) or lr < 0:
        raise ValueError(f"lr must be finite and >= 0, got {lr!r}")
    if len(betas) != 2 or not all(num(b) and 0.0 <= b < 1.0 for b in betas):
        raise ValueError(f"betas must be two values in [0, 1), got {betas!r}")
    if not num(eps) or not eps > 0:
        raise ValueError(f"eps must be > 0, got {eps!r}")
    if not num(weight_decay) or not weight_decay >= 0:
        raise ValueError(f"weight_decay must be >= 0, got {weight_decay!r}")
    if not num(max_norm) or math.isnan(max_norm):
        raise ValueError(f"max_norm must be a number (<= 0 turns the clip off), got {max_norm!r}")


class CTCTrainer:
    """GRU_CTC_Model + nn.CTCLoss(blank=0) + clip_grad_norm_ + optim.Adam on
    one device.  Owns an fp32 CTCModel built from a copy of `weights` (a flat
    blob, a state dict or a GRU_CTC_Model, none of which it changes).  One
    trainer's calls go on one stream."""

    def __init__(self, weights, vocab: int, device: int = 0, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.0, max_norm: float = 5.0, zero_infinity: bool = False,
                 idx_to_char: Optional[Mapping[int, str]] = None, dropout=0.0, seed: int = 0):
        check_hyper(lr, betas, eps, weight_decay, max_norm)
        self.dropout = dropout_pair(dropout)     # (p_enc, p_gru); the reference trains at 0.2 (ctc.py:34)
        self.load_rng_state(seed, 0)
        self.hyper = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                          weight_decay=float(weight_decay), max_norm=float(max_norm))
        self.vocab, self.device, self.zero_infinity = vocab, device, bool(zero_infinity)
        self.idx_to_char = dict(idx_to_char) if idx_to_char is not None else None
        if hasattr(weights, "state_dict") and callable(weights.state_dict):
            weights = weights.state_dict()
        if isinstance(weights, Mapping):
            weights = pack_state_dict(weights, vocab)
        blob = np.array(_as_f32(weights).reshape(-1), np.float32, copy=True)
        self.model = CTCModel(blob, vocab, device=device, precision="fp32", idx_to_char=idx_to_char)
        self._last = None        # (flat gradient, norm) of the last grad()

    def grad(self, feats, targets, input_lengths, target_lengths):
        """(B, T, 80) features, nn.CTCLoss's targets and lengths -> (mean CTC
        loss, the flat gradient in the blob's order, its 2-norm), on the
        device; kept for apply().  With dropout, the k-th call (from 0) draws
        its masks at offset k under the trainer's seed."""
        on = any(p > 0.0 for p in self.dropout)
        loss, flat, norm = self.model._loss_and_flat_grad(feats, targets, input_lengths, target_lengths, "mean",
                                                          self.zero_infinity, self.dropout if on else None, self._seed,
                                                          self._offset)
        self._offset += 1
        self._last = (flat, norm)
        return loss, flat, norm

    def apply(self, grads=None, norm=None) -> None:
        """The clip and one Adam step with the last grad()'s gradient and
        norm, or with `grads` (flat, blob order: e.g. averaged over ranks) and
        its `norm` (computed on the device when None)."""
        if grads is None:
            if self._last is None:
                raise ValueError("no gradients: call grad() first or pass them")
            grads, norm = self._last
        self.model.adam_step(grads, norm, **self.hyper)

    def step(self, feats, targets, input_lengths, target_lengths):
        """Forward, loss, backward, clip and Adam (ctc.py:390-402); returns the
        loss before the update as a 0-d device tensor.  No host sync."""
        loss, _, _ = self.grad(feats, targets, input_lengths, target_lengths)
        self.apply()
        return loss

    def rng_state(self) -> Tuple[int, int]:
        """(seed, offset): the dropout masks' seed and the number of grad() calls so far."""
        return self._seed, self._offset

    def load_rng_state(self, seed: int, offset: int) -> None:
        if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(offset) < 2 ** 63:
            raise ValueError(f"seed must lie in [0, 2^64) and offset in [0, 2^63), got {seed!r}, {offset!r}")
        self._seed, self._offset = int(seed), int(offset)

    def val_loss(self, feats, targets, input_lengths, target_lengths):
        """The validation loss of ctc.py:409-425 at the current weights: eval mode, no dropout."""
        return self.model.loss(feats, targets, input_lengths, target_lengths)

    def val_cer(self, feats, targets, input_lengths, target_lengths):
        """The edit totals of the greedy transcripts at the current weights
        (CTCModel.cer, the first input_lengths[b] frames of each utterance):
        EditStats.totals' row 0 as an (8,) int64 device tensor -- sum d, sum s,
        sum del, sum ins, sum M, sum N, utterances with d > 0, B -- so an epoch
        adds its batches' rows and reads back once (error_rate of the sum)."""
        return self.model.cer(feats, targets, target_lengths, input_lengths=input_lengths).totals[0]

    def weights(self):
        return self.model.weights()

    def state_dict(self) -> Dict[str, np.ndarray]:
        return self.model.state_dict()

    def optim_state(self):
        """(m, v, step): Adam's moments (flat device tensors) and step count."""
        return self.model.optim_state()

    def load_optim_state(self, m, v, step: int) -> None:
        self.model.set_optim_state(m, v, step)

    def to_model(self, precision: str = "fp32") -> CTCModel:
        """A fresh CTCModel of the current weights ('fp16': the inference path's fp16 GEMMs)."""
        return CTCModel(self.weights().cpu().numpy(), self.vocab, device=self.device, precision=precision,
                        idx_to_char=self.idx_to_char)


def train_ctc(train_loader: Iterable, val_loader: Iterable, vocab: int, num_epochs: int = 30, patience: int = 5,
              trainer=None, weights=None, history=None, **hyper):
    """THCHS30Trainer.train's loop (ctc.py:374-447) without the download, the
    file save and the plot.  Batches are (features, labels, feature_lengths,
    label_lengths), as collate_fn yields them.  Per epoch: one trainer.step
    per training batch, trainer.val_loss per validation batch; the state dict
    of the best mean validation loss is kept, and the loop stops after
    `patience` epochs without improvement (ctc.py:427-438).

    `trainer`: a CTCTrainer (or an object with step, val_loss and state_dict);
    built from `weights` -- default: torch's initialisation at seed 0 -- and
    **hyper when None.  **hyper are CTCTrainer's keywords; among them
    `dropout` (default 0: off; the reference trains at 0.2, ctc.py:34) and the
    masks' `seed`.  `history`: a dict; the loop then also measures each epoch's
    corpus character error rate on the validation set (trainer.val_cer per
    batch, summed on the device, error_rate of the sum) and appends it to
    history["val_cer"].  Model selection stays on the validation loss either
    way.  Returns (trainer, train_losses, val_losses, best_state_dict)."""
    if trainer is None:
        if weights is None:
            from .ctc import random_state_dict
            weights = random_state_dict(vocab, out_scale=1.0)
        trainer = CTCTrainer(weights, vocab, **hyper)
    elif hyper or weights is not None:
        raise ValueError("pass either a trainer or the arguments to build one")

    def mean(losses):      # (summed on the device: one read-back per epoch)
        total = None
        for x in losses:
            total = x if total is None else total + x
        return float(total) / len(losses) if losses else 0.0

    train_losses, val_losses = [], []
    best, best_sd, stale = float("inf"), None, 0
    for _ in range(num_epochs):
        train_losses.append(mean([trainer.step(*batch) for batch in train_loader]))
        val_losses.append(mean([trainer.val_loss(*batch) for batch in val_loader]))
        if history is not None:
            totals = None      # (summed on the device: one read-back per epoch)
            for batch in val_loader:
                row = trainer.val_cer(*batch)
                totals = row if totals is None else totals + row
            history.setdefault("val_cer", []).append(error_rate(totals) if totals is not None else float("nan"))
        if val_losses[-1] < best:
            best, best_sd, stale = val_losses[-1], trainer.state_dict(), 0
        else:
            stale += 1
            if stale >= patience:
                break
    return trainer, train_losses, val_losses, best_sd
