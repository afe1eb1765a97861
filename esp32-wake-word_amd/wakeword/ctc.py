"""GRU-CTC head: the reference's ml_models/ctc.py
inference surface on the HIP path (wk_ctc_* in the C ABI).

    model = wakeword.CTCModel(state_dict_or_flat_weights, vocab=V, idx_to_char=None)
    feats = model.features(audio, n_samples=48000)      # ctc.py:82-107, (B, T, 80)
    tokens, log_probs = model.forward(feats, return_log_probs=True)   # ctc.py:148-152 + 453-471
    tokens = model.transcribe(audio)                     # both
    texts = model.decode_predictions(log_probs)          # ctc.py:453-471 (idx_to_char map)
    texts = model.transcribe_text(audio)                 # device decode, then the map
    loss = wakeword.ctc_loss(log_probs, targets, input_lengths, target_lengths)   # nn.CTCLoss(blank=0), ctc.py:369
    loss = model.loss(feats, targets, input_lengths, target_lengths)              # validation loss, ctc.py:409-425
    al = wakeword.ctc_align(log_probs, targets, input_lengths, target_lengths)    # forced alignment: Alignment(states, tokens, ...)
    al = model.align(feats, targets, target_lengths); model.align_audio(audio, targets, target_lengths); span_seconds(al.spans)
    res = wakeword.ctc_beam_search(log_probs, beam=16, top_k=16, n_best=4)        # prefix beam search: BeamResult(tokens, lengths, scores)
    res = model.beam_decode(feats, beam=16); model.beam_decode_audio(audio, beam=16); beam_texts(res, idx_to_char)
    tokens = model.transcribe(audio, beam=16)            # the best hypothesis of the beam instead of the greedy path
    sp = wakeword.ctc_spot(log_probs, keywords, keyword_lengths)                  # keyword spotting: Spot(scores, spans, frame_scores)
    sp = model.spot(feats, keywords); model.spot_audio(audio, keywords); KeywordSpotter(model, char_to_idx, words).detect(audio)
    st = wakeword.edit_distance(tokens, lengths, targets, target_lengths)         # EditStats(distance, substitutions, deletions, ...)
    st = model.cer(feats, targets, target_lengths, beam=16, n_best=4); error_rate(st); error_rate(st, oracle=True)
    loss, grads, norm = model.loss_and_grad(feats, targets, input_lengths, target_lengths)   # ctc.py:393-401, fp32
    lp = model.forward_train(feats); flat = model.backward(dlogits); grads = unpack_grads(flat, V)   # its pieces
    model.adam_step(grads, norm)                         # clip_grad_norm_(5.0) + Adam(lr=1e-3) in place, ctc.py:401-402
    flat = model.weights(); model.set_weights(blob_or_state_dict)   # the weights after creation (wakeword.CTCTrainer: the loop)

A state dict is bound BY NAME: its keys must be exactly GRU_CTC_Model's
(ctc_state_dict_spec(), ctc.py:119-146: audio_encoder.{0,1}, gru.*_l{k}[_reverse],
output_layer) with the module's shapes; any order is accepted, missing, extra
or mis-shaped entries raise ValueError.  A flat blob must already be in that
order (wk_ctc_create's layout, include/wakeword.h).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import check, lib

MAX_AUDIO_SAMPLES = 8 * 16000   # Config.max_audio_length (ctc.py:29)
BLANK = 0                       # ctc.py:458 (prev_token = 0 = blank_idx)


def ctc_state_dict_spec(vocab: int, hidden: int = 128, layers: int = 2, n_mels: int = 80) -> List[Tuple[str, tuple]]:
    """(key, shape) of GRU_CTC_Model's state dict in registration order
    (ctc.py:119-146: audio_encoder = Sequential(Linear, LayerNorm, ReLU,
    Dropout), nn.GRU(bidirectional, num_layers=layers), output_layer) -- the
    order wk_ctc_create's flat blob concatenates."""
    spec = [("audio_encoder.0.weight", (hidden, n_mels)), ("audio_encoder.0.bias", (hidden,)),
            ("audio_encoder.1.weight", (hidden,)), ("audio_encoder.1.bias", (hidden,))]
    for k in range(layers):
        d_in = hidden if k == 0 else 2 * hidden
        for sfx in ("", "_reverse"):
            spec += [(f"gru.weight_ih_l{k}{sfx}", (3 * hidden, d_in)), (f"gru.weight_hh_l{k}{sfx}", (3 * hidden, hidden)),
                     (f"gru.bias_ih_l{k}{sfx}", (3 * hidden,)), (f"gru.bias_hh_l{k}{sfx}", (3 * hidden,))]
    spec += [("output_layer.weight", (vocab, 2 * hidden)), ("output_layer.bias", (vocab,))]
    return spec


def random_state_dict(vocab: int, seed: int = 0, hidden: int = 128, layers: int = 2, n_mels: int = 80,
                      out_scale: float = 4.0) -> Dict[str, np.ndarray]:
    """Seeded random GRU_CTC_Model weights (the reference ships no trained CTC
    weights; ctc.py:119-146).  torch's default initialisers, drawn in the
    module's registration order after torch.manual_seed(seed) -- nn.Linear,
    nn.LayerNorm, nn.GRU(bidirectional), nn.Linear -- so a torch model built
    the same way holds the same values.  out_scale multiplies the output
    layer's weight: 4 gives the greedy path decision margins (a default init is
    near-uniform over V)."""
    import torch
    from torch import nn
    gen_state = torch.random.get_rng_state()
    try:
        torch.manual_seed(seed)
        enc = nn.Linear(n_mels, hidden)
        ln = nn.LayerNorm(hidden)
        gru = nn.GRU(input_size=hidden, hidden_size=hidden, num_layers=layers, batch_first=True,
                     dropout=0.2 if layers > 1 else 0.0, bidirectional=True)
        out = nn.Linear(2 * hidden, vocab)
    finally:
        torch.random.set_rng_state(gen_state)
    sd = {"audio_encoder.0.weight": enc.weight, "audio_encoder.0.bias": enc.bias,
          "audio_encoder.1.weight": ln.weight, "audio_encoder.1.bias": ln.bias}
    sd.update({f"gru.{k}": v for k, v in gru.state_dict().items()})
    sd["output_layer.weight"] = out.weight * out_scale
    sd["output_layer.bias"] = out.bias
    return {k: v.detach().numpy().astype(np.float32) for k, v in sd.items()}


def _as_f32(v) -> np.ndarray:
    if hasattr(v, "detach"):          # torch tensor (any device)
        v = v.detach().cpu().numpy()
    return np.asarray(v, np.float32)


def pack_state_dict(sd: Mapping[str, object], vocab: int, hidden: int = 128, layers: int = 2,
                    n_mels: int = 80) -> np.ndarray:
    """Bind a GRU_CTC_Model state dict by name into wk_ctc_create's blob.
    Raises ValueError naming every missing, unexpected or mis-shaped key."""
    spec = ctc_state_dict_spec(vocab, hidden, layers, n_mels)
    want = dict(spec)
    missing = [k for k, _ in spec if k not in sd]
    extra = [k for k in sd if k not in want]
    if missing or extra:
        raise ValueError(f"GRU_CTC_Model state dict mismatch: missing {missing}, unexpected {extra}")
    parts = []
    for k, shape in spec:
        a = _as_f32(sd[k])
        if tuple(a.shape) != shape:
            raise ValueError(f"{k}: expected shape {shape}, got {tuple(a.shape)}")
        parts.append(a.reshape(-1))
    return np.concatenate(parts)


def unpack_grads(flat, vocab: int, hidden: int = 128, layers: int = 2, n_mels: int = 80) -> dict:
    """{state-dict key: view of `flat`} for a flat tensor or array in the
    weight blob's layout (CTCModel.backward's gradient, or the blob itself),
    each view in its parameter's shape."""
    spec = ctc_state_dict_spec(vocab, hidden, layers, n_mels)
    need = sum(int(np.prod(shape)) for _, shape in spec)
    if flat.ndim != 1 or flat.shape[0] != need:
        raise ValueError(f"expected a flat vector of {need} values for vocab={vocab}, got shape {tuple(flat.shape)}")
    out, off = {}, 0
    for k, shape in spec:
        n = int(np.prod(shape))
        out[k] = flat[off:off + n].reshape(shape)
        off += n
    return out


def tokens_to_text(seqs: Sequence[Sequence[int]], idx_to_char: Mapping[int, str]) -> List[str]:
    """decode_predictions' last step (ctc.py:468): ids -> characters, unknown
    ids as "<unk>", joined."""
    return ["".join(idx_to_char.get(int(i), "<unk>") for i in seq) for seq in seqs]


def greedy_tokens(log_probs) -> List[List[int]]:
    """ctc.py:454-466: first argmax per frame, blank (0) dropped, repeats
    collapsed with prev_token updated on every frame (blanks included)."""
    import torch
    pred = torch.as_tensor(log_probs).argmax(dim=-1).cpu().numpy()
    if pred.ndim == 1:
        pred = pred[None]
    seqs = []
    for row in pred:
        keep = (row != BLANK) & (row != np.concatenate([[BLANK], row[:-1]]))
        seqs.append(row[keep].tolist())
    return seqs


def decode_predictions(log_probs, idx_to_char: Mapping[int, str]) -> List[str]:
    """THCHS30Trainer.decode_predictions (ctc.py:453-471) on (B, T, V)
    log-probs (host-side; the batched device decode is CTCModel.decode)."""
    return tokens_to_text(greedy_tokens(log_probs), idx_to_char)


MAX_LABEL_LEN = 255             # wk_ctc_loss: 2 S + 1 <= 511 states, 8 registers per lane


def pad_targets(targets, target_lengths):
    """nn.CTCLoss's two target forms as one padded (B, max(S_max, 1)) int32
    tensor: 2-D (B, S) targets as they are (on their device, no sync); 1-D
    concatenated targets split by target_lengths and zero-padded, on the host
    (lengths on the device are read back)."""
    import torch
    t = torch.as_tensor(targets)
    if t.dim() == 2:
        return t.to(torch.int32) if t.shape[1] > 0 else torch.zeros((t.shape[0], 1), dtype=torch.int32, device=t.device)
    if t.dim() != 1:
        raise ValueError(f"targets must be (B, S) or 1-D concatenated, got {tuple(t.shape)}")
    lens = [int(n) for n in torch.as_tensor(target_lengths).reshape(-1).tolist()]
    if min(lens, default=0) < 0 or sum(lens) != t.numel():
        raise ValueError(f"target_lengths sum to {sum(lens)}, targets hold {t.numel()}")
    t = t.cpu().to(torch.int32)
    out = torch.zeros((len(lens), max(max(lens, default=0), 1)), dtype=torch.int32)
    off = 0
    for b, n in enumerate(lens):
        out[b, :n] = t[off:off + n]
        off += n
    return out


def _check_log_probs(log_probs) -> None:
    import torch
    if not (torch.is_tensor(log_probs) and log_probs.is_cuda and log_probs.dtype == torch.float32 and log_probs.dim() == 3):
        raise ValueError("log_probs must be a 3-D float32 tensor on the HIP device")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream_ptr(device):
    """The current stream of `device` as the C ABI takes it."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _workspace(nbytes: int, device, unsupported: str):
    """A wk_*_workspace_bytes result as a device buffer (the caching
    allocator's: no device malloc per call); 0 bytes means the shape is beyond
    the kernels' limits: WakewordError(unsupported)."""
    import torch
    if nbytes <= 0:
        raise _lib.WakewordError(unsupported)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _lengths(x, device):
    """Lengths as a tensor or sequence -> a flat contiguous int32 tensor on `device`."""
    import torch
    return torch.as_tensor(x).reshape(-1).to(device=device, dtype=torch.int32).contiguous()


def _label_args(lp, targets, input_lengths, target_lengths):
    """ctc_loss's label arguments for (B, T, V) log-probs lp -> (labels, in_len,
    lab_len, max_label_len), the tensors wk_ctc_loss and wk_ctc_align read, on
    lp's device."""
    B = lp.shape[0]
    labels = pad_targets(targets, target_lengths).to(lp.device).contiguous()
    in_len, lab_len = _lengths(input_lengths, lp.device), _lengths(target_lengths, lp.device)
    if labels.shape[0] != B or in_len.numel() != B or lab_len.numel() != B:
        raise ValueError(f"batch of {B}: targets {tuple(labels.shape)}, {in_len.numel()} input and {lab_len.numel()} target lengths")
    max_label_len = labels.shape[1]
    if max_label_len > MAX_LABEL_LEN:      # padding wider than the kernels' limit: the longest label decides (a host sync)
        max_label_len = int(lab_len.max())
    return labels, in_len, lab_len, max_label_len


def _wk_ctc_loss(lp, labels, in_len, lab_len, max_label_len, reduction: str, zero_infinity, want_grad: bool, unsupported: str):
    """One wk_ctc_loss call on the current stream -> (nll (B,), loss (1,), the
    gradient at the logits or None)."""
    import torch
    B, T, V = lp.shape
    L = lib()
    ws = _workspace(L.wk_ctc_loss_workspace_bytes(B, T, max_label_len), lp.device, unsupported)
    nll = torch.empty(B, dtype=torch.float32, device=lp.device)
    loss = torch.empty(1, dtype=torch.float32, device=lp.device)
    grad = torch.empty_like(lp) if want_grad else None
    check(L.wk_ctc_loss(_ptr(lp), B, T, V, _ptr(labels), labels.shape[1], _ptr(in_len), _ptr(lab_len), max_label_len,
                        _lib.WK_CTC_REDUCTION[reduction], int(zero_infinity), 1.0, _ptr(ws), _ptr(nll), _ptr(loss), _ptr(grad),
                        lp.device.index, _stream_ptr(lp.device)), "wk_ctc_loss")
    return nll, loss, grad


_loss_fn = None


def _ctc_loss_fn():
    """The autograd function behind ctc_loss (built on first use: torch is
    imported lazily throughout this package)."""
    global _loss_fn
    if _loss_fn is not None:
        return _loss_fn
    import torch

    class CTCLossFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, lp, labels, in_len, lab_len, max_label_len, reduction, zero_infinity):
            B, T, _ = lp.shape
            nll, loss, grad = _wk_ctc_loss(lp, labels, in_len, lab_len, max_label_len, reduction, zero_infinity,
                                           ctx.needs_input_grad[0],
                                           f"wk_ctc_loss: unsupported shape (B={B}, T={T}, max label length {max_label_len} "
                                           f"> {MAX_LABEL_LEN}?)")
            ctx.per_utterance = reduction == "none"
            ctx.save_for_backward(grad)
            return nll if reduction == "none" else loss.reshape(())

        @staticmethod
        def backward(ctx, grad_output):
            (grad,) = ctx.saved_tensors
            if ctx.per_utterance:
                grad_output = grad_output.reshape(-1, 1, 1)
            return grad * grad_output, None, None, None, None, None, None

    _loss_fn = CTCLossFn
    return _loss_fn


def ctc_loss(log_probs, targets, input_lengths, target_lengths, reduction: str = "mean", zero_infinity: bool = False,
             batch_first: bool = False):
    """F.ctc_loss(..., blank=0) on the HIP device (wk_ctc_loss; ctc.py:369,
    :394, :416): log_probs (T, B, V) float32 as the reference passes them, or
    (B, T, V) with batch_first=True -- what CTCModel.decode returns and what
    the kernels read, so that form is used without a copy; targets (B, S)
    padded or 1-D concatenated; lengths as tensors or sequences.  Runs on the
    current stream.  When log_probs requires grad the gradient is computed in
    this call (torch's native convention, exact through log_softmax's backward)
    and backward() only scales it by grad_output (per utterance for
    reduction="none")."""
    if reduction not in _lib.WK_CTC_REDUCTION:
        raise ValueError(f"reduction must be 'none', 'sum' or 'mean', got {reduction!r}")
    _check_log_probs(log_probs)
    lp = (log_probs if batch_first else log_probs.transpose(0, 1)).contiguous()
    labels, in_len, lab_len, max_label_len = _label_args(lp, targets, input_lengths, target_lengths)
    return _ctc_loss_fn().apply(lp, labels, in_len, lab_len, max_label_len, reduction, bool(zero_infinity))


class CTCLoss:
    """nn.CTCLoss(blank=0)'s call form over ctc_loss (stateless: no parameters)."""

    def __init__(self, reduction: str = "mean", zero_infinity: bool = False, batch_first: bool = False):
        if reduction not in _lib.WK_CTC_REDUCTION:
            raise ValueError(f"reduction must be 'none', 'sum' or 'mean', got {reduction!r}")
        self.reduction, self.zero_infinity, self.batch_first = reduction, zero_infinity, batch_first

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        return ctc_loss(log_probs, targets, input_lengths, target_lengths, self.reduction, self.zero_infinity,
                        self.batch_first)

    __call__ = forward


class Alignment(NamedTuple):
    """ctc_align's result, device tensors: states (B, T) int32, the lattice
    state per frame (0..2S, -1 past the input length or without an alignment);
    tokens (B, T) int32, its label (0 = blank, -1 as states); frame_log_probs
    (B, T) float32, that label's log-prob (0 where the state is -1); spans
    (B, S_max, 2) int32, label i's frames [start, end) (-1 for i >= S or
    without an alignment); scores (B,) float32, the path's log-probability
    (-inf without an alignment)."""
    states: object
    tokens: object
    frame_log_probs: object
    spans: object
    scores: object


def _align_args(log_probs, targets, input_lengths, target_lengths, batch_first: bool):
    """ctc_align's arguments as ctc_loss takes them -> (lp (B, T, V), labels,
    in_len, lab_len, max_label_len), the tensors wk_ctc_align reads, on
    log_probs' device."""
    lp = (log_probs if batch_first else log_probs.transpose(0, 1)).detach().contiguous()
    return (lp, *_label_args(lp, targets, input_lengths, target_lengths))


def ctc_align(log_probs, targets, input_lengths, target_lengths, batch_first: bool = False) -> Alignment:
    """CTC forced alignment on the HIP device (wk_ctc_align): the best path of
    each utterance's known transcript through its log-probs, blank = 0 --
    which frames every label occupies.  Arguments as ctc_loss: log_probs
    (T, B, V) float32, or (B, T, V) with batch_first=True (used without a
    copy); targets (B, S) padded or 1-D concatenated; lengths as tensors or
    sequences.  Runs on the current stream, no host sync; the result is
    defined bit for bit by the recurrence and tie rule in include/wakeword.h.
    span_seconds converts the spans to time."""
    import torch
    _check_log_probs(log_probs)
    lp, labels, in_len, lab_len, max_label_len = _align_args(log_probs, targets, input_lengths, target_lengths, batch_first)
    B, T, V = lp.shape
    L, dev, ptr = lib(), lp.device, _ptr
    ws = _workspace(L.wk_ctc_align_workspace_bytes(B, T, max_label_len), dev,
                    f"wk_ctc_align: unsupported shape (B={B}, T={T}, max label length {max_label_len} > {MAX_LABEL_LEN}?)")
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    tokens = torch.empty((B, T), dtype=torch.int32, device=dev)
    frame_lp = torch.empty((B, T), dtype=torch.float32, device=dev)
    spans = torch.empty((B, max_label_len, 2), dtype=torch.int32, device=dev)
    scores = torch.empty((B,), dtype=torch.float32, device=dev)
    check(L.wk_ctc_align(ptr(lp), B, T, V, ptr(labels), labels.shape[1], ptr(in_len), ptr(lab_len), max_label_len, ptr(ws),
                         ptr(states), ptr(tokens), ptr(frame_lp), ptr(spans), ptr(scores), dev.index, _stream_ptr(dev)),
          "wk_ctc_align")
    return Alignment(states, tokens, frame_lp, spans, scores)


def span_seconds(spans, hop: int = 160, sample_rate: int = 16000):
    """Alignment.spans in seconds: frame t of the centred STFT sits on sample
    t * hop, so label i covers [start * hop / sample_rate, end * hop /
    sample_rate) -- 10 ms per frame at the defaults.  float64, a tensor for a
    tensor and an array otherwise; rows without an alignment stay -1."""
    if hasattr(spans, "detach"):
        import torch
        return torch.where(spans < 0, -1.0, spans.to(torch.float64) * hop / sample_rate)
    s = np.asarray(spans)
    return np.where(s < 0, -1.0, s.astype(np.float64) * hop / sample_rate)


MAX_BEAM = 64                   # wk_ctc_beam: one lane per beam slot
MAX_TOP_K = 32                  # ... and one register per extension


class BeamResult(NamedTuple):
    """ctc_beam_search's result, device tensors, hypotheses in descending
    order of score: tokens (B, n_best, max_len) int32, -1 beyond each length;
    lengths (B, n_best) int32, the full length (it may exceed max_len; -1 for
    a slot without a hypothesis); scores (B, n_best) float32, the log of the
    summed probability of the hypothesis's paths the beam kept (-inf for an
    empty slot); candidates (B, T, top_k) int32 if asked for, the per-frame
    candidate tokens in descending log-prob (-1 past the input length)."""
    tokens: object
    lengths: object
    scores: object
    candidates: object = None


def _beam_args(log_probs, input_lengths, beam, top_k, n_best, max_len, batch_first: bool):
    """ctc_beam_search's arguments -> (lp (B, T, V), in_len or None, max_len),
    what wk_ctc_beam reads, on log_probs' device; ValueError for what the
    kernels do not take."""
    for name, v, lo, hi in (("beam", beam, 1, MAX_BEAM), ("top_k", top_k, 1, MAX_TOP_K), ("n_best", n_best, 1, beam)):
        if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
    lp = (log_probs if batch_first else log_probs.transpose(0, 1)).detach().contiguous()
    B, T, V = lp.shape
    if B < 1 or T < 1 or V < 2:
        raise ValueError(f"log_probs (B, T, V) = {(B, T, V)}: B and T must be positive and V at least 2")
    if max_len is None:
        max_len = T
    if not isinstance(max_len, int) or isinstance(max_len, bool) or max_len < 1:
        raise ValueError(f"max_len must be a positive integer, got {max_len!r}")
    in_len = None
    if input_lengths is not None:
        in_len = _lengths(input_lengths, lp.device)
        if in_len.numel() != B:
            raise ValueError(f"batch of {B}: {in_len.numel()} input lengths")
    return lp, in_len, max_len


def ctc_beam_search(log_probs, input_lengths=None, beam: int = 16, top_k: int = 16, n_best: int = 1,
                    max_len: Optional[int] = None, batch_first: bool = False, return_candidates: bool = False) -> BeamResult:
    """CTC prefix beam search on the HIP device (wk_ctc_beam): the n_best label
    sequences of each utterance with the largest summed path probability, as
    a beam of `beam` prefixes extended by the `top_k` most probable tokens of
    each frame finds them (the algorithm is stated in include/wakeword.h).
    log_probs (T, B, V) float32, or (B, T, V) with batch_first=True (used
    without a copy); input_lengths as a tensor or sequence, all T when None;
    max_len, the width of the token rows, defaults to T.  Runs on the current
    stream, no host sync."""
    import torch
    _check_log_probs(log_probs)
    lp, in_len, max_len = _beam_args(log_probs, input_lengths, beam, top_k, n_best, max_len, batch_first)
    B, T, V = lp.shape
    L, dev, ptr = lib(), lp.device, _ptr
    ws = _workspace(L.wk_ctc_beam_workspace_bytes(B, T, beam, top_k), dev,
                    f"wk_ctc_beam: unsupported shape (B={B}, T={T}, beam={beam}, top_k={top_k})")
    tokens = torch.empty((B, n_best, max_len), dtype=torch.int32, device=dev)
    lengths = torch.empty((B, n_best), dtype=torch.int32, device=dev)
    scores = torch.empty((B, n_best), dtype=torch.float32, device=dev)
    cand = torch.empty((B, T, top_k), dtype=torch.int32, device=dev) if return_candidates else None
    check(L.wk_ctc_beam(ptr(lp), B, T, V, ptr(in_len), beam, top_k, n_best, max_len, ptr(ws), ptr(tokens), ptr(lengths),
                        ptr(scores), ptr(cand), dev.index, _stream_ptr(dev)), "wk_ctc_beam")
    return BeamResult(tokens, lengths, scores, cand)


def beam_texts(result: BeamResult, idx_to_char: Mapping[int, str]) -> List[List[str]]:
    """A BeamResult as text: per utterance the strings of its hypotheses in
    order (tokens_to_text's mapping); slots without a hypothesis are left out,
    a hypothesis longer than the token rows is cut there."""
    tok, ln = result.tokens, result.lengths
    tok = tok.cpu().numpy() if hasattr(tok, "cpu") else np.asarray(tok)
    ln = ln.cpu().numpy() if hasattr(ln, "cpu") else np.asarray(ln)
    return [tokens_to_text([tok[b, i, :min(int(ln[b, i]), tok.shape[2])].tolist() for i in range(tok.shape[1]) if ln[b, i] >= 0],
                           idx_to_char) for b in range(tok.shape[0])]


MAX_KEYWORD_LEN = 32            # wk_ctc_spot: 2S-1 states, one lane each


class Spot(NamedTuple):
    """ctc_spot's result, device tensors: scores (B, K) float32, the best score
    of keyword k over all segments of utterance b (-inf without an occurrence;
    with normalize a log-ratio <= 0 whose exp is the confidence); spans
    (B, K, 2) int32, that segment's frames [start, end) (-1, -1 without);
    frame_scores (B, K, T) float32 if asked for, the best score of a segment
    ending at each frame (-inf past the input length), else None."""
    scores: object
    spans: object
    frame_scores: object = None


class Detection(NamedTuple):
    """One keyword found by KeywordSpotter.detect: the utterance's index in the
    batch, the keyword as given, exp(score) and the span in seconds."""
    utterance: int
    keyword: str
    confidence: float
    start_s: float
    end_s: float


def keyword_tokens(words: Sequence[str], char_to_idx: Mapping[str, int]) -> Tuple[np.ndarray, np.ndarray]:
    """Words -> (padded (K, S_max) int32 array, (K,) int32 lengths), one label
    per character.  KeyError for a character the map does not hold, ValueError
    for an empty word or one longer than 32."""
    if isinstance(words, str):
        words = [words]
    rows = []
    for w in words:
        if not 1 <= len(w) <= MAX_KEYWORD_LEN:
            raise ValueError(f"keyword {w!r}: length must be in [1, {MAX_KEYWORD_LEN}]")
        rows.append([int(char_to_idx[c]) for c in w])
    if not rows:
        raise ValueError("no keywords")
    out = np.zeros((len(rows), max(len(r) for r in rows)), dtype=np.int32)
    for k, r in enumerate(rows):
        out[k, :len(r)] = r
    return out, np.array([len(r) for r in rows], dtype=np.int32)


def _spot_args(log_probs, keywords, keyword_lengths, input_lengths, batch_first: bool):
    """ctc_spot's arguments -> (lp (B, T, V), keywords (K, stride) int32,
    lengths (K,) int32, in_len or None, max_keyword_len), what wk_ctc_spot
    reads, on log_probs' device; ValueError for what the kernels do not take."""
    import torch
    lp = (log_probs if batch_first else log_probs.transpose(0, 1)).detach().contiguous()
    B, T, V = lp.shape
    if B < 1 or T < 1 or V < 2:
        raise ValueError(f"log_probs (B, T, V) = {(B, T, V)}: B and T must be positive and V at least 2")
    if isinstance(keywords, (list, tuple)) and keywords and isinstance(keywords[0], (list, tuple)):     # a list of int lists
        if keyword_lengths is None:
            keyword_lengths = [len(w) for w in keywords]
        width = max(max(len(w) for w in keywords), 1)
        keywords = [list(w) + [0] * (width - len(w)) for w in keywords]
    kw = torch.as_tensor(np.asarray(keywords) if not torch.is_tensor(keywords) else keywords)
    if kw.dim() != 2 or kw.shape[0] < 1 or kw.shape[1] < 1:
        raise ValueError(f"keywords must be a non-empty (K, S) array or a list of label lists, got {tuple(kw.shape)}")
    kw = kw.to(device=lp.device, dtype=torch.int32).contiguous()
    K = kw.shape[0]
    if keyword_lengths is None:
        keyword_lengths = [kw.shape[1]] * K
    kl = _lengths(keyword_lengths, lp.device)
    if kl.numel() != K:
        raise ValueError(f"{K} keywords: {kl.numel()} keyword lengths")
    max_len = kw.shape[1]
    if max_len > MAX_KEYWORD_LEN:          # padding wider than the kernel's limit: the longest keyword decides (a host sync)
        max_len = max(int(kl.max()), 1)
        if max_len > MAX_KEYWORD_LEN:
            raise ValueError(f"a keyword of {max_len} labels: at most {MAX_KEYWORD_LEN}")
    in_len = None
    if input_lengths is not None:
        in_len = _lengths(input_lengths, lp.device)
        if in_len.numel() != B:
            raise ValueError(f"batch of {B}: {in_len.numel()} input lengths")
    return lp, kw, kl, in_len, max_len


def ctc_spot(log_probs, keywords, keyword_lengths=None, input_lengths=None, normalize: bool = True,
             frame_scores: bool = False, batch_first: bool = False) -> Spot:
    """CTC keyword spotting on the HIP device (wk_ctc_spot): for every
    (utterance, keyword) pair the best score of the keyword's label sequence
    over all segments of the utterance, and that segment.  log_probs (T, B, V)
    float32, or (B, T, V) with batch_first=True (used without a copy);
    keywords a padded (K, S) tensor or array with keyword_lengths (all S when
    None), or a list of label lists; input_lengths as a tensor or sequence,
    all T when None.  With normalize (the default) each frame's log-probs are
    taken relative to the frame's maximum, so the score is <= 0, exactly 0
    where the greedy path spells the keyword, and exp(score) is a confidence
    in (0, 1]; without it the score is the segment's path log-probability.
    frame_scores=True also returns the (B, K, T) per-frame trace.  Runs on the
    current stream, no host sync; the result is defined bit for bit by the
    recurrence and tie rule in include/wakeword.h.  span_seconds converts the
    spans to time."""
    import torch
    _check_log_probs(log_probs)
    lp, kw, kl, in_len, max_len = _spot_args(log_probs, keywords, keyword_lengths, input_lengths, batch_first)
    B, T, V = lp.shape
    K = kw.shape[0]
    L, dev, ptr = lib(), lp.device, _ptr
    ws = _workspace(L.wk_ctc_spot_workspace_bytes(B, T, K, max_len), dev,
                    f"wk_ctc_spot: unsupported shape (B={B}, T={T}, {K} keywords, max keyword length {max_len})")
    scores = torch.empty((B, K), dtype=torch.float32, device=dev)
    spans = torch.empty((B, K, 2), dtype=torch.int32, device=dev)
    trace = torch.empty((B, K, T), dtype=torch.float32, device=dev) if frame_scores else None
    check(L.wk_ctc_spot(ptr(lp), B, T, V, ptr(in_len), ptr(kw), kw.shape[1], ptr(kl), K, max_len, 1 if normalize else 0, ptr(ws),
                        ptr(scores), ptr(spans), ptr(trace), dev.index, _stream_ptr(dev)), "wk_ctc_spot")
    return Spot(scores, spans, trace)


class KeywordSpotter:
    """The reference's CTCKeywordDetector surface (ml_models/test.py:159-235)
    with a real confidence: where the reference greedy-decodes, tests for a
    substring and reports a constant 0.9, detect() scores every keyword over
    every segment of every utterance with CTCModel.spot_audio and reports
    exp(score) -- 1.0 where the greedy path spells the keyword, less where a
    competitor wins some frames -- with the segment's time.

        spotter = KeywordSpotter(model, char_to_idx, ["xiao", "a"], threshold=0.8)
        for d in spotter.detect(audio): d.utterance, d.keyword, d.confidence, d.start_s, d.end_s
    """

    def __init__(self, model, char_to_idx: Mapping[str, int], keywords: Sequence[str], threshold: float = 0.8,
                 hop: int = 160, sample_rate: int = 16000):
        self.model, self.keywords = model, [keywords] if isinstance(keywords, str) else list(keywords)
        self.tokens, self.lengths = keyword_tokens(self.keywords, char_to_idx)
        if not 0.0 <= threshold < 1.0:
            raise ValueError(f"threshold must be in [0, 1), got {threshold!r}")
        self.threshold, self.hop, self.sample_rate = float(threshold), hop, sample_rate

    def detections(self, spot: Spot) -> List[Detection]:
        """A Spot of this spotter's keywords -> the pairs with exp(score) >
        threshold, by utterance, then keyword."""
        conf = np.exp(spot.scores.cpu().numpy().astype(np.float64))
        sec = span_seconds(spot.spans.cpu().numpy(), self.hop, self.sample_rate)
        return [Detection(b, self.keywords[k], float(conf[b, k]), float(sec[b, k, 0]), float(sec[b, k, 1]))
                for b in range(conf.shape[0]) for k in range(conf.shape[1]) if conf[b, k] > self.threshold]

    def detect(self, audio, n_samples: int = MAX_AUDIO_SAMPLES) -> List[Detection]:
        return self.detections(self.model.spot_audio(audio, self.tokens, self.lengths, n_samples=n_samples))


MAX_REF_LEN = 1024              # wk_ctc_cer: 64 lanes x 16 reference columns
MAX_HYP_STRIDE = 32767          # ... d <= 32767 keeps d * 2^16 + s a positive int32
MAX_N_HYP = 64


class EditStats(NamedTuple):
    """edit_distance's result, device tensors.  distance, substitutions,
    deletions, insertions: int32, (B, n_hyp) -- (B,) for a 2-D hyp -- the
    Levenshtein distance d of each hypothesis to its utterance's reference, the
    fewest substitutions s among the alignments that reach d, and the del and
    ins that d = s + del + ins and ins - del = N - M then fix.  best (B,) int32:
    the hypothesis with the smallest (d, s, index), the oracle of an N-best
    list.  totals (2, 8) int64: row 0 over hypothesis 0 of every utterance, row
    1 over the oracle; columns sum d, sum s, sum del, sum ins, sum M (reference
    tokens), sum N (hypothesis tokens), utterances with d > 0, B."""
    distance: object
    substitutions: object
    deletions: object
    insertions: object
    best: object
    totals: object

    def error_rate(self, oracle: bool = False) -> float:
        return error_rate(self.totals, oracle)

    def sentence_error_rate(self, oracle: bool = False) -> float:
        """The share of utterances with d > 0 (one read-back)."""
        row = self.totals[1 if oracle else 0].tolist()
        return row[6] / row[7]


def _rate(errors: int, tokens: int) -> float:
    if tokens == 0:
        return float("nan") if errors == 0 else float("inf")
    return errors / tokens


def error_rate(totals, oracle: bool = False) -> float:
    """The corpus error rate sum d / sum M of a totals block ((2, 8), row 1 with
    oracle=True) or of one row ((8,), e.g. a sum of CTCTrainer.val_cer rows), as
    a float: one read-back.  nan when there are no reference tokens and no
    errors, inf when there are none but errors."""
    t = totals.totals if isinstance(totals, EditStats) else totals
    t = t.tolist() if hasattr(t, "tolist") else list(t)
    if t and isinstance(t[0], (list, tuple)):
        t = t[1 if oracle else 0]
    elif oracle:
        raise ValueError("oracle=True needs the (2, 8) totals, got one row")
    if len(t) != 8:
        raise ValueError(f"totals must be (2, 8) or (8,), got a row of {len(t)}")
    return _rate(int(t[0]), int(t[4]))


def _cer_args(hyp, hyp_lengths, ref, ref_lengths, collapse: bool):
    """edit_distance's arguments -> (hyp (B, n_hyp, stride) int32, hyp_len
    (B * n_hyp,) int32 or None, ref (B, ref_stride) int32, ref_len (B,) int32,
    max_ref_len), what wk_ctc_cer reads, on hyp's device; ValueError for what
    the kernel does not take."""
    import torch
    if not (torch.is_tensor(hyp) and hyp.dtype == torch.int32 and hyp.dim() in (2, 3)):
        raise ValueError("hyp must be a (B, N) or (B, n_hyp, N) int32 tensor")
    h = hyp.detach().unsqueeze(1) if hyp.dim() == 2 else hyp.detach()
    B, H, stride = h.shape
    if B < 1 or H < 1 or stride < 1:
        raise ValueError(f"hyp (B, n_hyp, N) = {(B, H, stride)}: every size must be positive")
    if H > MAX_N_HYP:
        raise ValueError(f"{H} hypotheses per utterance: at most {MAX_N_HYP}")
    if stride > MAX_HYP_STRIDE:
        raise ValueError(f"hypothesis rows of {stride}: at most {MAX_HYP_STRIDE}")
    if B * H > 2 ** 24 or B * H * stride > 2 ** 30:
        raise ValueError(f"hyp (B, n_hyp, N) = {(B, H, stride)}: B * n_hyp must be at most 2^24 and B * n_hyp * N at most 2^30")
    h = h.contiguous()
    hl = None
    if hyp_lengths is not None:
        hl = _lengths(hyp_lengths, h.device)
        if hl.numel() != B * H:
            raise ValueError(f"{B} x {H} hypotheses: {hl.numel()} hypothesis lengths")
    elif not collapse:
        raise ValueError("hyp_lengths is required unless collapse is set")
    r = torch.as_tensor(np.asarray(ref) if not torch.is_tensor(ref) else ref)
    if r.dim() != 2 or r.is_floating_point():
        raise ValueError(f"ref must be a (B, S) integer array, got {tuple(r.shape)} {r.dtype}")
    if r.shape[1] == 0:
        r = torch.zeros((r.shape[0], 1), dtype=torch.int32, device=r.device)
    r = r.to(device=h.device, dtype=torch.int32).contiguous()
    rl = _lengths(ref_lengths, h.device)
    if r.shape[0] != B or rl.numel() != B:
        raise ValueError(f"batch of {B}: ref {tuple(r.shape)}, {rl.numel()} reference lengths")
    max_ref_len = r.shape[1]
    if max_ref_len > MAX_REF_LEN:          # padding wider than the kernel's limit: the longest reference decides (a host sync)
        max_ref_len = max(int(rl.max()), 1)
        if max_ref_len > MAX_REF_LEN:
            raise ValueError(f"a reference of {max_ref_len} tokens: at most {MAX_REF_LEN}")
    return h, hl, r, rl, max_ref_len


def edit_distance(hyp, hyp_lengths, ref, ref_lengths, collapse: bool = False) -> EditStats:
    """Edit distance of hypotheses to references on the HIP device
    (wk_ctc_cer), with its split into substitutions, deletions and insertions,
    the oracle hypothesis per utterance and the corpus totals (error_rate turns
    them into a rate).  hyp: a (B, N) or (B, n_hyp, N) int32 device tensor,
    hypothesis h of utterance b against reference b -- CTCModel.decode's tokens
    and lengths, or ctc_beam_search's (a slot's -1 length is an empty
    hypothesis).  With collapse=True hyp holds per-frame labels
    (CTCModel.frame_argmax), the hypothesis is their greedy CTC collapse and
    hyp_lengths the frames per row, all N when None.  ref (B, S) padded, as a
    tensor or array, with ref_lengths.  Tokens are only compared for equality.
    Runs on the current stream, no host sync; every output is integer, defined
    bit for bit in include/wakeword.h."""
    import torch
    if not (torch.is_tensor(hyp) and hyp.is_cuda):
        raise ValueError("hyp must be an int32 tensor on the HIP device")
    squeeze = hyp.dim() == 2
    h, hl, r, rl, max_ref_len = _cer_args(hyp, hyp_lengths, ref, ref_lengths, collapse)
    B, H, stride = h.shape
    L, dev, ptr = lib(), h.device, _ptr
    ws = _workspace(L.wk_ctc_cer_workspace_bytes(B, H, stride, max_ref_len), dev,
                    f"wk_ctc_cer: unsupported shape (B={B}, n_hyp={H}, N={stride}, max reference length {max_ref_len})")
    stats = torch.empty((B, H, 4), dtype=torch.int32, device=dev)
    best = torch.empty((B,), dtype=torch.int32, device=dev)
    totals = torch.empty((2, 8), dtype=torch.int64, device=dev)
    check(L.wk_ctc_cer(ptr(h), ptr(hl), B, H, stride, ptr(r), r.shape[1], ptr(rl), max_ref_len, 1 if collapse else 0, ptr(ws),
                       ptr(stats), ptr(best), ptr(totals), dev.index, _stream_ptr(dev)), "wk_ctc_cer")
    cols = [stats[:, 0, k] if squeeze else stats[:, :, k] for k in range(4)]
    return EditStats(cols[0], cols[1], cols[2], cols[3], best, totals)


def dropout_pair(dropout) -> Tuple[float, float]:
    """`dropout` as (p_enc, p_gru): None is (0, 0), a float both sites, a pair
    itself.  wk_ctc_forward_train_dropout's rule, raised before any device
    work: each p in [0, 1)."""
    if dropout is None:
        return 0.0, 0.0
    pair = tuple(dropout) if isinstance(dropout, (tuple, list)) else (dropout, dropout)
    if len(pair) != 2 or not all(isinstance(p, (int, float)) and not isinstance(p, bool) and 0.0 <= p < 1.0 for p in pair):
        raise ValueError(f"dropout must be a probability in [0, 1) or a pair of them, got {dropout!r}")
    return float(pair[0]), float(pair[1])


class CTCModel:
    def __init__(self, weights: Union[np.ndarray, Mapping[str, np.ndarray]], vocab: int, device: int = 0,
                 precision: str = "fp32", idx_to_char: Optional[Mapping[int, str]] = None):
        if hasattr(weights, "state_dict") and callable(weights.state_dict):   # an nn.Module (GRU_CTC_Model)
            weights = weights.state_dict()
        if isinstance(weights, Mapping):
            weights = pack_state_dict(weights, vocab)
        if precision not in ("fp32", "fp16"):
            raise ValueError(f"precision must be 'fp32' or 'fp16', got {precision!r}")
        self.idx_to_char = dict(idx_to_char) if idx_to_char is not None else None
        w = np.ascontiguousarray(_as_f32(weights).reshape(-1))
        L = lib()
        self.cfg = _lib.WkCtcConfig(vocab, 128, 2, 80, device, {"fp32": 0, "fp16": 1}[precision])
        need = L.wk_ctc_num_weights(C.byref(self.cfg))
        if w.size != need:
            raise ValueError(f"expected {need} weights for vocab={vocab}, got {w.size}")
        self.vocab, self.device = vocab, device
        self._h = C.c_void_p()
        check(L.wk_ctc_create(C.byref(self.cfg), w.ctypes.data_as(C.c_void_p), C.byref(self._h)), "wk_ctc_create")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().wk_ctc_destroy(self._h)
        except Exception:
            pass

    def _stream(self, torch):
        return _stream_ptr(self.device)

    def features(self, audio, n_samples: int = MAX_AUDIO_SAMPLES):
        """(B, L) float waveform -> (B, T, 80) on device, T = 1 + n_samples // 160."""
        import torch
        x = torch.as_tensor(audio, dtype=torch.float32).to(f"cuda:{self.device}").contiguous()
        if x.dim() == 1:
            x = x.unsqueeze(0)
        B, L = x.shape
        T = 1 + n_samples // 160
        out = torch.empty((B, T, 80), dtype=torch.float32, device=x.device)
        check(lib().wk_ctc_features(self._h, C.c_void_p(x.data_ptr()), B, L, n_samples, L, C.c_void_p(out.data_ptr()),
                                    self._stream(torch)), "wk_ctc_features")
        return out

    def decode(self, feats, return_log_probs: bool = False):
        """(B, T, 80) -> device tensors, stream-ordered, no host sync: tokens
        (B, T) int32 (row b's first lengths[b] entries are its greedy CTC
        sequence, the rest -1), lengths (B,) int32, and (B, T, V) log-probs
        if asked (else None)."""
        import torch
        f = torch.as_tensor(feats, dtype=torch.float32).to(f"cuda:{self.device}").contiguous()
        B, T, _ = f.shape
        lp = torch.empty((B, T, self.vocab), dtype=torch.float32, device=f.device) if return_log_probs else None
        tok = torch.empty((B, T), dtype=torch.int32, device=f.device)
        ln = torch.empty((B,), dtype=torch.int32, device=f.device)
        check(lib().wk_ctc_forward(self._h, C.c_void_p(f.data_ptr()), B, T,
                                   C.c_void_p(lp.data_ptr()) if lp is not None else None, C.c_void_p(tok.data_ptr()),
                                   C.c_void_p(ln.data_ptr()), self._stream(torch)), "wk_ctc_forward")
        return tok, ln, lp

    def decode_audio(self, audio, n_samples: int = MAX_AUDIO_SAMPLES):
        """(B, L) float waveform -> (tokens (B, T) int32, lengths (B,) int32) on
        device, stream-ordered: wk_ctc_transcribe, i.e. features() then
        decode() in one call (fp16 mode: the z-score folded into the encoder)."""
        import torch
        x = torch.as_tensor(audio, dtype=torch.float32).to(f"cuda:{self.device}").contiguous()
        if x.dim() == 1:
            x = x.unsqueeze(0)
        B, L = x.shape
        T = 1 + n_samples // 160
        tok = torch.empty((B, T), dtype=torch.int32, device=x.device)
        ln = torch.empty((B,), dtype=torch.int32, device=x.device)
        check(lib().wk_ctc_transcribe(self._h, C.c_void_p(x.data_ptr()), B, L, n_samples, L, C.c_void_p(tok.data_ptr()),
                                      C.c_void_p(ln.data_ptr()), self._stream(torch)), "wk_ctc_transcribe")
        return tok, ln

    def frame_argmax(self, batch: int, T: int):
        """decode_predictions' per-frame `predictions` (ctc.py:454) of the last
        decode/forward on this model: (batch, T) int32 on device."""
        import torch
        out = torch.empty((batch, T), dtype=torch.int32, device=f"cuda:{self.device}")
        check(lib().wk_ctc_frame_argmax(self._h, batch, T, C.c_void_p(out.data_ptr()), self._stream(torch)),
              "wk_ctc_frame_argmax")
        return out

    def transcribe_stats(self, batch: int, T: int, return_raw: bool = False):
        """The z-score statistics of the last decode_audio on this model, when it
        took the fused path (fp16, T >= 6; else WakewordError): (batch, 2)
        float32 {mean, 1/std} per utterance on device, and with return_raw
        also the (batch, T, 80) un-normalised log-mel rows they are of."""
        import torch
        zs = torch.empty((batch, 2), dtype=torch.float32, device=f"cuda:{self.device}")
        raw = torch.empty((batch, T, 80), dtype=torch.float32, device=zs.device) if return_raw else None
        check(lib().wk_ctc_transcribe_stats(self._h, batch, T, _ptr(raw), _ptr(zs), self._stream(torch)),
              "wk_ctc_transcribe_stats")
        return (zs, raw) if return_raw else zs

    def forward(self, feats, return_log_probs: bool = False):
        """(B, T, 80) -> token id lists (greedy CTC, decode_predictions'
        output form), and (B, T, V) log-probs if asked."""
        tok, ln, lp = self.decode(feats, return_log_probs)
        tok, ln = tok.cpu().numpy(), ln.cpu().numpy()
        seqs = [tok[b, :ln[b]].tolist() for b in range(tok.shape[0])]
        return (seqs, lp) if return_log_probs else seqs

    def transcribe(self, audio, n_samples: int = MAX_AUDIO_SAMPLES, beam: Optional[int] = None) -> List[List[int]]:
        """audio -> token id lists (extract_features + model + decode_predictions);
        with beam=W the best hypothesis of beam_decode_audio instead of the
        greedy path."""
        if beam is not None:
            res = self.beam_decode_audio(audio, n_samples, beam=beam)
            tok, ln = res.tokens.cpu().numpy()[:, 0], res.lengths.cpu().numpy()[:, 0]
            return [tok[b, :max(ln[b], 0)].tolist() for b in range(tok.shape[0])]
        tok, ln = self.decode_audio(audio, n_samples)
        tok, ln = tok.cpu().numpy(), ln.cpu().numpy()
        return [tok[b, :ln[b]].tolist() for b in range(tok.shape[0])]

    def _char_map(self, idx_to_char):
        m = idx_to_char if idx_to_char is not None else self.idx_to_char
        if m is None:
            raise ValueError("no idx_to_char map: pass one here or to CTCModel(...)")
        return m

    def loss(self, feats, targets, input_lengths, target_lengths, reduction: str = "mean"):
        """The validation loss of ctc.py:409-425: decode(feats,
        return_log_probs=True), then ctc_loss on the (B, T, V) log-probs."""
        _, _, lp = self.decode(feats, return_log_probs=True)
        return ctc_loss(lp, targets, input_lengths, target_lengths, reduction=reduction, batch_first=True)

    def align(self, feats, targets, target_lengths, input_lengths=None) -> Alignment:
        """Forced alignment of known transcripts: decode(feats,
        return_log_probs=True), then ctc_align on the (B, T, V) log-probs
        (fp32 in an fp16 model too).  input_lengths: frames per utterance,
        all T when None."""
        _, _, lp = self.decode(feats, return_log_probs=True)
        if input_lengths is None:
            input_lengths = [lp.shape[1]] * lp.shape[0]
        return ctc_align(lp, targets, input_lengths, target_lengths, batch_first=True)

    def align_audio(self, audio, targets, target_lengths, n_samples: int = MAX_AUDIO_SAMPLES) -> Alignment:
        """audio -> Alignment: features(), then align() over all T = 1 +
        n_samples // 160 frames; span_seconds gives the labels' times."""
        return self.align(self.features(audio, n_samples), targets, target_lengths)

    def beam_decode(self, feats, beam: int = 16, top_k: int = 16, n_best: int = 1) -> BeamResult:
        """Prefix beam search over all T frames: decode(feats,
        return_log_probs=True), then ctc_beam_search on the (B, T, V)
        log-probs (fp32 in an fp16 model too)."""
        _, _, lp = self.decode(feats, return_log_probs=True)
        return ctc_beam_search(lp, None, beam=beam, top_k=top_k, n_best=n_best, batch_first=True)

    def beam_decode_audio(self, audio, n_samples: int = MAX_AUDIO_SAMPLES, beam: int = 16, top_k: int = 16,
                          n_best: int = 1) -> BeamResult:
        """audio -> BeamResult: features(), then beam_decode()."""
        return self.beam_decode(self.features(audio, n_samples), beam=beam, top_k=top_k, n_best=n_best)

    def spot(self, feats, keywords, keyword_lengths=None, input_lengths=None, normalize: bool = True,
             frame_scores: bool = False) -> Spot:
        """Keyword spotting: decode(feats, return_log_probs=True), then
        ctc_spot on the (B, T, V) log-probs (fp32 in an fp16 model too)."""
        _, _, lp = self.decode(feats, return_log_probs=True)
        return ctc_spot(lp, keywords, keyword_lengths, input_lengths, normalize=normalize, frame_scores=frame_scores,
                        batch_first=True)

    def spot_audio(self, audio, keywords, keyword_lengths=None, n_samples: int = MAX_AUDIO_SAMPLES, normalize: bool = True,
                   frame_scores: bool = False) -> Spot:
        """audio -> Spot: features(), then spot() over all T = 1 + n_samples
        // 160 frames; span_seconds gives the keywords' times."""
        return self.spot(self.features(audio, n_samples), keywords, keyword_lengths, normalize=normalize,
                         frame_scores=frame_scores)

    def cer(self, feats, targets, target_lengths, beam: Optional[int] = None, top_k: int = 16, n_best: int = 1,
            input_lengths=None) -> EditStats:
        """The edit statistics of this model's transcripts against `targets`
        (ctc_loss's forms), nothing leaving the device.  Greedy (beam=None):
        decode, frame_argmax, then edit_distance collapsing the per-frame
        labels.  beam=W: beam_decode's n_best hypotheses, all compared, so
        EditStats.best and totals[1] are the beam's oracle.  input_lengths:
        frames per utterance, all T when None.  error_rate(stats) is the CER."""
        import torch
        labels = pad_targets(targets, target_lengths)
        if beam is None:
            if n_best != 1:
                raise ValueError(f"n_best={n_best!r} needs a beam: the greedy path has one hypothesis")
            f = torch.as_tensor(feats, dtype=torch.float32)
            self.decode(f)
            return edit_distance(self.frame_argmax(f.shape[0], f.shape[1]), input_lengths, labels, target_lengths, collapse=True)
        _, _, lp = self.decode(feats, return_log_probs=True)
        res = ctc_beam_search(lp, input_lengths, beam=beam, top_k=top_k, n_best=n_best, batch_first=True)
        return edit_distance(res.tokens, res.lengths, labels, target_lengths)

    def cer_audio(self, audio, targets, target_lengths, n_samples: int = MAX_AUDIO_SAMPLES, beam: Optional[int] = None,
                  top_k: int = 16, n_best: int = 1) -> EditStats:
        """audio -> EditStats: features(), then cer() over all T = 1 + n_samples // 160 frames."""
        return self.cer(self.features(audio, n_samples), targets, target_lengths, beam=beam, top_k=top_k, n_best=n_best)

    # ---- parameter gradients (fp32 models; wk_ctc_forward_train / wk_ctc_backward) ----
    def forward_train(self, feats, dropout=None, seed: int = 0, offset: int = 0):
        """(B, T, 80) -> (B, T, V) log-probs on the device, with the
        activations backward() needs kept in the model's training workspace;
        no tokens are decoded.  Dropout is off by default: the eval-mode
        function, bit for bit decode(..., return_log_probs=True).  `dropout`
        (a probability for both sites, or (p_enc, p_gru); the reference
        trains at 0.2, ctc.py:34) applies the train-mode masks of
        wk_ctc_forward_train_dropout, a function of (seed, offset) alone:
        pass a new offset per step.  backward() differentiates whichever
        function the last forward_train computed."""
        import torch
        p_enc, p_gru = dropout_pair(dropout)
        if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(offset) < 2 ** 63:
            raise ValueError(f"seed must lie in [0, 2^64) and offset in [0, 2^63), got {seed!r}, {offset!r}")
        f = torch.as_tensor(feats, dtype=torch.float32).to(f"cuda:{self.device}").contiguous()
        B, T, _ = f.shape
        lp = torch.empty((B, T, self.vocab), dtype=torch.float32, device=f.device)
        if dropout is None:
            check(lib().wk_ctc_forward_train(self._h, C.c_void_p(f.data_ptr()), B, T, C.c_void_p(lp.data_ptr()),
                                             self._stream(torch)), "wk_ctc_forward_train")
        else:
            drop = _lib.WkCtcDropout(p_enc, p_gru, int(seed), int(offset))
            check(lib().wk_ctc_forward_train_dropout(self._h, C.c_void_p(f.data_ptr()), B, T, C.byref(drop),
                                                     C.c_void_p(lp.data_ptr()), self._stream(torch)),
                  "wk_ctc_forward_train_dropout")
        self._train_shape = (B, T)
        return lp

    def dropout_masks(self):
        """The masks of the last forward_train as two bool device tensors
        (True = kept): (B, T, 128) for the encoder output and (B, T, 256) for
        layer 0's output as layer 1's input; all True for a site that was off."""
        import torch
        if getattr(self, "_train_shape", None) is None:
            raise ValueError("no forward_train on this model yet")
        B, T = self._train_shape
        enc = torch.empty((B, T, 128), dtype=torch.uint8, device=f"cuda:{self.device}")
        gru = torch.empty((B, T, 256), dtype=torch.uint8, device=f"cuda:{self.device}")
        check(lib().wk_ctc_dropout_masks(self._h, C.c_void_p(enc.data_ptr()), C.c_void_p(gru.data_ptr()), self._stream(torch)),
              "wk_ctc_dropout_masks")
        return enc.bool(), gru.bool()

    def backward(self, dlogits, return_norm: bool = False):
        """The gradient of every parameter as one flat float32 device tensor in
        the weight blob's order (unpack_grads names its pieces), from dlogits
        (B, T, V): the gradient at the logits of the last forward_train, which
        is what wk_ctc_loss writes.  An upstream gradient G on the log-probs lp
        converts as  dlogits = G - lp.exp() * G.sum(-1, keepdim=True).
        return_norm: also the blob's 2-norm (a 0-d device tensor)."""
        import torch
        g = torch.as_tensor(dlogits, dtype=torch.float32).to(f"cuda:{self.device}").contiguous()
        if g.dim() != 3 or g.shape[2] != self.vocab:
            raise ValueError(f"dlogits must be (B, T, {self.vocab}), got {tuple(g.shape)}")
        B, T, _ = g.shape
        n = lib().wk_ctc_num_weights(C.byref(self.cfg))
        out = torch.empty((n,), dtype=torch.float32, device=g.device)
        norm = torch.empty((1,), dtype=torch.float32, device=g.device) if return_norm else None
        check(lib().wk_ctc_backward(self._h, B, T, C.c_void_p(g.data_ptr()), C.c_void_p(out.data_ptr()),
                                    C.c_void_p(norm.data_ptr()) if norm is not None else None, self._stream(torch)),
              "wk_ctc_backward")
        return (out, norm.reshape(())) if return_norm else out

    def loss_and_grad(self, feats, targets, input_lengths, target_lengths, reduction: str = "mean",
                      zero_infinity: bool = False, dropout=None, seed: int = 0, offset: int = 0):
        """The loss half of a training step (ctc.py:390-401, without the clip
        and the optimiser): forward_train, wk_ctc_loss with its gradient
        output, backward.  Returns (loss, {state-dict key: gradient view},
        gradient 2-norm), all on the device; loss is per utterance for
        reduction="none", whose gradient is that of the sum.  dropout, seed,
        offset: forward_train's (off by default)."""
        loss, flat, norm = self._loss_and_flat_grad(feats, targets, input_lengths, target_lengths, reduction, zero_infinity,
                                                    dropout, seed, offset)
        return loss, unpack_grads(flat, self.vocab), norm

    def _loss_and_flat_grad(self, feats, targets, input_lengths, target_lengths, reduction: str = "mean",
                            zero_infinity: bool = False, dropout=None, seed: int = 0, offset: int = 0):
        """loss_and_grad with the gradient as backward() returns it: one flat tensor."""
        if reduction not in _lib.WK_CTC_REDUCTION:
            raise ValueError(f"reduction must be 'none', 'sum' or 'mean', got {reduction!r}")
        lp = self.forward_train(feats, dropout, seed, offset)
        B, T, _ = lp.shape
        labels, in_len, lab_len, max_label_len = _label_args(lp, targets, input_lengths, target_lengths)
        nll, loss, grad = _wk_ctc_loss(lp, labels, in_len, lab_len, max_label_len, reduction, zero_infinity, True,
                                       f"wk_ctc_loss: unsupported shape (B={B}, T={T}, max label length {max_label_len})")
        flat, norm = self.backward(grad, return_norm=True)
        return (nll if reduction == "none" else loss.reshape(())), flat, norm

    # ---- the weights after creation, and the optimiser (fp32 models; wk_ctc_adam_step and its companions) ----
    def num_weights(self) -> int:
        return int(lib().wk_ctc_num_weights(C.byref(self.cfg)))

    def _flat(self, t, what: str):
        """`t` as a flat float32 device tensor of num_weights() values."""
        import torch
        f = torch.as_tensor(t, dtype=torch.float32).to(f"cuda:{self.device}").reshape(-1).contiguous()
        if f.numel() != self.num_weights():
            raise ValueError(f"{what}: expected {self.num_weights()} values for vocab={self.vocab}, got {f.numel()}")
        return f

    def weights(self):
        """The current weights as one flat float32 device tensor in the blob's
        order (unpack_grads names its pieces); stream-ordered, no host sync."""
        import torch
        out = torch.empty((self.num_weights(),), dtype=torch.float32, device=f"cuda:{self.device}")
        check(lib().wk_ctc_weights(self._h, C.c_void_p(out.data_ptr()), self._stream(torch)), "wk_ctc_weights")
        return out

    def state_dict(self) -> Dict[str, np.ndarray]:
        """{GRU_CTC_Model state-dict key: numpy array} of the current weights."""
        return {k: v.copy() for k, v in unpack_grads(self.weights().cpu().numpy(), self.vocab).items()}

    def set_weights(self, weights) -> None:
        """Replace the weights in place: a flat blob (host or device), a state
        dict or an nn.Module.  Every layout the kernels read is rebuilt on the
        device; the optimiser state is left as it is."""
        import torch
        if hasattr(weights, "state_dict") and callable(weights.state_dict):
            weights = weights.state_dict()
        if isinstance(weights, Mapping):
            weights = pack_state_dict(weights, self.vocab)
        w = self._flat(weights, "set_weights")
        check(lib().wk_ctc_set_weights(self._h, C.c_void_p(w.data_ptr()), self._stream(torch)), "wk_ctc_set_weights")

    def adam_step(self, grads, norm=None, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                  weight_decay: float = 0.0, max_norm: float = 5.0) -> None:
        """clip_grad_norm_(max_norm) then one torch.optim.Adam step (ctc.py:368,
        :401-402) on the model's own weights, in place.  grads: the flat
        gradient (backward's output) or a {key: gradient} dict; norm: its
        2-norm as a device tensor (loss_and_grad's), computed on the device
        when None.  max_norm <= 0: no clip.  No host sync."""
        import torch
        if isinstance(grads, Mapping):
            grads = torch.cat([torch.as_tensor(grads[k]).reshape(-1) for k, _ in ctc_state_dict_spec(self.vocab)])
        g = self._flat(grads, "adam_step")
        n = None
        if norm is not None:
            n = torch.as_tensor(norm, dtype=torch.float32).to(g.device).reshape(-1).contiguous()
            if n.numel() != 1:
                raise ValueError(f"norm must hold one value, got {n.numel()}")
        opt = _lib.WkCtcAdam(lr, betas[0], betas[1], eps, weight_decay, max_norm)
        check(lib().wk_ctc_adam_step(self._h, C.byref(opt), C.c_void_p(g.data_ptr()),
                                     C.c_void_p(n.data_ptr()) if n is not None else None, self._stream(torch)),
              "wk_ctc_adam_step")

    def optim_state(self):
        """(m, v, step): Adam's moments as flat device tensors (zeros before
        the first step) and the number of steps taken."""
        import torch
        m = torch.empty((self.num_weights(),), dtype=torch.float32, device=f"cuda:{self.device}")
        v = torch.empty_like(m)
        step = C.c_int64(0)
        check(lib().wk_ctc_optim_state(self._h, C.c_void_p(m.data_ptr()), C.c_void_p(v.data_ptr()), C.byref(step),
                                       self._stream(torch)), "wk_ctc_optim_state")
        return m, v, int(step.value)

    def set_optim_state(self, m=None, v=None, step: int = 0) -> None:
        """Adam's moments and step count; None means zeros, so the defaults reset the optimiser."""
        import torch
        mm = self._flat(m, "set_optim_state m") if m is not None else None
        vv = self._flat(v, "set_optim_state v") if v is not None else None
        check(lib().wk_ctc_set_optim_state(self._h, C.c_void_p(mm.data_ptr()) if mm is not None else None,
                                           C.c_void_p(vv.data_ptr()) if vv is not None else None, int(step),
                                           self._stream(torch)), "wk_ctc_set_optim_state")

    def decode_predictions(self, log_probs, idx_to_char: Optional[Mapping[int, str]] = None) -> List[str]:
        """THCHS30Trainer.decode_predictions (ctc.py:453-471) with this model's map."""
        return decode_predictions(log_probs, self._char_map(idx_to_char))

    def transcribe_text(self, audio, n_samples: int = MAX_AUDIO_SAMPLES,
                        idx_to_char: Optional[Mapping[int, str]] = None, beam: Optional[int] = None) -> List[str]:
        """audio -> text: the device greedy decode (beam=W: the beam's best
        hypothesis), then the idx_to_char map."""
        return tokens_to_text(self.transcribe(audio, n_samples, beam=beam), self._char_map(idx_to_char))
