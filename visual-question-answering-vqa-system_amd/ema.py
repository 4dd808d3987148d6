"""Exponential moving average (EMA) of the weights: the host side shared by HipTrainer (trainer.py: the average is kept by the
fused AdamW launch, vqa_adamw_ema / vqa_adamw_ranges_ema) and the drop-in utils.ema.ParameterEMA (dropin/utils/ema.py: one
vqa_ema_update launch per optimizer step of a torch.optim loop).

The average is ONE flat fp32 buffer with the layout of model._flat (layout.py), so that a kernel streams it next to the parameters.
Everything here is plain torch on whatever device the buffers live on; only `update` launches a kernel.
"""
from __future__ import annotations

import contextlib
from collections import OrderedDict

import torch

from . import layout as LY


def check_decay(decay, who: str = "ema_decay") -> float:
    """The decay as a float in [0, 1]; ValueError otherwise (NaN included).  Host logic, before anything is launched."""
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError(f"{who} must be a number in [0, 1], got {decay!r}") from None
    if not 0.0 <= d <= 1.0:                                # (NaN fails both comparisons)
        raise ValueError(f"{who} must lie in [0, 1], got {decay!r}")
    return d


def decay_at(decay: float, warmup: bool, t: int) -> float:
    """Decay of the update at step t >= 1 (the number of updates applied, this one included): the kernels' rule,
    min(decay, (1 + t) / (10 + t)) with warm-up, `decay` without."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def update(ema: torch.Tensor, flat: torch.Tensor, d: float):
    """ema = d * ema + (1 - d) * flat in one launch over the flat buffers (the expression the fused AdamW variants use)."""
    from ._lib import call, ptr
    if ema.shape != flat.shape or ema.dtype != torch.float32 or flat.dtype != torch.float32 or ema.device != flat.device:
        raise RuntimeError("ema.update: the average and the parameters must be fp32 flat buffers of one size on one device")
    call("vqa_ema_update", ptr(ema), ptr(flat), flat.numel(), float(d))


def state_dict(model, ema: torch.Tensor):
    """model.state_dict() with every parameter entry replaced by a clone of its slice of the average (the parameter's shape and
    dtype).  Buffers (BatchNorm running statistics, num_batches_tracked, the positional table) are the live model's: they are running
    averages already.  The keys are model.state_dict()'s, so the result loads with strict=True."""
    sd = model.state_dict()
    out = OrderedDict()
    avg = {e.name: e for e in model._param_entries}
    for k, v in sd.items():
        e = avg.get(k)
        out[k] = v.detach().clone() if e is None else LY.view_of(ema, e).to(v.dtype).clone()
    return out


def load_state_dict(model, ema: torch.Tensor, sd):
    """The inverse of state_dict for resuming: copies every parameter entry of `sd` into its slice of the average; buffer keys (and
    unknown keys) are ignored.  KeyError for a missing parameter, ValueError for a shape mismatch -- checked for every entry before
    the first one is written."""
    todo = []
    for e in model._param_entries:
        if e.name not in sd:
            raise KeyError(f"EMA state_dict has no entry for parameter {e.name!r}")
        v = sd[e.name]
        if tuple(v.shape) != tuple(e.shape):
            raise ValueError(f"EMA state_dict: {e.name!r} has shape {tuple(v.shape)}, the parameter has {tuple(e.shape)}")
        todo.append((e, v))
    with torch.no_grad():
        for e, v in todo:
            LY.view_of(ema, e).copy_(v)


@contextlib.contextmanager
def swapped(model, ema: torch.Tensor, keeps_cnn: bool = False):
    """Exchange the CONTENTS of model._flat and the average for the duration of the block, and exchange them back on exit (also when
    the block raises): validation on the averaged weights with the same model object.

    The exchange goes through torch ops on model._flat, so its version counter moves on entry and on exit: an ImageContext made on one
    side is refused on the other (VQAModel._ctx_stamp), and HipTrainer re-casts the bf16 operand copy at its next step (_param_sig).
    Captured inference graphs stay valid: they hold the flat buffer's POINTER and re-derive every working copy (the bf16 cast, the
    Conv+BN fold, the stem operands) from it on each replay, so a graph captured outside runs on the averaged weights inside.  The
    model epoch is bumped all the same, for whatever caches on it.  keeps_cnn: the caller knows that the average's image encoder
    equals the model's (HipTrainer: nothing wrote it since the average was made): cached ImageFeatures then stay valid on both sides (VQAModel._feat_stamp:
    the exchange's version bumps are excused); otherwise they are refused like the contexts."""
    flat = model._flat
    if ema.shape != flat.shape or ema.device != flat.device or ema.dtype != flat.dtype:
        raise RuntimeError("the average no longer matches model._flat (the model was moved with .to() after the average was made)")

    def exchange():
        v0 = model._feat_version() if keeps_cnn else 0
        with torch.no_grad():
            tmp = flat.clone()
            flat.copy_(ema)
            ema.copy_(tmp)
        model._ctx_epoch += 1
        if keeps_cnn:
            model._feat_excused += model._feat_version() - v0
        else:
            model._feat_epoch += 1

    exchange()
    try:
        yield model
    finally:
        if model._flat is not flat:
            raise RuntimeError("model._flat was replaced (.to()) while the averaged weights were swapped in")
        exchange()
