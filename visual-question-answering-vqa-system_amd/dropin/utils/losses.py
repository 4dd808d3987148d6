"""`nn.CrossEntropyLoss` with its constructor options as one fused HIP launch (training/train.py:120 builds the criterion).

    criterion = CrossEntropyLoss(weight=w, ignore_index=-100, label_smoothing=0.1)
    loss = criterion(model(images, ids, mask)[0], targets)         # any torch.optim loop; loss.backward() as usual

The loss and its gradient come from `vqa_cross_entropy_opts` (include/vqa_hip.h has the formulas): F.cross_entropy(logits, target,
weight=, ignore_index=, label_smoothing=, reduction="mean").  One deviation: when the batch has zero total weight (every target
ignored, or every kept target of class weight 0) the loss is NaN as in torch but the gradient is zero, where torch gives NaN in
the weighted case.  HipTrainer takes the same three options directly (label_smoothing=, class_weight=, ignore_index=).
There is no CPU path: host tensors raise.
"""
from __future__ import annotations

import importlib
import math
import os
from typing import Optional, Tuple

import torch
from torch import nn


def _pkg():
    import sys
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    root = os.path.dirname(here)
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module(os.path.basename(here))


# torch.ops.vqa_hip.cross_entropy_opts(logits, targets, weight | None, ignore_index, label_smoothing, need_grad)
#   -> (loss scalar, d loss / d logits or an empty tensor)
@torch.library.custom_op("vqa_hip::cross_entropy_opts", mutates_args=(), device_types="cuda")
def _cross_entropy_opts_op(logits: torch.Tensor, targets: torch.Tensor, weight: Optional[torch.Tensor], ignore_index: int,
                           label_smoothing: float, need_grad: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    K = _pkg().kernels
    lg = logits.detach().contiguous()
    err = torch.zeros(1, device=lg.device, dtype=torch.int32)
    loss, dlogits = K.cross_entropy_opts(lg, targets, class_weight=weight, ignore_index=ignore_index, label_smoothing=label_smoothing,
                                         need_grad=need_grad, err=err)
    bad = int(err.item())                                      # the one sync of this (slow) path: nn.CrossEntropyLoss raises here too
    if bad:
        raise IndexError(f"{bad} target(s) out of range [0, {lg.shape[1]}) (and not ignore_index = {ignore_index})")
    return loss, (dlogits if need_grad else lg.new_empty((0,)))


@_cross_entropy_opts_op.register_fake
def _(logits, targets, weight, ignore_index, label_smoothing, need_grad):
    return logits.new_empty((), dtype=torch.float32), (torch.empty_like(logits) if need_grad else logits.new_empty((0,)))


def _ceo_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _ceo_backward(ctx, gloss, _gdl):
    (dlogits,) = ctx.saved_tensors
    if dlogits.numel() == 0:
        raise RuntimeError("cross_entropy_opts was called with need_grad=False: there is no gradient to return")
    return dlogits * gloss.to(dlogits.dtype), None, None, None, None, None


torch.library.register_autograd("vqa_hip::cross_entropy_opts", _ceo_backward, setup_context=_ceo_setup)


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(weight, ignore_index, label_smoothing, reduction="mean") for fp32 or bf16 GPU logits [B, N] and class-index
    targets [B]: one fused HIP launch for the loss and its gradient, reached through autograd.  A target outside [0, N) that is not
    ignore_index raises IndexError (one device read per call)."""

    def __init__(self, weight=None, ignore_index: int = -100, label_smoothing: float = 0.0, reduction: str = "mean"):
        super().__init__()
        if reduction != "mean":
            raise ValueError(f"CrossEntropyLoss (HIP): only reduction='mean' is fused, got {reduction!r}")
        eps = float(label_smoothing)
        if not 0.0 <= eps <= 1.0 or math.isnan(eps):
            raise ValueError(f"CrossEntropyLoss (HIP): label_smoothing must lie in [0, 1], got {label_smoothing!r}")
        if isinstance(ignore_index, bool) or int(ignore_index) != ignore_index:
            raise ValueError(f"CrossEntropyLoss (HIP): ignore_index must be an integer, got {ignore_index!r}")
        if weight is not None:
            weight = torch.as_tensor(weight).detach().to(torch.float32)
            if weight.dim() != 1 or weight.numel() < 1:
                raise ValueError(f"CrossEntropyLoss (HIP): weight must be a vector with one entry per class, got shape {tuple(weight.shape)}")
            wc = weight.cpu()                                  # (a GPU weight costs one read, at construction only)
            if not bool(torch.isfinite(wc).all()) or bool((wc < 0).any()):
                raise ValueError("CrossEntropyLoss (HIP): weight must be finite and non-negative")
            weight = weight.contiguous()
        self.register_buffer("weight", weight)
        self.ignore_index, self.label_smoothing, self.reduction = int(ignore_index), eps, reduction

    def forward(self, logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dim() == 2):
            raise RuntimeError("CrossEntropyLoss (HIP): logits must be a [B, N] GPU tensor; there is no CPU path")
        if logits.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"CrossEntropyLoss (HIP): logits must be float32 or bfloat16, got {logits.dtype}")
        B, N = logits.shape
        if not isinstance(targets, torch.Tensor) or targets.dim() != 1 or targets.shape[0] != B or targets.is_floating_point():
            raise ValueError(f"CrossEntropyLoss (HIP): targets must be class indices [{B}], got "
                             f"{tuple(targets.shape) if isinstance(targets, torch.Tensor) else type(targets).__name__}")
        w = self.weight
        if w is not None:
            if w.shape[0] != N:
                raise ValueError(f"CrossEntropyLoss (HIP): weight has {w.shape[0]} entries, the logits have {N} classes")
            if w.device != logits.device:
                w = self.weight = w.to(logits.device)
        t = targets.to(logits.device, torch.int64).contiguous()
        need = torch.is_grad_enabled() and logits.requires_grad
        return torch.ops.vqa_hip.cross_entropy_opts(logits, t, w, self.ignore_index, self.label_smoothing, need)[0]
