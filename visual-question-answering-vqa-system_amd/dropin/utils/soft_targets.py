"""Sparse soft answer scores for VQA v2 (ten annotator answers per question; utils/metrics.py:12-19:
acc(ans) = min(1, #annotators who agree / 3)).

The standard recipe supervises with the soft scores of ALL annotator answers and reports the challenge accuracy.  A dense
[B, num_answers] target costs a scatter, an autograd chain through F.cross_entropy and 4 KB per question; here a question
carries at most A (id, weight, count) triples:

    soft = answer_scores(annotator_ids, num_answers)            # one vqa_answer_scores launch, no host sync
    loss, logits = trainer.step(images, ids, mask, soft, metrics=VQAChallengeAccuracy())      # fused path, or
    loss = SoftTargetCrossEntropy()(model(images, ids, mask)[0], soft)                        # any torch.optim loop

The VQA v2 recipe itself trains a sigmoid per answer with binary cross-entropy against the same scores: HipTrainer(model, loss="bce")
for the fused step, SoftTargetBCEWithLogits() in the place of SoftTargetCrossEntropy() for a torch.optim loop.

There is no CPU path: host tensors raise.
"""
from __future__ import annotations

import importlib
import os
from typing import NamedTuple, Optional, Tuple

import torch
from torch import nn

MAX_SLOTS = 64          # one 64-lane wave owns a question: a lane per slot


def _pkg():
    import sys
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    root = os.path.dirname(here)
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module(os.path.basename(here))


def _on(t: torch.Tensor, device) -> bool:
    d = torch.device(device)
    return t.device.type == d.type and (d.index is None or t.device.index == d.index)


class SoftTargets(NamedTuple):
    """Soft targets of B questions with K slots each: t[b, c] = sum of weights[b, k] over the slots with ids[b, k] == c.
    ids int32 [B, K] (-1: empty slot), weights float32 [B, K], counts int32 [B, K] or None (votes per slot: only the challenge
    accuracy needs them)."""
    ids: torch.Tensor
    weights: torch.Tensor
    counts: Optional[torch.Tensor] = None

    def validate(self, B: int, device) -> "SoftTargets":
        """Raise ValueError unless the three tensors are what the kernels read: [B, K] with 1 <= K <= 64, int32 / float32 / int32,
        contiguous, on `device`.  Host logic only (no launch, no sync)."""
        for name, t, dtype in (("ids", self.ids, torch.int32), ("weights", self.weights, torch.float32), ("counts", self.counts, torch.int32)):
            if t is None and name == "counts":
                continue
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"SoftTargets.{name} must be a tensor, got {type(t).__name__}")
            if t.dtype != dtype:
                raise ValueError(f"SoftTargets.{name} must be {dtype}, got {t.dtype}")
            if t.dim() != 2 or t.shape[0] != B or not 1 <= t.shape[1] <= MAX_SLOTS:
                raise ValueError(f"SoftTargets.{name} must be [{B}, K] with 1 <= K <= {MAX_SLOTS}, got {tuple(t.shape)}")
            if t.shape != self.ids.shape:
                raise ValueError(f"SoftTargets.{name} has shape {tuple(t.shape)}, ids has {tuple(self.ids.shape)}")
            if not _on(t, device):
                raise ValueError(f"SoftTargets.{name} must be on {device}, got {t.device}")
            if not t.is_contiguous():
                raise ValueError(f"SoftTargets.{name} must be contiguous")
        return self


def answer_scores(annotator_ids: torch.Tensor, num_answers: int, normalize: bool = False) -> SoftTargets:
    """annotator_ids [B, A] (answer-vocabulary ids, -1: the annotator's answer is not in the vocabulary, A <= 64) -> SoftTargets of
    the distinct ids in order of first occurrence, weights min(1, count / 3) (normalize: divided by the row's sum), counts.
    One launch, nothing read back: a row with an id outside [-1, num_answers) comes out as {num_answers, -1, ...} with zero weights,
    and the loss kernel rejects it like a hard label out of range."""
    if not (isinstance(annotator_ids, torch.Tensor) and annotator_ids.is_cuda):
        raise RuntimeError("answer_scores (HIP): annotator_ids must be a GPU tensor; there is no CPU path")
    if annotator_ids.dim() != 2 or not 1 <= annotator_ids.shape[1] <= MAX_SLOTS or annotator_ids.shape[0] < 1:
        raise ValueError(f"annotator_ids must be [B, A] with 1 <= A <= {MAX_SLOTS}, got {tuple(annotator_ids.shape)}")
    if annotator_ids.is_floating_point() or annotator_ids.dtype == torch.bool:
        raise ValueError(f"annotator_ids must hold integer ids, got {annotator_ids.dtype}")
    L = _pkg()._lib
    a = annotator_ids.to(torch.int64).contiguous()
    B, A = a.shape
    ids = torch.empty((B, A), device=a.device, dtype=torch.int32)
    weights = torch.empty((B, A), device=a.device, dtype=torch.float32)
    counts = torch.empty((B, A), device=a.device, dtype=torch.int32)
    L.call("vqa_answer_scores", a.data_ptr(), ids.data_ptr(), weights.data_ptr(), counts.data_ptr(), B, A, int(num_answers), int(bool(normalize)), None)
    return SoftTargets(ids, weights, counts)


def _soft_loss_op(name: str, entry: str):
    """Define torch.ops.vqa_hip.<name>(logits, ids, weights, need_grad) -> (loss scalar, d loss / d logits or an empty tensor): one
    launch of the C entry `entry` (vqa_cross_entropy_soft's arguments) for the loss and its gradient, with its fake and its autograd."""
    @torch.library.custom_op(f"vqa_hip::{name}", mutates_args=(), device_types="cuda")
    def op(logits: torch.Tensor, ids: torch.Tensor, weights: torch.Tensor, need_grad: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        L = _pkg()._lib
        lg = logits.detach().contiguous()
        B, N = lg.shape
        loss = torch.zeros((), device=lg.device, dtype=torch.float32)
        err = torch.zeros(1, device=lg.device, dtype=torch.int32)
        ws = torch.empty((B,), device=lg.device, dtype=torch.float32)
        dlogits = torch.empty_like(lg) if need_grad else lg.new_empty((0,))
        L.call(entry, L.dt(lg), lg.data_ptr(), ids.data_ptr(), weights.data_ptr(), ids.shape[1], loss.data_ptr(),
               dlogits.data_ptr() if need_grad else None, None, B, N, 1.0, err.data_ptr(), ws.data_ptr(), None, None)
        bad = int(err.item())                                  # the one sync of this (slow) path: nn.CrossEntropyLoss raises here too
        if bad:
            raise IndexError(f"{bad} row(s) with an answer id out of range [-1, {N})")
        return loss, dlogits

    @op.register_fake
    def _(logits, ids, weights, need_grad):
        return logits.new_empty((), dtype=torch.float32), (torch.empty_like(logits) if need_grad else logits.new_empty((0,)))

    def setup(ctx, inputs, output):
        ctx.save_for_backward(output[1])

    def backward(ctx, gloss, _gdl):
        (dlogits,) = ctx.saved_tensors
        if dlogits.numel() == 0:
            raise RuntimeError(f"{name} was called with need_grad=False: there is no gradient to return")
        return dlogits * gloss.to(dlogits.dtype), None, None, None

    torch.library.register_autograd(f"vqa_hip::{name}", backward, setup_context=setup)


_soft_loss_op("soft_cross_entropy", "vqa_cross_entropy_soft")
_soft_loss_op("soft_bce", "vqa_bce_soft")


class SoftTargetCrossEntropy(nn.Module):
    """F.cross_entropy(logits, t) (mean over rows) for the sparse t of a SoftTargets: one fused HIP launch for the loss and its
    gradient (`vqa_cross_entropy_soft`), reached through autograd like nn.CrossEntropyLoss in training/train.py:120."""

    def forward(self, logits: torch.Tensor, soft: SoftTargets) -> torch.Tensor:
        if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dim() == 2):
            raise RuntimeError("SoftTargetCrossEntropy (HIP): logits must be a [B, N] GPU tensor; there is no CPU path")
        soft.validate(logits.shape[0], logits.device)
        need = torch.is_grad_enabled() and logits.requires_grad
        return torch.ops.vqa_hip.soft_cross_entropy(logits, soft.ids, soft.weights, need)[0]


class SoftTargetBCEWithLogits(nn.Module):
    """F.binary_cross_entropy_with_logits(logits, t, reduction="sum") / B (summed over the answers, averaged over the questions) for
    the sparse t of a SoftTargets: one fused HIP launch for the loss and its gradient (`vqa_bce_soft`), reached through autograd.
    A question without an in-vocabulary answer contributes sigmoid(x) / B to the gradient (under SoftTargetCrossEntropy: nothing)."""

    def forward(self, logits: torch.Tensor, soft: SoftTargets) -> torch.Tensor:
        if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dim() == 2):
            raise RuntimeError("SoftTargetBCEWithLogits (HIP): logits must be a [B, N] GPU tensor; there is no CPU path")
        soft.validate(logits.shape[0], logits.device)
        need = torch.is_grad_enabled() and logits.requires_grad
        return torch.ops.vqa_hip.soft_bce(logits, soft.ids, soft.weights, need)[0]
