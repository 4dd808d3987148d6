"""`utils.metrics.VQAAccuracy` and `VQAChallengeAccuracy` drop-ins with device-resident counters (reference:
utils/metrics.py:29-135, :136-184).

The reference's `update` moves argmax / top-5 indices to the host and calls `.item()` on every batch
(utils/metrics.py:80-94): two device syncs per train step.  Here `update` launches one HIP kernel
(`vqa_accuracy_update`, include/vqa_hip.h) that adds {top-1 correct, top-5 correct, samples} into a 3-element
u64 device buffer; nothing is read back until `compute()`.  Same interface: reset / update / compute / __str__.
There is no CPU path: logits on the host raise.
"""
from __future__ import annotations

import importlib
import os
from typing import Dict, List, Optional

import torch


def _pkg():
    import sys
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    root = os.path.dirname(here)
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module(os.path.basename(here))


class VQAAccuracy:
    """Running top-1 / top-5 accuracy (utils/metrics.py:29-135), counters kept on the GPU."""

    def __init__(self):
        self._L = _pkg()._lib
        self._counters: Optional[torch.Tensor] = None      # int64 view of {correct, correct_top5, total}
        self.reset()

    def reset(self):                                          # utils/metrics.py:47-53
        if self._counters is not None:
            self._counters.zero_()
        self.per_type_correct: Dict[str, int] = {}
        self.per_type_total: Dict[str, int] = {}

    def _buf(self, device) -> torch.Tensor:
        if self._counters is None or self._counters.device != device:
            self._counters = torch.zeros(3, dtype=torch.int64, device=device)
        return self._counters

    def update(self, predictions: torch.Tensor, targets: torch.Tensor, question_types: Optional[List[str]] = None):
        """predictions: logits [B, C] (fp32, GPU) or indices [B]; targets: i64 [B] (utils/metrics.py:55-106)."""
        if not predictions.is_cuda:
            raise RuntimeError("VQAAccuracy (HIP) keeps its counters on the GPU: predictions must be a GPU tensor; there is no CPU path")
        targets = targets.to(predictions.device, torch.int64).contiguous()
        c = self._buf(predictions.device)
        if predictions.dim() == 2:
            lg = predictions.detach()
            lg = lg.float().contiguous() if lg.dtype != torch.float32 else lg.contiguous()
            self._L.call("vqa_accuracy_update", lg.data_ptr(), targets.data_ptr(), c.data_ptr(), lg.shape[0], lg.shape[1])
            mask = None
        else:                                                  # index predictions: top-1 only, still no host sync
            mask = predictions.to(torch.int64) == targets
            c[0] += mask.sum()
            c[2] += targets.shape[0]
        if question_types is not None:                         # per-type breakdown needs the per-sample mask on the host (one copy)
            if mask is None:
                mask = predictions.argmax(dim=-1) == targets
            mask = mask.cpu()
            for i, qtype in enumerate(question_types):
                self.per_type_total[qtype] = self.per_type_total.get(qtype, 0) + 1
                self.per_type_correct[qtype] = self.per_type_correct.get(qtype, 0) + int(mask[i])

    # the reference exposes these as plain attributes
    def _read(self):
        return [0, 0, 0] if self._counters is None else [int(v) for v in self._counters.cpu()]

    @property
    def correct(self) -> int:
        return self._read()[0]

    @property
    def correct_top5(self) -> int:
        return self._read()[1]

    @property
    def total(self) -> int:
        return self._read()[2]

    def compute(self) -> Dict[str, float]:                    # utils/metrics.py:108-130
        correct, top5, total = self._read()
        results = {"accuracy": correct / max(total, 1), "accuracy_top5": top5 / max(total, 1), "correct": correct, "total": total}
        if self.per_type_total:
            results["per_type"] = {q: self.per_type_correct[q] / max(self.per_type_total[q], 1) for q in self.per_type_total}
        return results

    def __str__(self) -> str:
        m = self.compute()
        return f"Accuracy: {m['accuracy']:.4f} | Top-5: {m['accuracy_top5']:.4f}"


def _is_soft(x) -> bool:
    """A utils.soft_targets.SoftTargets (by shape, not by class: the drop-in module may be imported under more than one name)."""
    return isinstance(x, tuple) and hasattr(x, "ids") and hasattr(x, "weights") and hasattr(x, "counts")


class VQAChallengeAccuracy:
    """VQA v2 challenge accuracy, acc(ans) = min(1, #annotators who gave ans / 3) (utils/metrics.py:136-184), same interface:
    reset / update / compute, attributes total_score and count.

    `update(predictions, annotator_answers)` takes GPU logits [B, N] (or predicted indices [B]) with either the annotator ids
    [B, A] (-1: not in the vocabulary) or a SoftTargets that carries `counts`.  Scores are kept in integer thirds in a 2-element
    device buffer {thirds, questions}: exact, and nothing is read back before compute() / total_score / count.  The reference's own
    call form, a list of predicted strings and a list of lists of annotator strings, is counted on the host as it does."""

    def __init__(self):
        self._counters: Optional[torch.Tensor] = None      # int64 {thirds, questions} on the GPU
        self.reset()

    def reset(self):                                          # utils/metrics.py:150-153
        if self._counters is not None:
            self._counters.zero_()
        self._host = [0, 0]                                    # the string call form: {thirds, questions} counted on the host

    def _fused_acc(self, device) -> torch.Tensor:
        """The device counters (HipTrainer.step hands them to the loss launch: `vqa_cross_entropy_soft` / `vqa_bce_soft` counts/acc)."""
        if self._counters is None or self._counters.device != device:
            if self._counters is not None:
                self._host = [h + int(v) for h, v in zip(self._host, self._counters.cpu())]
            self._counters = torch.zeros(2, dtype=torch.int64, device=device)
        return self._counters

    def update(self, predictions, annotator_answers):
        if not isinstance(predictions, torch.Tensor):          # utils/metrics.py:167-175, in thirds
            for pred, answers in zip(predictions, annotator_answers):
                self._host[0] += min(3, sum(1 for ans in answers if ans == pred))
                self._host[1] += 1
            return
        if not predictions.is_cuda:
            raise RuntimeError("VQAChallengeAccuracy (HIP) keeps its counters on the GPU: predictions must be a GPU tensor; there is no CPU path")
        B, dev = predictions.shape[0], predictions.device
        soft = _is_soft(annotator_answers)
        if soft:
            if annotator_answers.counts is None:
                raise TypeError("VQAChallengeAccuracy.update: these SoftTargets carry no `counts` (votes per slot)")
            annotator_answers.validate(B, dev)
        elif not (isinstance(annotator_answers, torch.Tensor) and annotator_answers.dim() == 2 and annotator_answers.shape[0] == B):
            raise TypeError("VQAChallengeAccuracy.update: annotator_answers must be annotator ids [B, A] or SoftTargets with counts")
        c = self._fused_acc(dev)
        if predictions.dim() == 2:
            lg = predictions.detach()
            lg = lg.float().contiguous() if lg.dtype != torch.float32 else lg.contiguous()
            if not soft:
                annotator_answers = _pkg().load_dropin_soft_targets().answer_scores(annotator_answers.to(dev), lg.shape[1])
            ids, cnt = annotator_answers.ids, annotator_answers.counts
            _pkg()._lib.call("vqa_challenge_accuracy_update", lg.data_ptr(), ids.data_ptr(), cnt.data_ptr(), ids.shape[1], c.data_ptr(),
                             lg.shape[0], lg.shape[1])
        else:                                                  # index predictions: still no host sync
            pred = predictions.to(torch.int64)[:, None]
            if soft:
                votes = ((annotator_answers.ids.to(torch.int64) == pred) * annotator_answers.counts.to(torch.int64)).sum(1)
            else:
                a = annotator_answers.to(dev, torch.int64)
                votes = ((a == pred) & (a >= 0)).sum(1)
            c[0] += votes.clamp(max=3).sum()
            c[1] += B

    def _read(self):
        dev = [0, 0] if self._counters is None else [int(v) for v in self._counters.cpu()]
        return self._host[0] + dev[0], self._host[1] + dev[1]

    @property
    def total_score(self) -> float:
        return self._read()[0] / 3.0

    @property
    def count(self) -> int:
        return self._read()[1]

    def compute(self) -> float:                               # utils/metrics.py:177-184
        thirds, count = self._read()
        return thirds / (3 * max(count, 1))
