"""Per-parameter training statistics for a `torch.optim` loop (the unchanged training/train.py), read back once per logging interval.

    mon = ParameterMonitor(model, every=100, slots=64)
    ...
    loss.backward()
    mon.before_step(); optimizer.step(); mon.after_step()          # around every optimizer step
    ...
    for rec in mon.read():                                         # one device-to-host copy
        print(rec.step, rec.worst("update_ratio"))

Every `every`-th call is DUE: before_step() copies the flat parameter buffer (`model._flat`) to a snapshot, after_step() launches
`vqa_tensor_stats` (include/vqa_hip.h) over the parameters and over parameters minus snapshot into a slot of a device ring -- what
HipTrainer(monitor=TensorMonitor(...)) does inside its fused step; the record type and read() are the package's monitor.py.  The
gradient is recorded too when every Parameter's `.grad` is the model's own slice of ONE flat gradient tensor in layout order, as the
model's backward hands them out; after anything replaced a `.grad` (a clone, a hook, set_to_none followed by a hand-made tensor) the
record's grad_* fields are None.  There is no CPU path: the model must be on the GPU.
"""
from __future__ import annotations

import importlib
import os

import torch


def _pkg():
    import sys
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    root = os.path.dirname(here)
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module(os.path.basename(here))


class ParameterMonitor:
    def __init__(self, model, every: int = 100, slots: int = 64):
        pkg = _pkg()
        self._ring = pkg.monitor.TensorMonitor(every=every, slots=slots)       # (ValueError for every < 1 or slots < 1)
        self._ring._attach(self)
        self._LY = pkg.layout
        self.model = model
        self.every, self.slots = every, slots
        self.calls = 0                                     # before_step() calls so far: the `step` of a record
        self._due = False

    @property
    def dropped(self) -> int:
        return self._ring.dropped

    def clear(self):
        self._ring.clear()

    def read(self):
        """The records still in the ring, oldest first (monitor.StatsRecord; `trainable` is each Parameter's requires_grad at the
        step); the ring is empty afterwards."""
        return self._ring.read()

    def _flat_grad(self):
        """The flat gradient tensor the Parameters' .grad are slices of, or None when any of them is something else."""
        flat = self.model._flat
        base = store = None
        for p, e in zip(self.model._param_list(), self.model._param_entries):
            g = p.grad
            if g is None or g.dtype != torch.float32 or g.device != flat.device or g.layout != torch.strided:
                return None
            want = self._LY.view_of(flat, e)
            if tuple(g.shape) != tuple(want.shape) or g.stride() != want.stride():
                return None
            s, b = g.untyped_storage().data_ptr(), g.storage_offset() - e.offset
            if store is None:
                store, base, first = s, b, g
            elif s != store or b != base:
                return None
        if store is None or base < 0 or first.untyped_storage().nbytes() < 4 * (base + flat.numel()):
            return None
        return torch.empty(0, device=flat.device, dtype=torch.float32).set_(first.untyped_storage(), base, (flat.numel(),), (1,))

    def before_step(self):
        """Ahead of optimizer.step(): counts the call; a due call keeps the weights as they are."""
        self.calls += 1
        self._due = self._ring.due(self.calls)
        if self._due:
            if not self.model._flat.is_cuda:
                raise RuntimeError("ParameterMonitor needs the model on the GPU: there is no CPU path")
            self._ring.snapshot(self.model._param_entries, self.model._flat)

    def after_step(self):
        """Behind optimizer.step(): a due call records param and update, and grad when the gradients are the model's flat slices."""
        if not self._due:
            return
        self._due = False
        mask = tuple(bool(p.requires_grad) for p in self.model._param_list())
        self._ring.record(self.calls, 1.0, None if all(mask) else mask, self.model._flat, grad=self._flat_grad())
