"""Exponential moving average of the weights for a `torch.optim` loop (the unchanged training/train.py), one HIP launch per update.

    ema = ParameterEMA(model, decay=0.999, warmup=True)
    ...
    optimizer.step(); ema.update()                                 # after every optimizer step
    ...
    with ema.average_weights():                                    # validate() on the averaged weights, same model object
        validate()
    torch.save({"model_state_dict": ema.state_dict(), ...}, path)  # save_checkpoint(): the averaged weights, model.state_dict()'s keys

The average is one flat fp32 buffer laid out like the model's parameters (`model._flat`), updated by `vqa_ema_update`
(include/vqa_hip.h): ema = d * ema + (1 - d) * p with d = decay, or min(decay, (1 + t) / (10 + t)) at update t with warm-up.
HipTrainer(ema_decay=...) keeps the same average inside its fused AdamW launch; both share the host code of the package's ema.py.
BatchNorm buffers are not averaged (they are running averages already): state_dict() takes them from the live model.
There is no CPU path: the model must be on the GPU.
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


class ParameterEMA:
    def __init__(self, model, decay: float, warmup: bool = False):
        self._E = _pkg().ema
        self.model = model
        self.decay = self._E.check_decay(decay, "ParameterEMA: decay")
        self.warmup = bool(warmup)
        self.num_updates = 0
        self._bind()

    def _bind(self):
        """(Re)start the average from the model's current flat buffer.  After model.to(...) replaced the buffer, the average moves with
        it (same values, new device) rather than starting over."""
        flat = self.model._flat
        old = self.__dict__.get("ema")
        if old is not None and old.numel() == flat.numel():
            self.ema = old.to(flat.device, torch.float32).clone() if old.device != flat.device else old
        else:
            self.ema = flat.detach().clone()
        self._flat = flat

    def _bound(self):
        if self.model._flat is not self._flat:             # .to() / .cuda() re-flattened the parameters into a new buffer
            self._bind()
        return self.ema

    def update(self):
        """One `vqa_ema_update` launch over the flat buffers; call it after every optimizer step."""
        ema = self._bound()
        if not self._flat.is_cuda:
            raise RuntimeError("ParameterEMA.update needs the model on the GPU: there is no CPU path")
        d = self._E.decay_at(self._E.check_decay(self.decay, "ParameterEMA: decay"), self.warmup, self.num_updates + 1)
        self._E.update(ema, self._flat, d)
        self.num_updates += 1

    def state_dict(self):
        """model.state_dict() with every parameter replaced by its average (HipTrainer.ema_state_dict()'s format: loads strict=True)."""
        return self._E.state_dict(self.model, self._bound())

    def load_state_dict(self, sd, num_updates=None):
        """Parameter entries of `sd` become the average (buffer keys ignored; KeyError / ValueError as HipTrainer.load_ema_state_dict).
        num_updates: where the warm-up resumes (kept as it is when None)."""
        self._E.load_state_dict(self.model, self._bound(), sd)
        if num_updates is not None:
            self.num_updates = int(num_updates)

    def average_weights(self):
        """Context manager: the model holds the averaged weights inside the block and its own again after it (HipTrainer.ema_weights)."""
        return self._E.swapped(self.model, self._bound())
