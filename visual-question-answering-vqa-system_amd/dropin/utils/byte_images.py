"""uint8 images end to end: `ByteImages` hands the model the bytes a decoder, a DataLoader or the GPU input pipeline holds.

Every route into the model takes normalised float32 NCHW images; what exists before that is uint8 HWC.  Normalising first costs a
pass that reads the bytes and writes a batch four times their size, which the stem kernels then read twice (forward and weight
gradient), the tape keeps until the stem backward and a captured train step copies into its static buffer on every replay.

    images = ByteImages(batch_u8)                               # uint8 [B, H, W, 3] on the model's device, ImageNet mean / std
    logits, _ = model(images, token_ids, mask)                  # eval, training under autograd, return_aux, image_index, ...
    loss, logits = trainer.step(images, token_ids, mask, targets)

With the bf16 compute dtype the three dedicated stem kernels read the bytes themselves and normalise while they stage their LDS
patch, through a bf16 [3][256] table of (v / 255 - mean[c]) / std[c]: the operand is bit-identical to the one they form from the
float32 batch, so every result equals the float route's bit for bit.  Every other route (float32 compute dtype, shapes the
dedicated kernels reject) normalises once with `to_float()` and runs unchanged.  Image gradients need float images.

A plain uint8 tensor keeps doing what it always did (`.float()`: values 0 ... 255, not normalised); this type is the explicit way in.
There is no CPU path: `to_float()` of a host batch raises.
"""
from __future__ import annotations

import importlib
import math
import os
from typing import Sequence, Tuple

import torch

IMAGENET_MEAN = [0.485, 0.456, 0.406]          # data/preprocess.py:34
IMAGENET_STD = [0.229, 0.224, 0.225]           # data/preprocess.py:35


def _pkg():
    import sys
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    root = os.path.dirname(here)
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module(os.path.basename(here))


def _three(values, name: str) -> Tuple[float, float, float]:
    try:
        out = tuple(float(v) for v in values)
    except TypeError:
        raise ValueError(f"ByteImages: `{name}` must hold three numbers, got {values!r}") from None
    if len(out) != 3 or not all(math.isfinite(v) for v in out):
        raise ValueError(f"ByteImages: `{name}` must hold three finite numbers, got {values!r}")
    return out


class ByteImages:
    """A uint8 [B, H, W, 3] contiguous image batch with the normalisation it stands for: channel c of a pixel v means
    (v / 255 - mean[c]) / std[c] -- ToTensor + Normalize of the reference pipeline (data/preprocess.py:34-35,117-121).  It is what
    `DeviceImageResizer(..., return_u8=True)`, `DeviceColorJitter(..., return_u8=True)` and `gpu_collate_fn(..., output="bytes")`
    return.  The constructor checks on the host and launches nothing: TypeError for another dtype, ValueError for a wrong rank, a
    last dimension that is not 3, a non-contiguous tensor, non-finite means, a zero or non-finite std."""
    __slots__ = ("data", "mean", "std")

    def __init__(self, data: torch.Tensor, mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD):
        if not isinstance(data, torch.Tensor):
            raise TypeError(f"ByteImages wraps a uint8 tensor, got {type(data).__name__}")
        if data.dtype != torch.uint8:
            raise TypeError(f"ByteImages wraps a uint8 tensor, got {data.dtype} (float images go to the model as they are)")
        if data.dim() != 4 or data.shape[-1] != 3:
            raise ValueError(f"ByteImages expects [B, H, W, 3] (HWC, as decoded), got {tuple(data.shape)}")
        if not data.is_contiguous():
            raise ValueError("ByteImages expects a contiguous tensor (the kernels address ((b*H + h)*W + w)*3 + c)")
        self.mean = _three(mean, "mean")
        self.std = _three(std, "std")
        if any(s == 0.0 for s in self.std):
            raise ValueError(f"ByteImages: `std` must not hold zero, got {std!r}")
        self.data = data

    @property
    def shape_nchw(self) -> Tuple[int, int, int, int]:
        B, H, W, _ = self.data.shape
        return (int(B), 3, int(H), int(W))

    @property
    def device(self) -> torch.device:
        return self.data.device

    @property
    def is_cuda(self) -> bool:
        return self.data.is_cuda

    @property
    def requires_grad(self) -> bool:
        return False

    def requires_grad_(self, requires_grad: bool = True):
        """Bytes carry no gradient: TypeError (an image gradient belongs to float images -- `to_float().requires_grad_()`)."""
        if requires_grad:
            raise TypeError("ByteImages cannot require grad: an image gradient needs float images; pass "
                            "images.to_float().requires_grad_() to the model instead")
        return self

    def __len__(self) -> int:
        return int(self.data.shape[0])

    def __repr__(self):
        return f"ByteImages(shape={tuple(self.data.shape)}, device={self.data.device}, mean={self.mean}, std={self.std})"

    def to_float(self) -> torch.Tensor:
        """The float32 [B, 3, H, W] batch the float pipeline would have produced: `vqa_image_normalize` without flip, or for a width
        that is no multiple of 4 the same IEEE expression in torch -- x / 255, then (x - mean) / std, both true divisions (by
        tensors: torch turns a division by a Python number into a multiplication by its reciprocal)."""
        x = self.data
        if not x.is_cuda:
            raise RuntimeError("ByteImages.to_float runs on the GPU only: move the uint8 batch to the device first (no CPU fallback)")
        B, _, H, W = self.shape_nchw
        if W % 4 == 0 and B > 0 and H > 0:
            out = torch.empty((B, 3, H, W), device=x.device, dtype=torch.float32)
            _pkg()._lib.call("vqa_image_normalize", x.data_ptr(), out.data_ptr(), None, B, H, W, *self.mean, *self.std)
            return out
        scalar = lambda v: torch.full((), v, device=x.device, dtype=torch.float32)     # (a fill launch: no host-to-device copy)
        t = x.permute(0, 3, 1, 2).to(torch.float32) / scalar(255.0)
        return torch.stack([(t[:, c] - scalar(self.mean[c])) / scalar(self.std[c]) for c in range(3)], 1)

