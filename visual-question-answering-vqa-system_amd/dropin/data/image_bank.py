"""Train from resident uint8 images, augmented as they are drawn.

The reference's training transform (data/preprocess.py:66-87) is `Resize((256, 256))`, which depends on the image alone, followed by
`RandomCrop(224)`, `RandomHorizontalFlip` and `ColorJitter`, which are drawn per sample.  `ImageBank` stores the deterministic prefix
once -- uint8 [capacity, size, size, 3] on the device, 196 608 B per 256-side image, filled through the `vqa_image_resize` path
(PIL.resize(BILINEAR) bit for bit) -- and `bank.batch(rows, ...)` is the random suffix as one `vqa_bank_batch` launch (crop window +
flip, bytes copied) and, with a jitter, the existing `DeviceColorJitter` launch behind it.  The result is a `ByteImages`, which
model(...), forward_grouped, HipTrainer.step / accumulate / step_graphed take as it is: after the fill the host touches no pixel.

    bank = ImageBank(capacity=len(images))                      # every rank holds the whole bank
    bank.append(decoded_uint8_images)                           # any sizes, CPU or GPU; once
    loader = BankLoader(bank, image_row, token_ids, attention_mask, answers, batch_size=512, crop=224, flip_p=0.5, jitter=jitter)
    for batch in loader: trainer.step(batch["images"], batch["token_ids"], batch["attention_mask"], batch["answers"])

With one generator state and the same source images, `bank.batch` returns the bytes `gpu_collate_fn(..., resizer=DeviceImageResizer(
size, crop, jitter=...), output="bytes")` returns: the draws are taken in its order from its distributions.  A second bank with
size=224 and no crop is the validation transform (a pure gather through the same kernel).
`BankSampler` (host only) orders an epoch, shards it over ranks and owns the generator of the augmentation draws; `BankLoader` keeps the
sample table on the device and yields `vqa_collate_fn`'s dict.  There is no CPU path: the bank lives on the GPU.
"""
from __future__ import annotations

import importlib
import os
from typing import Optional, Sequence

import torch


def _pkg():
    import sys
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    root = os.path.dirname(here)
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module(os.path.basename(here))


_P = _pkg().load_dropin_preprocess()
IMAGENET_MEAN, IMAGENET_STD = _P.IMAGENET_MEAN, _P.IMAGENET_STD
APPEND_CHUNK = 64                                   # images per vqa_image_resize call of ImageBank.append


def _upload(parts, device):
    """Host tensors -> device tensors through ONE pinned staging buffer and one asynchronous copy (no sync: torch's pinned allocator
    keeps the buffer until the copy has run).  Every part is padded to 8 bytes so that each view is aligned for its dtype."""
    parts = [p.contiguous() for p in parts]
    sizes = [(p.numel() * p.element_size() + 7) // 8 * 8 for p in parts]
    host = torch.empty(max(sum(sizes), 8), dtype=torch.uint8, pin_memory=torch.device(device).type == "cuda")
    off = 0
    for p, s in zip(parts, sizes):
        host[off: off + p.numel() * p.element_size()] = p.reshape(-1).view(torch.uint8)
        off += s
    dev = host.to(device, non_blocking=True)
    out, off = [], 0
    for p, s in zip(parts, sizes):
        out.append(dev[off: off + p.numel() * p.element_size()].view(p.dtype).view(p.shape))
        off += s
    return out


def _jitter_arguments(jitter_params, B: int):
    """(order uint8 [B, 4], factors float32 [B, 4]) as vqa_image_color_jitter reads them, on the host -- what DeviceColorJitter.__call__
    makes of its `order` / `factors` (the hue factor becomes torchvision's uint8(hue_factor * 255): truncated toward zero in double,
    wrapped modulo 256; Image.blend takes its factor as a C float).  That call uploads the two tensors from pageable memory, which
    makes the host wait for the stream on every batch; here they ride in the batch's one pinned asynchronous copy instead, and the
    same launch follows.  tests/test_gpu_image_bank.py holds the two routes to equal bytes."""
    order, factors = jitter_params
    order = torch.as_tensor(order).to("cpu", torch.uint8).reshape(-1, 4)
    factors = torch.as_tensor(factors).to("cpu", torch.float64).reshape(-1, 4).clone()
    if order.shape[0] != B or factors.shape[0] != B:
        raise RuntimeError(f"ImageBank.batch: jitter `order` / `factors` must hold one row per sample ({B})")
    hue = factors[:, 3]
    if bool(((hue < -0.5) | (hue > 0.5)).any()):
        raise ValueError("hue_factor is not in [-0.5, 0.5].")
    factors[:, 3] = torch.where(torch.isnan(hue), hue, torch.remainder(torch.trunc(hue * 255.0), 256.0))
    return order, factors.to(torch.float32)


class ImageBank:
    """uint8 [capacity, size, size, 3] on the device: the Resize((size, size)) of every training image, stored once.
    `rows` images are filled (append / append_resized), `tensor()` is a view of them, `nbytes` the allocation.  `bad_rows` is a device
    int32 that counts the samples `batch` skipped because a DEVICE index (or origin) was out of range -- nothing reads it back unless
    asked (`int(bank.bad_rows)`).  size must be a multiple of 4 (vqa_bank_batch writes whole dwords)."""

    def __init__(self, capacity: int, size: int = 256, mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD,
                 device="cuda"):
        capacity, size = int(capacity), int(size)
        if capacity < 1:
            raise ValueError(f"ImageBank: capacity must be at least 1, got {capacity}")
        if size < 4 or size % 4 or size > 32768:
            raise ValueError(f"ImageBank: size must be a multiple of 4 in [4, 32768], got {size}")
        self.capacity, self.size, self.rows = capacity, size, 0
        self.mean, self.std = [float(m) for m in mean], [float(s) for s in std]
        self.device = torch.device(device)
        self._L = _pkg()._lib
        self._BI = _pkg().load_dropin_byte_images().ByteImages
        self._resizer = None
        self._data = torch.empty((capacity, size, size, 3), dtype=torch.uint8, device=self.device)
        self.bad_rows = torch.zeros((), dtype=torch.int32, device=self.device)

    @property
    def nbytes(self) -> int:
        return self._data.numel()

    def tensor(self) -> torch.Tensor:
        """The filled rows, uint8 [rows, size, size, 3] (a view, not a copy)."""
        return self._data[: self.rows]

    def __len__(self) -> int:
        return self.rows

    def __repr__(self):
        return f"ImageBank(rows={self.rows}, capacity={self.capacity}, size={self.size}, device={self.device}, nbytes={self.nbytes})"

    def _room(self, n: int, what: str):
        if self.rows + n > self.capacity:
            raise ValueError(f"ImageBank.{what}: {n} more images do not fit ({self.rows} of {self.capacity} rows are filled)")

    def append(self, images) -> int:
        """Resize decoded uint8 [H_i, W_i, 3] images of any sizes (CPU or GPU) into the next rows; returns the first row index.
        RuntimeError for anything that is not uint8 HWC with 3 channels, ValueError when the bank would overflow; both before any
        row is written."""
        ts = []
        for im in images:
            t = torch.as_tensor(im)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
                raise RuntimeError("ImageBank.append expects decoded uint8 [H, W, 3] images")
            ts.append(t)
        self._room(len(ts), "append")
        if self._resizer is None:
            self._resizer = _P.DeviceImageResizer(size=self.size, mean=self.mean, std=self.std, device=self.device)
        first = self.rows
        for lo in range(0, len(ts), APPEND_CHUNK):
            chunk = ts[lo: lo + APPEND_CHUNK]
            self._data[self.rows: self.rows + len(chunk)] = self._resizer(chunk, output="bytes").data
            self.rows += len(chunk)
        return first

    def append_resized(self, images_u8: torch.Tensor) -> int:
        """Images that already are uint8 [n, size, size, 3] (CPU or GPU); returns the first row index.  Errors as `append`."""
        t = images_u8
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 4 or tuple(t.shape[1:]) != (self.size, self.size, 3):
            raise RuntimeError(f"ImageBank.append_resized expects a uint8 [n, {self.size}, {self.size}, 3] batch")
        self._room(t.shape[0], "append_resized")
        first = self.rows
        self._data[first: first + t.shape[0]].copy_(t, non_blocking=True)
        self.rows += t.shape[0]
        return first

    # ------------------------------------------------------------------------------------------------------------------ draws
    def draw(self, B: int, crop: Optional[int] = None, flip_p: float = 0.0, jitter=None, generator=None):
        """The per-sample draws of one batch as host tensors, in gpu_collate_fn's order and distributions: (flip bool [B] | None,
        crop_yx int64 [B, 2] | None, (order, factors) | None).  Host logic only."""
        O = self._out(crop)
        flip = (torch.rand(B, generator=generator) < flip_p) if flip_p > 0.0 else None
        crop_yx = torch.randint(0, self.size - O + 1, (B, 2), generator=generator) if O != self.size else None
        params = jitter.draw(B, generator) if jitter is not None else None
        return flip, crop_yx, params

    def _out(self, crop) -> int:
        O = int(crop or self.size)
        if O < 4 or O % 4 or O > self.size:
            raise ValueError(f"ImageBank: crop must be a multiple of 4 in [4, {self.size}], got {O}")
        return O

    def batch(self, rows, crop: Optional[int] = None, crop_yx=None, flip=None, flip_p: float = 0.0, jitter=None, jitter_params=None,
              generator=None):
        """ByteImages [B, O, O, 3] (O = crop or size, the bank's mean / std) of the images rows[b]: window origin crop_yx[b] = (y, x),
        mirrored where flip[b], then `jitter` (a DeviceColorJitter) with jitter_params = (order, factors).  What is not given is
        drawn from `generator` (see `draw`).  rows: 1-D integer tensor (or list); on the CPU it is range-checked here for free
        (IndexError) and uploaded without a sync; a device tensor is not read back: the kernel skips a bad sample and counts it in
        `bad_rows`.  crop_yx / flip follow the same rule (a CPU origin outside [0, size - O] is a ValueError)."""
        O = self._out(crop)
        rows = torch.as_tensor(rows)
        if rows.dim() != 1 or rows.is_floating_point() or rows.dtype == torch.bool:
            raise ValueError(f"ImageBank.batch: rows must be a 1-D integer tensor, got {rows.dtype} {tuple(rows.shape)}")
        B = rows.shape[0]
        # only what was not supplied is drawn, in draw()'s order
        d_flip, d_crop, d_params = self.draw(B, crop if crop_yx is None else None, flip_p if flip is None else 0.0,
                                             jitter if jitter_params is None else None, generator)
        flip = d_flip if flip is None else torch.as_tensor(flip)
        crop_yx = d_crop if crop_yx is None else torch.as_tensor(crop_yx)
        jitter_params = d_params if jitter_params is None else jitter_params
        host = []                                   # what still sits on the host goes up in one copy
        if not rows.is_cuda:
            if B and (int(rows.min()) < 0 or int(rows.max()) >= self.rows):
                bad = int(rows.min()) if int(rows.min()) < 0 else int(rows.max())
                raise IndexError(f"ImageBank.batch: row {bad} is outside [0, {self.rows}) ({self.rows} rows are filled)")
            host.append(("rows", rows.to(torch.int32)))
        if crop_yx is not None:
            if crop_yx.numel() != 2 * B:
                raise RuntimeError("crop_yx must hold one (y, x) origin per sample")
            crop_yx = crop_yx.reshape(B, 2)
            if not crop_yx.is_cuda:
                if B and (int(crop_yx.min()) < 0 or int(crop_yx.max()) > self.size - O):
                    raise ValueError(f"ImageBank.batch: a crop origin is outside [0, {self.size - O}]")
                host.append(("crop", crop_yx.to(torch.int32)))
        if flip is not None:
            if flip.numel() != B:
                raise RuntimeError(f"`flip` must hold one flag per sample ({B}), got {flip.numel()}")
            flip = flip.reshape(B)
            if not flip.is_cuda:
                host.append(("flip", flip.to(torch.uint8)))
        if jitter is not None:
            host += list(zip(("order", "factors"), _jitter_arguments(jitter_params, B)))
        if self.device.type != "cuda":
            raise RuntimeError("ImageBank.batch runs on the GPU only: the bank lives on the device (no CPU fallback)")
        dev = dict(zip([k for k, _ in host], _upload([t for _, t in host], self.device))) if host else {}
        rows_d = dev["rows"] if "rows" in dev else rows.to(device=self.device, dtype=torch.int32).contiguous()
        crop_d = None if crop_yx is None else (dev["crop"] if "crop" in dev else crop_yx.to(device=self.device, dtype=torch.int32).contiguous())
        flip_d = None if flip is None else (dev["flip"] if "flip" in dev else flip.to(device=self.device, dtype=torch.uint8).contiguous())
        out = torch.empty((B, O, O, 3), dtype=torch.uint8, device=self.device)
        if B:
            # rows beyond the filled ones are refused like rows beyond the allocation: n_rows is what has been written
            self._L.call("vqa_bank_batch", self._data.data_ptr(), max(self.rows, 1), self.size, rows_d.data_ptr(),
                         None if crop_d is None else crop_d.data_ptr(), None if flip_d is None else flip_d.data_ptr(), out.data_ptr(),
                         B, O, self.bad_rows.data_ptr())
        if jitter is not None and B:                 # DeviceColorJitter's launch with output="bytes": the uint8 result only
            mid, out = out, torch.empty_like(out)
            sums = torch.empty(B, dtype=torch.int64, device=self.device)
            self._L.call("vqa_image_color_jitter", mid.data_ptr(), dev["order"].data_ptr(), dev["factors"].data_ptr(), B, O, O,
                         out.data_ptr(), None, *jitter.mean, *jitter.std, sums.data_ptr())
        return self._BI(out, self.mean, self.std)


class BankSampler:
    """Host-side order of the epochs of N samples (no GPU needed).  Epoch e is torch.randperm(N) from a generator seeded with
    seed + e (shuffle=False: 0 ... N-1); rank r of `world` takes every world-th entry, starting at r, of the longest prefix whose
    length `world` divides, so the ranks are disjoint and equally long.  Iteration yields int64 index tensors of batch_size entries
    (the last one shorter, or dropped with drop_last).  `generator` -- seeded from (seed, epoch, rank) at set_epoch -- serves the
    augmentation draws of the batches.  state_dict() / load_state_dict() hold the epoch, the next batch and that generator's state: a
    loop stopped after batch k and resumed yields the same remaining index tensors and draws."""

    def __init__(self, num_samples: int, batch_size: int, shuffle: bool = True, drop_last: bool = False, seed: int = 0, rank: int = 0,
                 world: int = 1):
        num_samples, batch_size, rank, world = int(num_samples), int(batch_size), int(rank), int(world)
        if num_samples < 1 or batch_size < 1:
            raise ValueError("BankSampler: num_samples and batch_size must be at least 1")
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"BankSampler: rank {rank} is outside [0, {world})")
        if num_samples < world:
            raise ValueError(f"BankSampler: {num_samples} samples cannot be shared by {world} ranks")
        self.num_samples, self.batch_size, self.shuffle, self.drop_last = num_samples, batch_size, bool(shuffle), bool(drop_last)
        self.seed, self.rank, self.world = int(seed), rank, world
        self.per_rank = num_samples // world
        self.generator = torch.Generator()
        self.set_epoch(0)

    def __len__(self) -> int:
        return self.per_rank // self.batch_size if self.drop_last else -(-self.per_rank // self.batch_size)

    def set_epoch(self, epoch: int):
        self.epoch, self._next = int(epoch), 0
        self.generator.manual_seed(((self.seed * 1000003 + self.epoch) * 1000003 + self.rank + 1) % (1 << 63))
        self._order = None

    def indices(self) -> torch.Tensor:
        """This rank's samples of the current epoch, in order (int64 [N // world])."""
        if self._order is None:
            if self.shuffle:
                order = torch.randperm(self.num_samples, generator=torch.Generator().manual_seed(self.seed + self.epoch))
            else:
                order = torch.arange(self.num_samples)
            self._order = order[: self.per_rank * self.world][self.rank:: self.world].contiguous()
        return self._order

    def __iter__(self):
        if self._next >= len(self):                  # the epoch was consumed and no other was selected: the same epoch again
            self.set_epoch(self.epoch)
        order = self.indices()
        while self._next < len(self):
            k = self._next
            self._next += 1
            yield order[k * self.batch_size: (k + 1) * self.batch_size]

    def state_dict(self) -> dict:
        return {"epoch": self.epoch, "next_batch": self._next, "generator": self.generator.get_state().clone()}

    def load_state_dict(self, state: dict):
        self.set_epoch(state["epoch"])
        self._next = int(state["next_batch"])
        self.generator.set_state(state["generator"])


class BankLoader:
    """The DataLoader of training/train.py for a resident bank: iteration yields vqa_collate_fn's dict -- 'images' (a ByteImages drawn
    from `bank`), 'token_ids', 'attention_mask', 'answers' -- for the batches of a BankSampler (batch_size, shuffle, drop_last, seed,
    rank, world).  The sample table stays on the device: image_row int [N] (the bank row of each sample), token_ids / attention_mask
    [N, L], answers int64 [N] or a SoftTargets whose ids / weights / counts are gathered row-wise.  crop / flip_p / jitter are
    ImageBank.batch's, drawn from the sampler's generator.
    group_by_image=True: 'images' holds one row per distinct image of the batch and the dict also holds 'image_index' (int64 on the
    host, what HipTrainer.step(..., image_index=) and forward_grouped take); one augmentation draw is made per image and shared by its
    questions.
    Everything is enqueued on the current stream: no side stream, no prefetch thread, no host sync (the batch's indices go up in one
    pinned asynchronous copy; a copy of image_row kept on the host groups the images)."""

    def __init__(self, bank: ImageBank, image_row, token_ids, attention_mask, answers, batch_size: int, shuffle: bool = True,
                 drop_last: bool = False, seed: int = 0, rank: int = 0, world: int = 1, crop: Optional[int] = None, flip_p: float = 0.0,
                 jitter=None, group_by_image: bool = False):
        self.bank, self.crop, self.flip_p, self.jitter, self.group_by_image = bank, crop, float(flip_p), jitter, bool(group_by_image)
        bank._out(crop)
        dev = bank.device
        rows = torch.as_tensor(image_row)
        if rows.dim() != 1 or rows.is_floating_point() or rows.dtype == torch.bool:
            raise ValueError("BankLoader: image_row must be a 1-D integer tensor")
        N = rows.shape[0]
        self._rows_host = rows.to("cpu", torch.int64)
        self._ST = _pkg().load_dropin_soft_targets().SoftTargets
        self._soft = isinstance(answers, self._ST)
        table = [torch.as_tensor(token_ids), torch.as_tensor(attention_mask)]
        table += [t for t in answers if t is not None] if self._soft else [torch.as_tensor(answers, dtype=torch.long)]
        if any(t.shape[0] != N for t in table):
            raise ValueError(f"BankLoader: every table must hold one row per sample ({N})")
        self._has_counts = self._soft and answers.counts is not None
        self._table = [t.to(dev).contiguous() for t in table]
        self.sampler = BankSampler(N, batch_size, shuffle, drop_last, seed, rank, world)

    def __len__(self) -> int:
        return len(self.sampler)

    def set_epoch(self, epoch: int):
        self.sampler.set_epoch(epoch)

    def state_dict(self) -> dict:
        return self.sampler.state_dict()

    def load_state_dict(self, state: dict):
        self.sampler.load_state_dict(state)

    def __iter__(self):
        gen, dev = self.sampler.generator, self.bank.device
        for idx in self.sampler:
            rows = self._rows_host[idx]
            if self.group_by_image:
                first, image_index = _pkg().load_dropin().group_by_image(rows)
                rows = rows[first]
            images = self.bank.batch(rows, crop=self.crop, flip_p=self.flip_p, jitter=self.jitter, generator=gen)
            (idx_d,) = _upload([idx], dev)
            g = [t.index_select(0, idx_d) for t in self._table]
            answers = self._ST(g[2], g[3], g[4] if self._has_counts else None) if self._soft else g[2]
            batch = {"images": images, "token_ids": g[0], "attention_mask": g[1], "answers": answers}
            if self.group_by_image:
                batch["image_index"] = image_index   # on the host: the step's range check is then free (a device index costs it a read)
            yield batch
