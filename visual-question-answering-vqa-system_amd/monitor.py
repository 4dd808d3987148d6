"""Per-parameter training statistics on the device: which tensor carries the gradient norm, whose update-to-weight ratio is off,
which bias has had a zero gradient since step 0, how far the weights moved in one update.

    mon = TensorMonitor(every=100, slots=64)
    trainer = HipTrainer(model, ..., monitor=mon)
    ...                                                  # train; every 100th step() records, nothing is read back
    for rec in mon.read():                               # one device-to-host copy per logging interval
        print(rec.step, rec.worst("update_ratio"))

A record is three launches of `vqa_tensor_stats` (include/vqa_hip.h: a deterministic segmented reduction over a flat fp32 buffer, one
row {sumsq, absmax, nonfinite, zeros} per parameter) behind the step's AdamW launch, into a slot of a device ring:
  grad    the flat gradient `G` as the norm launch saw it -- after the data-parallel reduction, before the clip
  param   model._flat after the update
  update  model._flat minus a snapshot taken ahead of the AdamW launch (one device-to-device copy, on recording steps only)
The host keeps (calls, gscale, trainable mask) per slot and never waits.  This module is host logic; it is shared by HipTrainer,
HipTrainer.tensor_stats() and the drop-in utils.monitor.ParameterMonitor (torch.optim loops).
"""
from __future__ import annotations

import collections

import torch

from . import kernels as K

KINDS = ("grad", "param", "update")                        # what a monitored step records, in ring order
NOW_KINDS = ("grad", "param", "moment1", "moment2", "ema")   # what HipTrainer.tensor_stats() takes
_ZEROS_NAME = {"update": "update_unchanged"}               # the zeros of the difference are the elements the update left alone
FIELDS = tuple(f for k in KINDS + NOW_KINDS[2:] for f in (f"{k}_norm", f"{k}_absmax", f"{k}_nonfinite", _ZEROS_NAME.get(k, f"{k}_zeros"))
               ) + ("update_ratio",)


class StatsRecord:
    """One record: `step` (the trainer's `calls` of the step), `names` (list, layout order), `numel` (int64 [P]), `trainable`
    (bool [P]) and, per recorded kind k, CPU tensors of length P: k_norm and k_absmax (float64; the gradient's scaled by the step's
    gscale = 1 / (world * n), so grad_norm is the per-parameter share of HipTrainer.grad_norm()), k_nonfinite and k_zeros (int64;
    `update_unchanged` for the update).  norm and absmax run over the finite elements; nonfinite counts the rest.  update_ratio =
    update_norm / param_norm (0 where param_norm is 0).  A kind that was not recorded has None in its fields."""

    def __init__(self, step, names, numel, trainable, **fields):
        self.step, self.names, self.numel, self.trainable = step, names, numel, trainable
        for f in FIELDS:
            setattr(self, f, fields.pop(f, None))
        if fields:
            raise TypeError(f"StatsRecord: unknown field(s) {sorted(fields)}")

    def worst(self, key, k=5):
        """The names of the k parameters with the largest value of field `key` (e.g. "update_ratio", "grad_norm"), largest first."""
        if key not in FIELDS:
            raise KeyError(f"StatsRecord.worst: unknown field {key!r}")
        v = getattr(self, key)
        if v is None:
            raise ValueError(f"StatsRecord.worst: {key!r} was not recorded")
        idx = torch.topk(v.double(), min(int(k), v.numel())).indices.tolist()
        return [self.names[i] for i in idx]

    def __repr__(self):
        return f"StatsRecord(step={self.step}, P={len(self.names)}, fields={[f for f in FIELDS if getattr(self, f) is not None]})"


def layout_ranges(entries):
    """(lo, hi) of every parameter entry in layout order."""
    return [(e.offset, e.offset + e.numel) for e in entries]


def make_record(words, step, names, numel, trainable, gscale=1.0):
    """A StatsRecord from {kind: int32 [P][4] CPU tensor of vqa_tensor_stats rows}.  float64 from the fp32 words: sqrt and the scale
    are taken in double, so two records of the same bits give the same numbers."""
    fields = {}
    for kind, w in words.items():
        f = w[:, :2].contiguous().view(torch.float32).double()
        c = w[:, 2:].long() & 0xffffffff                   # the counts are unsigned words
        s = float(gscale) if kind == "grad" else 1.0
        fields[f"{kind}_norm"] = f[:, 0].sqrt() * s
        fields[f"{kind}_absmax"] = f[:, 1] * s
        fields[f"{kind}_nonfinite"] = c[:, 0].clone()
        fields[_ZEROS_NAME.get(kind, f"{kind}_zeros")] = c[:, 1].clone()
    if "update" in words and "param" in words:
        pn = fields["param_norm"]
        fields["update_ratio"] = torch.where(pn > 0, fields["update_norm"] / torch.where(pn > 0, pn, torch.ones_like(pn)), torch.zeros_like(pn))
    return StatsRecord(step, list(names), numel.clone(), trainable.clone(), **fields)


def check_now_kinds(kinds):
    """kinds of HipTrainer.tensor_stats(): a non-empty tuple out of NOW_KINDS without repeats; ValueError otherwise ("update" needs the
    snapshot only a monitored step takes)."""
    kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
    if not kinds or len(set(kinds)) != len(kinds):
        raise ValueError(f"tensor_stats: kinds must be a non-empty selection without repeats, got {kinds!r}")
    for k in kinds:
        if k == "update":
            raise ValueError('tensor_stats: "update" needs the snapshot a monitored step takes ahead of its AdamW launch; '
                             "use HipTrainer(monitor=TensorMonitor(...))")
        if k not in NOW_KINDS:
            raise ValueError(f"tensor_stats: unknown kind {k!r}; one of {NOW_KINDS}")
    return kinds


class TensorMonitor:
    """HipTrainer(monitor=TensorMonitor(every=100, slots=64)): every step whose `calls`, after it is counted, is a multiple of `every`
    records grad / param / update statistics of all parameters into slot `records % slots` of a device ring [slots, 3, P, 4]; the
    closing step() of an accumulation window counts, accumulate() never records.  Nothing is allocated before the first recording
    step, nothing is ever read back by a step.  read() returns the records still in the ring, oldest first, and empties it (one
    device-to-host copy); `dropped` counts the records a later one overwrote before they were read; clear() empties the ring without
    reading.  A monitor serves one trainer.  ValueError for every < 1 or slots < 1."""

    def __init__(self, every=100, slots=64):
        for name, v in (("every", every), ("slots", slots)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"TensorMonitor: {name} must be an integer >= 1, got {v!r}")
        self.every, self.slots = every, slots
        self.records = 0                                   # records ever taken
        self.dropped = 0
        self._live = collections.deque()                   # (slot, calls, gscale, trainable mask | None), oldest first
        self._owner = None
        self._ring = self._snap = self._table = None
        self._names = self._numel = None

    # ---- host logic
    def due(self, calls: int) -> bool:
        return calls % self.every == 0

    def _claim(self, calls, gscale, mask):
        """The slot of the next record; the host's note of it.  A full ring loses its oldest record."""
        slot = self.records % self.slots
        if len(self._live) == self.slots:
            self._live.popleft()
            self.dropped += 1
        self._live.append((slot, int(calls), float(gscale), None if mask is None else tuple(mask)))
        self.records += 1
        return slot

    def clear(self):
        self._live.clear()

    def _attach(self, owner):
        if self._owner is not None and self._owner is not owner:
            raise ValueError("TensorMonitor: this monitor already serves another trainer; make one per trainer")
        self._owner = owner

    # ---- device side
    def _bind(self, entries, flat):
        """Table, ring and snapshot for this layout on flat's device (first recording step; again after the buffer moved)."""
        if self._ring is not None and self._ring.device == flat.device and self._snap.numel() == flat.numel():
            return
        self._table = K.stats_table(layout_ranges(entries), flat.device)
        self._names = [e.name for e in entries]
        self._numel = torch.tensor([e.numel for e in entries], dtype=torch.int64)
        self._ring = torch.zeros((self.slots, len(KINDS), len(entries), 4), device=flat.device, dtype=torch.int32)
        self._snap = torch.empty_like(flat, requires_grad=False)
        self._live.clear()

    def snapshot(self, entries, flat):
        """Ahead of the update: the weights as they are (a device-to-device copy on the current stream)."""
        self._bind(entries, flat)
        with torch.no_grad():
            self._snap.copy_(flat.detach())

    def record(self, calls, gscale, mask, flat, grad=None):
        """Behind the update: the launches into the next slot (grad is skipped when None: its rows stay unread)."""
        slot = self._claim(calls, gscale if grad is not None else float("nan"), mask)
        ring = self._ring[slot]
        if grad is not None:
            K.tensor_stats(grad, self._table, out=ring[0])
        K.tensor_stats(flat.detach(), self._table, out=ring[1])
        K.tensor_stats(flat.detach(), self._table, y=self._snap, out=ring[2])

    def read(self):
        """The records still in the ring, oldest first, as StatsRecords; the ring is empty afterwards.  One device-to-host copy (a
        host sync); [] costs nothing."""
        live, self._live = list(self._live), collections.deque()
        if not live:
            return []
        idx = torch.tensor([s for s, _, _, _ in live], dtype=torch.int64, device=self._ring.device)
        host = self._ring.index_select(0, idx).cpu()
        out = []
        for i, (_, calls, gscale, mask) in enumerate(live):
            tr = torch.ones(len(self._names), dtype=torch.bool) if mask is None else torch.tensor(mask, dtype=torch.bool)
            kinds = KINDS if gscale == gscale else KINDS[1:]             # (NaN: the gradient was not recorded)
            words = {k: host[i, KINDS.index(k)] for k in kinds}
            out.append(make_record(words, calls, self._names, self._numel, tr, gscale))
        return out
