"""Data-parallel train-step harness (this repo's counterpart of Trainer.train_epoch, reference
training/train.py:168-208, non-AMP branch): zero_grad -> forward -> CrossEntropyLoss(mean) -> backward ->
[RCCL all-reduce of gradient buckets, overlapped with the remaining backward] -> clip_grad_norm_(1.0) -> AdamW.

Everything runs on device with no host synchronisation inside a step: the loss stays a device scalar, the
global gradient norm is consumed by the AdamW kernel straight from device memory.
One process per GPU; gradients are summed over ranks with torch.distributed (backend "nccl" = RCCL over xGMI,
or "gloo" in the CPU rehearsal tests) and divided by world size inside the optimizer kernel.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import struct
from typing import List, Optional

import torch
import torch.distributed as dist

from . import ema as EMA
from . import finetune as FT
from . import kernels as K
from . import layout as LY
from . import monitor as MON
from . import stepgraph as SG
from . import trainer_state as TS
from ._lib import call, dt, ptr


# Gradient segments (layout.bucket_ranges, reported by engine.backward in this order: answer_head, fusion, text_encoder, stage4 ...
# stem) are all-reduced in FOUR collectives: adjacent segments that finish close together travel as one message.
#   * head + fusion + text encoder (32.4 MB): the first two finish inside the latency-bound fusion chain right after the forward
#     (~120 dependent launches of 4-40 us).  Issuing a collective there costs host time exactly where the GPU is waiting for the
#     next launch (measured with a one-rank RCCL group at B=512: 9 collectives, three of them inside the chain: +0.9 ms per step);
#     merged, the message leaves when the text encoder's backward (side stream) reports, while the stage-4 convolutions run;
#   * stage 4 (33.7 MB) and stage 3 (8.4 MB): one message each, in flight under the stage-3 ... stem backward;
#   * stage 2 + stage 1 + stem (2.7 MB): one message at the end, together with the 4-byte bad-target counter.
# Larger messages also suit xGMI: a ring / direct all-reduce is per-link bound (7 links x ~153 GB/s per GPU), and a 2 MB message
# is mostly latency.
BUCKET_GROUPS = (("answer_head", "fusion", "text_encoder"), ("image_encoder.stage4",), ("image_encoder.stage3",),
                 ("image_encoder.stage2", "image_encoder.stage1", "image_encoder.stem"))


class GradBucketReducer:
    """Sum-all-reduce of contiguous gradient buckets, issued group by group while backward is still running.
    Device-agnostic (CUDA tensors: side stream + events, RCCL; CPU tensors: gloo) so the N>1 logic is testable on CPU."""

    def __init__(self, flat_grad: torch.Tensor, buckets, process_group=None, overlap=True, force=False, avoid_streams=()):
        """force: run the whole bucket choreography (communication stream, events, async all-reduce per bucket, waits) even in a
        world of ONE rank -- a single-rank RCCL group executes the same code path an 8-GPU job does, so the one-GPU test box can
        run it for real (tests/test_gpu_bench_ranks.py, bench.py --force-reducer); needs an initialised process group."""
        self.G = flat_grad
        self.buckets = list(buckets)
        self._range = {name: (lo, hi) for name, lo, hi in self.buckets}
        # merged groups: name -> (group index); a group is issued when its last segment has been reported
        self.groups = []
        for g in BUCKET_GROUPS:
            names = [n for n in g if n in self._range]
            if not names:
                continue
            lo, hi = min(self._range[n][0] for n in names), max(self._range[n][1] for n in names)
            if sum(self._range[n][1] - self._range[n][0] for n in names) != hi - lo:
                raise RuntimeError(f"gradient segments {names} are not adjacent in the flat buffer")
            self.groups.append((names, lo, hi))
        grouped = {n for names, _, _ in self.groups for n in names}
        for name, lo, hi in self.buckets:              # (a segment outside the table travels alone)
            if name not in grouped:
                self.groups.append(([name], lo, hi))
        self._group_of = {n: i for i, (names, _, _) in enumerate(self.groups) for n in names}
        self._pending = {}                             # group index -> (segments still missing, events collected)
        self._aux: List = []
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        if force and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("GradBucketReducer(force=True) needs an initialised torch.distributed process group")
        self.active = self.world > 1 or force
        self.overlap = overlap and flat_grad.is_cuda
        self.comm_stream = None
        if self.active and self.overlap:        # a stream that does not share a hardware queue with the compute streams (engine.py)
            from .engine import pick_concurrent_streams
            self.comm_stream = pick_concurrent_streams(flat_grad.device, 1, avoid=avoid_streams)[0]
        self._works: List = []
        self.issued: List[str] = []
        self._completed = 0
        self._send = [True] * len(self.groups)
        self.bytes_reduced = 0

    def set_trainable(self, ranges=None):
        """Fine-tuning: `ranges` = [(lo, hi, ...)] of the trainable flat elements (None: everything trains).  A group that holds no
        trainable parameter is not sent: its gradients are never read.  Like DDP, this needs the SAME trainable set on every rank --
        a group sent by some ranks and not by others would leave the collectives unmatched."""
        if ranges is None:
            self._send = [True] * len(self.groups)
        else:
            self._send = [any(r[0] < hi and r[1] > lo for r in ranges) for _, lo, hi in self.groups]

    def _issue(self, tensor, events=()):
        if self.comm_stream is not None:
            ev = torch.cuda.Event()
            ev.record()
            with torch.cuda.stream(self.comm_stream):
                self.comm_stream.wait_event(ev)
                for e in events:
                    self.comm_stream.wait_event(e)
                self._works.append(dist.all_reduce(tensor, op=dist.ReduceOp.SUM, group=self.pg, async_op=True))
        else:
            if tensor.is_cuda:
                cur = torch.cuda.current_stream()
                for e in events:
                    cur.wait_event(e)
            self._works.append(dist.all_reduce(tensor, op=dist.ReduceOp.SUM, group=self.pg, async_op=True))
        self.bytes_reduced += tensor.numel() * tensor.element_size()

    def reduce_aux(self, tensor: torch.Tensor):
        """Sum a small side tensor (the per-step bad-target counter) over the ranks: issued behind the last gradient message of
        the step (ordered after everything enqueued on the current stream by then), waited for in finish() with the buckets."""
        if self.active:
            self._aux.append(tensor)                   # travels with the LAST group: no collective inside the latency-bound chain

    def on_segment(self, name: str, events=()):
        """`events`: HIP events after which every gradient kernel of this segment has been enqueued-and-ordered (the engine
        records one on each stream that wrote the bucket: the data-gradient stream and the weight-gradient side stream).
        Only the COMMUNICATION stream waits for them -- the compute streams are never joined here, so the data-gradient chain
        keeps running ahead of the weight gradients exactly as in the 1-GPU step."""
        if not self.active or name not in self._range:
            return
        gi = self._group_of[name]
        names, lo, hi = self.groups[gi]
        missing, evs = self._pending.get(gi, (set(names), []))
        missing.discard(name)
        evs = evs + list(events)
        if self.G.is_cuda:                             # the stream that reports the segment (main, or the text encoder's side stream)
            e = torch.cuda.Event()
            e.record()
            evs.append(e)
        if missing:
            self._pending[gi] = (missing, evs)
            return
        self._pending.pop(gi, None)
        self._completed += 1
        if self._send[gi]:
            self.issued.append("+".join(names))
            self._issue(self.G[lo:hi], evs)
        if self._completed == len(self.groups):        # the last message of the step: the side tensors ride behind it
            for t in self._aux:
                self._issue(t)
            self._aux = []

    def finish(self):
        """Make the current stream (or the host, for gloo) wait for every bucket; returns the 1/world gradient scale."""
        if self._pending:
            raise RuntimeError(f"gradient segments never reported: {[sorted(m) for m, _ in self._pending.values()]}")
        for t in self._aux:                            # (a backward that reports no final group: still reduce the side tensors)
            self._issue(t)
        self._aux = []
        for w in self._works:
            w.wait()
        self._works = []
        self.issued = []
        self._completed = 0
        return 1.0 / self.world


def _is_soft(targets) -> bool:
    """A SoftTargets of the drop-in utils.soft_targets, recognised by its fields (that module can be imported under several names)."""
    return isinstance(targets, tuple) and hasattr(targets, "ids") and hasattr(targets, "weights") and hasattr(targets, "counts")


def _is_features(images) -> bool:
    """An ImageFeatures of the drop-in models.vqa_model, recognised by its fields (as _is_soft: the module has several import names)."""
    return hasattr(images, "_stamp") and hasattr(images, "_handle") and hasattr(images, "tensor") and hasattr(images, "select")


# HipTrainer.nonfinite_report(): the call number (trainer.calls) of the skipped step, its loss, (name, non-finite elements, numel) of
# every trainable parameter whose gradient holds a NaN or inf in layout order, and the int64 indices of the batch rows whose
# per-row loss term is not finite
NonFiniteReport = collections.namedtuple("NonFiniteReport", "step loss parameters rows")


class HipTrainer:
    _guard = None                                  # the non-finite guard's device words (set by the constructor when nonfinite is given)
    pending = 0                                    # micro-batches accumulated in the open window (accumulate(); 0: no window open)
    monitor = None                                 # the TensorMonitor (set by the constructor when monitor is given)
    _stats_tab = None

    def __init__(self, model, lr=1e-4, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0,
                 process_group=None, overlap=True, force_reducer=False, label_smoothing=0.0, class_weight=None, ignore_index=None,
                 ema_decay=None, ema_warmup=False, loss="ce", param_groups=None, nonfinite=None, monitor=None):
        """loss: "ce" (default: softmax cross-entropy, exactly the step without this option) or "bce" (sigmoid + binary cross-entropy on
        SoftTargets, see step()); readable afterwards as `loss_kind` (`loss` is the device scalar).
        ema_decay (None, or a float in [0, 1]): keep an exponential moving average of the weights, self.ema (a flat fp32 buffer laid out
        like model._flat, started at the initial weights): ema = d * ema + (1 - d) * p after every applied update, computed by the AdamW
        launch itself (vqa_adamw_ema / vqa_adamw_ranges_ema) from the updated parameter it still holds -- no extra launch.  ema_warmup:
        d = min(ema_decay, (1 + t) / (10 + t)) with Adam's step number t (per parameter when parts are frozen: the average of a
        parameter advances only while it trains).  A skipped step leaves the average untouched.  `ema_decay` stays a plain attribute that
        may be changed between steps, like `lr`.  None (default): no buffer, and the step issues exactly the launches it issues without
        this feature.  Data parallel: every rank applies the same update to identical parameters, so the averages stay identical and
        nothing is communicated.  ema_weights() / ema_state_dict() / load_ema_state_dict() evaluate on, export and restore the average.
        param_groups (None, or a list of dicts {"params": selector, "lr_scale": 1.0, "weight_decay": None}): a learning-rate scale and a
        weight decay per group of parameters.  A selector is an iterable of parameter names (state_dict names), name prefixes (strings
        that end in ".", e.g. "image_encoder.") and Parameter objects of this model; what no group selects forms an implicit last
        group (lr_scale 1, weight_decay None); weight_decay None follows the live `wd` of the trainer.  A parameter of group g is
        updated as torch.optim.AdamW([{"params": ..., "lr": lr * lr_scale_g, "weight_decay": wd_g}, ...], betas, eps) updates it, after
        clip_grad_norm_ over ALL trainable parameters (the norm stays global).  lr_scale 0 is not freezing: the moments, Adam's step
        number and the average advance, the parameter keeps its bits.  `param_groups` (attribute) is then the list of live dicts
        {"names", "lr_scale", "weight_decay"}: the two values may be changed between steps, like `lr`, and reach the kernels through a
        device block (vqa_group_hyper_set, launched only when a value changed) -- also those of a captured step, which is never
        re-captured for them.  finetune.no_weight_decay_groups(model) builds the usual two groups.  KeyError for an unknown name or a
        prefix that matches nothing; ValueError for a parameter in two groups, a parameter of another model, an empty group, more than
        16 groups, a value that is negative or not finite, or groups that need more than 512 ranges -- all before anything is
        allocated.  None (default): exactly the step without this feature, launch for launch.  Data parallel: the same groups on
        every rank give the same update; nothing is communicated and the reducer's trainable set does not change.
        nonfinite (None, "skip" or "raise"): the non-finite guard.  A step whose global gradient sum of squares -- the sum grad_norm()
        reports: over the trainable ranges, after the data-parallel reduction -- is NaN or +-inf is skipped ON THE DEVICE, with no host
        sync, in step() and in step_graphed() alike, and is treated as a step that never happened: parameters, both moments, the bf16
        operand copy, the average, the per-parameter lags and Adam's step number keep their bits, and so does every BatchNorm
        running_mean / running_var / num_batches_tracked (saved ahead of a train-mode CNN forward, restored behind the norm; the
        features route and an eval-mode CNN need neither).  The step still returns its NaN loss and logits; `calls` and the dropout
        stream advance as for any call; `metrics` count its rows as they come.  The verdict rests on the gradient alone: a zero-weight
        batch (NaN loss, zero gradient) keeps running AdamW as documented in step().  A step with an out-of-range target stays a
        bad-target step (check() raises IndexError for it, it is not counted as non-finite), but under the guard it restores the
        BatchNorm buffers too.  "raise": the same skipping, and check() raises FloatingPointError naming the steps skipped since the
        last check (the model is intact).  skipped_nonfinite() reads the counters, nonfinite_report() names the parameters and batch
        rows of the step just skipped; `t` counts both kinds of skip.  The fold block of the norm launch takes the decision
        (vqa_sumsq_guard / vqa_sumsq_ranges_guard): a clean step has no launch more than the unguarded one, bar the two over the
        BatchNorm buffers (40 KB).  Data parallel: every rank folds the same reduced gradient and decides the same; nothing is
        communicated.  ValueError for any other value, before anything is allocated.  None (default): exactly the step without
        this feature, launch for launch.
        monitor (None, or a monitor.TensorMonitor(every, slots)): per-parameter statistics on the device.  A step whose `calls`, after
        it is counted, is a multiple of `every` is DUE (the closing step() of an accumulation window counts; accumulate() never
        records): it copies model._flat to a snapshot ahead of the AdamW launch (device to device, on the step's stream) and issues
        three vqa_tensor_stats launches behind the step's last launch -- over `G` as the norm launch saw it (after the data-parallel
        reduction, before the clip; AdamW does not write it), over model._flat after the update, and over model._flat minus the
        snapshot -- into slot records % slots of the monitor's device ring.  Nothing is read back; the host notes (calls, gscale,
        trainable mask) per slot, and monitor.read() fetches the ring in one copy (monitor.py: StatsRecord).  The launches only read
        what the step computed: a monitored run keeps the unmonitored run's bits.  A skipped step (bad target, non-finite guard) is
        recorded like any due step: its update rows are zero with update_unchanged == numel, and under the guard its grad_nonfinite
        names the parameters nonfinite_report() names.  Frozen parameters keep their rows (trainable False, grad_zeros == numel,
        update_norm 0).  Data parallel: every rank records the same reduced gradient; nothing is communicated.  step_graphed() hands
        a due step to the eager step before any graph bookkeeping: it does not count towards a key's warm-up, is never captured and
        never replays, and no captured graph holds a statistics launch.  The monitor is not part of state_dict(); `calls` is, so a
        resumed run is due on the same steps.  A non-due step issues the plain step's launches; None (default): exactly the step
        without this feature, launch for launch.  TypeError for anything that is not a TensorMonitor, before anything is allocated."""
        self.model = model
        if monitor is not None:
            if not isinstance(monitor, MON.TensorMonitor):
                raise TypeError(f"HipTrainer: monitor must be a monitor.TensorMonitor or None, got {type(monitor).__name__}")
            monitor._attach(self)
        self.monitor = monitor
        self._stats_tab = None                     # tensor_stats(): the table of parameter ranges on the device
        # validated on the host before anything is allocated or launched
        self.nonfinite = TS.check_nonfinite(nonfinite)
        if not (isinstance(loss, str) and loss in ("ce", "bce")):
            raise ValueError(f'HipTrainer: loss must be "ce" or "bce", got {loss!r}')
        if loss == "bce" and not (label_smoothing == 0.0 and class_weight is None and ignore_index is None):
            raise ValueError('HipTrainer: label_smoothing / class_weight / ignore_index belong to the cross-entropy loss; '
                             'loss="bce" takes none of them')
        self.loss_kind = loss
        self._pg = None if param_groups is None else FT.ParamGroups(model._param_entries, model._param_list(), param_groups)
        self.param_groups = None if self._pg is None else self._pg.groups
        self.ema_decay = None if ema_decay is None else EMA.check_decay(ema_decay, "HipTrainer: ema_decay")
        self.ema_warmup = bool(ema_warmup)
        self.ema = None
        self._ema_swapped = False
        # what VQAModel._feat_stamp read of the image encoder when the average was cloned from the weights: while it reads the same, no
        # one wrote the image encoder since (this trainer, another one, torch.optim, load_state_dict), so the average's image-encoder
        # slice still equals the model's and ema_weights() leaves cached ImageFeatures valid.  None: unknown (an average was loaded)
        self._ema_cnn_stamp = None
        self.engine = model._ensure_engine()
        # nn.CrossEntropyLoss's constructor options for hard labels (all at their defaults: the plain loss launch, unchanged)
        self.label_smoothing, self.ignore_index, self.class_weight = self._check_loss_opts(label_smoothing, class_weight, ignore_index)
        self._loss_opts = self.label_smoothing != 0.0 or self.class_weight is not None or self.ignore_index is not None
        self.lr, self.wd, self.betas, self.eps, self.max_norm = lr, weight_decay, betas, eps, max_grad_norm
        flat = model._flat
        if self.ema_decay is not None:
            self.ema = flat.detach().clone()
            self._ema_cnn_stamp = self._cnn_stamp()
        self.G = torch.zeros_like(flat)
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        self.sumsq = torch.zeros(1 + 2048, device=flat.device, dtype=torch.float32)   # [0] = sum of squares, rest: block partials
        # one 8-byte scratch zeroed by ONE launch per step: [0] the loss (float32 view), [1] rows of THIS step whose target was
        # outside [0, num_answers) (int32; all-zero bits are 0.0f and 0).  The AdamW kernel skips the update when [1] != 0 and
        # accumulates {rows, steps} into `bad_targets` for check().
        self._scal = torch.zeros(2, device=flat.device, dtype=torch.int32)
        self.loss = self._scal[0:1].view(torch.float32)
        self.bad_step = self._scal[1:2]
        # {rows out of range, steps skipped} since the last check(), and [2]: steps skipped EVER (the AdamW kernel forms Adam's
        # step number as calls - skipped-ever on the device: a skipped step never advances the bias corrections, check() or not)
        self._bad = torch.zeros(3, device=flat.device, dtype=torch.int32)
        self.bad_targets = self._bad[:2]
        self._empty = torch.zeros(1, device=flat.device, dtype=torch.int32)   # steps whose batch had zero total weight since check()
        # the non-finite guard: _guard = {effective skip word of the step, non-finite skips since skipped_nonfinite(), ... ever},
        # written by the norm's fold block, which also keeps bad_targets; the AdamW launch reads the word and counts the launches
        # that were no step -- for either reason -- in an array of its own, so that a non-finite skip never lands in bad_targets
        if self.nonfinite is not None:
            self._guard = torch.zeros(3, device=flat.device, dtype=torch.int32)
            self._adam_skipped = torch.zeros(3, device=flat.device, dtype=torch.int32)
        self._nf_checked = 0                       # non-finite skips (ever) that check() / nonfinite_report() have seen
        self._nf_reported = 0
        self._last_ws = None                       # the last step's per-row loss terms (kept under the guard, for nonfinite_report)
        self._scan = None                          # nonfinite_report's table of parameter ranges and its counters
        self.calls = 0
        # gradient accumulation (accumulate(); `pending`, the class attribute above, counts the open window's micro-batches): the
        # window's trainable set and the BatchNorm buffers the guard saved ahead of the window's first train-mode CNN forward
        self._win_mask = None
        self._win_saved = None
        self._copy_sig = None                      # parameter-version signature right after the last fused AdamW launch
        self.buckets = LY.bucket_ranges(model._entries)
        self.reducer = GradBucketReducer(self.G, self.buckets, process_group, overlap, force=force_reducer,
                                         avoid_streams=[st for st in (self.engine.side, self.engine.side2) if st is not None])
        self.world = self.reducer.world
        self._norm_div = self.world                # what grad_norm() divides by: world * n of the last update (n: its window's micro-batches)
        # fine-tuning (frozen parameters): the optimizer runs over a device table of trainable ranges (finetune.trainable_ranges),
        # rebuilt only when the trainable set changes.  _lag_class groups parameters frozen during exactly the same steps; _lag[j]
        # (device) counts the applied steps parameter j spent frozen, so each range forms torch.optim.AdamW's per-parameter step.
        self._mask = None                          # trainable set of the current table (None: everything, the plain kernels)
        self._ever_frozen = False                  # some parameter was frozen at some step: the plain kernels' global step is off
        self._lag_class = [0] * len(model._param_entries)
        self._ranges = None                        # (table, R, n, frozen indices, nf) on the device
        self._ranges_gen = 0                       # how often that table was rebuilt (a captured step holds its address and sizes)
        self._lag = torch.zeros(len(model._param_entries), device=flat.device, dtype=torch.int32)
        # parameter groups: the device block of their values (vqa_group_hyper) and the values it holds (None: never written).  With
        # groups the optimizer always runs over the range table, whose ranges then also end at group boundaries; the group of every
        # range travels in an int32 array of its own, rebuilt with the table (_ranges[5])
        self._group_block = None if self._pg is None else torch.zeros(SG.GROUP_HYPER_BYTES // 4, device=flat.device, dtype=torch.int32)
        self._group_written = None
        # step_graphed: captured train steps (LRU, capped by model.graph_max_shapes like model._graphs), how often each key was seen
        # (the first two calls of a key run eagerly), and the device step-state block the captured launches read (stepgraph.py)
        self._graphs = {}
        self._graph_seen = {}
        self._state = None
        self.graph_captures = 0

    def _check_loss_opts(self, label_smoothing, class_weight, ignore_index):
        """Validated (label_smoothing float, ignore_index int | None, class_weight fp32 [num_answers] on the device | None); host
        logic on the caller's values, before anything is launched."""
        eps = float(label_smoothing)
        if not 0.0 <= eps <= 1.0:                          # (NaN fails both comparisons)
            raise ValueError(f"HipTrainer: label_smoothing must lie in [0, 1], got {label_smoothing!r}")
        if ignore_index is not None:
            if isinstance(ignore_index, bool) or int(ignore_index) != ignore_index:
                raise ValueError(f"HipTrainer: ignore_index must be an integer or None, got {ignore_index!r}")
            ignore_index = int(ignore_index)
        if class_weight is not None:
            n = self.model.num_answers
            w = torch.as_tensor(class_weight).detach().to("cpu", torch.float32)
            if w.dim() != 1 or w.shape[0] != n:
                raise ValueError(f"HipTrainer: class_weight must have {n} entries (num_answers), got shape {tuple(w.shape)}")
            if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
                raise ValueError("HipTrainer: class_weight must be finite and non-negative")
            class_weight = w.contiguous().to(self.model._flat.device)
        return eps, ignore_index, class_weight

    def _set_mask(self, trainable):
        """Trainable set of this step (tuple of bools in layout order, or None for all): rebuild the range table when it changed."""
        if trainable is not None and all(trainable):
            trainable = None
        grouped = self._pg is not None                 # (the table route even when nothing was ever frozen: all lags zero)
        if trainable == self._mask and (self._ranges is not None or not (self._ever_frozen or grouped)):
            return                                     # (a change of the groups' VALUES never comes here: the table stays)
        tr = trainable if trainable is not None else (True,) * len(self._lag_class)
        lag_class = FT.refine_classes(self._lag_class, tr)
        ranges = None
        if grouped:                                    # refused before anything of this trainer changes
            ranges = FT.trainable_ranges(self.model._param_entries, tr, lag_class, self._pg.group_of)
            if len(ranges) > FT.RANGES_MAX:
                raise ValueError(f"HipTrainer: this trainable set and these parameter groups need {len(ranges)} ranges; the optimizer's "
                                 f"table holds {FT.RANGES_MAX}")
        self._mask = trainable
        self._lag_class = lag_class
        self._ever_frozen = self._ever_frozen or trainable is not None
        if not self._ever_frozen and not grouped:
            self._ranges = None
            self.reducer.set_trainable(None)
            return
        if ranges is None:
            ranges = FT.trainable_ranges(self.model._param_entries, tr, self._lag_class)
        rows = FT.range_table_rows(ranges)
        n = sum(hi - lo for lo, hi, _ in ranges)
        dev = self.G.device
        table = torch.tensor(rows if rows else [[0, 0, 0, 0]], dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        frozen = [j for j, t in enumerate(tr) if not t]
        fidx = torch.tensor(frozen if frozen else [0], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        garr = None
        if grouped:
            gof = [self._pg.group_of[j] for _, _, j in ranges]
            garr = torch.tensor(gof if gof else [0], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        self._ranges = (table, len(rows), n, fidx, len(frozen), garr)
        self._ranges_gen += 1
        self.reducer.set_trainable(ranges if trainable is not None or not grouped else None)

    def step(self, images, token_ids, attention_mask, targets, metrics=None, image_index=None):
        """One full train step; returns (loss device scalar, logits fp32).  `metrics`: optional device-side accuracy tracker
        (dropin/utils/metrics.py VQAAccuracy) updated from the logits without a host sync (train.py:211-212 does two).
        image_index (many questions per image): images [U,3,H,W], token_ids / attention_mask [N,L], targets [N]; question i is asked of
        image image_index[i] and the step trains VQAModel.forward_grouped's composition (one CNN pass per image, loss per question).
        The range check is free for a CPU index (copied to the device without a sync) and costs one device-to-host read for a device
        index.  None: exactly the plain step.
        targets may be a SoftTargets (dropin/utils/soft_targets.py: sparse soft answer scores, ids / weights / counts [B, K]): the loss
        is then F.cross_entropy with those probability-style targets (`vqa_cross_entropy_soft`), everything around it is the same step.
        `metrics` must then be a VQAChallengeAccuracy (and the targets carry `counts`): it is counted inside the loss launch.
        With label_smoothing / class_weight / ignore_index given to the constructor the loss is F.cross_entropy with those options
        (`vqa_cross_entropy_opts`) and a VQAAccuracy is counted inside that launch over the rows that are not ignored; SoftTargets
        then raise TypeError.
        With loss="bce" given to the constructor (`trainer.loss_kind`) the targets must be SoftTargets and the loss is sigmoid + binary
        cross-entropy against the soft scores, F.binary_cross_entropy_with_logits(logits, t, reduction="sum") / B: summed over the
        answers, averaged over the questions (`vqa_bce_soft`, in the place of `vqa_cross_entropy_soft`, with the challenge accuracy
        riding in it the same way).  A question without an in-vocabulary answer then still pushes every logit down (under
        cross-entropy its gradient row is zero).  A label tensor raises TypeError: wrap hard labels as
        SoftTargets(labels.int()[:, None], ones).
        A batch of zero total weight (every target ignored, or every kept target of class weight 0) has a NaN
        loss and a ZERO gradient: the step still runs AdamW on it (weight decay and the moments' decay apply), which is what the
        reference loop does with torch when every target is ignored; torch's NaN gradient in the weighted case is not reproduced.
        Such steps are counted on the device and check() raises ValueError for them.
        images may be a ByteImages (dropin/utils/byte_images.py: the uint8 HWC batch as decoded, on the device): the stem kernels
        normalise while they load and the step equals the one on images.to_float() bit for bit; step_graphed then keeps a uint8 static
        image buffer and files the graph under the batch's mean / std as well.
        images may be an ImageFeatures (VQAModel.encode_features; with image_index: of the U images): the image encoder, which must be
        frozen and in eval mode, does not run, and everything after it is the same step -- the launches of the images step without the
        CNN forward, bit for bit.  RuntimeError before any launch when an image_encoder parameter requires grad, the image encoder is
        in train mode, or the features are stale.
        After k accumulate() calls the step closes their window: its own gradient is added to theirs and ONE update is applied with the
        mean of the k + 1 per-batch mean gradients (see accumulate())."""
        return self._enqueue(self._prologue("step", images, token_ids, attention_mask, targets, metrics, image_index))

    def accumulate(self, images, token_ids, attention_mask, targets, metrics=None, image_index=None):
        """A micro-batch of a gradient-accumulation window: step()'s arguments, checks and errors; forward, loss and backward run INTO the
        gradient already in `G` (every weight-gradient epilogue adds), and nothing else is launched: no norm, no AdamW, no collective.
        Returns (this micro-batch's loss, its fp32 logits); the loss is the device scalar step() returns, valid until the next call.
        The step() that follows k accumulate() calls closes the window with one update on the MEAN of the n = k + 1 per-batch mean
        gradients -- what (loss_i / n).backward() for each batch, clip_grad_norm_ and AdamW.step() apply; batches are not weighted by
        their row counts.  Nothing is rescaled in the loss launches (the bf16 d logits keep their bits): the closing AdamW launch
        takes gscale = 1 / (world * n), grad_norm() reports sqrt(sumsq) / (world * n), and `G` after the closing step holds the SUM
        over the window.  `pending` counts the open window's micro-batches (0: no window); discard_accumulated() drops it.
        Once per window, in the closing step: `calls`, Adam's step number, the per-parameter lags, the weight average.  Per
        micro-batch: the dropout stream (each draws its own masks), the engine's step_id / cnn_train_forwards, the model's
        _feat_epoch, `metrics`, and BatchNorm -- each micro-batch normalises with its OWN batch statistics and updates the running
        buffers, as two torch forwards would, so a window of train-mode BatchNorm is not the large batch.
        A bad target in ANY micro-batch skips the window's update: the bad-target word accumulates over the window, check() reports
        the window's bad rows and one skipped step.  Under the non-finite guard the verdict is taken once, by the closing norm
        launch, on the accumulated gradient, and a non-finite window never happened: the BatchNorm buffers are saved ahead of the
        window's first train-mode CNN forward only and restored behind the closing norm, which undoes the buffer updates of all its
        micro-batches together.  nonfinite_report() then names the parameters from the accumulated gradient and the rows of the
        CLOSING micro-batch only.
        The trainable set (requires_grad) must be the same for every call of a window: a change raises RuntimeError before anything
        is launched or counted -- close or discard the window first.  Routes may be mixed: images, ImageFeatures, image_index, any B.
        Data parallel: nothing is communicated here; the closing step reduces the accumulated `G` through the usual buckets,
        overlapped with its own backward, and the bad-target word with them.  Every rank must use the same n (as with DDP's no_sync).
        While a window is open step_graphed(), state_dict() and load_state_dict() raise RuntimeError: checkpoints are taken at window
        boundaries.  explain(), eval forwards, predict*, encode_* and ema_weights() blocks between two calls leave `G` alone."""
        return self._enqueue(self._prologue("accumulate", images, token_ids, attention_mask, targets, metrics, image_index, closing=False),
                             closing=False)

    def discard_accumulated(self):
        """Drop an open window: the accumulated gradient, its bad-target word and the BatchNorm buffers the guard saved for it are
        forgotten; the next step() is a plain step.  Nothing is launched: the next call, the first of a window or a plain step, zeroes
        `G` and the scratch words as it always does, and until then `G` still holds the discarded sum.  What the micro-batches'
        forwards did stays done, as after torch's zero_grad(): the BatchNorm running buffers moved and the dropout stream advanced.
        Nothing when no window is open."""
        self.pending, self._win_mask, self._win_saved = 0, None, None

    def _refuse_open(self, who):
        if self.pending:
            raise RuntimeError(f"HipTrainer.{who}: a gradient-accumulation window is open ({self.pending} micro-batch(es) pending); close it "
                               "with step() or drop it with discard_accumulated() first")

    def _prologue(self, who, images, token_ids, attention_mask, targets, metrics, image_index, closing=True):
        """The host half of a step: validation, the fine-tuning plan, the image index's device copy, the optimizer's range table and
        -- last, once nothing can be refused any more -- the bookkeeping (calls, the engine's step_id and cnn_train_forwards, the
        model's _feat_epoch).  Launches nothing through the C ABI.  Returns what _enqueue needs.  closing=False (accumulate): `calls` stays,
        it counts updates."""
        if self._ema_swapped:
            raise RuntimeError(f"HipTrainer.{who} inside ema_weights(): the model holds the averaged weights; leave the block first")
        eng = self.engine
        dev = self.G.device
        if self.ema is not None:                           # (ema_decay may have been changed since the constructor checked it)
            EMA.check_decay(self.ema_decay, "HipTrainer: ema_decay")
        group_values = None if self._pg is None else self._pg.effective(self.wd)      # (ValueError: a bad live value)
        soft = _is_soft(targets)
        bce = self.loss_kind == "bce"
        if bce and not soft:
            raise TypeError(f'HipTrainer.{who}: loss="bce" trains on SoftTargets; wrap hard labels as '
                            "SoftTargets(labels.int()[:, None], ones) with ones = torch.ones(B, 1) on the device")
        feats = images if _is_features(images) else None
        if feats is not None:
            images = feats.tensor()
        if soft and self._loss_opts:
            raise TypeError(f"HipTrainer.{who}: label_smoothing / class_weight / ignore_index apply to hard labels; "
                            "SoftTargets cannot be combined with them")
        if metrics is not None and soft != hasattr(metrics, "_fused_acc"):
            raise TypeError(f"HipTrainer.{who}: soft targets are scored by VQAChallengeAccuracy, hard labels by VQAAccuracy "
                            f"(got {type(metrics).__name__} with {'SoftTargets' if soft else 'a label tensor'})")
        if metrics is not None and soft and targets.counts is None:
            raise TypeError(f"HipTrainer.{who}: VQAChallengeAccuracy needs SoftTargets that carry `counts`")
        byt = images if K.is_byte_images(images) else None       # ByteImages: uint8 [B,H,W,3] (its constructor checked rank and channels)
        if byt is not None:
            images = byt.data
        for name, t in (("images", images), ("token_ids", token_ids)) + ((("targets", targets),) if not soft else ()):
            if not (isinstance(t, torch.Tensor) and t.device == dev):
                raise RuntimeError(f"HipTrainer.{who}: `{name}` must be a tensor on {dev} (there is no CPU path)")
        Bq = token_ids.shape[0] if (image_index is not None and token_ids.dim() == 2) else images.shape[0]
        if soft:
            targets.validate(Bq, dev)
        if images.dim() != 4 or (feats is None and byt is None and images.shape[1] != 3) or token_ids.dim() != 2 or token_ids.shape[0] != Bq or (not soft and targets.shape != (Bq,)):
            raise RuntimeError(f"HipTrainer.{who}: expected images [B,3,H,W], token_ids [B,L], targets [B]"
                               + ("" if image_index is None else " with B questions"))
        # fine-tuning: requires_grad and the parts' modes, resolved on every step (finetune.Plan; None: the plain step)
        plan = self.model._finetune_plan(self.model._param_list(), False, True)
        win_mask = None if plan is None or all(plan.trainable) else tuple(plan.trainable)
        if self.pending and win_mask != self._win_mask:    # (ahead of the index copy and the range table: nothing has gone out yet)
            raise RuntimeError(f"HipTrainer.{who}: the trainable set changed inside a gradient-accumulation window ({self.pending} "
                               "micro-batch(es) pending); close the window with step() or drop it with discard_accumulated() first")
        if feats is not None:                              # host checks, ahead of the image index's copy / range read: nothing has gone out yet
            if plan is None or plan.cnn_trains:
                raise RuntimeError(f"HipTrainer.{who}: ImageFeatures stand in for a frozen image encoder: call "
                                   "model.image_encoder.requires_grad_(False)")
            self.model._check_features(feats, f"HipTrainer.{who}")
        kv_index = None
        if image_index is not None:
            kv_index = self._device_index(image_index, images.shape[0], Bq, dev)
        if attention_mask is not None and not (isinstance(attention_mask, torch.Tensor) and attention_mask.device == dev
                                               and attention_mask.shape == token_ids.shape):
            raise RuntimeError(f"HipTrainer.{who}: `attention_mask` must be a [B,L] tensor on {dev} (or None)")
        eng._pos_enc(token_ids.shape[1])                   # (a question that is too long is refused here, before anything is counted)
        # the kernels read raw pointers: enforce the dtypes / contiguity VQAModel.forward enforces (vqa_model.py drop-in)
        if byt is not None:
            images = byt                                   # the bytes go to the engine as they are (and to the graph's static buffer)
        elif feats is None:
            images = images.contiguous().float()
        token_ids = token_ids.contiguous().long()
        if not soft:
            targets = targets.contiguous().long()
        maskf = None if attention_mask is None else attention_mask.contiguous().float()
        self._set_mask(None if plan is None else plan.trainable)
        # ---- bookkeeping: from here on the step counts
        if feats is None and (plan is None or plan.cnn_trains):      # this step's AdamW writes the image encoder: cached features go stale
            self.model._feat_epoch += 1
        eng.count_step(plan.modes if plan is not None else (True, True, True, True), runs_cnn=feats is None)
        if closing:
            self.calls += 1
        return dict(win_mask=win_mask, features=feats is not None, images=images, token_ids=token_ids, maskf=maskf, targets=targets, soft=soft, bce=bce,
                    metrics=metrics, kv_index=kv_index, plan=plan, group_values=group_values)

    def _write_groups(self, values):
        """The parameter groups' effective values go to their device block when they differ from what it holds: an eager one-thread
        launch on the current stream, ahead of the AdamW launch (or the replay) that reads the block."""
        if values is None or values == self._group_written:
            return
        scales, wds = values
        F = ctypes.c_float * len(scales)
        call("vqa_group_hyper_set", ptr(self._group_block), len(scales), F(*scales), F(*wds))
        self._group_written = values

    def _enqueue(self, c, state=None, closing=True):
        """The device half of a step: every launch, in the order the step has always issued them; returns (loss, logits fp32).
        state (step_graphed, while the step is being captured): the device step-state block.  The dropout seeds are then the flagged
        words that point into it, AdamW is the _dev entry that reads its hyper-parameters from it, and the bf16 operand copy the
        previous AdamW launch wrote is trusted (step_graphed re-casts it eagerly before a replay when the host check fails).
        closing=False (accumulate): the launches up to and including the backward, into the window's gradient; the step that closes
        a window adds its own gradient and runs the tail on the sum.  With no window open this is the step as it has always been."""
        eng = self.engine
        images, token_ids, maskf, targets, metrics, kv_index, plan = (c[k] for k in ("images", "token_ids", "maskf", "targets", "metrics",
                                                                                      "kv_index", "plan"))
        soft, bce = c["soft"], c["bce"]
        dev = self.G.device
        if state is None:                          # (a captured step: step_graphed wrote the block eagerly, beside the step state)
            self._write_groups(c["group_values"])
        if self.pending == 0:                      # the first call of a window, or a plain step
            self.G.zero_()
            self._scal.zero_()
        else:                                      # inside a window: this call's loss alone; the bad-target word accumulates
            self.loss.zero_()
        if state is not None:
            eng._wsrc_fresh = eng.adamw_copy_target() is not None
        elif self._copy_sig is not None and eng.adamw_copy_target() is not None and self._copy_sig == self._param_sig():
            eng._wsrc_fresh = True                 # (one-shot, consumed by the begin_step of the forward below)
        eng._seed_src = None if state is None else state.data_ptr() + SG.SEED_STEP_OFFSET
        # the guard: a train-mode CNN forward overwrites the BatchNorm running buffers long before the gradient is judged
        # (a window: saved ahead of its FIRST such forward only, so the restore undoes every micro-batch's updates together)
        running = self._win_saved
        if running is None and self._guard is not None and not c["features"] and (plan is None or plan.modes[0]):
            running = eng.running_buffers()
            call("vqa_buffers_save", ptr(running[0]), running[1], ptr(running[2]))
        try:
            if c["features"]:
                logits, _, tape = eng.forward_features(images, token_ids, maskf, True, False, need_tape=True, lowp_logits=True, kv_index=kv_index,
                                                       plan=plan, counted=True)
            else:
                logits, _, tape = eng.forward(images, token_ids, maskf, True, False, need_tape=True, lowp_logits=True, kv_index=kv_index, plan=plan,
                                              counted=True)
        finally:
            eng._seed_src = None
        B, N = logits.shape
        # the loss kernel reads the logits in the compute dtype, writes d logits in it and leaves the fp32 logits the caller gets:
        # the same values as logits.float() -> loss -> d logits.to(bf16), two elementwise launches less between forward and backward
        lowp = logits.dtype != torch.float32
        logits_f = torch.empty((B, N), device=images.device, dtype=torch.float32) if lowp else logits
        dlogits = torch.empty((B, N), device=images.device, dtype=logits.dtype)
        ce_ws = torch.empty((B,), device=images.device, dtype=torch.float32)
        if soft:                                           # the challenge accuracy rides in the same launch (counts + acc)
            acc = None if metrics is None else metrics._fused_acc(dev)
            call("vqa_bce_soft" if bce else "vqa_cross_entropy_soft", dt(logits), ptr(logits), ptr(targets.ids), ptr(targets.weights),
                 targets.ids.shape[1], ptr(self.loss), ptr(dlogits), ptr(logits_f) if lowp else None, B, N, 1.0, ptr(self.bad_step), ptr(ce_ws),
                 None if acc is None else ptr(targets.counts), ptr(acc))
        elif self._loss_opts:                              # VQAAccuracy's counters ride in the same launch (kept rows only)
            fused = metrics is not None and hasattr(metrics, "_buf")
            call("vqa_cross_entropy_opts", dt(logits), ptr(logits), ptr(targets), ptr(self.loss), ptr(dlogits), ptr(logits_f) if lowp else None,
                 B, N, 1.0, ptr(self.bad_step), ptr(ce_ws), ptr(self.class_weight), self.ignore_index or 0, int(self.ignore_index is not None),
                 self.label_smoothing, ptr(metrics._buf(dev)) if fused else None, ptr(self._empty))
        else:
            fused = False
            call("vqa_cross_entropy", dt(logits), ptr(logits), ptr(targets), ptr(self.loss), ptr(dlogits), ptr(logits_f) if lowp else None, B, N, 1.0,
                 ptr(self.bad_step), ptr(ce_ws))           # per-row loss terms, folded in row order (bit-reproducible)
        if closing:
            self.reducer.reduce_aux(self.bad_step)         # every rank must skip the update of a step ANY rank rejects
        if metrics is not None and not soft and not fused:
            metrics.update(logits_f, targets)
        eng.backward(tape, dlogits, self.G, on_segment=self.reducer.on_segment if (closing and self.reducer.active) else None)
        if not closing:                            # no collective, no norm, no AdamW: the parameters and the operand copy stay as they are
            self.pending, self._win_mask, self._win_saved = self.pending + 1, c["win_mask"], running
            return self.loss, logits_f
        gscale = self.reducer.finish()
        n = self.pending + 1                       # the update takes the mean of the window's n per-batch mean gradients
        if n > 1:
            gscale = 1.0 / (self.world * n)
        self._norm_div = self.world * n
        self.pending, self._win_mask, self._win_saved = 0, None, None
        b1, b2 = self.betas
        if state is not None:                      # the captured form: hyper-parameters, step number and gscale come from the block
            hyper, ema_args, sfx = (ptr(state),), (() if self.ema is None else (ptr(self.ema),)), "_dev"
        else:
            hyper, sfx = (self.lr, b1, b2, self.eps, self.wd, self.calls), ""
            ema_args = () if self.ema is None else (ptr(self.ema), float(self.ema_decay), int(bool(self.ema_warmup)))
        tail = () if state is not None else (float(self.max_norm), gscale)
        # the monitor: a due step keeps the weights of before the update (never inside a capture: step_graphed hands due steps here)
        due = self.monitor is not None and state is None and self.monitor.due(self.calls)
        if due:
            self.monitor.snapshot(self.model._param_entries, self.model._flat)
        # the guard: the norm's fold block turns the (reduced) bad-target count and its own verdict into the effective skip word and
        # keeps bad_targets; AdamW reads that word and counts the skipped launches of either kind in an array of the trainer's own
        if self._guard is None:
            gsfx, gtail, skip, skipped = "", (), self.bad_step, self._bad
        else:
            gsfx, gtail = "_guard", (ptr(self.bad_step), ptr(self._guard), ptr(self._bad), ptr(self._guard[1:]))
            skip, skipped = self._guard, self._adam_skipped
            self._last_ws = ce_ws
        if self._ranges is None:
            call("vqa_sumsq" + gsfx, ptr(self.G), self.G.numel(), ptr(self.sumsq), *gtail)
            call(("vqa_adamw_ema" if ema_args else "vqa_adamw") + sfx, ptr(self.model._flat), ptr(self.G), ptr(self.m), ptr(self.v), self.G.numel(),
                 *hyper, ptr(self.sumsq), *tail, ptr(skip), ptr(skipped), ptr(eng.adamw_copy_target()), *ema_args)
        else:                                      # frozen parameters: only the trainable ranges are read and written
            table, R, n, fidx, nf, garr = self._ranges
            # parameter groups: the same launch with every range's group and the block of the groups' values behind its arguments
            entry, gargs = ("vqa_adamw_ranges", ()) if garr is None else ("vqa_adamw_groups", (ptr(garr), ptr(self._group_block)))
            call("vqa_sumsq_ranges" + gsfx, ptr(self.G), ptr(table), R, n, ptr(self.sumsq), *gtail)
            call(entry + ("_ema" if ema_args else "") + sfx, ptr(self.model._flat), ptr(self.G), ptr(self.m), ptr(self.v),
                 ptr(table), R, n, *hyper, ptr(self.sumsq), *tail, ptr(skip), ptr(skipped), ptr(self._lag), ptr(fidx), nf,
                 ptr(eng.adamw_copy_target()), *ema_args, *gargs)
        if running is not None:                    # a skipped step never happened: the BatchNorm buffers go back (nothing when the word is 0)
            call("vqa_buffers_restore", ptr(running[0]), running[1], ptr(running[2]), ptr(self._guard))
        if due:                                    # behind the step's last launch: three reads of what it left
            self.monitor.record(self.calls, gscale, self._mask, self.model._flat, grad=self.G)
        # the kernel wrote the bf16 operand copy too: the next step() skips the cast launch if nothing touched the parameters in between
        self._copy_sig = self._param_sig() if eng.adamw_copy_target() is not None else None
        return self.loss, logits_f

    # ---- the captured step
    def step_graphed(self, images, token_ids, attention_mask, targets, metrics=None, image_index=None):
        """step() replayed from a captured HIP graph: same arguments, checks, errors and return value, bit-equal results, and the
        host enqueues three things per step instead of every launch.  The first two calls for a key (stepgraph.step_key: shapes and
        dtypes of the inputs, mask / index present, K of SoftTargets, features or images, the fine-tuning plan, the loss and its
        options, EMA on or off, the non-finite guard on or off, the `metrics` object, the parameter / operand-copy / packed-operand / range-table buffers) are eager steps; the third
        captures the launches of _enqueue on static copies of the inputs and replays them; later calls copy the inputs in, write the
        device step-state block (vqa_step_state_set: this step's seed word and Adam step number, and lr / betas / eps / wd /
        max_norm / ema_decay / ema_warmup as they read NOW -- changing them never re-captures; the parameter groups' lr_scale and
        weight_decay likewise, through vqa_group_hyper_set when one of them changed) and replay.  A torch-side write to
        the parameters since the last AdamW launch (load_state_dict, a torch optimizer, ema_weights(), an eager step() in between
        leaves the copy fresh) is answered by an eager vqa_convert ahead of the replay, as step() would cast.
        The returned logits (and the loss, as with step()) are the graph's static buffers: valid until the next call with the same
        key.  check(), t, grad_norm(), ema_*, params_changed() and `metrics` work as with step().
        RuntimeError before any launch: more than one rank or force_reducer=True (no collectives inside a graph), a current stream
        that is capturing, a call inside ema_weights()."""
        self._refuse_open("step_graphed")
        if self.reducer.active:
            raise RuntimeError("HipTrainer.step_graphed: a captured step holds no collectives -- it runs in a world of one rank "
                               "without force_reducer; use step()")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("HipTrainer.step_graphed: the current stream is capturing; a graph is not captured inside another")
        c = self._prologue("step_graphed", images, token_ids, attention_mask, targets, metrics, image_index)
        self._norm_div = self.world                        # a captured step is a window of one (gscale 1 / world): grad_norm() as with step()
        if self.monitor is not None and self.monitor.due(self.calls):
            return self._enqueue(c)                        # a due step runs eagerly and records; the graphs never see it
        eng = self.engine
        eng.ensure_operand_copy()                          # (its address is part of the key from the first call on)
        key = SG.step_key(features=c["features"], images=c["images"], token_ids=c["token_ids"], attention_mask=c["maskf"],
                          image_index=c["kv_index"], targets=c["targets"], plan=c["plan"], loss_kind=self.loss_kind,
                          loss_opts=(self.label_smoothing, self.ignore_index, None if self.class_weight is None else self.class_weight.data_ptr()),
                          ema=self.ema is not None, metrics=metrics, flat_ptr=self.model._flat.data_ptr(), wsrc_ptr=eng.wsrc.data_ptr(),
                          table_id=SG.table_id(None if self._ranges is None else self._ranges_gen, None if self._pg is None else self._pg.key(),
                                               guard=self._guard is not None))
        g = self._graphs.pop(key, None)
        if g is not None and g[4] != eng._wt_gen:
            # the engine laid its packed backward operands out anew since the capture (another trainable set needed more of them):
            # the graph holds the old buffer's address.  Dropped like an evicted one, and captured again as soon as the engine allows
            torch.cuda.synchronize()
            g = None
            self._graph_seen[key] = 2
        if g is None:
            seen = self._graph_seen.get(key, 0)
            if seen < 2 or not eng.operands_settled():                                   # a real step and the warm-up: _wt_plan, wsrc, one-time kernel attributes, caches
                if len(self._graph_seen) > 4 * max(1, self.model.graph_max_shapes):
                    self._graph_seen.clear()
                self._graph_seen[key] = seen + 1
                return self._enqueue(c)
        if self._state is None:
            self._state = torch.zeros(SG.STATE_BYTES // 4, device=self.G.device, dtype=torch.int32)
        # the operand copy: the graph trusts the one the previous AdamW launch wrote; when the host cannot vouch for it, cast now
        if eng.adamw_copy_target() is not None and not (self._copy_sig is not None and self._copy_sig == self._param_sig()):
            eng.refresh_operand_copy()
        b1, b2 = self.betas
        ema_on = self.ema is not None
        call("vqa_step_state_set", ptr(self._state), self.calls, SG.seed_step(self._seed_rank(), eng.seed_base, eng.step_id),
             float(self.lr), float(b1), float(b2), float(self.eps), float(self.wd), float(self.max_norm), 1.0,
             float(self.ema_decay) if ema_on else 0.0, int(bool(self.ema_warmup)) if ema_on else 0)
        self._write_groups(c["group_values"])
        if g is None:
            g = self._capture_step(c)
            self._graph_seen.pop(key, None)
        self._graph_put(key, g)                            # (re)inserted at the young end of the LRU order
        graph, static, out = g[:3]
        for name, dst in static.items():
            src = c[name]
            for d_, s_ in zip(dst, self._tensors_of(src)):
                d_.copy_(s_)
        graph.replay()
        if self._guard is not None:
            self._last_ws = g[3][3]
        # the captured AdamW wrote the operand copy: vouch for it as step() does
        self._copy_sig = self._param_sig() if eng.adamw_copy_target() is not None else None
        return out

    def _seed_rank(self):
        eng = self.engine
        if eng.seed_rank is None:
            eng.seed_rank = dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0
        return eng.seed_rank

    @staticmethod
    def _tensors_of(x):
        """The tensors of one step input, in a fixed order: a tensor itself, the fields of SoftTargets that are present, the uint8
        data of a ByteImages."""
        if _is_soft(x):
            return [t for t in (x.ids, x.weights, x.counts) if t is not None]
        if K.is_byte_images(x):
            return [x.data]
        return [x]

    def _capture_step(self, c):
        """Capture _enqueue on static copies of the inputs; returns (graph, {input name: static tensors}, (loss, logits), held,
        generation of the engine's packed operands)."""
        static, cc = {}, dict(c)
        for name in ("images", "token_ids", "maskf", "kv_index", "targets"):
            if c[name] is None:
                continue
            copies = [t.detach().clone() for t in self._tensors_of(c[name])]
            static[name] = copies
            if _is_soft(c[name]):
                it = iter(copies)
                cc[name] = type(c[name])(*(None if f is None else next(it) for f in (c[name].ids, c[name].weights, c[name].counts)))
            elif K.is_byte_images(c[name]):                # a uint8 static buffer; mean / std are part of the key (the table is baked in)
                cc[name] = type(c[name])(copies[0], c[name].mean, c[name].std)
            else:
                cc[name] = copies[0]
        sig = self._copy_sig
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self._enqueue(cc, state=self._state)
        self._copy_sig = sig                               # (nothing ran yet: the replay below sets it)
        eng = self.engine                                  # per-step operands the capture left behind live in the graph's pool: an
        eng._wt, eng._accbuf = {}, None                    # eager step must not pick them up (begin_step / _acc rebuild their own)
        self.graph_captures += 1
        # held: the static inputs' owners, the tracker whose counters the graph writes, the range table it reads
        # (and, under the guard, the per-row loss terms nonfinite_report() reads)
        return graph, static, out, (cc, c["metrics"], self._ranges, self._last_ws), self.engine._wt_gen

    def _graph_put(self, key, g):
        cap = max(1, int(self.model.graph_max_shapes))
        if len(self._graphs) >= cap:
            torch.cuda.synchronize()                       # an evicted graph's private pool must outlive its last replay in flight
            while len(self._graphs) >= cap:
                self._graphs.pop(next(iter(self._graphs)))
        self._graphs[key] = g

    def _device_index(self, image_index, U, N, dev):
        """int32 [N] device copy of a checked image index (VQAModel._image_index rules; None -> the implied index)."""
        on_dev = isinstance(image_index, torch.Tensor) and image_index.device == dev
        idx = self.model._image_index(image_index, U, N, dev if on_dev else torch.device("cpu"))
        if idx is None:
            return self.model._implied_index(U, N, dev)
        if not on_dev:                                     # checked on the host: a pinned copy goes out without a sync
            idx = idx.pin_memory().to(dev, non_blocking=True)
        return idx

    # ---- the weight average (ema_decay is not None)
    def _need_ema(self, what):
        if self.ema is None:
            raise RuntimeError(f"HipTrainer.{what} needs the weight average: construct the trainer with ema_decay=<float in [0, 1]>")
        return self.ema

    def ema_state_dict(self):
        """model.state_dict() with every parameter replaced by a clone of its slice of the average (same keys, shapes and dtypes: it loads
        with strict=True into this VQAModel and into the reference's).  Buffers -- the BatchNorm running statistics among them -- are the
        live model's: they are running averages already."""
        return EMA.state_dict(self.model, self._need_ema("ema_state_dict"))

    def load_ema_state_dict(self, sd):
        """The inverse of ema_state_dict(), for resuming: the parameter entries of `sd` become the average; buffer keys are ignored.
        KeyError for a missing parameter, ValueError for a shape mismatch (nothing is written then)."""
        EMA.load_state_dict(self.model, self._need_ema("load_ema_state_dict"), sd)
        self._ema_cnn_stamp = None

    # ---- the whole trainer state (trainer_state.py): stop a run and continue it
    def state_dict(self):
        """Everything a run needs to continue, as a torch.optim.AdamW state dict plus one block: {"state": {i: {"step", "exp_avg",
        "exp_avg_sq"}}, "param_groups": [...], "hip_trainer": {...}} -- plain containers and CPU tensors, so torch.save and
        torch.load(weights_only=True) carry it, and it fits the `optimizer_state_dict` slot of the reference's checkpoints.  The
        moments of every parameter in the Parameter's own shape (a never-updated one: zeros, step 0); `step` of parameter j is
        calls - skipped steps - lag[j], the number the AdamW kernels form; one param group (model.parameters() order) without
        trainer groups, one per trainer group with lr * lr_scale and the group's effective decay otherwise, with the keys the installed
        torch.optim.AdamW writes, so the dict loads into a torch.optim.AdamW over the same parameters or groups.  The block holds what
        torch has no place for: the parameter name of every index, calls and the counters check() reads, the frozen-time lags and
        their classes, the hyper-parameters and the groups' live values, the weight average, ema_decay / ema_warmup and the dropout
        stream (the engine's seed_base and step_id).  The model's own state (weights, BatchNorm buffers) is model.state_dict()'s.
        Under the non-finite guard the block also holds "nonfinite": {"mode", "since", "ever", "unchecked"} -- the guard's counters;
        "skipped_ever" stays the count of launches that were no step, for whichever reason.  Without the guard: the keys as ever.
        One host synchronisation.  RuntimeError inside ema_weights()."""
        if self._ema_swapped:
            raise RuntimeError("HipTrainer.state_dict inside ema_weights(): the model holds the averaged weights; leave the block first")
        self._refuse_open("state_dict")
        if self._guard is None:
            bad, nf = [int(x) for x in self._bad.tolist()], {}
        else:                                              # (one read: bad_targets, the launches that were no step, the guard's counters)
            w = [int(x) for x in torch.cat([self._bad[:2], self._ever(), self._guard[1:]]).tolist()]
            bad = w[:3]
            nf = dict(nonfinite=self.nonfinite, nonfinite_skipped=(w[3], w[4], w[4] - self._nf_checked))
        eng = self.engine
        return TS.export(self.model._param_entries, [n for n, _ in self.model.named_parameters()], self.m, self.v, calls=self.calls,
                         skipped_ever=bad[2], bad_targets=bad[:2], **nf, empty=int(self._empty.item()), lag=self._lag.tolist(),
                         lag_class=self._lag_class, ever_frozen=self._ever_frozen, lr=self.lr, betas=self.betas, eps=self.eps,
                         weight_decay=self.wd, max_grad_norm=self.max_norm, groups=self.param_groups, ema=self.ema,
                         ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, seed_base=eng.seed_base, step_id=eng.step_id)

    def load_state_dict(self, sd):
        """The inverse of state_dict(), and the way in for a dict a torch.optim.AdamW wrote.  Everything is validated on the host
        first: a ValueError leaves the trainer as it was.
        With the "hip_trainer" block (an exact resume; load the model's state_dict first): parameters are matched by name; the
        moments, the average, calls and the counters, the lags and their classes, lr / betas / eps / weight decay / max_grad_norm
        (live attributes again), the groups' live values and the engine's seed_base / step_id are restored, and the run continues
        bit for bit.  ValueError for an unknown version, a missing or unknown parameter name, a wrong shape, groups whose membership
        differs from this trainer's, and an average in the dict when this trainer was built without ema_decay.  A trainer WITH
        ema_decay given a dict without an average restarts the average from the model's current weights, as its constructor does, and
        keeps its own ema_decay / ema_warmup.  The non-finite guard's counters are restored into a guarded trainer (zero when the
        dict has none) and ignored by an unguarded one; the mode stays the constructor's.
        Without the block (torch.optim.AdamW.state_dict()): only the moments and the step numbers are read.  Index i is the i-th
        parameter of the concatenated param_groups: model.parameters() order for the one group of a trainer without groups; with
        trainer groups the dict's group sizes must equal theirs.  An index without state gets zero moments and step 0; calls becomes
        the largest step, no step counts as skipped, and parameters whose steps differ get lags (the range kernels honour them).  A
        trainer without groups takes lr, betas, eps and weight_decay from the one group, as torch does; a trainer with groups keeps
        its live values.  The counters of check(), the average and the dropout stream keep their values.  ValueError for amsgrad,
        maximize or decoupled_weight_decay=False.
        After either load the bf16 operand copy is re-cast at the next step, the optimizer's range table and the groups' device block
        are rebuilt, and every captured step graph is dropped: step_graphed behaves like a fresh trainer's.  One host
        synchronisation.  RuntimeError inside ema_weights()."""
        if self._ema_swapped:
            raise RuntimeError("HipTrainer.load_state_dict inside ema_weights(): the model holds the averaged weights; leave the block first")
        self._refuse_open("load_state_dict")
        r = TS.load(self.model._param_entries, [n for n, _ in self.model.named_parameters()], sd, self.m, self.v, self.ema,
                    self.param_groups)
        dev = self.G.device
        self.calls = r["calls"]
        self._lag.copy_(torch.tensor(r["lag"], dtype=torch.int32))
        self._lag_class = list(r["lag_class"])
        self._ever_frozen = r["ever_frozen"]
        self._ever().fill_(r["skipped_ever"])
        if r["bad_targets"] is not None:
            self._bad[:2].copy_(torch.tensor(r["bad_targets"], dtype=torch.int32))
            self._empty.fill_(r["empty"])
        if self._guard is not None:                        # (a dict written without the guard: the new counters start at zero)
            nf = r["nonfinite"] or {"since": 0, "ever": 0, "unchecked": 0}
            self._guard.copy_(torch.tensor([0, nf["since"], nf["ever"]], dtype=torch.int32))
            self._nf_checked = nf["ever"] - nf["unchecked"]
            self._nf_reported = nf["ever"]
            self._last_ws = None
        for attr, key in (("lr", "lr"), ("betas", "betas"), ("eps", "eps"), ("wd", "weight_decay"), ("max_norm", "max_grad_norm"),
                          ("ema_decay", "ema_decay"), ("ema_warmup", "ema_warmup")):
            if r[key] is not None:
                setattr(self, attr, r[key])
        if r["group_values"] is not None:
            for g, (scale, wd) in zip(self.param_groups, r["group_values"]):
                g["lr_scale"], g["weight_decay"] = scale, wd
        if r["ema"] == "loaded":
            self._ema_cnn_stamp = None
        elif r["ema"] == "restart":
            with torch.no_grad():
                self.ema.copy_(self.model._flat)
            self._ema_cnn_stamp = self._cnn_stamp()
        if r["rng"] is not None:
            self.engine.seed_base, self.engine.step_id = r["rng"]["seed_base"], r["rng"]["step_id"]
        self._copy_sig = None
        self._group_written = None
        self._mask = None
        self._ranges = None
        self.reducer.set_trainable(None)                   # (with the mask: the next step's _set_mask narrows it again where parts are frozen)
        if dev.type == "cuda":
            torch.cuda.synchronize()                       # a dropped graph's private pool must outlive its last replay in flight
        self._graphs.clear()
        self._graph_seen.clear()

    @contextlib.contextmanager
    def ema_weights(self):
        """`with trainer.ema_weights():` -- the model holds the averaged weights inside the block (validation with the same model object:
        eager eval forward, forward_graphed, predict, predict_topk, encode_images + answer, graphs captured earlier included) and its
        own weights again afterwards, also when the block raises.  The contents of model._flat and self.ema are exchanged through torch
        ops and exchanged back: parameters, average and both moments have their earlier bits after the block, an ImageContext from one
        side is refused on the other, and the next step() re-casts the bf16 operand copy.  step() inside the block raises RuntimeError.
        ImageFeatures stay valid across the block as long as nothing wrote the image encoder since the average was made (the average
        of a frozen parameter is the parameter); otherwise they are refused like the contexts."""
        ema = self._need_ema("ema_weights")
        if self._ema_swapped:
            raise RuntimeError("HipTrainer.ema_weights() is not re-entrant")
        # (getattr: tests/test_ema_ref_cpu.py makes its trainer with __new__, without the constructor's attributes)
        made = getattr(self, "_ema_cnn_stamp", None)
        with EMA.swapped(self.model, ema, keeps_cnn=made is not None and made == self._cnn_stamp()):
            self._ema_swapped = True
            try:
                yield self.model
            finally:
                self._ema_swapped = False

    def _cnn_stamp(self):
        m = self.model
        return (m._feat_epoch, m._feat_version() - m._feat_excused)

    def params_changed(self):
        """Tell the trainer that the parameters were written behind torch's back (through `.data`, a raw pointer, another C-ABI call):
        the next step re-casts the bf16 operand copy instead of trusting the one the last AdamW launch wrote.  Writes through torch
        (load_state_dict, optimizers, in-place ops on the Parameters or the flat buffer) are noticed without this call."""
        self._copy_sig = None

    def _param_sig(self):
        """Version counters of the flat buffer and of every Parameter view: any torch-side write (load_state_dict, an optimizer, .copy_)
        bumps one of them.  (The C-ABI kernels do not: the fused AdamW launch is the one writer this class accounts for itself.)"""
        return (self.model._flat.data_ptr(), self.model._flat._version) + tuple(p._version for p in self.model._param_list())

    @property
    def t(self) -> int:
        """Adam's step number = optimizer updates actually applied (one host sync; the kernels never need it from the host).  Under
        the non-finite guard both kinds of skipped step are left out."""
        return self.calls - int(self._ever())

    def _ever(self):
        """The device count of launches that were no step: AdamW's own array under the non-finite guard, else _bad[2]."""
        return self._bad[2:3] if self._guard is None else self._adam_skipped[2:3]

    # ---- the non-finite guard (nonfinite="skip" | "raise")
    def _need_guard(self, what):
        if self._guard is None:
            raise RuntimeError(f'HipTrainer.{what} needs the non-finite guard: construct the trainer with nonfinite="skip" or "raise"')

    def skipped_nonfinite(self):
        """(steps skipped for a non-finite gradient since the last call, ... ever); one host sync.  Bad-target steps are not among
        them: check() reports those."""
        self._need_guard("skipped_nonfinite")
        since, ever = (int(x) for x in self._guard[1:].tolist())
        if since:
            self._guard[1:2].zero_()
        return since, ever

    def nonfinite_report(self):
        """What blew up in the step just skipped; one host sync.  None when the last step's gradient was finite (or the step was a
        bad-target step: check() speaks for those), else a NonFiniteReport(step, loss, parameters, rows): the step's call number
        (`calls`), its loss, (name, non-finite elements, numel) in layout order for every trainable parameter whose gradient holds a
        NaN or inf (vqa_nonfinite_scan over the flat gradient, launched here and never inside a step), and the int64 indices of the
        batch rows whose per-row loss term is not finite.  The gradient and the loss terms are the last step's: call this before
        the next step.  RuntimeError when a non-finite step has gone by unreported and a later step has overwritten its gradient."""
        self._need_guard("nonfinite_report")
        if self._last_ws is None:                          # no step yet (or a state was loaded since)
            return None
        entries = self.model._param_entries
        if self._scan is None or self._scan[1].device != self.G.device:
            table = torch.tensor([[e.offset, e.offset + e.numel] for e in entries], dtype=torch.int64).to(self.G.device)
            self._scan = (table, torch.zeros(len(entries), device=self.G.device, dtype=torch.int32))
        table, counts = self._scan
        counts.zero_()
        call("vqa_nonfinite_scan", ptr(self.G), ptr(table), len(entries), ptr(counts))
        rows = (~torch.isfinite(self._last_ws)).to(torch.int32)
        w = torch.cat([self._scal, self._guard, counts, rows]).tolist()      # the one device-to-host read
        loss, bad_rows, word, ever = struct.unpack("f", struct.pack("i", w[0]))[0], w[1], w[2], w[4]
        counts, rows = w[5:5 + len(entries)], w[5 + len(entries):]
        unreported, self._nf_reported = ever > self._nf_reported, ever
        if word == 0 or bad_rows != 0:
            if unreported:
                raise RuntimeError("HipTrainer.nonfinite_report: a step was skipped for a non-finite gradient, but a later step has "
                                   "overwritten its gradient; call nonfinite_report() right after the step, before the next one")
            return None
        mask = self._mask
        params = [(e.name, n, e.numel) for j, (e, n) in enumerate(zip(entries, counts)) if n and (mask is None or mask[j])]
        # (self.calls is that step's call number: no later step has run, or the branch above would have been taken)
        return NonFiniteReport(self.calls, loss, params, torch.tensor([i for i, r in enumerate(rows) if r], dtype=torch.int64))

    def tensor_stats(self, kinds=("grad", "param")):
        """Per-parameter statistics of the trainer's flat buffers as they are NOW, between steps: one vqa_tensor_stats launch per kind
        and one device-to-host copy; returns a monitor.StatsRecord (step = `calls`) whose other fields are None.  kinds out of "grad"
        (`G`: the last update's gradient, or an accumulating window's sum once it is closed; norm and absmax scaled like
        grad_norm()), "param" (model._flat), "moment1" / "moment2" (Adam's m and v) and "ema" (the weight average; RuntimeError
        without ema_decay).  ValueError for "update" -- there is no snapshot to compare with; a monitored step records it --, an
        unknown kind, a repeat or an empty selection.  RuntimeError inside ema_weights() and while an accumulation window is open.
        Works with or without a monitor and does not touch its ring."""
        kinds = MON.check_now_kinds(kinds)
        if self._ema_swapped:
            raise RuntimeError("HipTrainer.tensor_stats inside ema_weights(): the model holds the averaged weights; leave the block first")
        self._refuse_open("tensor_stats")
        src = {"grad": lambda: self.G, "param": lambda: self.model._flat.detach(), "moment1": lambda: self.m, "moment2": lambda: self.v,
               "ema": lambda: self._need_ema('tensor_stats("ema")')}
        bufs = [src[k]() for k in kinds]
        entries = self.model._param_entries
        if self._stats_tab is None or self._stats_tab[0].device != self.G.device:
            self._stats_tab = K.stats_table(MON.layout_ranges(entries), self.G.device)
        out = torch.empty((len(kinds), len(entries), 4), device=self.G.device, dtype=torch.int32)
        for i, b in enumerate(bufs):
            K.tensor_stats(b, self._stats_tab, out=out[i])
        host = out.cpu()
        mask = self._mask
        trainable = torch.ones(len(entries), dtype=torch.bool) if mask is None else torch.tensor(mask, dtype=torch.bool)
        return MON.make_record({k: host[i] for i, k in enumerate(kinds)}, self.calls, [e.name for e in entries],
                               torch.tensor([e.numel for e in entries], dtype=torch.int64), trainable, 1.0 / self._norm_div)

    def grad_norm(self) -> torch.Tensor:
        """The global gradient norm the last update clipped: sqrt(sumsq) / (world * n), n the micro-batches of its window (1: a plain step)."""
        return self.sumsq[:1].sqrt() / self._norm_div

    def check(self):
        """Host-side error check (one sync; call it per logging interval, not per step): raises like nn.CrossEntropyLoss does
        (training/train.py:120) if any step since the last check saw a target outside [0, num_answers).  With loss options it also
        raises ValueError if any step's batch had zero total weight (see step()).  With nonfinite="raise" it raises FloatingPointError
        for the steps skipped for a non-finite gradient since the last check (after the IndexError, when both are due); a non-finite
        skip never raises IndexError."""
        if self.nonfinite == "raise":                      # (one read for both)
            n, skipped, ever = (int(x) for x in torch.cat([self.bad_targets, self._guard[2:]]).tolist())
        else:
            (n, skipped), ever = (int(x) for x in self.bad_targets.tolist()), None
        if n:
            self.bad_targets.zero_()
            raise IndexError(f"{n} target(s) out of range [0, {self.model.num_answers}) since the last check: {skipped} step(s) were "
                             "skipped on every rank (parameters and optimizer state untouched; that step's loss and gradients are NaN)")
        if ever is not None and ever > self._nf_checked:
            k, self._nf_checked = ever - self._nf_checked, ever
            raise FloatingPointError(f"{k} step(s) since the last check had a non-finite gradient and were skipped on every rank "
                                     "(parameters, optimizer state and BatchNorm buffers untouched); nonfinite_report() right after "
                                     "such a step names the parameters and batch rows")
        if self._loss_opts:
            e = int(self._empty.item())
            if e:
                self._empty.zero_()
                raise ValueError(f"{e} step(s) since the last check had a batch of zero total weight (every target ignored, or every kept "
                                 "target of class weight 0): their loss is NaN and AdamW ran on a zero gradient")
