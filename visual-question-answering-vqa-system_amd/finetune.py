"""Fine-tuning with frozen parts: which parameters train, which mode each part runs in, and what the backward may skip.

Pure host logic (no GPU): the drop-in model resolves a `Plan` from `requires_grad` and the `.training` flags of its parts, the engine
reads it on the forward (BatchNorm / dropout per part, whether the CNN keeps a tape) and on the backward (which weight gradients and
which part of the data-gradient chain run), and HipTrainer turns the trainable set into a device table of ranges for the optimizer.
Parameter groups (HipTrainer(param_groups=...)) are resolved here too: which parameter belongs to which group, and the live values.
"""
from __future__ import annotations

import math
from bisect import bisect_right
from typing import Dict, List, Optional, Sequence, Tuple

from . import layout as LY

# the four top-level parts whose mode is read (VQAModel's children in the reference module tree)
PARTS = ("image_encoder", "text_encoder", "fusion", "answer_head")
STAGES = (1, 2, 3, 4)


def part_modes(model) -> Tuple[bool, bool, bool, bool]:
    """`.training` of image_encoder, text_encoder, fusion and answer_head.  A submodule whose mode differs from its part's
    (model.image_encoder.stage3.eval() alone) raises NotImplementedError naming it: the engine runs one mode per part."""
    modes = []
    for name in PARTS:
        part = getattr(model, name)
        mode = part.training
        for sub, mod in part.named_modules(prefix=name):
            if mod.training != mode:
                raise NotImplementedError(f"{sub} is in {'train' if mod.training else 'eval'} mode but {name} is in "
                                          f"{'train' if mode else 'eval'} mode: the HIP engine runs one mode per part "
                                          f"({', '.join(PARTS)}); set the whole part with {name}.train() / .eval()")
        modes.append(mode)
    return tuple(modes)


def slot_end(e: LY.Entry) -> int:
    return e.offset + (e.numel + LY.ALIGN - 1) // LY.ALIGN * LY.ALIGN


def trainable_ranges(param_entries: Sequence[LY.Entry], trainable: Sequence[bool], lag_class: Optional[Sequence[int]] = None,
                     group: Optional[Sequence[int]] = None) -> List[Tuple[int, int, int]]:
    """[(lo, hi, first parameter index)] over the parameters' 8-element slots: adjacent trainable parameters merged, except where
    their lag classes differ (parameters frozen during different steps have different Adam step counts) or, with `group` (the
    parameter group of every parameter), where their groups differ: a range has one lag and one group, those of its first parameter."""
    out: List[List[int]] = []
    prev = None
    for j, (e, t) in enumerate(zip(param_entries, trainable)):
        if not t:
            prev = None
            continue
        cls = (0 if lag_class is None else lag_class[j], 0 if group is None else group[j])
        if prev is not None and out and out[-1][1] == e.offset and prev == cls:
            out[-1][1] = slot_end(e)
        else:
            out.append([e.offset, slot_end(e), j])
        prev = cls
    return [tuple(r) for r in out]


def range_table_rows(ranges: Sequence[Tuple[int, int, int]]) -> List[List[int]]:
    """Rows {lo, hi, pos, lag index} of vqa_sumsq_ranges / vqa_adamw_ranges; pos = start of the range in their concatenation."""
    rows, pos = [], 0
    for lo, hi, j in ranges:
        rows.append([lo, hi, pos, j])
        pos += hi - lo
    return rows


def refine_classes(classes: Sequence[int], trainable: Sequence[bool]) -> List[int]:
    """Split every lag class by this step's trainable bit (parameters in one class were frozen during exactly the same steps)."""
    ids: Dict[Tuple[int, bool], int] = {}
    return [ids.setdefault((c, bool(t)), len(ids)) for c, t in zip(classes, trainable)]


class Plan:
    """What a taped forward / its backward do for one trainable set and one set of part modes.

    modes        (cnn, text, fusion, head) training flags
    cnn_trains   some image_encoder parameter trains (cached image features do not survive such a step)
    cnn_tape     the CNN keeps its activations (some image_encoder parameter trains, or the images require grad)
    cnn_low      lowest CNN level the data-gradient chain reaches: None (no CNN backward), 4 ... 1 (stage), 0 (stem)
    text         the text encoder's backward runs (some text_encoder parameter trains)
    fusion_bwd   the fusion backward runs (a fusion parameter trains, or a gradient must pass it on)
    need_dfused  the answer head hands a gradient to the fusion part
    need_dfeat / need_denc   the fusion part hands a gradient to the CNN / the text encoder
    features_grad   the gradient at the image features is itself the result (explain_plan): the fusion part hands it on although
                    no CNN backward follows
    no_param_grads  such a plan with nothing to train: the backward writes no parameter gradient at all, so its gradient buffer
                    is never read or written (the engine hands the parameter buffer in as a base address for frozen())
    """

    def __init__(self, param_entries: Sequence[LY.Entry], trainable: Sequence[bool], modes: Tuple[bool, bool, bool, bool],
                 images_grad: bool, features_grad: bool = False):
        self.modes = tuple(bool(m) for m in modes)
        self.trainable = tuple(bool(t) for t in trainable)
        self.images_grad = bool(images_grad)
        self.features_grad = bool(features_grad)
        self.no_param_grads = self.features_grad and not any(self.trainable)
        names = [e.name for e in param_entries]
        tr = dict(zip(names, self.trainable))

        def any_of(prefix):
            return any(t for n, t in tr.items() if n.startswith(prefix))

        self.cnn_trains = any_of("image_encoder.")        # an optimizer step under this plan writes the image encoder
        self.cnn_tape = self.cnn_trains or self.images_grad
        if self.images_grad or any_of("image_encoder.stem."):
            self.cnn_low: Optional[int] = 0
        else:
            self.cnn_low = next((s for s in STAGES if any_of(f"image_encoder.stage{s}.")), None)
        self.text = any_of("text_encoder.")
        self.need_dfeat = self.cnn_low is not None or self.features_grad
        self.need_denc = self.text
        self.fusion_bwd = any_of("fusion.") or self.need_dfeat or self.need_denc
        self.need_dfused = self.fusion_bwd
        # frozen flat slots (sorted, disjoint): a weight-gradient launch whose output lies entirely inside them is skipped
        spans = []
        for e, t in zip(param_entries, self.trainable):
            if not t:
                if spans and spans[-1][1] == e.offset:
                    spans[-1][1] = slot_end(e)
                else:
                    spans.append([e.offset, slot_end(e)])
        self._flo = [s[0] for s in spans]
        self._fhi = [s[1] for s in spans]

    def frozen(self, lo: int, n: int) -> bool:
        """True when the flat elements [lo, lo + n) belong to frozen parameters only."""
        i = bisect_right(self._flo, lo) - 1
        return i >= 0 and lo + n <= self._fhi[i]

    def cnn_levels(self) -> List[str]:
        """CNN segments whose backward runs, in backward order."""
        if self.cnn_low is None:
            return []
        out = [f"image_encoder.stage{s}" for s in (4, 3, 2, 1) if s >= max(self.cnn_low, 1)]
        if self.cnn_low == 0:
            out.append("image_encoder.stem")
        return out

    def key(self):
        return (self.modes, self.trainable, self.images_grad) + ((True,) if self.features_grad else ())


def resolve(param_entries, params, modes, images_grad, cache: Optional[dict] = None) -> Optional[Plan]:
    """The plan of a taped forward, or None for today's route (every parameter trains and every part runs in one mode).  `cache`
    keeps the last plan: a step whose trainable set and modes did not change costs one pass over `params`."""
    trainable = tuple(p.requires_grad for p in params)
    if all(trainable) and len(set(modes)) == 1:
        return None
    key = (tuple(modes), trainable, bool(images_grad))
    if cache is not None and cache.get("key") == key:
        return cache["plan"]
    plan = Plan(param_entries, trainable, modes, images_grad)
    if cache is not None:
        cache["key"], cache["plan"] = key, plan
    return plan


def explain_plan(param_entries) -> Plan:
    """The plan of the backward that stops at the image features (HipEngine.explain_route): every part in eval mode, nothing trains, no
    image gradient, no text-encoder backward -- and the fusion part still hands dfeat on.  No weight-gradient launch is issued under
    it (every slot is frozen) and the CNN keeps no tape."""
    return Plan(param_entries, (False,) * len(param_entries), (False,) * 4, False, features_grad=True)


# ---- parameter groups: a learning-rate scale and a weight decay per group of parameters (HipTrainer(param_groups=...))
GROUPS_MAX = 16          # VQA_GROUPS_MAX of include/vqa_hip.h: the entries of the device block vqa_group_hyper
RANGES_MAX = 512         # VQA_RANGES_MAX: the rows of the optimizer's range table


def check_group_value(x, what: str) -> float:
    """A group's lr_scale or weight decay: a finite float >= 0 (ValueError otherwise)."""
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x < 0:
        raise ValueError(f"{what} must be a finite number >= 0, got {x!r}")
    return float(x)


class ParamGroups:
    """The groups of one trainer, resolved against the model's parameter table on the host.

    groups     the live dicts {"names": tuple, "lr_scale": float, "weight_decay": float | None} (HipTrainer.param_groups): the two
               values may be changed between steps; weight_decay None follows the trainer's own
    group_of   the group index of every parameter, in layout order -- the groups' STRUCTURE (what key() returns)
    """

    def __init__(self, param_entries: Sequence[LY.Entry], params: Sequence, spec):
        names = [e.name for e in param_entries]
        index = {n: j for j, n in enumerate(names)}
        by_id = {id(p): j for j, p in enumerate(params)}
        if isinstance(spec, dict) or not hasattr(spec, "__iter__"):
            raise TypeError("param_groups must be a list of dicts {'params': ..., 'lr_scale': ..., 'weight_decay': ...}")
        group_of: List[Optional[int]] = [None] * len(names)
        self.groups: List[dict] = []
        for gi, g in enumerate(spec):
            if not isinstance(g, dict) or "params" not in g:
                raise TypeError(f"param_groups[{gi}] must be a dict with a 'params' entry")
            unknown = set(g) - {"params", "lr_scale", "weight_decay"}
            if unknown:
                raise TypeError(f"param_groups[{gi}]: unknown keys {sorted(unknown)} (per-group betas, eps and max_norm are not supported)")
            sel = g["params"]
            sel = [sel] if isinstance(sel, str) or not hasattr(sel, "__iter__") else list(sel)
            members: List[int] = []
            for s in sel:
                if isinstance(s, str):
                    if s.endswith("."):
                        hit = [j for j, n in enumerate(names) if n.startswith(s)]
                        if not hit:
                            raise KeyError(f"param_groups[{gi}]: the prefix {s!r} matches no parameter")
                    elif s in index:
                        hit = [index[s]]
                    else:
                        raise KeyError(f"param_groups[{gi}]: {s!r} is not a parameter of this model (a prefix ends in '.')")
                elif id(s) in by_id:
                    hit = [by_id[id(s)]]
                else:
                    raise ValueError(f"param_groups[{gi}]: a selector is neither a name nor a parameter of this model: {type(s).__name__}")
                members += hit
            if not members:
                raise ValueError(f"param_groups[{gi}] is empty")
            for j in members:
                if group_of[j] is not None:
                    raise ValueError(f"parameter {names[j]!r} is in two groups (param_groups[{group_of[j]}] and param_groups[{gi}])"
                                     if group_of[j] != gi else f"parameter {names[j]!r} is selected twice in param_groups[{gi}]")
                group_of[j] = gi
            wd = g.get("weight_decay")
            self.groups.append({"names": tuple(names[j] for j in sorted(members)),
                                "lr_scale": check_group_value(g.get("lr_scale", 1.0), f"param_groups[{gi}]: lr_scale"),
                                "weight_decay": None if wd is None else check_group_value(wd, f"param_groups[{gi}]: weight_decay")})
        rest = [j for j, gi in enumerate(group_of) if gi is None]
        if rest:                                           # the implicit last group: what no group selected
            for j in rest:
                group_of[j] = len(self.groups)
            self.groups.append({"names": tuple(names[j] for j in rest), "lr_scale": 1.0, "weight_decay": None})
        if not self.groups:
            raise ValueError("param_groups is empty")
        if len(self.groups) > GROUPS_MAX:
            raise ValueError(f"{len(self.groups)} parameter groups (the implicit last one included): at most {GROUPS_MAX}")
        self.group_of: Tuple[int, ...] = tuple(group_of)
        rows = len(trainable_ranges(param_entries, (True,) * len(names), None, self.group_of))
        if rows > RANGES_MAX:
            raise ValueError(f"these parameter groups split the parameters into {rows} ranges: the optimizer's table holds {RANGES_MAX}")

    def key(self) -> Tuple[int, ...]:
        """The structure of the groups (which parameter is in which group), without their values."""
        return self.group_of

    def effective(self, wd) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
        """(lr_scale per group, weight decay per group with None resolved to `wd`), validated: ValueError for a value that is
        negative or not finite."""
        scales, wds = [], []
        for gi, g in enumerate(self.groups):
            scales.append(check_group_value(g["lr_scale"], f"param_groups[{gi}]['lr_scale']"))
            own = g["weight_decay"]
            wds.append(check_group_value(wd, "weight_decay") if own is None else
                       check_group_value(own, f"param_groups[{gi}]['weight_decay']"))
        return tuple(scales), tuple(wds)


def no_weight_decay_groups(model, lr_scale: float = 1.0) -> List[dict]:
    """Two groups for HipTrainer(param_groups=...): the parameters with at most one dimension (BatchNorm / LayerNorm scales and shifts,
    every bias) with weight_decay 0.0, and the rest following the trainer's weight decay; both with `lr_scale`.  From the shapes in
    model._param_entries alone.  To add a backbone rate, split each by the prefix "image_encoder." (INTEGRATION.md, section 15)."""
    flat = [e.name for e in model._param_entries if len(e.shape) <= 1]
    rest = [e.name for e in model._param_entries if len(e.shape) > 1]
    return [{"params": flat, "lr_scale": lr_scale, "weight_decay": 0.0}, {"params": rest, "lr_scale": lr_scale, "weight_decay": None}]
