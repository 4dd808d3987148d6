"""HipTrainer.state_dict / load_state_dict, host side: the trainer's state as a torch.optim.AdamW state dict plus one extra block.

    {"state":        {i: {"step": fp32 scalar, "exp_avg": tensor, "exp_avg_sq": tensor}},      every parameter, in its own shape
     "param_groups": [{"lr", "betas", "eps", "weight_decay", ..., "params": [indices]}],       the keys the installed AdamW emits
     "hip_trainer":  {"version": 1, "names": [name of index i], counters, lags, hyper-parameters, groups, average, rng}}

torch.optim.AdamW.load_state_dict ignores the extra block, so the dict fits the `optimizer_state_dict` slot of the reference's
checkpoints (training/train.py:266-320) in both directions; with the block a load is an exact resume, without it (a dict a
torch.optim.AdamW wrote) the moments and the step numbers come over and everything else keeps its value.

Pure functions over layout entries and tensors: plain torch on whatever device the buffers live on, no kernel, no library.  The
per-parameter tensors are layout.view_of views of the flat buffers (OIHW for the KRSC-stored conv weights) and are addressed by name,
never by flat offset.  `load` validates the whole dict on the host before it writes anything.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch

from . import ema as EMA
from . import finetune as FT
from . import layout as LY

VERSION = 1
BLOCK = "hip_trainer"
NONFINITE_MODES = (None, "skip", "raise")


def check_nonfinite(value):
    """HipTrainer's `nonfinite` option: None (no guard), "skip" or "raise"; ValueError for anything else."""
    if value is None or (isinstance(value, str) and value in NONFINITE_MODES):
        return value
    raise ValueError(f'HipTrainer: nonfinite must be None, "skip" or "raise", got {value!r}')


# ---- flat buffer <-> named tensors
def named_tensors(flat: torch.Tensor, entries: Sequence[LY.Entry]) -> Dict[str, torch.Tensor]:
    """{name: CPU clone of the entry's view of `flat`} in the parameters' own shapes; one device-to-host copy of the buffer."""
    host = flat.detach().to("cpu")
    return {e.name: LY.view_of(host, e).clone() for e in entries}


def write_named(flat: torch.Tensor, entries: Sequence[LY.Entry], named: Dict[str, torch.Tensor]):
    """The inverse: every entry's view of `flat` becomes named[name], or zero where `named` has no such name.  The caller has
    checked the shapes; the padding between the slots is not touched."""
    with torch.no_grad():
        for e in entries:
            t = named.get(e.name)
            if t is None:
                LY.view_of(flat, e).zero_()
            else:
                LY.view_of(flat, e).copy_(t)


# ---- per-parameter step numbers <-> (calls, skipped steps, lags, lag classes)
def steps_of(calls: int, skipped_ever: int, lags: Sequence[int]) -> List[int]:
    """Adam's step number of every parameter, calls - skipped_ever - lag: the number the AdamW kernels form on the device."""
    return [calls - skipped_ever - l for l in lags]


def counters_of(steps: Sequence[int]):
    """(calls, lags, lag classes) that give back `steps` with no skipped step: calls = the largest step, one class per distinct lag."""
    calls = max(steps, default=0)
    lags = [calls - s for s in steps]
    ids: Dict[int, int] = {}
    return calls, lags, [ids.setdefault(l, len(ids)) for l in lags]


# ---- export
def index_names(order: Sequence[str], groups) -> List[str]:
    """The parameter name of every state index: `order` (model.parameters() order) without trainer groups, the groups' names one
    group after the other with them -- the order in which torch.optim numbers the parameters of its param_groups."""
    return list(order) if groups is None else [n for g in groups for n in g["names"]]


def torch_group(lr, betas, eps, weight_decay, params: List[int]) -> dict:
    """One entry of "param_groups" with exactly the keys (and defaults) the installed torch.optim.AdamW writes."""
    opt = torch.optim.AdamW([torch.zeros(1, requires_grad=True)], lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                            weight_decay=float(weight_decay))
    g = dict(opt.state_dict()["param_groups"][0])
    g["params"] = list(params)
    return g


def export(entries: Sequence[LY.Entry], order: Sequence[str], m: torch.Tensor, v: torch.Tensor, *, calls: int, skipped_ever: int,
           bad_targets: Sequence[int], empty: int, lag: Sequence[int], lag_class: Sequence[int], ever_frozen: bool, lr, betas, eps,
           weight_decay, max_grad_norm, groups, ema: Optional[torch.Tensor], ema_decay, ema_warmup, seed_base: int, step_id: int,
           nonfinite=None, nonfinite_skipped: Sequence[int] = (0, 0, 0)) -> dict:
    """The state dict.  `lag` and `lag_class` come in layout order (one per entry) and leave in index order, like everything
    per-parameter in the dict; `groups` are the trainer's live dicts {"names", "lr_scale", "weight_decay"} or None.
    nonfinite ("skip" / "raise": the trainer runs the non-finite guard): the block then also carries "nonfinite": {"mode", "since"
    (steps skipped for a non-finite gradient since the last skipped_nonfinite()), "ever", "unchecked" (since the last check())} from
    nonfinite_skipped = (since, ever, unchecked); `skipped_ever` stays the count of ALL launches that were no step.  None: the
    block has exactly the keys it had before the guard existed."""
    check_nonfinite(nonfinite)
    names = index_names(order, groups)
    by_name = {e.name: j for j, e in enumerate(entries)}
    if sorted(names) != sorted(by_name):
        raise ValueError("trainer state: the parameter order does not name every parameter of the layout exactly once")
    at = [by_name[n] for n in names]
    steps = steps_of(int(calls), int(skipped_ever), [int(lag[j]) for j in at])
    mm, vv = named_tensors(m, entries), named_tensors(v, entries)
    state = {i: {"step": torch.tensor(float(steps[i]), dtype=torch.float32), "exp_avg": mm[n], "exp_avg_sq": vv[n]}
             for i, n in enumerate(names)}
    if groups is None:
        pgs = [torch_group(lr, betas, eps, weight_decay, list(range(len(names))))]
    else:
        pgs, lo = [], 0
        for g in groups:
            wd = weight_decay if g["weight_decay"] is None else g["weight_decay"]
            pgs.append(torch_group(float(lr) * float(g["lr_scale"]), betas, eps, wd, list(range(lo, lo + len(g["names"])))))
            lo += len(g["names"])
    block = {
        "version": VERSION, "names": names, "calls": int(calls), "skipped_ever": int(skipped_ever),
        "bad_targets": [int(x) for x in bad_targets], "empty": int(empty),
        "lag": [int(lag[j]) for j in at], "lag_class": [int(lag_class[j]) for j in at], "ever_frozen": bool(ever_frozen),
        "lr": float(lr), "betas": (float(betas[0]), float(betas[1])), "eps": float(eps), "weight_decay": float(weight_decay),
        "max_grad_norm": float(max_grad_norm),
        "groups": None if groups is None else [{"names": list(g["names"]), "lr_scale": float(g["lr_scale"]),
                                                "weight_decay": None if g["weight_decay"] is None else float(g["weight_decay"])}
                                               for g in groups],
        "ema": None if ema is None else named_tensors(ema, entries),
        "ema_decay": None if ema is None else float(ema_decay), "ema_warmup": bool(ema_warmup),
        "rng": {"seed_base": int(seed_base), "step_id": int(step_id)},
    }
    if nonfinite is not None:
        since, ever, unchecked = (int(x) for x in nonfinite_skipped)
        block["nonfinite"] = {"mode": nonfinite, "since": since, "ever": ever, "unchecked": unchecked}
    return {"state": state, "param_groups": pgs, BLOCK: block}


# ---- validation
def _int(x, what: str, lo: int = 0) -> int:
    if isinstance(x, torch.Tensor) and x.numel() == 1:
        x = x.item()
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or int(x) != x or x < lo:
        raise ValueError(f"trainer state: {what} must be an integer >= {lo}, got {x!r}")
    return int(x)


def _num(x, what: str) -> float:
    if isinstance(x, torch.Tensor) and x.numel() == 1:
        x = x.item()
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
        raise ValueError(f"trainer state: {what} must be a finite number, got {x!r}")
    return float(x)


def _betas(x, what: str):
    if not isinstance(x, (tuple, list)) or len(x) != 2:
        raise ValueError(f"trainer state: {what} must be a pair, got {x!r}")
    return _num(x[0], what), _num(x[1], what)


def _names(names, entries, what: str) -> List[str]:
    """`names` as a list that holds every entry's name exactly once (ValueError naming what is missing or unknown)."""
    if not isinstance(names, (list, tuple)) or not all(isinstance(n, str) for n in names):
        raise ValueError(f"trainer state: {what} must be a list of parameter names")
    have, want = set(names), {e.name for e in entries}
    if have != want or len(names) != len(want):
        missing, unknown = sorted(want - have), sorted(have - want)
        raise ValueError(f"trainer state: {what} do not match the model: missing {missing[:3]}{'...' if len(missing) > 3 else ''}, "
                         f"unknown {unknown[:3]}{'...' if len(unknown) > 3 else ''}, {len(names)} entries for {len(want)} parameters")
    return list(names)


def _tensors(named, entries, what: str, partial: bool) -> Dict[str, torch.Tensor]:
    """{name: tensor} checked against the entries' shapes; `partial`: a name may be absent."""
    by_name = {e.name: e for e in entries}
    for n, t in named.items():
        if n not in by_name:
            raise ValueError(f"trainer state: {what} has an entry for {n!r}, which is not a parameter of this model")
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(by_name[n].shape):
            got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"trainer state: {what} of {n!r} has shape {got}, the parameter has {tuple(by_name[n].shape)}")
    if not partial and len(named) != len(by_name):
        missing = sorted(set(by_name) - set(named))
        raise ValueError(f"trainer state: {what} has no entry for {missing[:3]}{'...' if len(missing) > 3 else ''}")
    return named


def _moments(state, ids: Sequence, names: Sequence[str], entries):
    """(exp_avg by name, exp_avg_sq by name, step by name) of the state entries ids[k] -> names[k]; an id without state is absent
    from all three (zero moments, step 0)."""
    if not isinstance(state, dict):
        raise ValueError("trainer state: 'state' must be a dict")
    unknown = set(state) - set(ids)
    if unknown:
        raise ValueError(f"trainer state: 'state' has entries {sorted(unknown, key=str)[:3]} that no param_group lists")
    mm, vv, steps = {}, {}, {}
    for i, n in zip(ids, names):
        s = state.get(i)
        if s is None:
            continue
        if not isinstance(s, dict) or not all(k in s for k in ("step", "exp_avg", "exp_avg_sq")):
            raise ValueError(f"trainer state: state[{i!r}] ({n}) needs 'step', 'exp_avg' and 'exp_avg_sq'")
        mm[n], vv[n], steps[n] = s["exp_avg"], s["exp_avg_sq"], _int(s["step"], f"state[{i!r}]['step']")
    _tensors(mm, entries, "exp_avg", True)
    _tensors(vv, entries, "exp_avg_sq", True)
    return mm, vv, steps


def _param_ids(sd):
    pgs = sd.get("param_groups")
    if not isinstance(pgs, (list, tuple)) or not pgs or not all(isinstance(g, dict) and isinstance(g.get("params"), (list, tuple)) for g in pgs):
        raise ValueError("trainer state: 'param_groups' must be a non-empty list of dicts with a 'params' list")
    ids = [i for g in pgs for i in g["params"]]
    if len(set(ids)) != len(ids):
        raise ValueError("trainer state: a parameter index appears twice in 'param_groups'")
    return pgs, ids


# ---- load
def load(entries: Sequence[LY.Entry], order: Sequence[str], sd, m: torch.Tensor, v: torch.Tensor, ema: Optional[torch.Tensor], groups):
    """Validate `sd` against the layout, the trainer's live groups (or None) and whether it keeps an average (`ema`), then -- only
    then -- write the moments into `m` / `v` and the average into `ema`.  Returns the host-side values for the trainer to take over;
    a value of None means "keep yours":

        calls, skipped_ever, lag, lag_class (layout order), ever_frozen            always
        bad_targets, empty, max_grad_norm, rng, group_values                      None for a plain torch.optim.AdamW dict
        lr, betas, eps, weight_decay                                              None for a plain dict unless it has one group and the
                                                                                  trainer has no groups
        ema: "loaded" | "restart" (the trainer keeps an average, the dict has none: restart it from the weights) | None
        ema_decay, ema_warmup                                                     None unless an average was loaded
        nonfinite: {"mode", "since", "ever", "unchecked"}                         None unless the dict was written by a guarded trainer

    ValueError for everything that does not fit; nothing is written then."""
    if not isinstance(sd, dict) or "state" not in sd:
        raise ValueError("trainer state: expected a dict with 'state' and 'param_groups' (HipTrainer.state_dict() or torch.optim.AdamW's)")
    by_name = {e.name: j for j, e in enumerate(entries)}
    out = dict.fromkeys(("bad_targets", "empty", "max_grad_norm", "rng", "group_values", "lr", "betas", "eps", "weight_decay", "ema",
                         "ema_decay", "ema_warmup", "nonfinite"))
    block = sd.get(BLOCK)
    avg = None
    if block is not None:                                  # ---- an exact resume
        if not isinstance(block, dict) or block.get("version") != VERSION:
            got = block.get("version") if isinstance(block, dict) else type(block).__name__
            raise ValueError(f"trainer state: '{BLOCK}' block of version {got!r}; this build reads version {VERSION}")
        names = _names(block.get("names"), entries, "the names")
        n = len(names)
        mm, vv, _ = _moments(sd["state"], list(range(n)), names, entries)      # (the counters come from the block, not from 'step')
        calls, skipped = _int(block.get("calls"), "calls"), _int(block.get("skipped_ever"), "skipped_ever")
        lag_i, cls_i = block.get("lag"), block.get("lag_class")
        if not isinstance(lag_i, (list, tuple)) or not isinstance(cls_i, (list, tuple)) or len(lag_i) != n or len(cls_i) != n:
            raise ValueError(f"trainer state: 'lag' and 'lag_class' must be lists of {n} integers")
        lag, lag_class = [0] * n, [0] * n
        for i, name in enumerate(names):
            lag[by_name[name]] = _int(lag_i[i], f"lag[{i}]")
            lag_class[by_name[name]] = _int(cls_i[i], f"lag_class[{i}]")
        if skipped > calls or max(lag, default=0) > calls - skipped:
            raise ValueError(f"trainer state: calls {calls}, skipped_ever {skipped} and a lag of {max(lag, default=0)} give a negative step")
        bt = block.get("bad_targets")
        if not isinstance(bt, (list, tuple)) or len(bt) != 2:
            raise ValueError("trainer state: 'bad_targets' must be [rows, steps]")
        out["bad_targets"] = [_int(bt[0], "bad_targets[0]"), _int(bt[1], "bad_targets[1]")]
        out["empty"] = _int(block.get("empty"), "empty")
        ever_frozen = bool(block.get("ever_frozen"))
        out["lr"], out["eps"] = _num(block.get("lr"), "lr"), _num(block.get("eps"), "eps")
        out["weight_decay"], out["max_grad_norm"] = _num(block.get("weight_decay"), "weight_decay"), _num(block.get("max_grad_norm"), "max_grad_norm")
        out["betas"] = _betas(block.get("betas"), "betas")
        bg = block.get("groups")
        if (bg is None) != (groups is None):
            raise ValueError("trainer state: the dict was written " + ("without" if bg is None else "with") + " parameter groups, this "
                             "trainer was built " + ("without" if groups is None else "with") + " them")
        if bg is not None:
            if not isinstance(bg, (list, tuple)) or len(bg) != len(groups) or not all(isinstance(g, dict) for g in bg) or \
                    any(tuple(g.get("names", ())) != tuple(mine["names"]) for g, mine in zip(bg, groups)):
                raise ValueError("trainer state: the parameter groups of the dict differ in membership from this trainer's")
            try:
                out["group_values"] = [(FT.check_group_value(g.get("lr_scale"), f"groups[{gi}]['lr_scale']"),
                                        None if g.get("weight_decay") is None else
                                        FT.check_group_value(g["weight_decay"], f"groups[{gi}]['weight_decay']")) for gi, g in enumerate(bg)]
            except ValueError as err:
                raise ValueError(f"trainer state: {err}") from None
        avg = block.get("ema")
        if avg is not None:
            if ema is None:
                raise ValueError("trainer state: the dict holds a weight average, this trainer was built without ema_decay: loading it "
                                 "would drop the average silently")
            if not isinstance(avg, dict):
                raise ValueError("trainer state: 'ema' must be a dict {name: tensor}")
            _tensors(avg, entries, "the average", False)
            out["ema"] = "loaded"
            out["ema_decay"] = EMA.check_decay(block.get("ema_decay"), "trainer state: ema_decay")
            out["ema_warmup"] = bool(block.get("ema_warmup"))
        elif ema is not None:
            out["ema"] = "restart"
        rng = block.get("rng")
        if not isinstance(rng, dict):
            raise ValueError("trainer state: 'rng' must be a dict {seed_base, step_id}")
        out["rng"] = {"seed_base": _int(rng.get("seed_base"), "rng['seed_base']"), "step_id": _int(rng.get("step_id"), "rng['step_id']")}
        nf = block.get("nonfinite")
        if nf is not None:
            if not isinstance(nf, dict) or nf.get("mode") not in ("skip", "raise"):
                raise ValueError("trainer state: 'nonfinite' must be a dict {mode: 'skip' | 'raise', since, ever, unchecked}")
            out["nonfinite"] = {"mode": nf["mode"], **{k: _int(nf.get(k), f"nonfinite['{k}']") for k in ("since", "ever", "unchecked")}}
            if max(out["nonfinite"]["since"], out["nonfinite"]["unchecked"]) > out["nonfinite"]["ever"] or out["nonfinite"]["ever"] > skipped:
                raise ValueError(f"trainer state: nonfinite counters {nf} do not fit skipped_ever {skipped}")
    else:                                                  # ---- a plain torch.optim.AdamW dict: the moments and the steps
        pgs, ids = _param_ids(sd)
        for gi, g in enumerate(pgs):
            for flag in ("amsgrad", "maximize"):
                if g.get(flag):
                    raise ValueError(f"trainer state: param_groups[{gi}] has {flag}=True, which the fused AdamW does not implement")
            if g.get("decoupled_weight_decay") is False:
                raise ValueError(f"trainer state: param_groups[{gi}] has decoupled_weight_decay=False (Adam's L2 penalty); the fused "
                                 "optimizer is AdamW")
        sizes = [len(g["params"]) for g in pgs]
        if groups is None:
            if len(pgs) != 1:
                raise ValueError(f"trainer state: the dict has {len(pgs)} param_groups, this trainer has none: their concatenation is "
                                 "not model.parameters() order")
        elif sizes != [len(g["names"]) for g in groups]:
            raise ValueError(f"trainer state: param_groups of sizes {sizes}, this trainer's groups have {[len(g['names']) for g in groups]}")
        names = index_names(order, groups)
        if len(ids) != len(names) or sorted(names) != sorted(by_name):
            raise ValueError(f"trainer state: the dict lists {len(ids)} parameters, the model has {len(by_name)}")
        mm, vv, st = _moments(sd["state"], ids, names, entries)
        steps = [0] * len(names)
        for name, s in st.items():
            steps[by_name[name]] = s
        calls, lag, lag_class = counters_of(steps)
        skipped = 0
        ever_frozen = len(set(steps)) > 1
        if groups is None:
            g = pgs[0]
            out["lr"], out["eps"], out["weight_decay"] = _num(g.get("lr"), "lr"), _num(g.get("eps"), "eps"), _num(g.get("weight_decay"), "weight_decay")
            out["betas"] = _betas(g.get("betas"), "betas")
    out.update(calls=calls, skipped_ever=skipped, lag=lag, lag_class=lag_class, ever_frozen=ever_frozen)
    # ---- everything fits: write
    write_named(m, entries, mm)
    write_named(v, entries, vv)
    if avg is not None:
        write_named(ema, entries, avg)
    return out
