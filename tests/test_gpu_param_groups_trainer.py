"""GPU: parameter groups of HipTrainer (param_groups=: a learning-rate scale and a weight decay per group of parameters).

Neutral groups train bit-identically to no groups; a grouped step follows torch.optim.AdamW in float64 with one torch param group per
group, fed the trainer's own gradient and the global clip coefficient (bounds of tests/test_gpu_optimizer_ranges.py); the groups' values
are live between steps and reach a captured step without a new capture; frozen parts keep their own Adam step numbers; a trainer without
groups issues the launches it always issued; a bad live value is refused before anything is launched or counted.

The reference's hyper-parameters.  The C ABI carries lr, the betas, eps and the groups' values as `float`, so the reference is given
those fp32 values (as doubles) and computes everything in float64 from them.  It matters for beta2 alone: float32(0.999) is
0.99900001287, and 1 - beta2 -- the whole second moment after a first step from zero state, which is what a trainer test sees --
is then 1.287e-5 smaller, relatively, than 1 - 0.999.  Fed the double 0.999 the same steps measure dv/max = 1.28e-5 ... 1.29e-5
(fp32 and bf16, |dp| 6e-8, dm/max 2.6e-7) against the bound of 1e-5: the distance between the two beta2, not an error of the update.
Every AdamW entry has formed 1 - beta2 this way since before the groups; the kernel tests start from second moments of 1e-3 and so
never saw it."""
import math

import pytest
import torch

from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = O.full_config(dropout=0.0, answer_dropout=0.0, vocab_size=100, num_answers=10, embed_dim=32)
_CACHE = {}


def _sd():
    if "sd" not in _CACHE:
        _CACHE["sd"] = O.init_state_dict(CFG, 47, jitter=True)
    return _CACHE["sd"]


def _model(dtype="bf16"):
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype=dtype)
    m.load_state_dict(_sd())
    return m.to(DEV).train()


def _batch(seed, B=4):
    key = (seed, B)
    if key not in _CACHE:
        _CACHE[key] = [t.to(DEV) for t in O.synthetic_batch(B, seed=seed, image_size=64, seq_len=10, vocab=100, num_answers=10)]
    return _CACHE[key]


def _trainer(m, **kw):
    return pkg().trainer.HipTrainer(m, **dict(dict(lr=1e-3), **kw))


def _recipe(m, backbone=0.1):
    """no_weight_decay_groups composed with a backbone rate: split by the prefix "image_encoder." first"""
    out = []
    for g in sub("finetune").no_weight_decay_groups(m):
        cnn = [n for n in g["params"] if n.startswith("image_encoder.")]
        out += [dict(g, params=cnn, lr_scale=backbone), dict(g, params=[n for n in g["params"] if not n.startswith("image_encoder.")])]
    return out


def _bits(t):
    return t.detach().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _snap(m, tr):
    torch.cuda.synchronize()
    return tuple(t.detach().cpu().clone() for t in (m._flat, tr.m, tr.v))


def _mask(m, pred):
    mask = torch.zeros(m._flat.numel(), dtype=torch.bool)
    for e in m._param_entries:
        if pred(e.name):
            mask[e.offset: e.offset + e.numel] = True
    return mask


class _Calls:
    """Names of the launches that go through _lib.call, in order."""

    def __enter__(self):
        L = sub("_lib")
        self.names, self._old = [], L._HOOK[0]
        L._HOOK[0] = lambda name, args: self.names.append(name)
        return self

    def __exit__(self, *a):
        sub("_lib")._HOOK[0] = self._old


def _f32(x):
    """the value a `float` argument of the C ABI carries, as a double"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _check_fp64(m, tr, snap, steps=None, what=""):
    """The step just taken against torch.optim.AdamW in float64: one fp64 tensor per trainable parameter with Adam's state preset to the
    snapshot (step number steps[j] - 1, default the trainer's), one torch param group per trainer group with lr * lr_scale and the
    group's effective weight decay, gradients = the trainer's own times the fp64 clip coefficient of the GLOBAL norm.  Frozen parameters
    must have kept their bits."""
    torch.cuda.synchronize()
    flat0, m0, v0 = snap
    pe, pg = m._param_entries, tr._pg
    scales, wds = ([_f32(x) for x in vals] for vals in pg.effective(tr.wd))
    lr, betas, eps = _f32(tr.lr), tuple(_f32(b) for b in tr.betas), _f32(tr.eps)
    G = tr.G.detach().cpu().double()
    trainable = [p.requires_grad for p in m._param_list()]
    sl = [slice(e.offset, e.offset + e.numel) for e in pe]
    norm = math.sqrt(sum(float((G[s] ** 2).sum()) for s, t in zip(sl, trainable) if t))
    assert abs(float(tr.grad_norm()) - norm) / norm < 1e-5
    c = tr.max_norm / (norm + 1e-6)
    coef = c if c < 1 else 1.0
    by_group, qs = {}, {}
    for j, s in enumerate(sl):
        if trainable[j]:
            q = flat0[s].double().clone().requires_grad_()
            q.grad = G[s] * coef
            qs[j] = q
            by_group.setdefault(pg.group_of[j], []).append(q)
    opt = torch.optim.AdamW([{"params": ps, "lr": lr * scales[g], "weight_decay": wds[g]} for g, ps in sorted(by_group.items())],
                            lr=lr, betas=betas, eps=eps, foreach=False)
    for j, q in qs.items():
        t = tr.t if steps is None else steps[j]
        opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0[sl[j]].double().clone(), "exp_avg_sq": v0[sl[j]].double().clone()}
    opt.step()
    flat1, m1, v1 = _snap(m, tr)
    ep = em = ev = mm = vm = 0.0
    for j, s in enumerate(sl):
        if not trainable[j]:
            assert _same(flat1[s], flat0[s]) and _same(m1[s], m0[s]) and _same(v1[s], v0[s]), pe[j].name
            continue
        st = opt.state[qs[j]]
        ep = max(ep, float((flat1[s].double() - qs[j].detach()).abs().max()))
        em = max(em, float((m1[s].double() - st["exp_avg"]).abs().max()))
        ev = max(ev, float((v1[s].double() - st["exp_avg_sq"]).abs().max()))
        mm, vm = max(mm, float(st["exp_avg"].abs().max())), max(vm, float(st["exp_avg_sq"].abs().max()))
    print(f"   {what} |dp| {ep:.2e}  dm/max {em / mm:.2e}  dv/max {ev / vm:.2e}  (clip {'on' if c < 1 else 'off'})")
    assert ep < 2e-6 and em / mm < 1e-5 and ev / vm < 1e-5, what
    if tr.engine.adamw_copy_target() is not None:                   # the bf16 operand copy of the same launch
        assert torch.equal(tr.engine.wsrc.cpu(), m._flat.detach().cpu().to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------------------ a. neutral groups
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_neutral_groups_train_bit_identically_to_no_groups(dtype):
    ma, mb = _model(dtype), _model(dtype)
    ta = _trainer(ma, ema_decay=0.99)
    tb = _trainer(mb, ema_decay=0.99, param_groups=[{"params": ["image_encoder."], "lr_scale": 1.0, "weight_decay": None},
                                                     {"params": [n for n, _ in mb.named_parameters() if not n.startswith("image_encoder.")]}])
    assert ta.param_groups is None and len(tb.param_groups) == 2
    for step in range(3):
        batch = _batch(900 + step)
        la, ga = ta.step(*batch)
        lb, gb = tb.step(*batch)
        torch.cuda.synchronize()
        assert _same(la, lb) and _same(ga, gb), step
        assert _same(ma._flat, mb._flat) and _same(ta.m, tb.m) and _same(ta.v, tb.v) and _same(ta.ema, tb.ema), step
    assert ta._ranges is None and tb._ranges is not None and tb._ranges[1] == 2       # the table route: two ranges, split at the prefix
    assert not _same(tb.ema, mb._flat)
    ta.check(); tb.check()


# ------------------------------------------------------------------------------------------------ b. one grouped step against fp64
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_grouped_step_follows_fp64_adamw_per_group(dtype):
    m, twin = _model(dtype), _model(dtype)
    tr, tt = _trainer(m, param_groups=_recipe(m)), _trainer(twin)
    assert [(g["lr_scale"], g["weight_decay"]) for g in tr.param_groups] == [(0.1, 0.0), (1.0, 0.0), (0.1, None), (1.0, None)]
    assert sum(len(g["names"]) for g in tr.param_groups) == len(m._param_entries)
    snap = _snap(m, tr)
    batch = _batch(910)
    l1, g1 = tr.step(*batch)
    l2, g2 = tt.step(*batch)
    _check_fp64(m, tr, snap, what=dtype)
    assert _same(l1, l2) and _same(g1, g2)                          # the same forward and loss
    assert not _same(m._flat, twin._flat)                           # another update
    for (na, a), (nb, b) in zip(sorted(m.named_buffers()), sorted(twin.named_buffers())):      # BN running statistics, counters, pe
        assert na == nb and torch.equal(a, b), na
    assert _same(tr.G, tt.G)
    tr.check()


# ------------------------------------------------------------------------------------------------------------- c. live values
def test_group_values_are_live_between_steps():
    m = _model()
    tr = _trainer(m, weight_decay=0.01, param_groups=[{"params": ["image_encoder."], "lr_scale": 0.5},
                                                      {"params": ["text_encoder."], "weight_decay": 0.1}])
    cnn = _mask(m, lambda n: n.startswith("image_encoder."))
    gen = tr._ranges_gen
    tr.step(*_batch(920))
    gen1 = tr._ranges_gen
    assert gen1 == gen + 1
    # lr_scale 0: that group's parameters keep their bits, its moments move, the others train
    tr.param_groups[0]["lr_scale"] = 0.0
    snap = _snap(m, tr)
    tr.step(*_batch(921))
    flat1, m1, v1 = _snap(m, tr)
    assert _same(flat1[cnn], snap[0][cnn]) and not _same(m1[cnn], snap[1][cnn]) and not _same(v1[cnn], snap[2][cnn])
    assert not _same(flat1[~cnn], snap[0][~cnn])
    # back to 0.5, and the trainer's weight decay changes: the groups with weight_decay None follow, the one with its own does not
    tr.param_groups[0]["lr_scale"] = 0.5
    tr.wd = 0.2
    assert tr._pg.effective(tr.wd) == ((0.5, 1.0, 1.0), (0.2, 0.1, 0.2))
    snap = _snap(m, tr)
    tr.step(*_batch(922))
    _check_fp64(m, tr, snap, what="wd 0.2")
    # a decay of 0.2 against 0.01 moves p by lr * 0.19 * |p| ~ 2e-4 |p|: far outside the bound had the block kept the old values
    assert tr._ranges_gen == gen1                                   # values only: the table was not rebuilt
    tr.check()


# ------------------------------------------------------------------------------------------------------------ d. frozen parts
def test_frozen_parts_keep_their_own_step_numbers_under_groups():
    m = _model()
    tr = _trainer(m, param_groups=_recipe(m, backbone=0.5))
    cnn = _mask(m, lambda n: n.startswith("image_encoder."))
    is_cnn = [e.name.startswith("image_encoder.") for e in m._param_entries]
    m.image_encoder.requires_grad_(False)
    flat0 = m._flat.detach().cpu().clone()
    for step in range(2):
        snap = _snap(m, tr)
        tr.step(*_batch(930 + step))
        _check_fp64(m, tr, snap, steps=[step + 1] * len(is_cnn), what=f"frozen step {step + 1}")
        assert _same(m._flat.detach().cpu()[cnn], flat0[cnn])
    gen = tr._ranges_gen
    m.image_encoder.requires_grad_(True)
    snap = _snap(m, tr)
    tr.step(*_batch(932))
    assert tr._ranges_gen == gen + 1                                # the trainable set changed: a new table
    _check_fp64(m, tr, snap, steps=[1 if c else 3 for c in is_cnn], what="thawed")
    assert not _same(m._flat.detach().cpu()[cnn], flat0[cnn])
    # a shared step number would miss by a large fraction of lr: bias correction 1 at step 1 is 0.1, at step 3 it is 0.271
    tr.check()


# ------------------------------------------------------------------------------------------------------------- e. step_graphed
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graphed_grouped_steps_are_bit_equal_and_never_recapture_for_values(dtype):
    ma, mb = _model(dtype), _model(dtype)
    ta, tb = (_trainer(m, ema_decay=0.99, param_groups=_recipe(m)) for m in (ma, mb))
    changes = {1: lambda t: setattr(t, "lr", 5e-4),
               3: lambda t: t.param_groups[0].__setitem__("lr_scale", 0.3),
               4: lambda t: t.param_groups[3].__setitem__("weight_decay", 0.05),
               5: lambda t: (setattr(t, "lr", 2e-3), t.param_groups[1].__setitem__("lr_scale", 0.0))}
    names = []
    for step in range(6):
        for t in (ta, tb):
            changes.get(step, lambda t: None)(t)
        batch = _batch(940 + step % 3)
        la, ga = ta.step(*batch)
        with _Calls() as c:
            lb, gb = tb.step_graphed(*batch)
        names.append(c.names)
        torch.cuda.synchronize()
        assert _same(la, lb) and _same(ga, gb), step
        assert _same(ma._flat, mb._flat) and _same(ta.m, tb.m) and _same(ta.v, tb.v) and _same(ta.ema, tb.ema), step
        for (_, a), (_, b) in zip(sorted(ma.named_buffers()), sorted(mb.named_buffers())):
            assert torch.equal(a, b), step
    assert tb.graph_captures == 1
    replays = [n for n in names if "vqa_adamw_groups_ema" not in n and "vqa_adamw_groups_ema_dev" not in n]
    assert len(replays) >= 2                                        # (replays issue no AdamW launch from the host)
    for n in replays:
        assert n[0] == "vqa_step_state_set" and set(n) <= {"vqa_step_state_set", "vqa_group_hyper_set", "vqa_convert"}
    assert names[-1][:2] == ["vqa_step_state_set", "vqa_group_hyper_set"]     # step 5 changed a value: written beside the step state


# ----------------------------------------------------------------------------------------------------------------- f. launches
def _tail(names):
    return [n for n in names if n.startswith(("vqa_sumsq", "vqa_adamw", "vqa_group"))]


def test_launches_with_and_without_groups():
    m, mg = _model(), _model()
    tr, tg = _trainer(m), _trainer(mg, param_groups=_recipe(mg))
    plain, grouped = [], []
    for step in range(4):
        if step == 2:
            tg.param_groups[2]["lr_scale"] = 0.2
        with _Calls() as a:
            tr.step(*_batch(950 + step))
        with _Calls() as b:
            tg.step(*_batch(950 + step))
        plain.append(a.names); grouped.append(b.names)
    torch.cuda.synchronize()
    for names in plain:                                             # what a trainer without groups has always issued
        assert _tail(names) == ["vqa_sumsq", "vqa_adamw"]
    assert tg._ranges[1] == 87 and all(tg.reducer._send) and tg.reducer._send == tr.reducer._send      # nothing frozen: the reducer sends everything
    sets = ["vqa_group_hyper_set" in n for n in grouped]
    assert sets == [True, False, True, False]                       # the first step and the step after a value change
    swap = {"vqa_sumsq_ranges": "vqa_sumsq", "vqa_adamw_groups": "vqa_adamw"}
    for a, b in zip(plain, grouped):
        assert _tail(b) == (["vqa_group_hyper_set"] if "vqa_group_hyper_set" in b else []) + ["vqa_sumsq_ranges", "vqa_adamw_groups"]
        assert b.count("vqa_group_hyper_set") <= 1
        assert [swap.get(n, n) for n in b if n != "vqa_group_hyper_set"] == a          # everything else: the same launches in the same order
    # with the weight average: the _ema entry; a trainer.wd change behind a None group is a value change too
    me = _model()
    te = _trainer(me, ema_decay=0.9, param_groups=[{"params": ["fusion."], "lr_scale": 2.0}])
    seen = []
    for step in range(3):
        if step == 2:
            te.wd = 0.05
        with _Calls() as c:
            te.step(*_batch(950))
        seen.append(_tail(c.names))
    assert seen == [["vqa_group_hyper_set", "vqa_sumsq_ranges", "vqa_adamw_groups_ema"], ["vqa_sumsq_ranges", "vqa_adamw_groups_ema"],
                    ["vqa_group_hyper_set", "vqa_sumsq_ranges", "vqa_adamw_groups_ema"]]
    # the captured step: the _dev entry
    for _ in range(2):
        te.step_graphed(*_batch(950))
    with _Calls() as c:
        te.step_graphed(*_batch(950))
    assert te.graph_captures == 1 and _tail(c.names) == ["vqa_sumsq_ranges", "vqa_adamw_groups_ema_dev"] and c.names[0] == "vqa_step_state_set"
    with _Calls() as c:
        te.step_graphed(*_batch(950))
    assert c.names == ["vqa_step_state_set"]
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- g. refusals
@pytest.mark.parametrize("key,bad", [("lr_scale", float("nan")), ("lr_scale", -0.5), ("weight_decay", float("inf")), ("weight_decay", -1.0)])
def test_a_bad_live_value_is_refused_before_anything_is_launched_or_counted(key, bad):
    m = _model()
    tr = _trainer(m, param_groups=[{"params": ["image_encoder."], "lr_scale": 0.1, "weight_decay": 0.0}])
    batch = _batch(960)
    tr.step(*batch)
    snap = _snap(m, tr)
    eng = tr.engine
    counters = (tr.calls, eng.step_id, eng.cnn_train_forwards, m._feat_epoch)
    good = tr.param_groups[0][key]
    tr.param_groups[0][key] = bad
    with _Calls() as c:
        with pytest.raises(ValueError):
            tr.step(*batch)
        with pytest.raises(ValueError):
            tr.step_graphed(*batch)
    assert c.names == [] and (tr.calls, eng.step_id, eng.cnn_train_forwards, m._feat_epoch) == counters
    after = _snap(m, tr)
    assert all(_same(a, b) for a, b in zip(snap, after))
    tr.param_groups[0][key] = good                                  # and the trainer is as usable as before
    tr.step(*batch)
    _check_fp64(m, tr, after, what="after the refusal")
    tr.check()
