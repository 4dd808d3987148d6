"""HipTrainer.state_dict / load_state_dict, host side (trainer_state.py) on CPU buffers over a real layout table: flat buffer <-> named
tensors (KRSC conv weights included), step numbers <-> (calls, lags, classes), the exported dict through torch.save /
torch.load(weights_only=True) and into torch.optim.AdamW (one group, two groups), a plain torch dict with indices missing, and every
refusal -- after which the destination buffers hold their earlier bytes.  No GPU."""
import io

import pytest
import torch

from _pkg import sub
from oracle import vqa_oracle as O

CFG = O.full_config(vocab_size=100, num_answers=10, embed_dim=32)


def _ts():
    return sub("trainer_state")


def _entries(cfg=CFG):
    return [e for e in sub("layout").build_entries(cfg) if e.is_param]


def _flat(entries, seed):
    """A flat buffer with random contents in every slot and zeros in the padding between them."""
    LY = sub("layout")
    flat = torch.zeros(LY.flat_size(entries))
    g = torch.Generator().manual_seed(seed)
    for e in entries:
        LY.view_of(flat, e).copy_(torch.randn(e.shape, generator=g))
    return flat


def _groups(entries):
    """Two trainer groups as HipTrainer.param_groups holds them: <= 1-D parameters without decay, the rest following the trainer."""
    return [{"names": tuple(e.name for e in entries if len(e.shape) <= 1), "lr_scale": 0.5, "weight_decay": 0.0},
            {"names": tuple(e.name for e in entries if len(e.shape) > 1), "lr_scale": 1.0, "weight_decay": None}]


def _export(entries, groups=None, ema=False, calls=7, skipped=1, lag=None, **kw):
    n = len(entries)
    args = dict(calls=calls, skipped_ever=skipped, bad_targets=[3, 1], empty=2, lag=[0] * n if lag is None else lag,
                lag_class=[0] * n if lag is None else [0 if l == 0 else 1 for l in lag], ever_frozen=lag is not None, lr=2e-4,
                betas=(0.9, 0.98), eps=1e-7, weight_decay=0.05, max_grad_norm=2.0, groups=groups, ema=_flat(entries, 3) if ema else None,
                ema_decay=0.99 if ema else None, ema_warmup=ema, seed_base=0x5EED, step_id=9)
    args.update(kw)
    return _ts().export(entries, [e.name for e in entries], _flat(entries, 1), _flat(entries, 2).square(), **args)


def _load(entries, sd, groups=None, ema=False):
    """Load into fresh buffers; returns (host values, m, v, ema)."""
    m, v = _flat(entries, 11), _flat(entries, 12)
    avg = _flat(entries, 13) if ema else None
    r = _ts().load(entries, [e.name for e in entries], sd, m, v, avg, groups)
    return r, m, v, avg


# ------------------------------------------------------------------------------------------------------ flat buffer <-> named tensors
def test_flat_to_named_and_back_is_exact_krsc_included():
    TS, LY = _ts(), sub("layout")
    entries = _entries()
    flat = _flat(entries, 5)
    named = TS.named_tensors(flat, entries)
    assert list(named) == [e.name for e in entries]
    for e in entries:
        assert tuple(named[e.name].shape) == tuple(e.shape) and named[e.name].device.type == "cpu"
        assert named[e.name].untyped_storage().data_ptr() != flat.untyped_storage().data_ptr()       # a copy, not a view
    conv = next(e for e in entries if e.krsc and e.shape[1] > 1 and e.shape[2] == 3)
    co, ci, R, S = conv.shape
    t = named[conv.name]                                                                             # OIHW, stored [Cout][R][S][Cin]
    for o, i, r, s in ((0, 0, 0, 0), (1, 2, 0, 1), (co - 1, ci - 1, R - 1, S - 1), (3, 1, 2, 0)):
        assert t[o, i, r, s] == flat[conv.offset + ((o * R + r) * S + s) * ci + i]
    back = torch.zeros_like(flat)
    TS.write_named(back, entries, named)
    assert torch.equal(back, flat)
    # a name that is absent becomes zero; the padding between the slots is never written
    back.fill_(7.0)
    del named[conv.name]
    TS.write_named(back, entries, named)
    assert not LY.view_of(back, conv).any()
    pad = torch.ones_like(back, dtype=torch.bool)
    for e in entries:
        pad[e.offset: e.offset + e.numel] = False
    assert pad.any() and bool((back[pad] == 7.0).all())
    back[pad] = 0.0
    LY.view_of(back, conv).copy_(LY.view_of(flat, conv))
    assert torch.equal(back, flat)


# ---------------------------------------------------------------------------------------------- steps <-> (calls, lags, classes)
def test_steps_and_counters_round_trip():
    TS = _ts()
    assert TS.steps_of(5, 0, [0, 0, 0, 0]) == [5, 5, 5, 5]
    assert TS.counters_of([5, 5, 5, 5]) == (5, [0, 0, 0, 0], [0, 0, 0, 0])
    steps = TS.steps_of(9, 1, [0, 0, 2, 5])
    assert steps == [8, 8, 6, 3]
    calls, lags, classes = TS.counters_of(steps)
    assert (calls, lags) == (8, [0, 0, 2, 5])                          # skipped steps fold into calls: calls - 0 - lag = step
    assert TS.steps_of(calls, 0, lags) == steps
    assert classes[0] == classes[1] and len({classes[0], classes[2], classes[3]}) == 3
    assert TS.counters_of([]) == (0, [], [])


def test_export_writes_the_steps_the_kernels_form():
    entries = _entries()
    n = len(entries)
    lag = [0] * n
    lag[2], lag[5] = 2, 5
    sd = _export(entries, calls=9, skipped=1, lag=lag)
    steps = [float(sd["state"][i]["step"]) for i in range(n)]
    assert steps == [float(9 - 1 - l) for l in lag]
    assert all(sd["state"][i]["step"].dtype == torch.float32 and sd["state"][i]["step"].dim() == 0 for i in range(n))
    r, _, _, _ = _load(entries, sd)
    assert (r["calls"], r["skipped_ever"], r["lag"], r["ever_frozen"]) == (9, 1, lag, True)
    assert r["lag_class"] == [0 if l == 0 else 1 for l in lag]


# ------------------------------------------------------------------------------------------------- the dict, torch.save, torch.optim
@pytest.mark.parametrize("grouped", [False, True])
def test_export_survives_weights_only_and_loads_into_torch_adamw(grouped):
    entries = _entries()
    groups = _groups(entries) if grouped else None
    sd = _export(entries, groups=groups, ema=True)
    buf = io.BytesIO()
    torch.save({"optimizer_state_dict": sd}, buf)
    buf.seek(0)
    sd2 = torch.load(buf, weights_only=True)["optimizer_state_dict"]
    blk, blk2 = sd["hip_trainer"], sd2["hip_trainer"]
    assert blk2["version"] == 1 and blk2["names"] == blk["names"] and sorted(blk2["names"]) == sorted(e.name for e in entries)
    for k in ("calls", "skipped_ever", "bad_targets", "empty", "lag", "lag_class", "ever_frozen", "lr", "eps", "weight_decay",
              "max_grad_norm", "groups", "ema_decay", "ema_warmup", "rng"):
        assert blk2[k] == blk[k], k
    assert tuple(blk2["betas"]) == (0.9, 0.98)
    shape = {e.name: tuple(e.shape) for e in entries}
    for i, name in enumerate(blk["names"]):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sd2["state"][i][k], sd["state"][i][k])
        assert tuple(sd2["state"][i]["exp_avg"].shape) == shape[name]
        assert torch.equal(blk2["ema"][name], blk["ema"][name])
    # into torch.optim.AdamW over CPU parameters of the same shapes, built the way the dict numbers them
    P = {e.name: torch.nn.Parameter(torch.zeros(e.shape)) for e in entries}
    if grouped:
        assert [len(g["params"]) for g in sd2["param_groups"]] == [len(g["names"]) for g in groups]
        opt = torch.optim.AdamW([{"params": [P[n] for n in g["names"]]} for g in groups])
    else:
        assert blk["names"] == [e.name for e in entries] and len(sd2["param_groups"]) == 1
        opt = torch.optim.AdamW([P[e.name] for e in entries])
    assert [set(g) for g in sd2["param_groups"]] == [set(g) for g in opt.state_dict()["param_groups"]]      # torch's own key set
    opt.load_state_dict(sd2)
    if grouped:
        assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(2e-4 * 0.5, 0.0), (2e-4, 0.05)]
    else:
        assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(2e-4, 0.05)]
    assert all(g["betas"] == (0.9, 0.98) and g["eps"] == 1e-7 and not g["amsgrad"] for g in opt.param_groups)
    for i, name in enumerate(blk["names"]):
        st = opt.state[P[name]]
        assert torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"]) and torch.equal(st["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
        assert float(st["step"]) == 6.0
    for p in P.values():
        p.grad = torch.ones_like(p)
    opt.step()
    assert all(float(opt.state[p]["step"]) == 7.0 and bool(torch.isfinite(p).all()) and bool(p.any()) for p in P.values())
    # and the way back: torch's dict (no block) into trainer buffers
    r, m, v, _ = _load(entries, opt.state_dict(), groups=groups)
    LY = sub("layout")
    for e in entries:
        assert torch.equal(LY.view_of(m, e), opt.state[P[e.name]]["exp_avg"]) and torch.equal(LY.view_of(v, e), opt.state[P[e.name]]["exp_avg_sq"])
    assert r["calls"] == 7 and r["skipped_ever"] == 0 and not any(r["lag"]) and not r["ever_frozen"]
    assert all(r[k] is None for k in ("bad_targets", "empty", "rng", "ema", "ema_decay", "max_grad_norm", "group_values"))
    if grouped:                                                        # several groups: the live values stay
        assert r["lr"] is None and r["betas"] is None
    else:
        assert (r["lr"], r["betas"], r["eps"], r["weight_decay"]) == (2e-4, (0.9, 0.98), 1e-7, 0.05)


def test_exact_load_restores_buffers_and_host_values():
    entries = _entries()
    groups = _groups(entries)
    n = len(entries)
    lag = [0] * n
    lag[4] = 3
    sd = _export(entries, groups=groups, ema=True, lag=lag)
    mine = [dict(g, lr_scale=1.0, weight_decay=None) for g in groups]          # the receiving trainer's live values differ
    r, m, v, avg = _load(entries, sd, groups=mine, ema=True)
    assert torch.equal(m, _flat(entries, 1)) and torch.equal(v, _flat(entries, 2).square()) and torch.equal(avg, _flat(entries, 3))
    assert (r["calls"], r["skipped_ever"], r["bad_targets"], r["empty"], r["lag"]) == (7, 1, [3, 1], 2, lag)
    assert (r["lr"], r["betas"], r["eps"], r["weight_decay"], r["max_grad_norm"]) == (2e-4, (0.9, 0.98), 1e-7, 0.05, 2.0)
    assert r["group_values"] == [(0.5, 0.0), (1.0, None)]
    assert (r["ema"], r["ema_decay"], r["ema_warmup"]) == ("loaded", 0.99, True)
    assert r["rng"] == {"seed_base": 0x5EED, "step_id": 9}
    # a trainer that keeps an average, a dict without one: restart, the buffer is left for the trainer to fill
    r, _, _, avg = _load(entries, _export(entries), ema=True)
    assert r["ema"] == "restart" and r["ema_decay"] is None and torch.equal(avg, _flat(entries, 13))


def test_plain_torch_dict_with_missing_indices_imports_zeros_and_step_zero():
    LY = sub("layout")
    entries = _entries()
    P = [torch.nn.Parameter(torch.zeros(e.shape)) for e in entries]
    opt = torch.optim.AdamW(P, lr=3e-4, weight_decay=0.02)
    absent = {0, 7, len(P) - 1}
    g = torch.Generator().manual_seed(0)
    for _ in range(2):
        for j, p in enumerate(P):
            p.grad = None if j in absent else torch.randn(p.shape, generator=g)
        opt.step()
    P[3].grad = None                                                   # and one parameter a step behind the others
    opt.step()
    sd = opt.state_dict()
    assert set(sd["state"]) == set(range(len(P))) - absent
    r, m, v, _ = _load(entries, sd)
    for j, e in enumerate(entries):
        if j in absent:
            assert not LY.view_of(m, e).any() and not LY.view_of(v, e).any()
        else:
            assert torch.equal(LY.view_of(m, e), opt.state[P[j]]["exp_avg"]) and torch.equal(LY.view_of(v, e), opt.state[P[j]]["exp_avg_sq"])
    want = [0 if j in absent else (2 if j == 3 else 3) for j in range(len(P))]
    assert r["calls"] == 3 and r["skipped_ever"] == 0 and r["ever_frozen"]
    assert _ts().steps_of(r["calls"], 0, r["lag"]) == want
    cls = r["lag_class"]
    assert len(set(cls)) == 3 and all((cls[a] == cls[b]) == (want[a] == want[b]) for a in range(len(P)) for b in (0, 1, 3))
    assert (r["lr"], r["weight_decay"]) == (3e-4, 0.02)


# ------------------------------------------------------------------------------------------------------------------- the refusals
def _renamed(sd, i, name):
    sd["hip_trainer"]["names"][i] = name


def _bad_cases():
    """(label, mutation of an exported dict, kwargs of the receiving side)"""
    def version(sd): sd["hip_trainer"]["version"] = 2
    def unknown_name(sd): _renamed(sd, 3, "image_encoder.nothing.weight")
    def missing_name(sd): sd["hip_trainer"]["names"].pop()
    def wrong_shape(sd): sd["state"][5]["exp_avg_sq"] = torch.zeros(3, 3)
    def wrong_ema_shape(sd): sd["hip_trainer"]["ema"][sd["hip_trainer"]["names"][2]] = torch.zeros(2)
    def missing_ema_name(sd): sd["hip_trainer"]["ema"].pop(sd["hip_trainer"]["names"][2])
    def membership(sd):
        g0, g1 = sd["hip_trainer"]["groups"]
        g1["names"].append(g0["names"].pop())
    def negative_step(sd): sd["hip_trainer"]["lag"][1] = 50
    def nothing(sd): pass
    yield "unknown version", version, {}
    yield "unknown parameter name", unknown_name, {}
    yield "missing parameter name", missing_name, {}
    yield "wrong shape", wrong_shape, {}
    yield "wrong shape in the average", wrong_ema_shape, dict(ema=True, with_ema=True)
    yield "name missing from the average", missing_ema_name, dict(ema=True, with_ema=True)
    yield "group membership", membership, dict(grouped=True, with_groups=True)
    yield "groups in the dict only", nothing, dict(grouped=True)
    yield "groups in the trainer only", nothing, dict(with_groups=True)
    yield "an average the trainer cannot keep", nothing, dict(ema=True)
    yield "a lag beyond the steps taken", negative_step, {}


def _torch_cases():
    def amsgrad(sd): sd["param_groups"][0]["amsgrad"] = True
    def maximize(sd): sd["param_groups"][0]["maximize"] = True
    def two_groups(sd):
        g = sd["param_groups"][0]
        sd["param_groups"].append(dict(g, params=[g["params"].pop()]))
    def short(sd): sd["param_groups"][0]["params"].pop()
    def wrong_shape(sd): sd["state"][4]["exp_avg"] = torch.zeros(5)
    def stray_state(sd): sd["state"][10 ** 6] = dict(sd["state"][4])
    def fractional_step(sd): sd["state"][4]["step"] = torch.tensor(1.5)
    def nothing(sd): pass
    yield "amsgrad", amsgrad, {}
    yield "maximize", maximize, {}
    yield "two groups into a trainer without groups", two_groups, {}
    yield "one group into a trainer with two", nothing, dict(with_groups=True)
    yield "fewer parameters than the model", short, {}
    yield "wrong shape", wrong_shape, {}
    yield "state of an index no group lists", stray_state, {}
    yield "a step that is no integer", fractional_step, {}


def _torch_dict(entries):
    P = [torch.nn.Parameter(torch.zeros(e.shape)) for e in entries]
    opt = torch.optim.AdamW(P)
    for p in P:
        p.grad = torch.ones_like(p)
    opt.step()
    return opt.state_dict()


@pytest.mark.parametrize("label,mutate,kw", [pytest.param(*c, id=c[0]) for c in _bad_cases()] +
                         [pytest.param("torch: " + c[0], c[1], dict(c[2], plain=True), id="torch: " + c[0]) for c in _torch_cases()])
def test_every_refusal_is_a_value_error_and_writes_nothing(label, mutate, kw):
    entries = _entries()
    if kw.get("plain"):
        sd = _torch_dict(entries)
    else:
        sd = _export(entries, groups=_groups(entries) if kw.get("grouped") else None, ema=kw.get("ema", False))
    mutate(sd)
    m, v, avg = _flat(entries, 11), _flat(entries, 12), (_flat(entries, 13) if kw.get("with_ema") else None)
    m0, v0, a0 = m.clone(), v.clone(), None if avg is None else avg.clone()
    with pytest.raises(ValueError):
        _ts().load(entries, [e.name for e in entries], sd, m, v, avg, _groups(entries) if kw.get("with_groups") else None)
    assert m.numpy().tobytes() == m0.numpy().tobytes() and v.numpy().tobytes() == v0.numpy().tobytes(), label
    assert avg is None or avg.numpy().tobytes() == a0.numpy().tobytes(), label


def test_the_unmutated_dicts_of_the_refusal_cases_load():
    """The control of the test above: without a mutation, each kind of dict is accepted by the side it was written for."""
    entries = _entries()
    _load(entries, _export(entries))
    _load(entries, _export(entries, ema=True), ema=True)
    _load(entries, _export(entries, groups=_groups(entries)), groups=_groups(entries))
    _load(entries, _torch_dict(entries))


# ------------------------------------------------------------------------------------ the two trainer methods, on a trainer without a GPU
class _Engine:
    seed_base, step_id = 0x5EED, 0


class _Reducer:
    sent = "some groups"

    def set_trainable(self, ranges=None):
        self.sent = ranges


def _stub_trainer(seed, ema=True):
    """A HipTrainer that was never constructed (no engine, no device buffers; tests/test_ema_ref_cpu.py does the same): state_dict /
    load_state_dict are host logic over the buffers, which may live on the CPU."""
    from _pkg import pkg
    T = pkg().trainer.HipTrainer
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype="fp32", seed=5)
    entries = m._param_entries
    tr = T.__new__(T)
    tr.model, tr._ema_swapped, tr.engine, tr.reducer = m, False, _Engine(), _Reducer()
    tr.m, tr.v = _flat(entries, seed), _flat(entries, seed + 1).square()
    tr.G = torch.zeros_like(tr.m)
    tr.ema = _flat(entries, seed + 2) if ema else None
    tr.ema_decay, tr.ema_warmup, tr._ema_cnn_stamp = (0.9 if ema else None), False, "made"
    tr._bad, tr._empty = torch.zeros(3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    tr._lag, tr._lag_class, tr._ever_frozen = torch.zeros(len(entries), dtype=torch.int32), [0] * len(entries), False
    tr.calls, tr.lr, tr.betas, tr.eps, tr.wd, tr.max_norm, tr.param_groups = 0, 1e-4, (0.9, 0.999), 1e-8, 0.01, 1.0, None
    tr._copy_sig, tr._group_written, tr._mask, tr._ranges = "sig", "written", (True,), "table"
    tr._graphs, tr._graph_seen, tr.graph_captures = {"key": object()}, {"key": 2, "other": 1}, 1
    return tr


def test_trainer_methods_round_trip_and_reset_what_the_next_step_rebuilds():
    a = _stub_trainer(21)
    n = len(a._lag_class)
    a.calls, a.lr, a.wd, a.max_norm, a.ema_decay, a.ema_warmup = 9, 3e-4, 0.1, 0.5, 0.95, True
    a._bad.copy_(torch.tensor([4, 2, 2], dtype=torch.int32))
    a._empty.fill_(1)
    a._lag[3], a._lag_class[3], a._ever_frozen = 2, 1, True
    a.engine.step_id = 11
    sd = a.state_dict()
    assert a.t == 7 and float(sd["state"][0]["step"]) == 7.0
    names = sd["hip_trainer"]["names"]
    assert names == [k for k, _ in a.model.named_parameters()]
    j3 = names.index(a.model._param_entries[3].name)
    assert float(sd["state"][j3]["step"]) == 5.0 and sd["hip_trainer"]["lag"][j3] == 2
    b = _stub_trainer(31)
    b.load_state_dict(sd)
    assert torch.equal(b.m, a.m) and torch.equal(b.v, a.v) and torch.equal(b.ema, a.ema)
    assert torch.equal(b._bad, a._bad) and torch.equal(b._empty, a._empty) and torch.equal(b._lag, a._lag)
    assert (b.calls, b.t, b._lag_class, b._ever_frozen) == (9, 7, a._lag_class, True)
    assert (b.lr, b.betas, b.eps, b.wd, b.max_norm, b.ema_decay, b.ema_warmup) == (3e-4, (0.9, 0.999), 1e-8, 0.1, 0.5, 0.95, True)
    assert (b.engine.seed_base, b.engine.step_id) == (0x5EED, 11) and b._ema_cnn_stamp is None
    # what the next step rebuilds, and the captured steps: step_graphed starts over like a fresh trainer's
    assert b._copy_sig is None and b._group_written is None and b._mask is None and b._ranges is None
    assert b._graphs == {} and b._graph_seen == {} and b.reducer.sent is None
    sd2 = b.state_dict()
    assert sd2["hip_trainer"].keys() == sd["hip_trainer"].keys()
    for k, v in sd["hip_trainer"].items():
        if k != "ema":
            assert sd2["hip_trainer"][k] == v, k
    assert all(torch.equal(sd2["state"][i][k], sd["state"][i][k]) for i in range(n) for k in ("step", "exp_avg", "exp_avg_sq"))
    # a refusal leaves the host side alone too; inside ema_weights() both methods refuse
    c = _stub_trainer(41, ema=False)
    with pytest.raises(ValueError):
        c.load_state_dict(sd)
    assert c.calls == 0 and c._graphs and c._copy_sig == "sig" and c.reducer.sent == "some groups" and torch.equal(c.m, _flat(c.model._param_entries, 41))
    c._ema_swapped = True
    with pytest.raises(RuntimeError):
        c.state_dict()
    with pytest.raises(RuntimeError):
        c.load_state_dict(sd)


def test_trainer_takes_a_torch_dict_and_keeps_its_counters_average_and_stream():
    a = _stub_trainer(51)
    a._bad.copy_(torch.tensor([4, 2, 2], dtype=torch.int32))
    a._empty.fill_(3)
    a.engine.step_id = 8
    ema0 = a.ema.clone()
    P = list(a.model.parameters())
    opt = torch.optim.AdamW(P, lr=5e-4, betas=(0.8, 0.9), eps=1e-6, weight_decay=0.2)
    for rep in range(2):
        for j, p in enumerate(P):
            p.grad = None if (j == 2 and rep == 0) else torch.ones_like(p)
        opt.step()
    a.load_state_dict(opt.state_dict())
    assert (a.calls, a.t, a._ever_frozen) == (2, 2, True) and a._bad.tolist() == [4, 2, 0] and int(a._empty) == 3
    assert a._lag.tolist() == [1 if j == 2 else 0 for j in range(len(P))]
    assert (a.lr, a.betas, a.eps, a.wd, a.max_norm) == (5e-4, (0.8, 0.9), 1e-6, 0.2, 1.0)
    assert torch.equal(a.ema, ema0) and a.ema_decay == 0.9 and a.engine.step_id == 8 and a._ema_cnn_stamp == "made"
    LY = sub("layout")
    for e, p in zip(a.model._param_entries, a.model._param_list()):
        assert torch.equal(LY.view_of(a.m, e), opt.state[p]["exp_avg"]) and torch.equal(LY.view_of(a.v, e), opt.state[p]["exp_avg_sq"])
    opt2 = torch.optim.AdamW(P)
    opt2.load_state_dict(a.state_dict())                               # and back: the steps torch had
    assert [float(opt2.state[p]["step"]) for p in P] == [float(opt.state[p]["step"]) for p in P]
