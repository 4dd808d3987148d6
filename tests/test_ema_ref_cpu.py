"""CPU: the float64 reference of the weight average (tests/_emaref.py) pinned against torch.lerp and hand-written decays, and the host
logic of the average (ema.py, HipTrainer's EMA methods, utils.ema.ParameterEMA) on a trainer that makes no GPU call."""
import math

import pytest
import torch

import _emaref as R
from _pkg import pkg, sub
from oracle import vqa_oracle as O

CFG = O.full_config(embed_dim=32, vocab_size=100, num_answers=10)


# ---- the reference itself
def test_reference_is_torch_lerp_in_float64():
    g = torch.Generator().manual_seed(1)
    ema, p = torch.randn(1000, generator=g, dtype=torch.float64), torch.randn(1000, generator=g, dtype=torch.float64)
    for d in (0.0, 0.3, 0.999, 1.0):
        got = R.ema_step(ema, p, d, False, 7)
        ref = torch.lerp(p, ema, d)                                 # p + d * (ema - p) = d * ema + (1 - d) * p
        assert float((got - ref).abs().max()) <= 4 * 2.0 ** -52 * float(torch.maximum(ema.abs(), p.abs()).max())
    assert torch.equal(R.ema_step(ema, p, 0.0, False, 1), p) and torch.equal(R.ema_step(ema, p, 1.0, False, 1), ema)


def test_warmup_decays_by_hand():
    for t, d in ((1, 2 / 11), (2, 3 / 12), (10, 11 / 20), (10_000, 0.999)):
        assert R.decay_at(0.999, True, t) == d
        assert R.decay_at(0.999, False, t) == 0.999
    assert R.decay_at(0.1, True, 1) == 0.1                          # the decay caps the warm-up, also at the first step
    E = sub("ema")                                                  # the host rule ParameterEMA uses is the same rule
    for t in (1, 2, 10, 8990, 8991, 10_000):
        assert E.decay_at(0.999, True, t) == R.decay_at(0.999, True, t) and E.decay_at(0.999, False, t) == 0.999


def test_skip_and_per_range_steps():
    g = torch.Generator().manual_seed(2)
    ema, p = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
    assert torch.equal(R.ema_step(ema, p, 0.9, True, 3, skip=True), ema)
    ranges = [(8, 24, 0), (32, 60, 1)]
    out = R.ema_step_ranges(ema, p, ranges, [3, 1], 0.999, True)
    inside = torch.zeros(64, dtype=torch.bool)
    inside[8:24] = True; inside[32:60] = True
    assert torch.equal(out[~inside], ema[~inside])                  # outside: untouched
    assert torch.equal(out[8:24], (4 / 13) * ema[8:24] + (1 - 4 / 13) * p[8:24])      # t = 3
    assert torch.equal(out[32:60], (2 / 11) * ema[32:60] + (1 - 2 / 11) * p[32:60])   # t = 1: its own warm-up
    assert torch.equal(R.ema_step_ranges(ema, p, ranges, [3, 1], 0.999, True, skip=True), ema)
    # replay = the steps one after the other
    snaps = [torch.randn(64, generator=g) for _ in range(3)]
    e = ema
    for t, s in enumerate(snaps, start=1):
        e = R.ema_step(e, s, 0.9, True, t)
    assert torch.equal(R.replay(ema, snaps, 0.9, True), e)


# ---- host logic, no GPU
def _stub_trainer():
    """A HipTrainer that was never constructed (no engine, no device buffers): the EMA methods only need .model and .ema."""
    T = pkg().trainer.HipTrainer
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype="fp32", seed=5)
    tr = T.__new__(T)
    tr.model, tr._ema_swapped = m, False
    g = torch.Generator().manual_seed(9)
    tr.ema = torch.randn(m._flat.numel(), generator=g)
    return tr, m


def test_ema_state_dict_has_the_models_keys_parameters_from_the_average_buffers_from_the_model():
    tr, m = _stub_trainer()
    msd = m.state_dict()
    sd = tr.ema_state_dict()
    assert list(sd.keys()) == list(msd.keys())
    names = {n for n, _ in m.named_parameters()}
    lay = sub("layout")
    ent = {e.name: e for e in m._param_entries}
    assert names == set(ent)
    for k, v in sd.items():
        assert v.shape == msd[k].shape and v.dtype == msd[k].dtype, k
        assert v.data_ptr() != msd[k].data_ptr()                    # a clone: not the model's storage
        if k in names:
            assert torch.equal(v, lay.view_of(tr.ema, ent[k])), k
            assert v.untyped_storage().data_ptr() != tr.ema.untyped_storage().data_ptr()
        else:
            assert torch.equal(v, msd[k]), k
    assert any("running_mean" in k for k in sd) and len(names) == 164
    # loads strict=True into a second model, which then holds the average
    m2 = pkg().load_dropin().VQAModel(**CFG, compute_dtype="fp32", seed=6)
    m2.load_state_dict(sd, strict=True)
    for e in m._param_entries:
        assert torch.equal(lay.view_of(m2._flat, e), lay.view_of(tr.ema, e)), e.name


def test_load_ema_state_dict_round_trip_and_errors():
    tr, m = _stub_trainer()
    sd = tr.ema_state_dict()
    before = tr.ema.clone()
    tr.ema.zero_()
    tr.load_ema_state_dict(sd)
    lay = sub("layout")
    for e in m._param_entries:
        assert torch.equal(lay.view_of(tr.ema, e), lay.view_of(before, e)), e.name
    # buffer keys are ignored: a dict of the parameters alone loads
    only_params = {k: v for k, v in sd.items() if k in dict(m.named_parameters())}
    tr.load_ema_state_dict(only_params)
    first, last = m._param_entries[0].name, m._param_entries[-1].name
    missing = {k: v for k, v in sd.items() if k != last}
    kept = tr.ema.clone()
    with pytest.raises(KeyError):
        tr.load_ema_state_dict(missing)
    bad = dict(sd)
    bad[last] = torch.zeros(tuple(sd[last].shape) + (2,))
    bad[first] = torch.full_like(sd[first], 7.0)
    with pytest.raises(ValueError):
        tr.load_ema_state_dict(bad)
    assert torch.equal(tr.ema, kept)                                # checked before anything is written


@pytest.mark.parametrize("decay", [-0.1, 1.1, float("nan")])
def test_bad_decay_raises_before_anything_is_touched(decay):
    T = pkg().trainer.HipTrainer

    class Untouchable:                                              # any attribute access would be a launch-side effect
        def __getattr__(self, name):
            raise AssertionError(f"model.{name} was touched before ema_decay was validated")

    with pytest.raises(ValueError):
        T(Untouchable(), ema_decay=decay)
    with pytest.raises(ValueError):
        pkg().load_dropin_ema().ParameterEMA(Untouchable(), decay)
    # the attribute may be changed between steps and is validated again when it is used
    E = sub("ema")
    with pytest.raises(ValueError):
        E.check_decay(decay)
    for ok in (0, 0.0, 1, 1.0, 0.999):
        assert E.check_decay(ok) == float(ok)


def test_no_average_without_ema_decay():
    tr, _ = _stub_trainer()
    tr.ema = None
    for call in (tr.ema_state_dict, lambda: tr.load_ema_state_dict({}), lambda: tr.ema_weights().__enter__()):
        with pytest.raises(RuntimeError):
            call()


def test_swapped_exchanges_and_restores_also_after_an_exception():
    tr, m = _stub_trainer()
    p0, e0 = m._flat.clone(), tr.ema.clone()
    v0, ep0 = m._flat._version, m._ctx_epoch
    with tr.ema_weights() as inner:
        assert inner is m and tr._ema_swapped
        assert torch.equal(m._flat, e0) and torch.equal(tr.ema, p0)
        assert m._flat._version > v0 and m._ctx_epoch > ep0         # what invalidates contexts and the bf16 operand copy
        v1 = m._flat._version
        assert torch.equal(dict(m.named_parameters())[m._param_entries[3].name], sub("layout").view_of(e0, m._param_entries[3]))
        with pytest.raises(RuntimeError):
            tr.step(None, None, None, None)                         # refused before anything else is looked at
        with pytest.raises(RuntimeError):
            tr.ema_weights().__enter__()                            # not re-entrant
    assert not tr._ema_swapped and m._flat._version > v1
    assert torch.equal(m._flat, p0) and torch.equal(tr.ema, e0)
    with pytest.raises(ZeroDivisionError):
        with tr.ema_weights():
            1 / 0
    assert not tr._ema_swapped and torch.equal(m._flat, p0) and torch.equal(tr.ema, e0)


def test_parameter_ema_host_side():
    P = pkg().load_dropin_ema().ParameterEMA
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype="fp32", seed=5)
    ema = P(m, 0.999, warmup=True)
    assert ema.num_updates == 0 and torch.equal(ema.ema, m._flat) and ema.ema.data_ptr() != m._flat.data_ptr()
    with pytest.raises(RuntimeError):
        ema.update()                                                # CPU model: no CPU path, nothing is counted
    assert ema.num_updates == 0
    sd = ema.state_dict()
    assert list(sd.keys()) == list(m.state_dict().keys())
    avg = ema.ema.clone()
    with torch.no_grad():
        m._flat.mul_(2.0)
    live = m._flat.clone()
    with ema.average_weights():
        assert torch.equal(m._flat, avg) and torch.equal(ema.ema, live)
    assert torch.equal(m._flat, live) and torch.equal(ema.ema, avg)
    ema.load_state_dict(m.state_dict(), num_updates=12)
    assert ema.num_updates == 12 and torch.equal(ema.ema, m._flat)
    # .to() re-flattens the parameters into a new buffer: the average re-binds to it and keeps its values
    old = ema.ema.clone()
    m.to(torch.float32)                                             # (_apply always re-flattens)
    assert m._flat is not ema._flat
    ema.state_dict()
    assert ema._flat is m._flat and torch.equal(ema.ema, old)
    assert math.isclose(sub("ema").decay_at(ema.decay, ema.warmup, ema.num_updates + 1), 14 / 23)


def test_utils_ema_resolves_in_a_bound_checkout():
    B = sub("binding")
    assert B._DROPIN_ONLY["utils.ema"] == ("utils", "ema.py")
    spec = B._DropinOnlyFinder().find_spec("utils.ema")
    assert spec is not None and spec.origin.endswith("dropin/utils/ema.py")
    import os
    assert os.path.isfile(spec.origin)
