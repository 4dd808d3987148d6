"""GPU: HipTrainer(monitor=TensorMonitor(...)), HipTrainer.tensor_stats() and the drop-in utils.monitor.ParameterMonitor.

Small model of tests/test_gpu_nonfinite_trainer.py (embed_dim 32, 10 answers, 64-px images, B = 4, L = 10), fp32 and bf16.  Values are
compared with the float64 reference of tests/_statsref.py computed from trainer.G, model._flat and a clone of the weights taken before
the step: counts and absmax exactly, norms within the kernel's derived bound (_statsref.sumsq_bound; a norm is a square root, so half
of it, and the comparison allows one fp64-rounding more).  Every test fails without the feature: the constructor has no `monitor`."""
import math

import pytest
import torch

import _statsref as R
from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(vocab_size=100, num_answers=10, embed_dim=32)
CFG = O.full_config(dropout=0.1, answer_dropout=0.1, **SMALL)
DTYPES = ["fp32", "bf16"]
_CACHE = {}


def _sd():
    if "sd" not in _CACHE:
        _CACHE["sd"] = O.init_state_dict(CFG, 41, jitter=True)
    return _CACHE["sd"]


def _batch(seed, poison=None, bad_target=False):
    key = ("batch", seed)
    if key not in _CACHE:
        _CACHE[key] = [t.to(DEV) for t in O.synthetic_batch(4, seed=seed, image_size=64, seq_len=10, vocab=100, num_answers=10)]
    images, ids, mask, answers = _CACHE[key]
    if poison is not None:
        images = images.clone()
        images[1, 0, 5, 5] = poison
    if bad_target:
        answers = answers.clone()
        answers[2] = 10
    return images, ids, mask, answers


def _model(dtype, frozen_cnn=False):
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype=dtype)
    m.load_state_dict(_sd())
    m = m.to(DEV).train()
    if frozen_cnn:
        m.image_encoder.requires_grad_(False)
        m.image_encoder.eval()
    return m


def _mon(**kw):
    return sub("monitor").TensorMonitor(**kw)


def _trainer(m, **kw):
    return pkg().trainer.HipTrainer(m, **dict(dict(lr=1e-3, ema_decay=0.99), **kw))


class _Calls:
    """Names of the launches that go through _lib.call, in order."""

    def __enter__(self):
        L = sub("_lib")
        self.names, self._old = [], L._HOOK[0]
        L._HOOK[0] = lambda name, args: self.names.append(name)
        return self

    def __exit__(self, *a):
        sub("_lib")._HOOK[0] = self._old


def _ranges(m):
    return sub("monitor").layout_ranges(m._param_entries)


def _close(got, ref_sumsq, numel, scale=1.0, pair=False, what=""):
    """norm fields (float64 [P]) against sqrt of the reference's float64 sums of squares, each within its row's bound"""
    C = sub("kernels").STATS_CHUNK
    for j, (g, r, n) in enumerate(zip(got.tolist(), ref_sumsq.tolist(), numel)):
        want = math.sqrt(r) * scale
        assert abs(g - want) <= (R.sumsq_bound(n, C, pair) + 2.0 ** -50) * want, (what, j, n, g, want)


def _check_record(rec, m, G, flat_before, gscale, what=""):
    """A record against float64 from the gradient, the weights as they are and the weights of before the step."""
    ranges = _ranges(m)
    numel = [hi - lo for lo, hi in ranges]
    flat = m._flat.detach()
    assert rec.names == [e.name for e in m._param_entries] and rec.numel.tolist() == numel
    g, p, u = R.table(G, ranges), R.table(flat, ranges), R.table(flat, ranges, flat_before)
    _close(rec.grad_norm, g["sumsq"], numel, gscale, what=what + " grad")
    _close(rec.param_norm, p["sumsq"], numel, what=what + " param")
    _close(rec.update_norm, u["sumsq"], numel, pair=True, what=what + " update")
    assert torch.equal(rec.grad_absmax, g["absmax"] * gscale), what    # (an fp32 word times the scale, in double)
    assert torch.equal(rec.param_absmax, p["absmax"]) and torch.equal(rec.update_absmax, u["absmax"]), what
    assert torch.equal(rec.grad_nonfinite, g["nonfinite"]) and torch.equal(rec.grad_zeros, g["zeros"]), what
    assert torch.equal(rec.param_nonfinite, p["nonfinite"]), what
    assert torch.equal(rec.update_unchanged, u["zeros"]), what
    ratio = torch.where(rec.param_norm > 0, rec.update_norm / rec.param_norm.clamp_min(1e-300), torch.zeros_like(rec.param_norm))
    assert torch.equal(rec.update_ratio, ratio), what


# ----------------------------------------------------------------------------------------------------------------- launch lists
@pytest.mark.parametrize("dtype", DTYPES)
def test_launch_lists(dtype):
    plain_tr = _trainer(_model(dtype))
    assert plain_tr.monitor is None
    lists = []
    for s in (200, 201, 202):
        with _Calls() as c:
            plain_tr.step(*_batch(s))
        lists.append(list(c.names))
    assert not any("vqa_tensor_stats" in l for l in lists)             # monitor=None: never
    mon = _mon(every=3, slots=4)
    tr = _trainer(_model(dtype), monitor=mon)
    got = []
    for s in (200, 201, 202):
        with _Calls() as c:
            tr.step(*_batch(s))
        got.append(list(c.names))
    assert got[0] == lists[0] and got[1] == lists[1]                   # the two non-due steps: the plain step's list
    due = got[2]
    assert [n for n in due if n != "vqa_tensor_stats"] == lists[2]
    assert due.count("vqa_tensor_stats") == 3 and due[-3:] == ["vqa_tensor_stats"] * 3
    last_adamw = max(i for i, n in enumerate(due) if n.startswith("vqa_adamw"))
    assert last_adamw < len(due) - 3
    assert mon.records == 1 and mon.dropped == 0
    with pytest.raises(TypeError):
        _trainer(_model(dtype), monitor=object())


# ------------------------------------------------------------------------------------------------------------------- reads only
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_monitored_run_keeps_the_unmonitored_bits(dtype):
    def run(monitor):
        m = _model(dtype)
        tr = _trainer(m, monitor=monitor)
        outs = []
        for s in range(6):
            loss, logits = tr.step(*_batch(210 + s))
            outs.append((loss.clone(), logits.clone()))
        torch.cuda.synchronize()
        return m, tr, outs
    ma, ta, oa = run(None)
    mon = _mon(every=2, slots=8)
    mb, tb, ob = run(mon)
    for (la, ga), (lb, gb) in zip(oa, ob):
        assert torch.equal(la, lb) and torch.equal(ga, gb)
    for a, b in ((ma._flat, mb._flat), (ta.m, tb.m), (ta.v, tb.v), (ta.ema, tb.ema)):
        assert torch.equal(a.detach(), b.detach())
    for (na, a), (nb, b) in zip(sorted(ma.named_buffers()), sorted(mb.named_buffers())):
        assert na == nb and torch.equal(a, b), na
    assert [r.step for r in mon.read()] == [2, 4, 6] and mon.read() == []


# ----------------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_due_steps_record_against_float64(dtype):
    m = _model(dtype)
    mon = _mon(every=2, slots=4)
    tr = _trainer(m, monitor=mon)
    tr.step(*_batch(220))
    before = m._flat.detach().clone()
    tr.step(*_batch(221))
    (rec,) = mon.read()
    assert rec.step == 2 and rec.trainable.all()
    _check_record(rec, m, tr.G, before, 1.0, what=dtype)
    assert int(rec.update_unchanged.sum()) < int(rec.numel.sum()) and float(rec.update_ratio.max()) > 0
    # the per-parameter norms add up to the global norm the step clipped.  That one is vqa_sumsq's fp32 sum, folded in another order
    # with a chain no longer than a single row of all n_all elements would have here: twice that row's bound covers both sums
    total = math.sqrt(float((rec.grad_norm[rec.trainable] ** 2).sum()))
    n_all = sum(hi - lo for lo, hi in _ranges(m))
    print(f"global norm: sum of rows {total!r}, grad_norm() {float(tr.grad_norm())!r}")
    assert abs(total - float(tr.grad_norm())) <= 2 * R.sumsq_bound(n_all, sub("kernels").STATS_CHUNK) * total
    assert rec.worst("grad_norm", k=1) == [rec.names[int(rec.grad_norm.argmax())]]


# ----------------------------------------------------------------------------------------------------------------- interactions
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_bad_target_step_records_a_zero_update(dtype):
    m = _model(dtype)
    mon = _mon(every=1, slots=4)
    tr = _trainer(m, monitor=mon)
    tr.step(*_batch(230))
    before = m._flat.detach().clone()
    tr.step(*_batch(231, bad_target=True))
    recs = mon.read()
    assert [r.step for r in recs] == [1, 2]
    bad = recs[1]
    assert torch.equal(m._flat.detach(), before)
    assert torch.equal(bad.update_unchanged, bad.numel) and not bad.update_norm.any() and not bad.update_absmax.any() and not bad.update_ratio.any()
    assert float(recs[0].update_norm.max()) > 0
    with pytest.raises(IndexError):
        tr.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_poisoned_step_under_the_guard_names_the_reports_parameters(dtype):
    m = _model(dtype)
    mon = _mon(every=1, slots=4)
    tr = _trainer(m, nonfinite="skip", monitor=mon)
    tr.step(*_batch(240))
    before = m._flat.detach().clone()
    tr.step(*_batch(241, poison=float("nan")))
    rep = tr.nonfinite_report()
    rec = mon.read()[1]
    assert rep is not None and rep.step == rec.step == 2
    named = [(n, int(c), int(k)) for n, c, k in zip(rec.names, rec.grad_nonfinite.tolist(), rec.numel.tolist()) if c]
    assert named == [tuple(p) for p in rep.parameters] and named
    assert torch.equal(m._flat.detach(), before) and torch.equal(rec.update_unchanged, rec.numel) and not rec.update_norm.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_parameters_keep_their_rows(dtype):
    m = _model(dtype, frozen_cnn=True)
    mon = _mon(every=1, slots=2)
    tr = _trainer(m, monitor=mon)
    before = m._flat.detach().clone()
    tr.step(*_batch(250))
    (rec,) = mon.read()
    frozen = torch.tensor([not p.requires_grad for p in m._param_list()])
    assert frozen.any() and not frozen.all() and torch.equal(rec.trainable, ~frozen)
    assert torch.equal(rec.grad_zeros[frozen], rec.numel[frozen]) and not rec.update_norm[frozen].any()
    assert torch.equal(rec.update_unchanged[frozen], rec.numel[frozen]) and float(rec.param_norm[frozen].max()) > 0
    assert float(rec.update_norm[~frozen].max()) > 0
    _check_record(rec, m, tr.G, before, 1.0, what="frozen")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_window_is_one_record_scaled_by_its_size(dtype):
    m = _model(dtype)
    mon = _mon(every=1, slots=4)
    tr = _trainer(m, monitor=mon)
    before = m._flat.detach().clone()
    with _Calls() as c:
        tr.accumulate(*_batch(260))
        tr.accumulate(*_batch(261))
    assert "vqa_tensor_stats" not in c.names and mon.records == 0     # accumulate() never records
    with pytest.raises(RuntimeError):
        tr.tensor_stats()                                              # a window is open
    tr.step(*_batch(262))
    (rec,) = mon.read()
    assert rec.step == 1 == tr.calls
    _check_record(rec, m, tr.G, before, 1.0 / 3.0, what="window")     # G holds the window's SUM; the record is scaled by 1 / 3


def test_step_graphed_hands_due_steps_to_the_eager_step():
    def run(monitor):
        m = _model("bf16")
        tr = _trainer(m, monitor=monitor)
        outs = []
        for s in range(8):
            loss, logits = tr.step_graphed(*_batch(270 + s % 3))
            outs.append((loss.clone(), logits.clone()))
        torch.cuda.synchronize()
        return m, tr, outs
    ma, ta, oa = run(None)
    mon = _mon(every=2, slots=8)
    mb, tb, ob = run(mon)
    for (la, ga), (lb, gb) in zip(oa, ob):
        assert torch.equal(la, lb) and torch.equal(ga, gb)
    for a, b in ((ma._flat, mb._flat), (ta.m, tb.m), (ta.v, tb.v), (ta.ema, tb.ema)):
        assert torch.equal(a.detach(), b.detach())
    assert [r.step for r in mon.read()] == [2, 4, 6, 8]
    assert ta.graph_captures >= 1 and tb.graph_captures >= 1          # the non-due calls still reach their graph


def test_a_full_ring_drops_its_oldest_record():
    m = _model("bf16")
    mon = _mon(every=1, slots=2)
    tr = _trainer(m, monitor=mon)
    for s in range(3):
        tr.step(*_batch(280 + s))
    recs = mon.read()
    assert [r.step for r in recs] == [2, 3] and mon.dropped == 1 and mon.records == 3
    tr.step(*_batch(283))
    mon.clear()
    assert mon.read() == [] and mon.dropped == 1
    assert "monitor" not in tr.state_dict()["hip_trainer"] and tr.state_dict()["hip_trainer"]["calls"] == 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_stats_between_steps(dtype):
    m = _model(dtype)
    tr = _trainer(m)                                                   # (no monitor needed)
    tr.step(*_batch(290))
    tr.step(*_batch(291))
    with _Calls() as c:
        rec = tr.tensor_stats(("grad", "param", "moment2"))
    assert c.names == ["vqa_tensor_stats"] * 3
    ranges = _ranges(m)
    numel = [hi - lo for lo, hi in ranges]
    assert rec.step == 2 and rec.update_norm is None and rec.update_ratio is None and rec.moment1_norm is None
    for field, buf in (("grad", tr.G), ("param", m._flat.detach()), ("moment2", tr.v)):
        ref = R.table(buf, ranges)
        _close(getattr(rec, field + "_norm"), ref["sumsq"], numel, what=field)
        assert torch.equal(getattr(rec, field + "_absmax"), ref["absmax"]) and torch.equal(getattr(rec, field + "_nonfinite"), ref["nonfinite"])
        assert torch.equal(getattr(rec, field + "_zeros"), ref["zeros"])
    e = tr.tensor_stats("ema")
    _close(e.ema_norm, R.table(tr.ema, ranges)["sumsq"], numel, what="ema")
    for bad in (("update",), ("grad", "grad"), (), ("weights",)):
        with pytest.raises(ValueError):
            tr.tensor_stats(bad)
    with tr.ema_weights():
        with pytest.raises(RuntimeError):
            tr.tensor_stats()
    with pytest.raises(RuntimeError):
        pkg().trainer.HipTrainer(m, lr=1e-3).tensor_stats(("ema",))


# -------------------------------------------------------------------------------------------------------------- torch.optim loops
def test_parameter_monitor_on_a_torch_optim_loop():
    PM = pkg().load_dropin_monitor()
    m = _model("fp32")
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    mon = PM.ParameterMonitor(m, every=1, slots=4)
    ranges = _ranges(m)
    numel = [hi - lo for lo, hi in ranges]
    for s in range(3):
        images, ids, mask, answers = _batch(300 + s)
        opt.zero_grad(set_to_none=True)
        logits, _ = m(images, ids, mask)
        torch.nn.functional.cross_entropy(logits, answers).backward()
        if s == 2:                                                     # a .grad that is no slice of the flat gradient any more
            p = m._param_list()[3]
            p.grad = p.grad.clone()
        before = m._flat.detach().clone()
        grads = [p.grad.detach().clone() for p in m._param_list()]
        mon.before_step()
        opt.step()
        mon.after_step()
        rec = mon.read()[-1]
        assert rec.step == s + 1 == mon.calls
        flat = m._flat.detach()
        p_ref, u_ref = R.table(flat, ranges), R.table(flat, ranges, before)
        _close(rec.param_norm, p_ref["sumsq"], numel, what="param")
        _close(rec.update_norm, u_ref["sumsq"], numel, pair=True, what="update")
        assert torch.equal(rec.param_absmax, p_ref["absmax"]) and torch.equal(rec.update_absmax, u_ref["absmax"])
        assert torch.equal(rec.update_unchanged, u_ref["zeros"]) and float(rec.update_norm.max()) > 0
        if s < 2:
            want = [math.sqrt(float((g.double() ** 2).sum())) for g in grads]
            for j, (g, w) in enumerate(zip(rec.grad_norm.tolist(), want)):
                assert abs(g - w) <= (R.sumsq_bound(numel[j], sub("kernels").STATS_CHUNK) + 2.0 ** -50) * w, (j, g, w)
            assert not rec.grad_nonfinite.any()
        else:
            assert rec.grad_norm is None and rec.grad_absmax is None and rec.grad_nonfinite is None and rec.grad_zeros is None
    assert mon.dropped == 0
