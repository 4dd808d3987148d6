"""HipTrainer(nonfinite="skip" | "raise"): a step whose gradient is not finite is skipped on the device and never happened.
Small model of tests/test_gpu_step_graph.py (embed_dim 32, 10 answers, 64-px images, B = 4, L = 10), fp32 and bf16.  The poison is
one pixel of the float image tensor, images[1, 0, 5, 5] = NaN (once +inf): with the CNN in train mode the batch statistics carry it
into every row, with a frozen eval-mode CNN it stays in row 1.  Every comparison is torch.equal."""
import math
import multiprocessing as mp
import os
import socket
import time

import pytest
import torch
import torch.distributed as dist

from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(vocab_size=100, num_answers=10, embed_dim=32)
CFG = O.full_config(dropout=0.1, answer_dropout=0.1, **SMALL)
CFG0 = O.full_config(dropout=0.0, answer_dropout=0.0, **SMALL)
DTYPES = ["fp32", "bf16"]
NEW_ENTRIES = {"vqa_sumsq_guard", "vqa_sumsq_ranges_guard", "vqa_buffers_save", "vqa_buffers_restore", "vqa_nonfinite_scan"}
_CACHE = {}


def _sd():
    if "sd" not in _CACHE:
        _CACHE["sd"] = O.init_state_dict(CFG, 41, jitter=True)
    return _CACHE["sd"]


def _batch(seed, poison=None):
    key = ("batch", seed)
    if key not in _CACHE:
        _CACHE[key] = [t.to(DEV) for t in O.synthetic_batch(4, seed=seed, image_size=64, seq_len=10, vocab=100, num_answers=10)]
    images, ids, mask, answers = _CACHE[key]
    if poison is not None:
        images = images.clone()
        images[1, 0, 5, 5] = poison
    return images, ids, mask, answers


def _model(dtype, frozen_cnn=False, cfg=CFG):
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(_sd())
    m = m.to(DEV).train()
    if frozen_cnn:
        m.image_encoder.requires_grad_(False)
        m.image_encoder.eval()
    return m


def _trainer(m, **kw):
    return pkg().trainer.HipTrainer(m, **dict(dict(lr=1e-3, ema_decay=0.99), **kw))


def _state(m, tr):
    """Everything a skipped step must leave alone: the model's state dict (BatchNorm buffers and num_batches_tracked included),
    both moments, the average, the lags and the bf16 operand copy when there is one."""
    torch.cuda.synchronize()
    out = {"model." + k: v.detach().clone() for k, v in m.state_dict().items()}
    out.update(m=tr.m.clone(), v=tr.v.clone(), lag=tr._lag.clone())
    if tr.ema is not None:
        out["ema"] = tr.ema.clone()
    copy = tr.engine.adamw_copy_target()
    if copy is not None:
        out["operand_copy"] = copy.clone()
    return out


def _assert_same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


class _Calls:
    """Names of the launches that go through _lib.call, in order."""

    def __enter__(self):
        L = sub("_lib")
        self.names, self._old = [], L._HOOK[0]
        L._HOOK[0] = lambda name, args: self.names.append(name)
        return self

    def __exit__(self, *a):
        sub("_lib")._HOOK[0] = self._old


# ------------------------------------------------------------------------------------------------------- the option is opt-in
@pytest.mark.parametrize("dtype", DTYPES)
def test_without_the_option_the_step_issues_none_of_the_new_launches(dtype):
    m = _model(dtype)
    tr = _trainer(m)
    assert tr.nonfinite is None
    with _Calls() as c:
        tr.step(*_batch(200))
    plain = list(c.names)
    with _Calls() as c:
        tr.step(*_batch(201))
    assert not NEW_ENTRIES & set(plain + c.names)
    assert plain.count("vqa_sumsq") == c.names.count("vqa_sumsq") == 1 and plain.count("vqa_adamw_ema") == c.names.count("vqa_adamw_ema") == 1
    assert "nonfinite" not in tr.state_dict()["hip_trainer"]
    for name in ("skipped_nonfinite", "nonfinite_report"):
        with pytest.raises(RuntimeError, match="nonfinite"):
            getattr(tr, name)()
    # the guarded step: the same launches with the guarded norm in the plain one's place and the two over the BatchNorm buffers
    g = _trainer(_model(dtype), nonfinite="skip")
    with _Calls() as cg:
        g.step(*_batch(200))
    assert [n for n in cg.names if not n.startswith("vqa_buffers_")] == ["vqa_sumsq_guard" if n == "vqa_sumsq" else n for n in plain]
    assert cg.names[0] == "vqa_buffers_save" and cg.names[-1] == "vqa_buffers_restore" and cg.names.count("vqa_buffers_save") == 1
    # a frozen eval-mode CNN moves no BatchNorm buffer: neither launch
    f = _trainer(_model(dtype, frozen_cnn=True), nonfinite="skip")
    with _Calls() as cf:
        f.step(*_batch(200))
    assert "vqa_sumsq_ranges_guard" in cf.names and not any(n.startswith("vqa_buffers_") for n in cf.names)


# ---------------------------------------------------------------------------------- a poisoned step X after a clean step A
def _poisoned_step(dtype, mode, poison, **kw):
    m = _model(dtype)
    tr = _trainer(m, nonfinite=mode, **kw)
    la, _ = tr.step(*_batch(200))
    assert math.isfinite(la.item()) and tr.t == 1 and tr.skipped_nonfinite() == (0, 0) and tr.nonfinite_report() is None
    before = _state(m, tr)
    lx, logits = tr.step(*_batch(201, poison))
    after = _state(m, tr)
    _assert_same(before, after, "X")
    assert math.isnan(lx.item()) and logits.shape == (4, 10) and not bool(torch.isfinite(logits).any())
    assert not bool(torch.isfinite(tr.grad_norm()).any())
    assert tr.t == 1 and tr.calls == 2
    assert tr.skipped_nonfinite() == (1, 1) and tr.skipped_nonfinite() == (0, 1)
    rep = tr.nonfinite_report()
    assert rep.step == 2 and math.isnan(rep.loss) and rep.rows.dtype == torch.int64 and rep.rows.tolist() == [0, 1, 2, 3]
    names = [e.name for e in m._param_entries]
    assert rep.parameters and [n for n, _, _ in rep.parameters] == [n for n in names if n in {p[0] for p in rep.parameters}]
    assert all(1 <= k <= numel for _, k, numel in rep.parameters)
    if mode == "skip":
        tr.check()
    else:
        with pytest.raises(FloatingPointError, match="1 step"):
            tr.check()
        tr.check()
    _assert_same(before, _state(m, tr), "after check")
    lb, _ = tr.step(*_batch(202))                        # the run goes on
    assert math.isfinite(lb.item()) and tr.t == 2
    tr.check()


@pytest.mark.parametrize("mode,poison", [("skip", float("nan")), ("raise", float("nan")), ("skip", float("inf"))])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_poisoned_step_leaves_every_bit_of_the_state(dtype, mode, poison):
    _poisoned_step(dtype, mode, poison)


# ------------------------------------------------------------------------------------------------ a skipped step never happened
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_skipped_step_never_happened(dtype):
    """Dropout 0, so that the dropout stream's advance over X changes nothing: A, X, B on the guarded trainer equals A, B."""
    ma, mb = _model(dtype, cfg=CFG0), _model(dtype, cfg=CFG0)
    ta, tb = _trainer(ma, nonfinite="skip"), _trainer(mb, nonfinite="skip")
    for seed, poison in ((200, None), (201, float("nan")), (202, None)):
        la, lga = ta.step(*_batch(seed, poison))
    for seed in (200, 202):
        lb, lgb = tb.step(*_batch(seed))
    assert math.isfinite(la.item()) and torch.equal(la, lb) and torch.equal(lga, lgb)
    _assert_same(_state(ma, ta), _state(mb, tb))
    assert ta.t == tb.t == 2 and (ta.calls, tb.calls) == (3, 2)
    assert ta.skipped_nonfinite() == (1, 1) and tb.skipped_nonfinite() == (0, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_under_the_guard_a_bad_target_step_restores_the_batchnorm_buffers_and_stays_a_bad_target_step(dtype):
    m = _model(dtype)
    tr = _trainer(m, nonfinite="raise")
    tr.step(*_batch(200))
    before = _state(m, tr)
    images, ids, mask, answers = _batch(201)
    bad = answers.clone()
    bad[2] = 10
    tr.step(images, ids, mask, bad)
    _assert_same(before, _state(m, tr))
    assert tr.t == 1 and tr.skipped_nonfinite() == (0, 0) and tr.nonfinite_report() is None
    with pytest.raises(IndexError):
        tr.check()
    tr.check()


# ------------------------------------------------------------------------------------------------------------ ranges and groups
@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_cnn_with_parameter_groups(dtype):
    m = _model(dtype, frozen_cnn=True)
    tr = _trainer(m, nonfinite="skip", param_groups=sub("finetune").no_weight_decay_groups(m))
    tr.step(*_batch(200))
    assert tr.nonfinite_report() is None                                  # after a clean step
    before = _state(m, tr)
    with _Calls() as c:
        lx, _ = tr.step(*_batch(201, float("nan")))
    assert "vqa_sumsq_ranges_guard" in c.names and "vqa_adamw_groups_ema" in c.names and not NEW_ENTRIES & set(c.names) - {"vqa_sumsq_ranges_guard"}
    _assert_same(before, _state(m, tr))
    assert math.isnan(lx.item()) and tr.t == 1 and tr.skipped_nonfinite() == (1, 1)
    rep = tr.nonfinite_report()
    assert rep.rows.tolist() == [1]                                       # an eval-mode CNN keeps the NaN in its row
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    assert rep.parameters and all(n in trainable and not n.startswith("image_encoder.") for n, _, _ in rep.parameters)
    assert all(1 <= k <= numel for _, k, numel in rep.parameters)
    assert tr.nonfinite_report() is not None                              # still the last step
    tr.step(*_batch(202))
    assert tr.nonfinite_report() is None and tr.t == 2                    # reported above: nothing went by unseen


@pytest.mark.parametrize("dtype", DTYPES)
def test_report_raises_once_a_later_step_has_overwritten_the_gradient(dtype):
    m = _model(dtype, frozen_cnn=True)
    tr = _trainer(m, nonfinite="skip")
    assert tr.nonfinite_report() is None                                  # before any step
    tr.step(*_batch(200))
    assert tr.nonfinite_report() is None
    tr.step(*_batch(201, float("nan")))
    tr.step(*_batch(202))
    with pytest.raises(RuntimeError, match="before the next"):
        tr.nonfinite_report()
    assert tr.nonfinite_report() is None and tr.skipped_nonfinite() == (1, 1)


# ----------------------------------------------------------------------------------------------------------------- step_graphed
@pytest.mark.parametrize("frozen_cnn", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_step_graphed_skips_inside_a_replay(dtype, frozen_cnn):
    """Five calls on the images route, dropout 0.1: two eager, the capture, and two replays, the first of them poisoned.  The guarded
    eager trainer on a second model is the yardstick after every call.  (frozen_cnn False adds the BatchNorm buffers' save and
    restore to the captured launches.)"""
    ma, mb = _model(dtype, frozen_cnn), _model(dtype, frozen_cnn)
    ta, tb = _trainer(ma, nonfinite="raise"), _trainer(mb, nonfinite="raise")
    for call in range(5):
        batch = _batch(200 + call, float("nan") if call == 3 else None)
        before = _state(mb, tb)
        la, lga = ta.step(*batch)
        lb, lgb = tb.step_graphed(*batch)
        sa, sb = _state(ma, ta), _state(mb, tb)
        _assert_same(sa, sb, call)
        if call == 3:
            assert math.isnan(la.item()) and math.isnan(lb.item())
            _assert_same(before, sb, "X")
            assert tb.nonfinite_report().rows.tolist() == ([1] if frozen_cnn else [0, 1, 2, 3])
        else:
            assert math.isfinite(la.item()) and torch.equal(la, lb) and torch.equal(lga, lgb)
            assert tb.nonfinite_report() is None
    assert tb.graph_captures == 1 and ta.t == tb.t == 4
    assert ta.skipped_nonfinite() == tb.skipped_nonfinite() == (1, 1)
    with pytest.raises(FloatingPointError):
        tb.check()


# ------------------------------------------------------------------------------------------------------------------- state dict
def test_counters_travel_through_the_state_dict():
    dtype = "bf16"
    m = _model(dtype, frozen_cnn=True)
    tr = _trainer(m, nonfinite="raise")
    tr.step(*_batch(200))
    tr.step(*_batch(201, float("nan")))
    tr.step(*_batch(202))
    sd, msd = tr.state_dict(), {k: v.clone() for k, v in m.state_dict().items()}
    assert sd["hip_trainer"]["nonfinite"] == {"mode": "raise", "since": 1, "ever": 1, "unchecked": 1}
    assert sd["hip_trainer"]["skipped_ever"] == 1 and sd["hip_trainer"]["bad_targets"] == [0, 0]
    m2 = _model(dtype, frozen_cnn=True)
    m2.load_state_dict(msd)
    t2 = _trainer(m2, nonfinite="raise")
    t2.load_state_dict(sd)
    assert t2.t == 2 and t2.calls == 3
    with pytest.raises(FloatingPointError, match="1 step"):
        t2.check()
    assert t2.skipped_nonfinite() == (1, 1) and t2.nonfinite_report() is None
    la, _ = tr.step(*_batch(203))
    lb, _ = t2.step(*_batch(203))                                          # the resumed run continues bit for bit
    assert torch.equal(la, lb)
    _assert_same(_state(m, tr), _state(m2, t2))
    # a guarded dict loads into an unguarded trainer: the launches that were no step still count as such
    m3 = _model(dtype, frozen_cnn=True)
    m3.load_state_dict(msd)
    t3 = _trainer(m3)
    t3.load_state_dict(sd)
    assert t3.t == 2 and "nonfinite" not in t3.state_dict()["hip_trainer"]
    # ... and a dict from an unguarded trainer into a guarded one, with the new counters at zero
    t4 = _trainer(_model(dtype, frozen_cnn=True), nonfinite="skip")
    t4.load_state_dict(t3.state_dict())
    assert t4.t == 2 and t4.skipped_nonfinite() == (0, 0)
    t4.check()
    assert t4.state_dict()["hip_trainer"]["nonfinite"] == {"mode": "skip", "since": 0, "ever": 0, "unchecked": 0}


# ---------------------------------------------------------------------------------------------------- the forced one-rank reducer
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _reducer_worker(port, q):
    """A process of its own, so that no other test of this session sees a process group: one rank over gloo, as
    tests/test_gpu_stream_schedule.py makes it, and the poisoned-step test unchanged on HipTrainer(force_reducer=True)."""
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=0, world_size=1)
        torch.cuda.set_device(0)
        _poisoned_step("bf16", "raise", float("nan"), force_reducer=True)
        dist.destroy_process_group()
        q.put(("ok", ""))
    except BaseException as e:                                 # the parent reports it
        q.put(("failed", f"{type(e).__name__}: {e}"))
        raise


def test_a_poisoned_step_with_the_forced_one_rank_reducer():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_reducer_worker, args=(_free_port(), q))
    p.start()
    try:
        deadline = time.monotonic() + 240
        while q.empty() and p.is_alive() and time.monotonic() < deadline:      # (returns as soon as the child has answered or died)
            p.join(timeout=0.05)
        status, what = q.get(timeout=5) if (not q.empty() or not p.is_alive()) else ("failed", "no answer within 240 s")
    finally:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()
    assert status == "ok", what
    assert p.exitcode == 0
