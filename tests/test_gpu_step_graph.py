"""HipTrainer.step_graphed: the train step replayed from a captured HIP graph.  The yardstick everywhere is step() on a second model
built from the same state dict: the graph holds step()'s launches (dropout seeds read through the device step-state block, AdamW in
its _dev form), so every comparison is torch.equal, after every step.  Small model of tests/test_gpu_cached_features.py (embed_dim
32, 10 answers, 64-px images, B = 4, L = 10, U = 3 / N = 7 grouped), dropout 0.1 so that the seeds matter, fp32 and bf16."""
import pytest
import torch

from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(vocab_size=100, num_answers=10, embed_dim=32)
CFG = O.full_config(dropout=0.1, answer_dropout=0.1, **SMALL)
DTYPES = ["fp32", "bf16"]
GROUP_INDEX = [0, 1, 1, 0, 1, 0, 0]          # U = 3 images, N = 7 questions
_CACHE = {}


def _sd():
    if "sd" not in _CACHE:
        _CACHE["sd"] = O.init_state_dict(CFG, 41, jitter=True)
    return _CACHE["sd"]


def _batch(seed, B=4):
    key = ("batch", seed, B)
    if key not in _CACHE:
        _CACHE[key] = [t.to(DEV) for t in O.synthetic_batch(B, seed=seed, image_size=64, seq_len=10, vocab=100, num_answers=10)]
    return _CACHE[key]


def _grouped(seed):
    images, ids, mask, answers = _batch(seed, B=7)
    return images[:3].contiguous(), ids, mask, answers, torch.tensor(GROUP_INDEX)


def _model(dtype, frozen_cnn):
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype=dtype)
    m.load_state_dict(_sd())
    m = m.to(DEV).train()
    if frozen_cnn:
        m.image_encoder.requires_grad_(False)
        m.image_encoder.eval()
    return m


def _encode(m, images):
    m.eval()
    with torch.no_grad():
        f = m.encode_features(images)
    m.train()
    m.image_encoder.eval()
    return f


def _soft(answers):
    ST = pkg().load_dropin_soft_targets()
    ids = torch.stack([answers, (answers + 1) % 10], dim=1).int().contiguous()
    w = torch.tensor([0.7, 0.3], device=DEV).repeat(answers.shape[0], 1).contiguous()
    cnt = torch.tensor([7, 3], device=DEV, dtype=torch.int32).repeat(answers.shape[0], 1).contiguous()
    return ST.SoftTargets(ids, w, cnt)


class _Calls:
    """Names of the launches that go through _lib.call, in order."""

    def __enter__(self):
        L = sub("_lib")
        self.names, self._old = [], L._HOOK[0]
        L._HOOK[0] = lambda name, args: self.names.append(name)
        return self

    def __exit__(self, *a):
        sub("_lib")._HOOK[0] = self._old


class _Pair:
    """Two models from one state dict with one trainer each: `a` is stepped eagerly, `b` through step_graphed."""

    def __init__(self, dtype, route="features", **kw):
        self.route = route
        frozen = route != "images"
        self.a, self.b = _model(dtype, frozen), _model(dtype, frozen)
        kw = dict(dict(lr=1e-3, ema_decay=0.99), **kw)
        T = pkg().trainer.HipTrainer
        self.ta, self.tb = T(self.a, **kw), T(self.b, **kw)
        self.steps = 0

    def inputs(self, m, images):
        return _encode(m, images) if self.route == "features" else images

    def state(self, m, tr, loss, logits):
        out = [loss.clone(), logits.clone(), m._flat.detach().clone(), tr.m.clone(), tr.v.clone(), tr._bad.clone(), tr._lag.clone()]
        if tr.ema is not None:
            out.append(tr.ema.clone())
        if self.route == "images":                             # BatchNorm running statistics and counters
            out += [b.detach().clone() for _, b in sorted(m.named_buffers())]
        return out

    def step(self, images, ids, mask, tgt, idx=None, metrics=(None, None), eager_b=False, nan_loss=False):
        """One step on both sides and the comparison; returns b's launch names."""
        fa, fb = self.inputs(self.a, images), self.inputs(self.b, images)
        la, lga = self.ta.step(fa, ids, mask, tgt, metrics=metrics[0], image_index=idx)
        with _Calls() as c:
            lb, lgb = (self.tb.step if eager_b else self.tb.step_graphed)(fb, ids, mask, tgt, metrics=metrics[1], image_index=idx)
        torch.cuda.synchronize()
        sa, sb = self.state(self.a, self.ta, la, lga), self.state(self.b, self.tb, lb, lgb)
        assert len(sa) == len(sb)
        if nan_loss:
            assert bool(torch.isnan(sa[0]).all()) and bool(torch.isnan(sb[0]).all())
            sa, sb = sa[1:], sb[1:]
        else:
            assert bool(torch.isfinite(la).all())
        for i, (x, y) in enumerate(zip(sa, sb)):
            assert torch.equal(x, y), (self.steps, i)
        self.steps += 1
        return c.names

    def run(self, n=6, seed=200, grouped=False, target=lambda s, answers: answers, metrics=(None, None)):
        for s in range(n):
            if grouped:
                images, ids, mask, answers, idx = _grouped(seed + 100 + s % 6)
            else:
                (images, ids, mask, answers), idx = _batch(seed + s % 6), None
            self.step(images, ids, mask, target(s, answers), idx, metrics)


# ------------------------------------------------------------------------------------------- two eager calls, the capture, replays
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["plain", "grouped", "soft_bce", "loss_opts", "ema_warmup", "images"])
def test_graphed_steps_are_bit_equal_to_eager_steps(dtype, case):
    MET = pkg().load_dropin_metrics()
    if case == "plain":
        p = _Pair(dtype)
        p.run()
    elif case == "grouped":
        p = _Pair(dtype)
        p.run(grouped=True)
    elif case == "soft_bce":
        p = _Pair(dtype, loss="bce")
        mets = (MET.VQAChallengeAccuracy(), MET.VQAChallengeAccuracy())
        p.run(target=lambda s, a: _soft(a), metrics=mets)
        assert mets[0]._read() == mets[1]._read() and mets[0].count == 24
    elif case == "loss_opts":
        p = _Pair(dtype, label_smoothing=0.1, ignore_index=-100)
        mets = (MET.VQAAccuracy(), MET.VQAAccuracy())

        def tgt(s, a):
            a = a.clone()
            a[1] = -100                                        # an ignored row
            return a
        p.run(target=tgt, metrics=mets)
        assert mets[0]._read() == mets[1]._read() and mets[0].total == 18
    elif case == "ema_warmup":
        p = _Pair(dtype, ema_decay=0.999, ema_warmup=True)
        p.run()
    else:                                                      # (+ VQAAccuracy on the plain loss: its own launch, inside the graph)
        p = _Pair(dtype, route="images")
        mets = (MET.VQAAccuracy(), MET.VQAAccuracy())
        p.run(metrics=mets)
        assert mets[0]._read() == mets[1]._read() and mets[0].total == 24
    assert p.tb.graph_captures == 1 and len(p.tb._graphs) == 1
    p.ta.check(); p.tb.check()
    assert p.ta.t == p.tb.t == 6


# ------------------------------------------------------------------------------------------------ 1: hyper-parameters stay live
@pytest.mark.parametrize("dtype", DTYPES)
def test_lr_and_ema_decay_change_between_replays_without_a_new_graph(dtype):
    p = _Pair(dtype)
    p.run(4)
    for tr in (p.ta, p.tb):
        tr.lr, tr.ema_decay = 3e-4, 0.9
    p.run(2, seed=204)
    for tr in (p.ta, p.tb):
        tr.lr, tr.betas, tr.eps, tr.wd, tr.max_norm, tr.ema_warmup = 2e-3, (0.8, 0.99), 1e-6, 0.05, 0.05, True
    p.run(2, seed=200)
    assert p.tb.graph_captures == 1


# ------------------------------------------------------------------------------------------------------------- 2: a skipped step
@pytest.mark.parametrize("dtype", DTYPES)
def test_out_of_range_target_at_a_replayed_step_skips_the_update(dtype):
    p = _Pair(dtype)
    p.run(4)
    images, ids, mask, answers = _batch(204)
    bad = answers.clone()
    bad[2] = 10                                                # outside [0, 10)
    before = p.b._flat.detach().clone()
    p.step(images, ids, mask, bad, nan_loss=True)
    assert torch.equal(p.b._flat.detach(), before)
    for tr in (p.ta, p.tb):
        with pytest.raises(IndexError):
            tr.check()
    p.run(2, seed=202)
    assert p.tb.graph_captures == 1 and p.ta.t == p.tb.t == 6
    p.ta.check(); p.tb.check()


# ------------------------------------------------------------------------------------- 3: things that happen between two replays
@pytest.mark.parametrize("dtype", DTYPES)
def test_eager_step_load_state_dict_and_ema_evaluation_between_replays(dtype):
    p = _Pair(dtype)
    p.run(4)
    images, ids, mask, answers = _batch(204)
    p.step(images, ids, mask, answers, eager_b=True)           # an eager step() on the graphed side
    p.run(1, seed=205)
    sd = {k: v.clone() for k, v in p.a.state_dict().items()}
    for k in sd:
        if k.startswith("answer_head.") and sd[k].is_floating_point():
            sd[k] = sd[k] * 0.5
    p.a.load_state_dict(sd); p.b.load_state_dict(sd)
    p.run(1, seed=200)
    outs = []
    for m, tr in ((p.a, p.ta), (p.b, p.tb)):                   # validation on the averaged weights
        with tr.ema_weights():
            m.eval()
            with torch.no_grad():
                outs.append(m(images, ids, mask)[0].clone())
            m.train(); m.image_encoder.eval()
    assert torch.equal(outs[0], outs[1])
    p.run(2, seed=201)
    assert p.tb.graph_captures == 1


# ----------------------------------------------------------------------------------------------------- 4: new keys, the LRU cap
@pytest.mark.parametrize("dtype", DTYPES)
def test_new_batch_size_or_trainable_set_gives_a_new_graph_and_the_cap_holds(dtype):
    p = _Pair(dtype)
    p.b.graph_max_shapes = 2
    p.run(4)
    assert p.tb.graph_captures == 1
    images, ids, mask, answers = _batch(210, B=3)              # another batch size
    for _ in range(4):
        p.step(images, ids, mask, answers)
    assert p.tb.graph_captures == 2 and len(p.tb._graphs) == 2
    for m in (p.a, p.b):                                       # another trainable set: the text encoder is frozen too
        m.text_encoder.requires_grad_(False)
    p.run(4, seed=202)
    assert p.tb.graph_captures == 3 and len(p.tb._graphs) == 2
    for _ in range(2):                                         # B = 3 under the new range table: a new key, two eager calls
        p.step(images, ids, mask, answers)
    for m in (p.a, p.b):
        m.text_encoder.requires_grad_(True)
    p.run(4, seed=200)
    assert len(p.tb._graphs) <= 2
    p.ta.check(); p.tb.check()


# ------------------------------------------------------------------------------------------------------------------ 5: refusals
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_raise_before_any_launch(dtype, monkeypatch):
    p = _Pair(dtype)
    images, ids, mask, answers = _batch(200)
    feats = p.inputs(p.b, images)
    calls0, step0 = p.tb.calls, p.tb.engine.step_id
    with _Calls() as c:
        monkeypatch.setattr(p.tb.reducer, "active", True)      # what a world of several ranks or force_reducer=True sets
        with pytest.raises(RuntimeError, match="collectives"):
            p.tb.step_graphed(feats, ids, mask, answers)
        monkeypatch.setattr(p.tb.reducer, "active", False)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="capturing"):
            p.tb.step_graphed(feats, ids, mask, answers)
        monkeypatch.undo()
        with p.tb.ema_weights():
            with pytest.raises(RuntimeError, match="ema_weights"):
                p.tb.step_graphed(feats, ids, mask, answers)
        with pytest.raises(RuntimeError):
            p.tb.step_graphed(feats, ids.new_zeros((4, 4096)), None, answers)        # a question that is too long
    assert c.names == [] and (p.tb.calls, p.tb.engine.step_id) == (calls0, step0)
    p.run(3)                                                   # and the trainer is as usable as before


# ------------------------------------------------------------------------------------------- 6, 7: what the host issues per call
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["features", "images"])
def test_launches_of_the_capture_and_of_a_replay(dtype, route):
    p = _Pair(dtype, route=route)
    data = [_batch(200 + s) for s in range(5)]
    for s in range(2):
        p.step(*data[s])
    images, ids, mask, answers = data[2]
    fa, fb = p.inputs(p.a, images), p.inputs(p.b, images)
    with _Calls() as eager:                                    # the third eager step on the eager side
        p.ta.step(fa, ids, mask, answers)
    with _Calls() as cap:
        p.tb.step_graphed(fb, ids, mask, answers)
    torch.cuda.synchronize()
    assert torch.equal(p.a._flat.detach(), p.b._flat.detach())
    adam = [n for n in eager.names if n.startswith("vqa_adamw")]
    assert adam == ["vqa_adamw_ranges_ema" if route == "features" else "vqa_adamw_ema"]
    assert cap.names == ["vqa_step_state_set"] + [n + "_dev" if n.startswith("vqa_adamw") else n for n in eager.names]
    assert p.step(*data[3]) == ["vqa_step_state_set"]
    # a torch-side write to the parameters: the operand copy is re-cast eagerly ahead of the replay (bf16; fp32 has no copy)
    with torch.no_grad():
        for m in (p.a, p.b):
            dict(m.named_parameters())["answer_head.classifier.0.weight"].mul_(0.5)
    assert p.step(*data[4]) == (["vqa_convert"] if dtype == "bf16" else []) + ["vqa_step_state_set"]


# ----------------------------------------------------------------------------------------------------------- 8: forty in a row
@pytest.mark.parametrize("dtype", DTYPES)
def test_forty_graphed_steps_back_to_back_equal_forty_eager_ones(dtype):
    p = _Pair(dtype)
    data = [_batch(200 + s) for s in range(6)]
    fa = [p.inputs(p.a, d[0]) for d in data]
    fb = [p.inputs(p.b, d[0]) for d in data]
    torch.cuda.synchronize()
    for s in range(40):
        _, ids, mask, answers = data[s % 6]
        la, lga = p.ta.step(fa[s % 6], ids, mask, answers)
    for s in range(40):                                        # no host synchronisation inside the loop
        _, ids, mask, answers = data[s % 6]
        lb, lgb = p.tb.step_graphed(fb[s % 6], ids, mask, answers)
    torch.cuda.synchronize()
    for x, y in zip(p.state(p.a, p.ta, la, lga), p.state(p.b, p.tb, lb, lgb)):
        assert torch.equal(x, y)
    assert p.tb.graph_captures == 1 and p.ta.t == p.tb.t == 40
