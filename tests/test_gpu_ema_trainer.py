"""GPU: the weight average of HipTrainer (ema_decay=, kept by the fused AdamW launch) and of utils.ema.ParameterEMA (torch.optim
loops): the training run itself is bit-identical with and without the average; the average follows the float64 replay of the
per-step parameter snapshots (tests/_emaref.py, bound 2^-22 * max(|ema|, |p|) per update); a rejected step and frozen parameters leave it
alone; ema_weights() puts the averaged weights under every eval route -- graphs captured earlier included -- and restores every bit."""
import pytest
import torch
import torch.nn.functional as F

import _emaref as R
from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = O.full_config(dropout=0.0, answer_dropout=0.0, vocab_size=100, num_answers=10, embed_dim=32)


def _model(seed, dtype="bf16"):
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype=dtype)
    m.load_state_dict(O.init_state_dict(CFG, seed, jitter=True))
    return m.to(DEV).train()


def _batch(seed, B=4):
    return [t.to(DEV) for t in O.synthetic_batch(B, seed=seed, image_size=64, seq_len=10, vocab=100, num_answers=10)]


def _trainer(m, **kw):
    return pkg().trainer.HipTrainer(m, lr=1e-3, **kw)


def _bits(t):
    return t.detach().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _param_mask(m, pred):
    """bool mask over the flat buffer: elements of the parameters whose name satisfies pred."""
    mask = torch.zeros(m._flat.numel(), dtype=torch.bool)
    for e in m._param_entries:
        if pred(e.name):
            mask[e.offset: e.offset + e.numel] = True
    return mask


@pytest.mark.parametrize("dtype,warmup", [("fp32", False), ("bf16", False), ("bf16", True)])
def test_twin_trainers_train_bit_identically_and_the_average_follows_the_replay(dtype, warmup):
    ma, mb = _model(41, dtype), _model(41, dtype)
    ta, tb = _trainer(ma, ema_decay=None), _trainer(mb, ema_decay=0.9, ema_warmup=warmup)
    assert getattr(ta, "ema", None) is None and tb.ema is not None
    assert _same(tb.ema, mb._flat) and tb.ema.data_ptr() != mb._flat.data_ptr()      # starts at the initial weights, its own buffer
    ema0, ref = tb.ema.cpu().clone(), R.Tracker(tb.ema.cpu())
    for step in range(4):
        batch = _batch(800 + step)
        la, ga = ta.step(*batch)
        lb, gb = tb.step(*batch)
        torch.cuda.synchronize()
        assert _same(la, lb) and _same(ga, gb), step
        assert _same(ma._flat, mb._flat) and _same(ta.m, tb.m) and _same(ta.v, tb.v), step
        ref.step(mb._flat.detach().cpu(), 0.9, warmup, step + 1).check(tb.ema.cpu(), f"{dtype} step {step + 1}")
    ta.check(); tb.check()
    assert not _same(tb.ema, mb._flat) and not torch.equal(tb.ema.cpu(), ema0)
    if dtype == "bf16":                                             # the variant wrote the bf16 operand copy too
        assert torch.equal(tb.engine.wsrc, mb._flat.to(torch.bfloat16))
    # the decay is a plain attribute: changed between steps, validated on the host before anything is launched
    tb.ema_decay = 0.5
    tb.step(*_batch(899)); ta.step(*_batch(899))
    torch.cuda.synchronize()
    ref.step(mb._flat.detach().cpu(), 0.5, warmup, 5).check(tb.ema.cpu(), "decay changed")
    assert _same(ma._flat, mb._flat)
    before, calls = tb.ema.clone(), tb.calls
    tb.ema_decay = 1.5
    with pytest.raises(ValueError):
        tb.step(*_batch(899))
    torch.cuda.synchronize()
    assert tb.calls == calls and _same(tb.ema, before) and _same(ma._flat, mb._flat)


def test_a_rejected_step_leaves_the_average_alone():
    m = _model(42, "fp32")
    tr = _trainer(m, ema_decay=0.9, ema_warmup=True)
    images, ids, mask, answers = _batch(810)
    tr.step(images, ids, mask, answers)
    torch.cuda.synchronize()
    e0, p0, t0 = tr.ema.clone(), m._flat.detach().clone(), tr.t
    bad = answers.clone()
    bad[1] = 10                                                     # outside [0, num_answers)
    tr.step(images, ids, mask, bad)
    torch.cuda.synchronize()
    assert _same(tr.ema, e0) and _same(m._flat, p0) and tr.t == t0
    with pytest.raises(IndexError):
        tr.check()
    tr.step(images, ids, mask, answers)                             # the next applied step is update 2 of the warm-up, not 3
    torch.cuda.synchronize()
    R.Tracker(e0.cpu()).step(m._flat.detach().cpu(), 0.9, True, 2).check(tr.ema.cpu(), "after the skipped step")


def test_frozen_part_keeps_its_average_at_the_initial_weights():
    m = _model(43)
    m.image_encoder.requires_grad_(False)
    tr = _trainer(m, ema_decay=0.9, ema_warmup=True)
    ema0, ref = tr.ema.cpu().clone(), R.Tracker(tr.ema.cpu())
    frozen = _param_mask(m, lambda n: n.startswith("image_encoder."))
    train = _param_mask(m, lambda n: not n.startswith("image_encoder."))
    assert int(frozen.sum()) > 0 and int(train.sum()) > 0
    for step in range(3):
        tr.step(*_batch(820 + step))
        torch.cuda.synchronize()
        ref.step(m._flat.detach().cpu(), 0.9, True, step + 1)
    assert tr._ranges is not None                                   # the ranges variant ran
    ema = tr.ema.cpu()
    assert _same(ema[frozen], ema0[frozen]) and _same(m._flat.detach().cpu()[frozen], ema0[frozen])
    ref.check(ema, "trainable slices", sel=train)
    assert not torch.equal(ema[train], ema0[train])


def _eval_eager(m, images, ids, mask):
    with torch.no_grad():
        return m._forward_eager_eval(images.contiguous().float(), ids.contiguous().long(), mask.contiguous().float()).clone()


def test_ema_weights_puts_the_average_under_every_eval_route_and_restores_every_bit():
    m, mt = _model(44), _model(44)
    tr, twin = _trainer(m, ema_decay=0.9), _trainer(mt, ema_decay=0.9)         # the twin never enters the context
    for step in range(2):
        tr.step(*_batch(830 + step)); twin.step(*_batch(830 + step))
    torch.cuda.synchronize()
    images, ids, mask, _ = _batch(840, B=3)
    # the references: a second model that loaded the exported average, and the twin for the live weights
    m2 = pkg().load_dropin().VQAModel(**CFG, compute_dtype="bf16")
    sd = tr.ema_state_dict()
    assert list(sd.keys()) == list(m.state_dict().keys())
    m2.load_state_dict(sd, strict=True)
    m2 = m2.to(DEV).eval()
    m.eval(); mt.eval()
    ref_avg, ref_live = _eval_eager(m2, images, ids, mask), _eval_eager(mt, images, ids, mask)
    assert not torch.equal(ref_avg, ref_live)
    with torch.no_grad():
        top_avg, top_live = m2.predict_topk(images, ids, mask, top_k=3), mt.predict_topk(images, ids, mask, top_k=3)
        ans_avg = m2.answer(m2.encode_images(images), ids, mask)[0]
        # (ii) every graph is captured BEFORE entering
        assert torch.equal(m.forward_graphed(images, ids, mask), ref_live)
        assert torch.equal(m.predict_topk(images, ids, mask, top_k=3).probs, top_live.probs)
        outside = m.encode_images(images)
        ans_live = m.answer(outside, ids, mask)[0]
    pred_live = m.predict(images, ids, mask, top_k=3)
    kept = [t.detach().clone() for t in (m._flat, tr.ema, tr.m, tr.v)]
    graphs = len(m._graphs)

    with tr.ema_weights() as inner:
        assert inner is m
        assert _same(m._flat, kept[1]) and _same(tr.ema, kept[0])
        assert torch.equal(_eval_eager(m, images, ids, mask), ref_avg)                       # (i)
        with torch.no_grad():
            assert torch.equal(m.forward_graphed(images, ids, mask), ref_avg)                # (ii): the graph captured outside
            assert len(m._graphs) == graphs                                                  # ... replayed, not captured again
            assert torch.equal(m(images, ids, mask)[0], ref_avg)
            tk = m.predict_topk(images, ids, mask, top_k=3)
            assert torch.equal(tk.probs, top_avg.probs) and torch.equal(tk.indices, top_avg.indices)
            with pytest.raises(RuntimeError):
                m.answer(outside, ids, mask)                                                 # (v) a context from outside is refused
            inside = m.encode_images(images)
            assert torch.equal(m.answer(inside, ids, mask)[0], ans_avg)
        pi, pp = m.predict(images, ids, mask, top_k=3)
        assert torch.equal(pp, F.softmax(ref_avg, dim=-1).topk(3, dim=-1)[0])
        with pytest.raises(RuntimeError):
            tr.step(*_batch(850))                                                            # (iii)
    torch.cuda.synchronize()
    for a, b in zip(kept, (m._flat, tr.ema, tr.m, tr.v)):                                    # (iv)
        assert _same(a, b)
    with torch.no_grad():
        assert torch.equal(m.forward_graphed(images, ids, mask), ref_live)                   # (ii) live again
        with pytest.raises(RuntimeError):
            m.answer(inside, ids, mask)                                                      # ... and the inside context is stale
        assert torch.equal(m.answer(m.encode_images(images), ids, mask)[0], ans_live)
    assert torch.equal(m.predict(images, ids, mask, top_k=3)[1], pred_live[1])
    with pytest.raises(ZeroDivisionError):                                                   # the exchange is undone when the body raises
        with tr.ema_weights():
            assert torch.equal(_eval_eager(m, images, ids, mask), ref_avg)
            1 / 0
    for a, b in zip(kept, (m._flat, tr.ema, tr.m, tr.v)):
        assert _same(a, b)
    # the next step is the twin's, bit for bit (the bf16 operand copy was re-cast, not trusted)
    m.train(); mt.train()
    la, ga = tr.step(*_batch(860))
    lb, gb = twin.step(*_batch(860))
    torch.cuda.synchronize()
    assert _same(la, lb) and _same(ga, gb)
    assert _same(m._flat, mt._flat) and _same(tr.ema, twin.ema) and _same(tr.m, twin.m) and _same(tr.v, twin.v)


def test_parameter_ema_in_a_torch_optim_loop():
    P = pkg().load_dropin_ema().ParameterEMA
    m = _model(45, "fp32")
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    ema = P(m, 0.999, warmup=True)
    ref, snaps = R.Tracker(ema.ema.cpu()), []
    assert _same(ema.ema, m._flat)
    for step in range(3):
        images, ids, mask, answers = _batch(870 + step)
        opt.zero_grad()
        logits, _ = m(images, ids, mask)
        F.cross_entropy(logits, answers).backward()
        opt.step()
        ema.update()
        torch.cuda.synchronize()
        snaps.append(m._flat.detach().cpu().clone())
        ref.step(snaps[-1], 0.999, True, step + 1)                  # d = 2/11, 3/12, 4/13
    assert ema.num_updates == 3 and not torch.equal(snaps[0], snaps[2])
    ref.check(ema.ema.cpu(), "ParameterEMA")
    sd = ema.state_dict()
    m2 = pkg().load_dropin().VQAModel(**CFG, compute_dtype="fp32")
    m2.load_state_dict(sd, strict=True)
    m2 = m2.to(DEV).eval()
    assert _same(m2._flat, ema.ema)
    images, ids, mask, _ = _batch(880, B=2)
    m.eval()
    live = m._flat.detach().clone()
    with ema.average_weights():
        assert torch.equal(_eval_eager(m, images, ids, mask), _eval_eager(m2, images, ids, mask))
    assert _same(m._flat, live)
    ema2 = P(m, 0.999, warmup=True)
    ema2.load_state_dict(sd, num_updates=3)
    assert _same(ema2.ema, ema.ema) and ema2.num_updates == 3
