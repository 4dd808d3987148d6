"""GPU: HipTrainer.state_dict / load_state_dict.  A run stopped after three steps, saved with torch.save, loaded with
torch.load(weights_only=True) into a NEW model and a NEW trainer and continued, against the run that never stopped: torch.equal for
the loss and the logits of steps 4 to 6 and for the parameters, both moments, the average, the BatchNorm buffers, Adam's step number
and the lags -- plain (fp32, bf16), with the weight average, with parameter groups whose live value changed, with a frozen part whose
lags cross the checkpoint and with a skipped step behind it.  The moments' transfer to and from
torch.optim.AdamW is exact, a transferred state continues like torch's, and every refusal leaves the trainer as it was.
Shapes of tests/test_gpu_grouped_train.py: O.full_config(), B = 4, 224 x 224, L = 20, dropout on unless stated."""
import io

import pytest
import torch
import torch.nn.functional as F

from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDX = [2, 0, 0, 2, 2, 0, 2]              # U = 3 images, N = 7 questions (tests/test_gpu_grouped_train.py)
_CACHE = {}


def _init_sd(cfg, seed):
    key = ("sd", tuple(sorted(cfg.items())), seed)
    if key not in _CACHE:                                              # computed once, never written (load_state_dict copies)
        _CACHE[key] = O.init_state_dict(cfg, seed, jitter=True)
    return _CACHE[key]


def _model(dtype, cfg, seed=11):
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(_init_sd(cfg, seed))
    return m.to(DEV).train()


def _fresh(dtype, cfg):
    """A model with weights of its own (not the run's initial ones): everything a resumed run computes comes from the checkpoint."""
    return pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype, seed=12345).to(DEV).train()


def _batch(k, B=4):
    key = ("batch", k, B)
    if key not in _CACHE:
        images, ids, mask, answers = O.synthetic_batch(B, seed=300 + k)
        mask[:, 0] = 1
        _CACHE[key] = tuple(t.to(DEV) for t in (images, ids, mask, answers))
    return _CACHE[key]


def _bn(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}


def _trainer(m, kw, groups):
    T = sub("trainer").HipTrainer
    if groups:
        kw = dict(kw, param_groups=sub("finetune").no_weight_decay_groups(m))
    return T(m, **kw)


# ---- the scenarios: constructor arguments, what happens before a step, what the resumed model is told, what is checked at the end
def _nothing(k, m, tr):
    pass


def _scale_before_step_2(k, m, tr):
    if k == 2:
        tr.param_groups[0]["lr_scale"] = 0.5


def _freeze_text_3_to_4(k, m, tr):
    if k == 3:
        m.text_encoder.requires_grad_(False)
    if k == 5:
        m.text_encoder.requires_grad_(True)


SCENARIOS = {
    "plain-fp32": dict(dtype="fp32"),
    "plain-bf16": dict(dtype="bf16"),
    "ema-warmup-bf16": dict(dtype="bf16", kw=dict(ema_decay=0.99, ema_warmup=True)),
    "groups-live-lr-scale": dict(dtype="bf16", groups=True, before=_scale_before_step_2),
    "frozen-history": dict(dtype="bf16", before=_freeze_text_3_to_4, at_resume=lambda m: m.text_encoder.requires_grad_(False)),
    "skipped-step": dict(dtype="bf16", bad_at=2),
}


def _steps(sc, m, tr, first, last, keep_flat_after=None):
    """Steps first .. last (1-based) on the shared batches; returns ([(loss, logits) of steps >= 4], flat after step keep_flat_after)."""
    rec, flat = [], None
    for k in range(first, last + 1):
        sc.get("before", _nothing)(k, m, tr)
        images, ids, mask, t = _batch(k)
        if sc.get("bad_at") == k:                                      # a handled input: the kernels skip the update
            t = t.clone()
            t[2] = m.num_answers
        loss, logits = tr.step(images, ids, mask, t)
        if k >= 4:
            rec.append((loss.clone(), logits.clone()))
        if k == keep_flat_after:
            flat = m._flat.detach().clone()
    torch.cuda.synchronize()
    return rec, flat


def _final(m, tr):
    out = {"flat": m._flat.detach().clone(), "m": tr.m.clone(), "v": tr.v.clone(), "lag": tr._lag.clone(), "bad": tr._bad.clone(),
           "t": torch.tensor(tr.t), "calls": torch.tensor(tr.calls)}
    if tr.ema is not None:
        out["ema"] = tr.ema.clone()
    out.update({"bn:" + k: v for k, v in _bn(m).items()})
    return out


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_resume_is_bit_exact(name):
    sc = SCENARIOS[name]
    cfg = O.full_config()                                              # dropout on (0.1 / 0.3)
    kw = dict(sc.get("kw", {}), lr=1e-3)
    control = name == "plain-fp32"
    # A: six steps without a stop
    ma = _model(sc["dtype"], cfg)
    ta = _trainer(ma, kw, sc.get("groups"))
    rec_a, flat4 = _steps(sc, ma, ta, 1, 6, keep_flat_after=4 if control else None)
    fin_a = _final(ma, ta)
    # B: three steps, the checkpoint through torch.save / torch.load(weights_only=True)
    mb = _model(sc["dtype"], cfg)
    tb = _trainer(mb, kw, sc.get("groups"))
    _steps(sc, mb, tb, 1, 3)
    buf = io.BytesIO()
    torch.save({"model_state_dict": mb.state_dict(), "optimizer_state_dict": tb.state_dict()}, buf)
    del mb, tb
    buf.seek(0)
    ck = torch.load(buf, weights_only=True)
    # a new model and a new trainer with the same constructor arguments, both loaded, steps 4 to 6
    mc = _fresh(sc["dtype"], cfg)
    mc.load_state_dict(ck["model_state_dict"])
    sc.get("at_resume", lambda m: None)(mc)
    tc = _trainer(mc, kw, sc.get("groups"))
    tc.load_state_dict(ck["optimizer_state_dict"])
    rec_c, _ = _steps(sc, mc, tc, 4, 6)
    fin_c = _final(mc, tc)
    assert len(rec_a) == len(rec_c) == 3
    for k, ((la, ga), (lc, gc)) in enumerate(zip(rec_a, rec_c), start=4):
        assert torch.equal(la, lc) and torch.equal(ga, gc), f"step {k}"
    assert fin_a.keys() == fin_c.keys()
    for key in fin_a:
        assert torch.equal(fin_a[key], fin_c[key]), key
    assert int(fin_a["calls"]) == 6
    if name == "frozen-history":                                       # the lags crossed the checkpoint: two frozen steps, one before it
        assert int(fin_a["lag"].max()) == 2 and int(fin_a["lag"].min()) == 0 and ck["optimizer_state_dict"]["hip_trainer"]["ever_frozen"]
        assert max(ck["optimizer_state_dict"]["hip_trainer"]["lag"]) == 1
    if name == "groups-live-lr-scale":
        assert tc.param_groups[0]["lr_scale"] == 0.5 and ck["optimizer_state_dict"]["param_groups"][0]["lr"] == 1e-3 * 0.5
    if name == "skipped-step":                                         # skipped_ever crossed the checkpoint; check() reads the same counters
        assert int(fin_a["t"]) == 5 and ck["optimizer_state_dict"]["hip_trainer"]["skipped_ever"] == 1
        texts = []
        for tr in (ta, tc):
            with pytest.raises(IndexError) as err:
                tr.check()
            texts.append(str(err.value))
        assert texts[0] == texts[1] and texts[0].startswith("1 target(s) out of range")
    if control:
        # so that the equalities cannot be vacuous: the same resume with the model loaded and the trainer left fresh differs at step 4
        md = _fresh(sc["dtype"], cfg)
        md.load_state_dict(ck["model_state_dict"])
        td = _trainer(md, kw, sc.get("groups"))
        _steps(sc, md, td, 4, 4)
        assert not torch.equal(md._flat, flat4)
        assert torch.equal(rec_c[0][1], rec_a[0][1])


# ---------------------------------------------------------------------------------------------------- to and from torch.optim.AdamW
def _deep_equal(a, b, path=""):
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a.keys()) == list(b.keys()), path
        for k in a:
            _deep_equal(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _deep_equal(x, y, f"{path}/{i}")
    else:
        assert a == b and type(a) is type(b), path


def test_transfer_to_and_from_torch_is_exact():
    LY = sub("layout")
    cfg = O.full_config()
    m = _model("bf16", cfg)
    tr = _trainer(m, dict(ema_decay=0.999), False)
    for k in (1, 2):
        tr.step(*_batch(k))
    sd = tr.state_dict()
    P = dict(m.named_parameters())
    order = [n for n, _ in m.named_parameters()]
    assert sd["hip_trainer"]["names"] == order and len(sd["param_groups"]) == 1
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
    opt.load_state_dict(sd)
    assert tr.t == 2
    for e in m._param_entries:
        st = opt.state[P[e.name]]
        assert torch.equal(st["exp_avg"], LY.view_of(tr.m, e)) and torch.equal(st["exp_avg_sq"], LY.view_of(tr.v, e)), e.name
        assert float(st["step"]) == tr.t and bool(st["exp_avg"].any())
    # the converse: torch's own dict into a trainer that has never stepped
    t2 = _trainer(m, {}, False)
    t2.load_state_dict(opt.state_dict())
    for e in m._param_entries:
        st = opt.state[P[e.name]]
        assert torch.equal(LY.view_of(t2.m, e), st["exp_avg"]) and torch.equal(LY.view_of(t2.v, e), st["exp_avg_sq"]), e.name
    assert torch.equal(t2.m, tr.m) and torch.equal(t2.v, tr.v)         # the padding between the slots included (zero on both sides)
    assert t2.t == tr.t == 2 and t2.calls == 2 and not t2._ever_frozen and not bool(t2._lag.any())
    # a trainer's own dict loaded into itself changes nothing
    tr.load_state_dict(sd)
    _deep_equal(tr.state_dict(), sd)


def _diff_figures(flat, ref):
    d = (flat.detach() - ref.detach()).abs()
    return d.max().item(), (d > 1e-6).float().mean().item()


def test_a_transferred_state_continues_like_torch():
    """fp32, dropout 0, lr 1e-4, three steps of the torch loop of test_trainer_step_with_an_image_index (cross-entropy,
    clip_grad_norm_(1.0), torch.optim.AdamW through forward_grouped) as the reference T, against M1 (two torch steps, the optimizer's
    dict into a HipTrainer, one fused step), M2 (two fused steps, the trainer's dict into torch.optim.AdamW, one torch step) and the
    control C (three fused steps, no transfer: no new code).  That test's bars, max |p - T| <= 2.5e-4 and a share of elements above
    1e-6 below 1e-3, were set for ONE step: where C itself is outside them at step 3, M1 and M2 get twice C's two figures (sign
    flips at the fp32 noise floor are discrete and batch-dependent).  A wrong step number after a transfer moves every element by
    a multiple of lr = 1e-4, far outside either.
    Measured on an MI355X (profiles/checkpoint_bench.json, "transfer_control"): C is inside the one-step bars at step 3, max 4.08e-5 and
    a share of 3.46e-4, so the bars stand as they are; M1 1.2e-7 and 0 (torch made both moments, one fused update on top), M2 4.08e-5
    and 3.46e-4 (C's own distance: the two fused steps made it, the transfer and the torch step added nothing)."""
    HipTrainer = sub("trainer").HipTrainer
    cfg0 = O.full_config(dropout=0.0, answer_dropout=0.0)
    idx = torch.tensor(IDX)
    batches = []
    for k in range(3):
        images, _, _, _ = O.synthetic_batch(3, seed=71 + 10 * k)
        _, ids, mask, answers = O.synthetic_batch(len(IDX), seed=72 + 10 * k)
        mask[:, 0] = 1
        batches.append(tuple(t.to(DEV) for t in (images, ids, mask, answers)))

    def torch_step(m, opt, b):
        x, ids, mask, t = b
        opt.zero_grad()
        logits, _ = m.forward_grouped(x, ids, mask, image_index=idx)
        F.cross_entropy(logits.float(), t).backward()
        torch.nn.utils.clip_grad_norm_(list(m.parameters()), 1.0)
        opt.step()

    def fused_step(tr, b):
        x, ids, mask, t = b
        tr.step(x, ids, mask, t, image_index=idx)

    def adamw(m):
        return torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.01)

    mt = _model("fp32", cfg0, seed=17)
    ot = adamw(mt)
    for b in batches:
        torch_step(mt, ot, b)
    mc = _model("fp32", cfg0, seed=17)
    tc = HipTrainer(mc)
    for b in batches:
        fused_step(tc, b)
    m1 = _model("fp32", cfg0, seed=17)
    o1 = adamw(m1)
    for b in batches[:2]:
        torch_step(m1, o1, b)
    t1 = HipTrainer(m1)
    t1.load_state_dict(o1.state_dict())
    fused_step(t1, batches[2])
    m2 = _model("fp32", cfg0, seed=17)
    t2 = HipTrainer(m2)
    for b in batches[:2]:
        fused_step(t2, b)
    o2 = adamw(m2)
    o2.load_state_dict(t2.state_dict())
    torch_step(m2, o2, batches[2])
    torch.cuda.synchronize()
    assert t1.t == 3 and t1.calls == 3 and float(o2.state[next(iter(m2.parameters()))]["step"]) == 3.0
    c_max, c_share = _diff_figures(mc._flat, mt._flat)
    figures = {"C": (c_max, c_share), "M1": _diff_figures(m1._flat, mt._flat), "M2": _diff_figures(m2._flat, mt._flat)}
    print("transferred-state figures (max |p - T|, share above 1e-6):", figures)
    inside = c_max <= 2.5e-4 and c_share < 1e-3
    bar_max, bar_share = (2.5e-4, 1e-3) if inside else (2 * c_max, 2 * c_share)
    for who in ("M1", "M2"):
        assert figures[who][0] <= bar_max and figures[who][1] < bar_share, (who, figures, inside)


# --------------------------------------------------------------------------------------------------------- errors on the real trainer
def test_refusals_leave_the_trainer_as_it_was():
    cfg = O.full_config()
    m = _model("bf16", cfg)
    tr = _trainer(m, {}, False)
    tr.step(*_batch(1))
    me = _model("bf16", cfg)
    te = _trainer(me, dict(ema_decay=0.99), False)
    te.step(*_batch(1))
    other = pkg().load_dropin().VQAModel(**dict(cfg, num_answers=cfg["num_answers"] - 1), compute_dtype="bf16", seed=3).to(DEV).train()
    sd_ema, sd_other, sd_own = te.state_dict(), sub("trainer").HipTrainer(other).state_dict(), tr.state_dict()
    assert sd_ema["hip_trainer"]["ema"] is not None

    def unchanged(t, before):
        torch.cuda.synchronize()
        return torch.equal(t.m, before[0]) and torch.equal(t.v, before[1]) and t.t == before[2] and t.calls == before[3]

    before = (tr.m.clone(), tr.v.clone(), tr.t, tr.calls)
    assert bool(before[0].any()) and before[2] == 1
    with pytest.raises(ValueError, match="average"):
        tr.load_state_dict(sd_ema)                                     # an average this trainer could not keep
    assert unchanged(tr, before)
    with pytest.raises(ValueError, match="shape"):
        tr.load_state_dict(sd_other)                                   # a model with another num_answers
    assert unchanged(tr, before)
    before_e = (te.m.clone(), te.v.clone(), te.t, te.calls)
    with te.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            te.state_dict()
        with pytest.raises(RuntimeError, match="ema_weights"):
            te.load_state_dict(sd_ema)
    assert unchanged(te, before_e)
    # a trainer that keeps an average, given a dict without one, restarts it from the weights (the constructor's rule)
    te.load_state_dict(sd_own)
    assert torch.equal(te.ema, me._flat) and torch.equal(te.m, tr.m) and te.ema_decay == 0.99
