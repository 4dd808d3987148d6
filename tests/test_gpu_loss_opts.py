"""GPU: cross entropy with nn.CrossEntropyLoss's options (class weights, ignore_index, label smoothing) as one fused launch --
the kernel vqa_cross_entropy_opts against torch in fp64, its exact properties and edges, the drop-in criterion utils.losses
.CrossEntropyLoss under autograd and HipTrainer(label_smoothing=, class_weight=, ignore_index=) against the autograd route."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _ceref as R
from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
HALF_ULP_F32 = 6e-8
BS = (1, 3, 4, 5, 9)                 # partial and full four-row workgroups
NS = (5, 64, 65, 1000)               # below, at and past one wave's stride, and the model's width
SMALL = dict(dropout=0.0, answer_dropout=0.0, vocab_size=100, num_answers=10, embed_dim=32)
SMALL_BATCH = dict(image_size=64, seq_len=10, vocab=100, num_answers=10)


def _units(a, ref):
    """worst |a - ref| in units of (1 + |ref|)"""
    return float(((a.double() - ref).abs() / (1 + ref.abs())).max())


def _fp32_bound(cpu_fp32, ref):
    """test_gpu_layernorm_fp64.py's rule: 8 x the error of torch's own fp32 F.cross_entropy on the CPU against fp64 on the same inputs,
    the CPU figure floored at half an ulp of fp32 (6e-8 of 1 + |ref|)."""
    return 8 * max(_units(cpu_fp32, ref), HALF_ULP_F32)


def _run(x, t, w=None, ii=None, eps=0.0, ws=True, grad=True, f32=True, acc=None, gscale=1.0):
    """One launch on device copies; returns (loss, dlogits | None, logits_f32 | None, err, empty) on the CPU."""
    K = sub("kernels")
    xd = x.to(DEV).contiguous()
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    empty = torch.zeros(1, device=DEV, dtype=torch.int32)
    lf = torch.full(x.shape, 7.0, device=DEV, dtype=F32) if f32 else None
    loss, dl = K.cross_entropy_opts(xd, t.to(DEV), class_weight=None if w is None else w.float().to(DEV), ignore_index=ii, label_smoothing=eps,
                                    need_grad=grad, logits_f32=lf, gscale=gscale, err=err, fixed_order=ws, acc=acc, empty=empty)
    torch.cuda.synchronize()
    return loss.cpu(), None if dl is None else dl.cpu(), None if lf is None else lf.cpu(), int(err.item()), int(empty.item())


def _case(kind, B, N, dtype):
    """Seeded inputs of one case: (x in dtype, targets, weights fp32 | None, ignore_index | None, eps, rows that are ignored)."""
    g = torch.Generator().manual_seed(7919 * B + 13 * N + len(kind))
    x = (torch.randn(B, N, generator=g) * 3).to(dtype)
    t = torch.randint(0, N, (B,), generator=g)
    w = torch.rand(N, generator=g) + 0.1
    ii, eps, use_w = None, 0.0, False
    if kind in ("ignore_valid", ):
        ii = 2
        t[t == 2] = 3
    if kind in ("ignore_neg", "all", "offset"):
        ii = -100
    if ii is not None and B > 1:
        t[B // 2] = ii
    if kind in ("weights", "all", "offset"):
        use_w = True
        if B > 2:                                              # a class of weight 0 that is row B-1's target; row 0 keeps W > 0
            z = int(t[B - 1])
            w[z] = 0.0
            t[0] = (z + 1) % N
        else:
            w[(int(t[0]) + 1) % N] = 0.0
    if kind in ("eps", "all", "offset"):
        eps = 0.1
    if kind == "offset":                                       # rows at +300 / -300: the softmax must stay stable
        x = (x.float() + 300.0 * (1 - 2 * (torch.arange(B) % 2))[:, None]).to(dtype)
    ign = torch.zeros(B, dtype=torch.bool) if ii is None else t == ii
    return x, t, (w if use_w else None), ii, eps, ign


KINDS = ("eps", "weights", "ignore_neg", "ignore_valid", "all", "offset")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_kernel_matches_torch_fp64(dtype, kind):
    """Every B in {1, 3, 4, 5, 9} x N in {5, 64, 65, 1000} of one kind of options.  The reference is F.cross_entropy + autograd in fp64
    on the CPU, on the logits as the kernel reads them (bf16-rounded for bf16).  Bounds, per case and recomputed here: loss and
    dlogits within 8 x the error of torch's CPU fp32 F.cross_entropy on the same inputs (floored at 6e-8) in units of 1 + |ref|;
    bf16 dlogits get one bf16 ulp, 2^-8 |ref|, for the final rounding on top.  logits_f32 is exact.
    CPU fp32 errors measured with these inputs, over the six kinds and both dtypes: loss 6.0e-8 (floor; raw 6e-11) ... 2.0e-7,
    gradient 6.0e-8 (floor; raw 4e-9) ... 2.2e-7 -> the kernel is allowed 4.8e-7 ... 1.6e-6 on the loss and 4.8e-7 ... 1.8e-6 on the
    gradient; each case prints its own figures.  The rows at +-300 ("offset") carry weights and smoothing: with either the kernel
    evaluates the row as lp = (x - m) - log(s); without both it keeps vqa_cross_entropy's lse form for its bits."""
    gscale = 0.5 if kind == "all" else 1.0
    for B in BS:
        for N in NS:
            x, t, w, ii, eps, ign = _case(kind, B, N, dtype)
            ref_l, ref_g = R.torch_ce(x, t, w, ii, eps)
            ref_g = ref_g * gscale
            cpu_l, cpu_g = R.torch_ce(x, t, w, ii, eps, dtype=F32)
            b_l, b_g = _fp32_bound(cpu_l, ref_l), _fp32_bound(cpu_g * gscale, ref_g)
            loss, dl, lf, err, empty = _run(x, t, w, ii, eps, gscale=gscale)
            e_l = _units(loss, ref_l)
            e_g = float((((dl.double() - ref_g).abs() - (2.0 ** -8 * ref_g.abs() if dtype == BF16 else 0)) / (1 + ref_g.abs())).max())
            print(f"CE opts {kind} {B}x{N} {dtype}: loss err {e_l:.2e} bound {b_l:.2e} | grad err {e_g:.2e} bound {b_g:.2e}")
            assert err == 0 and empty == 0
            assert e_l <= b_l, (B, N)
            assert e_g <= b_g, (B, N)
            assert torch.equal(lf, x.float())
            if bool(ign.any()):
                assert torch.equal(dl[ign], torch.zeros_like(dl[ign]))         # ignored rows: an all-zero gradient row


def _plain(x, t, ws=True, grad=True, f32=True):
    """vqa_cross_entropy on the same inputs."""
    L = sub("_lib")
    xd, td = x.to(DEV).contiguous(), t.to(DEV)
    B, N = x.shape
    loss = torch.zeros((), device=DEV, dtype=F32)
    dl = torch.empty_like(xd) if grad else None
    lf = torch.full(x.shape, 7.0, device=DEV, dtype=F32) if f32 else None
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    wsb = torch.empty(B, device=DEV, dtype=F32) if ws else None
    L.call("vqa_cross_entropy", L.dt(xd), L.ptr(xd), L.ptr(td), L.ptr(loss), L.ptr(dl), L.ptr(lf), B, N, 1.0, L.ptr(err), L.ptr(wsb))
    torch.cuda.synchronize()
    return loss.cpu(), dl.cpu(), lf.cpu(), int(err.item())


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)) if a.dim() else a.view(torch.int32).item() == b.view(torch.int32).item()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_default_options_are_bit_equal_to_the_plain_kernel(dtype):
    for B, N in ((1, 5), (5, 65), (9, 1000), (4, 64)):
        g = torch.Generator().manual_seed(B * N)
        x = (torch.randn(B, N, generator=g) * 4).to(dtype)
        t = torch.randint(0, N, (B,), generator=g)
        pl, pd, pf, _ = _plain(x, t)
        for ii in (None, -100):                                # has_ignore without an ignored target changes nothing either
            loss, dl, lf, err, empty = _run(x, t, ii=ii)
            assert err == 0 and empty == 0
            assert _bits(loss, pl) and _bits(dl, pd) and _bits(lf, pf), (B, N, ii)


def test_workspace_runs_repeat_bit_for_bit_and_agree_with_atomics_and_loss_only():
    for kind, B, N in (("all", 9, 1000), ("offset", 5, 65), ("weights", 3, 5)):
        x, t, w, ii, eps, _ = _case(kind, B, N, F32)
        a = _run(x, t, w, ii, eps)
        b = _run(x, t, w, ii, eps)
        assert _bits(a[0], b[0]) and _bits(a[1], b[1])
        ref_l, _ = R.torch_ce(x, t, w, ii, eps)
        bound = _fp32_bound(R.torch_ce(x, t, w, ii, eps, dtype=F32)[0], ref_l)
        c = _run(x, t, w, ii, eps, ws=False)                   # float atomics on *loss: any order of the B terms
        assert _units(c[0], ref_l) <= bound and abs(float(c[0]) - float(a[0])) <= 2 * bound * (1 + abs(float(ref_l)))
        assert _bits(c[1], a[1])                               # the gradient does not depend on the loss reduction
        d = _run(x, t, w, ii, eps, grad=False, f32=False)      # dlogits NULL: the loss alone, unchanged bit for bit
        assert d[1] is None and _bits(d[0], a[0])


def test_zero_total_weight_gives_nan_loss_zero_gradient_and_counts_empty():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 65, generator=g)
    w = torch.rand(65, generator=g) + 0.1
    for dtype in (F32, BF16):
        # every row ignored, unweighted and weighted
        t = torch.full((5,), -100)
        for ww in (None, w):
            loss, dl, lf, err, empty = _run(x.to(dtype), t, ww, -100, 0.1)
            assert math.isnan(float(loss)) and torch.equal(dl, torch.zeros_like(dl)) and (err, empty) == (0, 1)
            assert torch.equal(lf, x.to(dtype).float())
        # every kept row has class weight 0 (torch: NaN gradient; this entry: zero, documented)
        t = torch.tensor([3, 3, -100, 9, 3])
        wz = w.clone()
        wz[3] = wz[9] = 0.0
        for eps in (0.0, 0.1):
            loss, dl, _, err, empty = _run(x.to(dtype), t, wz, -100, eps)
            assert math.isnan(float(loss)) and torch.equal(dl, torch.zeros_like(dl)) and (err, empty) == (0, 1)
    loss, dl, _, err, empty = _run(x, torch.full((5,), 2), None, 2, 0.0, ws=False)       # an ignore_index inside [0, N), atomics
    assert math.isnan(float(loss)) and torch.equal(dl, torch.zeros_like(dl)) and (err, empty) == (0, 1)


@pytest.mark.parametrize("weighted", [False, True])
def test_one_bad_target_among_ignored_rows(weighted):
    """Ignored rows are never counted in err, in the counters or in W; the bad row alone is NaN (it is never read out of bounds)."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(6, 65, generator=g)
    w = (torch.rand(65, generator=g) + 0.1) if weighted else None
    for badv in (65, -1, 2 ** 40):
        t = torch.tensor([-100, -100, badv, -100, -100, -100])
        acc = torch.zeros(3, device=DEV, dtype=torch.int64)
        loss, dl, lf, err, empty = _run(x, t, w, -100, 0.1, acc=acc)
        assert (err, empty) == (1, 0) and math.isnan(float(loss))
        assert bool(torch.isnan(dl[2]).all()) and torch.equal(dl[[0, 1, 3, 4, 5]], torch.zeros(5, 65))
        assert acc.tolist() == [0, 0, 1] and torch.equal(lf, x)
    # among KEPT rows: the other rows keep finite gradients (W counts the bad row with weight 1)
    t = torch.tensor([1, 2, 65, -100, 4, 5])
    loss, dl, _, err, empty = _run(x, t, w, -100, 0.0)
    assert (err, empty) == (1, 0) and math.isnan(float(loss)) and bool(torch.isnan(dl[2]).all())
    assert bool(torch.isfinite(dl[[0, 1, 4, 5]]).all()) and torch.equal(dl[3], torch.zeros(65))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_fused_counters_equal_the_reference(dtype):
    g = torch.Generator().manual_seed(5)
    B, N = 9, 65
    x = torch.randn(B, N, generator=g).to(dtype)
    t = torch.randint(0, N, (B,), generator=g)
    x[0, 7] = x[0, 3] = 9.0                                    # a tied maximum: index 3 wins
    t[0] = 7
    x[1, 64] = 9.0                                             # top-1 at the last column
    t[1] = 64
    x[2, :] = 1.0                                              # a whole row of ties: rank = the target's index
    t[2] = 4
    t[3] = 5
    x[3, :] = 1.0                                              # ... rank 5: not in the top five
    t[4] = -100                                                # an ignored row
    t[5] = 2                                                   # the ignored class id below
    ref = R.accuracy_counts(x.float(), t, ii=-100)
    acc = torch.full((3,), 10, device=DEV, dtype=torch.int64)  # counters are added to
    base = _run(x, t, None, -100, 0.1)
    out = _run(x, t, None, -100, 0.1, acc=acc)
    assert acc.tolist() == [10 + ref[0], 10 + ref[1], 10 + ref[2]] and ref[2] == 8
    assert _bits(out[0], base[0]) and _bits(out[1], base[1])   # counting changes no value
    acc.zero_()
    _run(x, t.clamp(min=0), None, 2, 0.0, acc=acc)             # a valid class id as ignore_index
    assert acc.tolist() == R.accuracy_counts(x.float(), t.clamp(min=0), ii=2)
    # the separate metric kernel on the kept rows gives the same counts
    M = pkg().load_dropin_metrics().VQAAccuracy()
    keep = t != -100
    M.update(x.float().to(DEV)[keep.to(DEV)], t[keep].to(DEV))
    assert [M.correct, M.correct_top5, M.total] == ref


def test_argument_errors_return_status_1000_without_a_launch():
    L = sub("_lib")
    x = torch.randn(4, 8, device=DEV)
    t = torch.zeros(4, device=DEV, dtype=torch.int64)
    loss = torch.zeros((), device=DEV)
    dl = torch.full_like(x, 5.0)

    def args(dtype=0, logits=x, targets=t, B=4, N=8, gscale=1.0, eps=0.0):
        return (dtype, L.ptr(logits), L.ptr(targets), L.ptr(loss), L.ptr(dl), None, B, N, gscale, None, None, None, -100, 0, eps, None, None)
    for kw in (dict(logits=None), dict(targets=None), dict(B=0), dict(N=0), dict(B=-1), dict(eps=-0.1), dict(eps=1.5), dict(eps=float("nan")),
               dict(eps=float("inf")), dict(dtype=2), dict(dtype=-1), dict(gscale=float("inf")), dict(gscale=float("nan"))):
        assert L.lib().vqa_cross_entropy_opts(*args(**kw), L.stream()) == 1000, kw
        with pytest.raises(RuntimeError, match="status 1000"):
            L.call("vqa_cross_entropy_opts", *args(**kw))
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and bool((dl == 5.0).all())      # nothing ran
    assert L.lib().vqa_cross_entropy_opts(*args(eps=1.0), L.stream()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- criterion
def test_criterion_matches_torch_through_backward():
    CE = pkg().load_dropin_losses().CrossEntropyLoss
    x, t, w, ii, eps, ign = _case("all", 9, 1000, F32)
    crit = CE(weight=w, ignore_index=ii, label_smoothing=eps)
    xd = x.to(DEV).requires_grad_(True)
    loss = crit(xd, t.to(DEV))
    assert loss.dim() == 0 and loss.requires_grad
    (loss * 3.0).backward()                                    # an incoming gradient other than 1
    ref_l, ref_g = R.torch_ce(x, t, w, ii, eps)
    cpu_l, cpu_g = R.torch_ce(x, t, w, ii, eps, dtype=F32)
    assert _units(loss.detach().cpu(), ref_l) <= _fp32_bound(cpu_l, ref_l)
    assert _units(xd.grad.cpu(), 3.0 * ref_g) <= _fp32_bound(3.0 * cpu_g, 3.0 * ref_g)
    assert torch.equal(xd.grad.cpu()[ign], torch.zeros(int(ign.sum()), 1000))
    assert crit.weight.device.type == "cuda"                   # moved once, kept
    with torch.no_grad():
        lv = crit(xd, t.to(DEV))
    assert not lv.requires_grad and _bits(lv.cpu(), loss.detach().cpu())
    xb = x.to(DEV).bfloat16().requires_grad_(True)             # bf16 logits: the gradient arrives in bf16
    crit(xb, t.to(DEV)).backward()
    assert xb.grad.dtype == BF16
    tb = t.clone()
    tb[0] = 1000
    with pytest.raises(IndexError):
        crit(xd, tb.to(DEV))
    with pytest.raises(ValueError):
        crit(xd[:, :999], t.to(DEV))                           # weight length
    with pytest.raises(ValueError):
        crit(xd, t[:3].to(DEV))
    # the defaults are nn.CrossEntropyLoss(): ignore_index -100 is live
    t2 = t.clone()
    t2[1] = -100
    l2 = CE()(x.to(DEV), t2.to(DEV))
    r2 = F.cross_entropy(x.double(), t2)
    assert abs(float(l2) - float(r2)) <= 1e-6 * (1 + abs(float(r2)))


# ------------------------------------------------------------------------------------------------------------- trainer
def _model(cfg, sd, dtype="fp32"):
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _opts(N, seed=5):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(N, generator=g) + 0.2
    w[1] = 0.0
    return dict(label_smoothing=0.1, class_weight=w, ignore_index=-100)


def test_trainer_steps_match_the_autograd_route():
    """Three fp32 steps, dropout 0, all three options, against forward -> F.cross_entropy(options) -> clip_grad_norm_ -> torch.optim
    .AdamW on a second copy of the model.  Bounds of test_gpu_soft_targets.py's whole-step comparison: loss 1e-4, clip norm 5e-3
    relative, per-tensor update 2e-2 relative (atol 1e-7); its logits bound, 1e-3, is a single-step bound and is asserted at step 0
    only, where both routes hold the same parameters.  Later steps compare two trajectories: Adam's first updates are +-lr per
    element whatever the gradient's size, so an element whose gradient is rounding noise may legitimately move in opposite
    directions on the two routes (2 lr apart), and the logits inherit that; they are printed.  The difference between the routes
    in a later step's update grows with lr for the same reason, so the bounds are used with the learning rate of the test they
    come from, the default 1e-4, which is also what training/train.py runs.  (Measured on an MI355X at lr 1e-3: step 0 equal to the
    last bit in logits and loss, clip norm 2.7e-7; at step 2 logits 1.5e-3, loss 4.3e-5, clip norm 7.2e-4, and one tensor of 164 at
    2.04e-2 of its update -- trajectory divergence, not the loss: the routes agree bit for bit at step 0.)"""
    cfg = O.full_config(**SMALL)
    N = cfg["num_answers"]
    sd = O.init_state_dict(cfg, 41, jitter=True)
    opts = _opts(N)
    m1, m2 = _model(cfg, sd), _model(cfg, sd)
    tr = pkg().trainer.HipTrainer(m1, **opts)                  # the set-up those bounds belong to: HipTrainer's defaults (lr 1e-4)
    opt = torch.optim.AdamW(m2.parameters(), lr=1e-4, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)
    wd = opts["class_weight"].to(DEV)
    names = [n for n, _ in m1.named_parameters()]
    for s in range(3):
        images, ids, mask, t = [v.to(DEV) for v in O.synthetic_batch(4, seed=700 + s, **SMALL_BATCH)]
        t = t.clone()
        t[s % 4] = -100
        P1, P2 = dict(m1.named_parameters()), dict(m2.named_parameters())
        b1 = {n: P1[n].detach().clone() for n in names}
        b2 = {n: P2[n].detach().clone() for n in names}
        loss, logits = tr.step(images, ids, mask, t)
        opt.zero_grad()
        lg2, _ = m2(images, ids, mask)
        l2 = F.cross_entropy(lg2, t, weight=wd, ignore_index=-100, label_smoothing=0.1)
        l2.backward()
        gn = torch.nn.utils.clip_grad_norm_(m2.parameters(), 1.0)
        opt.step()
        torch.cuda.synchronize()
        tr.check()
        d_logits = (logits - lg2.detach()).abs().max().item()
        d_loss = abs(float(loss.item()) - float(l2.detach()))
        d_norm = abs(float(tr.grad_norm().item()) - float(gn)) / float(gn)
        print(f"opts step {s}: logits {d_logits:.3e}, loss {d_loss:.3e} (ref {float(l2.detach()):.4f}), clip norm rel {d_norm:.3e}")
        assert (s > 0 or d_logits < 1e-3) and d_loss < 1e-4 and d_norm < 5e-3
        delta = np.array([float((P1[n].detach() - b1[n]).double().norm()) for n in names])
        ref_delta = np.array([float((P2[n].detach() - b2[n]).double().norm()) for n in names])
        np.testing.assert_allclose(delta, ref_delta, rtol=2e-2, atol=1e-7)


def _state(m, tr):
    bn = [v.detach().clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k]
    return [m._flat.detach().clone(), tr.m.clone(), tr.v.clone(), tr.loss.clone()] + bn


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_default_keywords_leave_the_step_bit_equal_and_launch_the_plain_loss(dtype):
    cfg = O.full_config(**SMALL)
    sd = O.init_state_dict(cfg, 31, jitter=True)
    batches = [[t.to(DEV) for t in O.synthetic_batch(4, seed=900 + s, **SMALL_BATCH)] for s in range(2)]
    L = sub("_lib")
    out, names = [], []
    for kw in (dict(), dict(label_smoothing=0.0, class_weight=None, ignore_index=None)):
        m = _model(cfg, sd, dtype)
        tr = pkg().trainer.HipTrainer(m, lr=1e-3, **kw)
        acc = pkg().load_dropin_metrics().VQAAccuracy()
        seen = []
        old = L._HOOK[0]
        L._HOOK[0] = lambda name, args: seen.append(name)
        try:
            for images, ids, mask, answers in batches:
                _, logits = tr.step(images, ids, mask, answers, metrics=acc)
        finally:
            L._HOOK[0] = old
        torch.cuda.synchronize()
        tr.check()
        names.append(seen)
        out.append(_state(m, tr) + [logits.clone(), torch.tensor(acc._read())])
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert names[0] == names[1] and "vqa_cross_entropy" in names[1] and "vqa_accuracy_update" in names[1]
    assert "vqa_cross_entropy_opts" not in names[1]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fused_metric_counts_the_kept_rows_without_a_metric_launch(dtype):
    cfg = O.full_config(**SMALL)
    N = cfg["num_answers"]
    sd = O.init_state_dict(cfg, 23, jitter=True)
    m = _model(cfg, sd, dtype)
    tr = pkg().trainer.HipTrainer(m, lr=1e-3, **_opts(N))
    MET = pkg().load_dropin_metrics()
    fused, alone = MET.VQAAccuracy(), MET.VQAAccuracy()
    L = sub("_lib")
    seen, kept = [], []
    old = L._HOOK[0]
    L._HOOK[0] = lambda name, args: seen.append(name)
    try:
        for s in range(2):
            images, ids, mask, t = [v.to(DEV) for v in O.synthetic_batch(4, seed=300 + s, **SMALL_BATCH)]
            t = t.clone()
            t[1 + s] = -100
            _, logits = tr.step(images, ids, mask, t, metrics=fused)
            kept.append((logits[t != -100], t[t != -100]))
    finally:
        L._HOOK[0] = old
    names = list(seen)
    for lg, tt in kept:                                        # the separate metric launch, outside the recorded window
        alone.update(lg, tt)
    torch.cuda.synchronize()
    tr.check()
    assert names.count("vqa_cross_entropy_opts") == 2 and "vqa_accuracy_update" not in names and "vqa_cross_entropy" not in names
    assert fused._read() == alone._read() and fused.total == 6


def test_refusals_soft_targets_with_options_and_a_zero_weight_batch():
    cfg = O.full_config(**SMALL)
    N = cfg["num_answers"]
    m = _model(cfg, O.init_state_dict(cfg, 1))
    HT = pkg().trainer.HipTrainer
    images, ids, mask, t = [v.to(DEV) for v in O.synthetic_batch(2, seed=1, **SMALL_BATCH)]
    ST = pkg().load_dropin_soft_targets()
    soft = ST.SoftTargets(t.int()[:, None].contiguous(), torch.ones(2, 1, device=DEV))
    L = sub("_lib")
    for kw in (dict(label_smoothing=0.1), dict(class_weight=torch.ones(N)), dict(ignore_index=-100)):
        tr = HT(m, **kw)
        seen = []
        old = L._HOOK[0]
        L._HOOK[0] = lambda name, args: seen.append(name)
        try:
            with pytest.raises(TypeError):
                tr.step(images, ids, mask, soft)
        finally:
            L._HOOK[0] = old
        assert seen == []                                      # refused before any launch
    for kw in (dict(label_smoothing=1.5), dict(class_weight=torch.ones(N + 1)), dict(class_weight=-torch.ones(N))):
        with pytest.raises(ValueError):
            HT(m, **kw)
    tr = HT(m, ignore_index=-100)
    tr.step(images, ids, mask, t)
    torch.cuda.synchronize()
    tr.check()
    p0 = m._flat.detach().clone()
    loss, _ = tr.step(images, ids, mask, torch.full_like(t, -100))
    torch.cuda.synchronize()
    assert math.isnan(float(loss.item())) and bool(torch.isfinite(m._flat).all())
    assert not torch.equal(m._flat.detach(), p0)               # AdamW ran on the zero gradient (weight decay, decayed moments)
    with pytest.raises(ValueError, match="1 step"):
        tr.check()
    tr.check()                                                 # the counter was cleared
