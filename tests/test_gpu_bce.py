"""GPU: sigmoid + binary cross-entropy on the soft answer scores through every layer -- vqa_bce_soft against
F.binary_cross_entropy_with_logits(reduction="sum") / B in fp64 (the bounds of
test_gpu_soft_targets.py::test_soft_cross_entropy_kernel_matches_torch), its bad-target rule, its bit-reproducible workspace mode and
its fused challenge accuracy; HipTrainer(loss="bce") against the CPU oracle driven by autograd (tests/_bceref.py BCEOracleTrainer),
its launch list, the skipped step, the cached-features route; SoftTargetBCEWithLogits under autograd; the host errors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bceref as R
from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(dropout=0.0, answer_dropout=0.0, vocab_size=100, num_answers=10, embed_dim=32)
SMALL_BATCH = dict(image_size=64, seq_len=10, vocab=100, num_answers=10)
SHAPES = ((512, 1000), (7, 10), (33, 2000))
EXTREMES = (90.0, -90.0, 88.7, -104.0)
_CACHE = {}


def _ST():
    return pkg().load_dropin_soft_targets()


def _model(cfg, sd, dtype="fp32"):
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _annotators(B, N, seed, A=10):
    """tests/test_gpu_soft_targets.py::_annotators: each question draws from a pool of three answers, ~20 % of the entries are out of
    the vocabulary (-1), row 0 has no in-vocabulary answer at all when B > 2."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.randint(0, N, (B, 3), generator=g)
    pick = torch.randint(0, 3, (B, A), generator=g) * (torch.rand(B, A, generator=g) < 0.7)
    a = torch.gather(pool, 1, pick)
    a[torch.rand(B, A, generator=g) < 0.2] = -1
    if B > 2:
        a[0] = -1
    return a


def _case(dtype, K, B, N):
    """One seeded kernel case and its fp64 torch reference (on the logits as the kernel reads them), computed once and left unchanged:
    (logits on the host in `dtype`, ids, weights, reference loss, reference gradient)."""
    key = (dtype, K, B, N)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * K + B)
        x = torch.randn(B, N, generator=g) * 3
        x[0, :4] = torch.tensor(EXTREMES)
        x = x.to(dtype)
        ids, w = R.random_soft(B, N, K, g)
        xin = x.double().requires_grad_(True)
        ref = F.binary_cross_entropy_with_logits(xin, R.dense(ids, w, N), reduction="sum") / B
        ref.backward()
        _CACHE[key] = (x, ids, w, float(ref.detach()), xin.grad)
    return _CACHE[key]


def _bce(L, dtype, logits, ids, w, ws=True, counts=None, acc=None, want_grad=True, err=None, gscale=1.0):
    B, N = logits.shape
    loss = torch.zeros(1, device=DEV)
    dl = torch.empty(B, N, device=DEV, dtype=dtype) if want_grad else None
    lf = torch.empty(B, N, device=DEV)
    wsb = torch.empty(B, device=DEV) if ws else None
    L.call("vqa_bce_soft", L.dt(dtype), logits.data_ptr(), ids.data_ptr(), w.data_ptr(), ids.shape[1], loss.data_ptr(),
           L.ptr(dl), lf.data_ptr(), B, N, gscale, L.ptr(err), L.ptr(wsb), L.ptr(counts), L.ptr(acc))
    torch.cuda.synchronize()
    return loss, dl, lf


# ---------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("K", [1, 4, 10, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bce_kernel_matches_torch(dtype, K):
    L = sub("_lib")
    for B, N in SHAPES:
        x, ids, w, ref, gref = _case(dtype, K, B, N)
        xd, idd, wd = x.to(DEV), ids.to(DEV), w.to(DEV)
        tol = 1e-6 if dtype == torch.float32 else 4e-3 * float(gref.abs().max())
        err = torch.zeros(1, device=DEV, dtype=torch.int32)
        for ws in (True, False):
            loss, dl, lf = _bce(L, dtype, xd, idd, wd, ws=ws, err=err)
            d_loss = abs(loss.item() - ref)
            d_grad = (dl.double().cpu() - gref).abs().max().item()
            print(f"BCE {dtype} K={K} B={B} N={N} ws={ws}: |loss - ref| = {d_loss:.3e} (ref {ref:.4f}), max|grad - ref| = {d_grad:.3e} (tol {tol:.3e})")
            assert np.isfinite(loss.item()) and torch.isfinite(dl).all()       # x = +-90 and beyond: the stable form
            assert d_loss < 1e-5 * max(1.0, abs(ref))
            assert d_grad < tol
            assert torch.equal(lf.cpu(), x.float())
            # rows without any answer: sigmoid(x) / B, not a zero row
            empty = (ids < 0).all(1)
            assert empty.any()
            sg = torch.sigmoid(x.double()[empty]) / B
            assert (dl.double().cpu()[empty] - sg).abs().max().item() < tol
            assert (dl.cpu()[empty] != 0).any(1).all()
            if ws:
                loss_ws = loss
        assert int(err.item()) == 0
        loss2, dl2, lf2 = _bce(L, dtype, xd, idd, wd, want_grad=False)            # validation: the loss alone, the same bits
        assert dl2 is None and torch.equal(loss2, loss_ws) and torch.equal(lf2.cpu(), x.float())


def test_gscale_multiplies_the_gradient():
    L = sub("_lib")
    x, ids, w, _, gref = _case(torch.float32, 4, 7, 10)
    _, dl, _ = _bce(L, torch.float32, x.to(DEV), ids.to(DEV), w.to(DEV), gscale=0.25)
    assert (dl.double().cpu() - 0.25 * gref).abs().max().item() < 1e-6


def test_bce_rejects_out_of_range_ids_without_reading_them():
    L = sub("_lib")
    B, N, K, PAD = 6, 10, 3, 64
    nan = float("nan")
    big = torch.full((PAD + B * N + PAD,), nan, device=DEV)                # NaN all around the logits: an out-of-bounds read poisons a good row
    logits = big[PAD:PAD + B * N].view(B, N)
    logits.copy_(torch.randn(B, N, generator=torch.Generator().manual_seed(8)))
    ids = torch.tensor([[1, -1, -1], [10, 2, -1], [3, 3, -1], [-2, 1, 1], [9, -1, 0], [2, 1 << 30, -1]], device=DEV, dtype=torch.int32)
    w = torch.full((B, K), 1.0 / 3.0, device=DEV)
    outs = [torch.full((PAD + B * N + PAD,), 5.0, device=DEV) for _ in range(2)]
    dl, lf = (o[PAD:PAD + B * N].view(B, N) for o in outs)
    loss = torch.zeros(1, device=DEV)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    L.call("vqa_bce_soft", 0, logits.data_ptr(), ids.data_ptr(), w.data_ptr(), K, loss.data_ptr(), dl.data_ptr(), lf.data_ptr(), B, N, 1.0,
           err.data_ptr(), None, None, None)
    torch.cuda.synchronize()
    bad = R.bad_rows(ids, N)
    assert bad.tolist() == [False, True, False, True, False, True]
    assert int(err.item()) == int(bad.sum()) == 3
    assert torch.isnan(loss).all()
    assert torch.isnan(dl.cpu()[bad]).all() and torch.isfinite(dl.cpu()[~bad]).all()
    assert torch.equal(lf, logits)
    for o in outs:                                                         # nothing written outside the rows
        assert (o[:PAD] == 5.0).all() and (o[PAD + B * N:] == 5.0).all()
    # the good rows alone: finite loss and gradient, equal to torch's
    good = (~bad).nonzero().flatten().to(DEV)
    xg, ig, wg = logits[good].contiguous(), ids[good].contiguous(), w[good].contiguous()
    loss_g, dl_g, _ = _bce(L, torch.float32, xg, ig, wg)
    xin = xg.cpu().double().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(xin, R.dense(ig, wg, N), reduction="sum") / len(good)
    ref.backward()
    assert abs(loss_g.item() - ref.item()) < 1e-5 * max(1.0, abs(ref.item()))
    assert (dl_g.double().cpu() - xin.grad).abs().max().item() < 1e-6


def test_two_runs_with_a_workspace_are_bit_identical():
    L = sub("_lib")
    B, N, K = 512, 1000, 10
    for dtype in (torch.float32, torch.bfloat16):
        x, ids, w, _, _ = _case(dtype, K, B, N)
        a = _bce(L, dtype, x.to(DEV), ids.to(DEV), w.to(DEV))
        b = _bce(L, dtype, x.to(DEV), ids.to(DEV), w.to(DEV))
        for u, v in zip(a, b):
            assert torch.equal(u, v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_thirds_equal_the_metric_kernel_and_the_reference(dtype):
    L = sub("_lib")
    for (B, N), K in zip(SHAPES, (10, 64, 4)):
        g = torch.Generator().manual_seed(50 + K)
        x = (torch.randn(B, N, generator=g) * 3).to(dtype)
        ids, w = R.random_soft(B, N, K, g)
        cnt = torch.randint(0, 5, (B, K), generator=g).int()
        # the prediction is one of the row's answers in most rows; row 1's maximum is tied: the lowest index wins
        rows = torch.arange(B)[(ids[:, 0] >= 0)]
        x[rows, ids[rows, 0].long()] = 20.0
        lo, hi = 2, N - 1
        x[1] = -1.0
        x[1, lo] = x[1, hi] = 21.0
        ids[1, 0], cnt[1, 0] = hi, 3
        if K > 1:
            ids[1, 1:] = -1
            ids[1, 1], cnt[1, 1] = lo, 1
        _, _, _, want = R.bce(x, ids, w, cnt)
        acc_f = torch.zeros(2, device=DEV, dtype=torch.int64)
        acc_a = torch.zeros(2, device=DEV, dtype=torch.int64)
        xd, idd, cd = x.to(DEV), ids.to(DEV), cnt.to(DEV)
        _bce(L, dtype, xd, idd, w.to(DEV), counts=cd, acc=acc_f)
        xf = xd.float()
        L.call("vqa_challenge_accuracy_update", xf.data_ptr(), idd.data_ptr(), cd.data_ptr(), K, acc_a.data_ptr(), B, N)
        torch.cuda.synchronize()
        assert acc_f.tolist() == acc_a.tolist() == want, (B, N, K)
        assert 0 < want[0] < 3 * B
    # the tie alone: class 2 (one vote) wins over class 7 (three votes)
    x = torch.zeros(1, 10, device=DEV, dtype=dtype)
    x[0, 2] = x[0, 7] = 4.0
    acc = torch.zeros(2, device=DEV, dtype=torch.int64)
    _bce(L, dtype, x, torch.tensor([[7, 2, -1]], device=DEV, dtype=torch.int32), torch.ones(1, 3, device=DEV),
         counts=torch.tensor([[3, 1, 0]], device=DEV, dtype=torch.int32), acc=acc)
    assert acc.tolist() == [1, 1]


# ------------------------------------------------------------------------------------------------------------- whole step
@pytest.mark.parametrize("tag,cfgkw,seed,B,bkw", [
    ("full", dict(dropout=0.0, answer_dropout=0.0), 2, 4, dict(image_size=224, seq_len=20, vocab=1000, num_answers=1000)),
    ("small", SMALL, 3, 2, SMALL_BATCH),
])
def test_bce_step_matches_the_oracle_driven_by_autograd(tag, cfgkw, seed, B, bkw):
    """The project's step bounds: logits 1e-3, clip norm 5e-3 relative, per-tensor update 2e-2 relative, BatchNorm buffers 1e-4.  The
    loss sums N terms per question, so it is compared with fp64 BCE evaluated on the RETURNED logits at 1e-5 * max(1, |ref|)."""
    cfg = O.full_config(**cfgkw)
    N = cfg["num_answers"]
    sd = O.init_state_dict(cfg, seed, jitter=True)
    m = _model(cfg, sd)
    tr = pkg().trainer.HipTrainer(m, loss="bce")
    assert tr.loss_kind == "bce"
    ot = R.BCEOracleTrainer(sd, cfg)
    images, ids, mask, _ = O.synthetic_batch(B, seed=seed + 100, **bkw)
    soft = _ST().answer_scores(_annotators(B, N, seed + 7).to(DEV), N)
    t = R.dense(soft.ids, soft.weights, N)
    lo, lref, gno = ot.step(images, ids, mask, t.float())
    names = O.parameter_names(cfg)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    loss, logits = tr.step(images.to(DEV), ids.to(DEV), mask.to(DEV), soft)
    torch.cuda.synchronize()
    tr.check()
    ref = float(F.binary_cross_entropy_with_logits(logits.cpu().double(), t, reduction="sum") / B)
    d_logits = (logits.cpu() - lref).abs().max().item()
    d_loss = abs(float(loss.item()) - ref)
    d_norm = abs(float(tr.grad_norm().item()) - float(gno)) / float(gno)
    print(f"BCE step {tag}: logits {d_logits:.3e}, loss {d_loss:.3e} (ref {ref:.4f}, oracle {float(lo):.4f}), clip norm rel {d_norm:.3e}")
    assert d_logits < 1e-3 and d_loss < 1e-5 * max(1.0, abs(ref)) and d_norm < 5e-3
    P = dict(m.named_parameters())
    delta = np.array([float((P[n].detach() - before[n]).double().norm()) for n in names])
    ref_delta = np.array([float((ot.sd[n].detach() - sd[n]).double().norm()) for n in names])
    np.testing.assert_allclose(delta, ref_delta, rtol=2e-2, atol=1e-7)
    st = m.state_dict()
    for k, v in ot.sd.items():
        if "running_" in k:
            assert (st[k].cpu() - v).abs().max().item() < 1e-4, k


def test_bce_step_swaps_one_launch_name_and_the_default_step_is_unchanged():
    L = sub("_lib")
    M = pkg().load_dropin_metrics()
    cfg = O.full_config(**SMALL)
    N = cfg["num_answers"]
    sd = O.init_state_dict(cfg, 5, jitter=True)
    images, ids, mask, answers = [t.to(DEV) for t in O.synthetic_batch(4, seed=300, **SMALL_BATCH)]
    soft = _ST().answer_scores(_annotators(4, N, 9).to(DEV), N)

    def entries(targets, metrics, **kw):
        m = _model(cfg, sd, "bf16")
        tr = pkg().trainer.HipTrainer(m, **kw)
        tr.step(images, ids, mask, targets, metrics=metrics)                # (the first step also casts the parameters)
        seen, old = [], L._HOOK[0]

        def hook(name, args):
            seen.append(name)
            return old(name, args) if old is not None else None
        L._HOOK[0] = hook
        try:
            tr.step(images, ids, mask, targets, metrics=metrics)
        finally:
            L._HOOK[0] = old
        torch.cuda.synchronize()
        tr.check()
        return seen
    hard = entries(answers, None)
    hard_ce = entries(answers, None, loss="ce")
    soft_ce = entries(soft, None)
    ch = M.VQAChallengeAccuracy()
    bce_m = entries(soft, ch, loss="bce")
    bce_p = entries(soft, None, loss="bce")
    assert hard == hard_ce and hard.count("vqa_cross_entropy") == 1 and "vqa_bce_soft" not in hard and "vqa_bce_soft" not in soft_ce
    assert soft_ce.count("vqa_cross_entropy_soft") == 1
    swapped = ["vqa_bce_soft" if n == "vqa_cross_entropy_soft" else n for n in soft_ce]
    assert bce_m == swapped and bce_p == swapped
    assert ch.count == 8 and 0 <= ch.total_score <= 8


def test_a_bce_step_with_a_bad_annotator_id_is_skipped():
    cfg = O.full_config(**SMALL)
    N = cfg["num_answers"]
    m = _model(cfg, O.init_state_dict(cfg, 1))
    tr = pkg().trainer.HipTrainer(m, loss="bce")
    images, ids, mask, _ = [t.to(DEV) for t in O.synthetic_batch(2, seed=1, **SMALL_BATCH)]
    ann = _annotators(2, N, 3)
    tr.step(images, ids, mask, _ST().answer_scores(ann.to(DEV), N))
    torch.cuda.synchronize()
    tr.check()
    p0, m0, v0, t0 = m._flat.detach().clone(), tr.m.clone(), tr.v.clone(), tr.t
    assert t0 == 1 and not tr.reducer.active
    ann[1, 4] = N
    tr.step(images, ids, mask, _ST().answer_scores(ann.to(DEV), N))
    torch.cuda.synchronize()
    assert bool(torch.isnan(tr.loss).all())
    assert torch.equal(m._flat.detach(), p0) and torch.equal(tr.m, m0) and torch.equal(tr.v, v0)
    assert tr.t == t0 and tr.calls == t0 + 1
    with pytest.raises(IndexError, match="out of range"):
        tr.check()
    tr.check()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bce_steps_from_features_are_bit_equal_to_the_images_steps(dtype):
    """loss="bce" with an image index and a frozen eval-mode CNN: the step on ImageFeatures against the step on the images."""
    cfg = O.full_config(**SMALL)
    sd = O.init_state_dict(cfg, 41, jitter=True)
    M = pkg().load_dropin_metrics()
    index = torch.tensor([0, 1, 1, 0, 1, 0, 0])                              # 3 images, 7 questions, image 2 without a question
    models, trainers, metrics = [], [], []
    for _ in range(2):
        m = _model(cfg, sd, dtype)
        m.image_encoder.requires_grad_(False)
        m.image_encoder.eval()
        models.append(m)
        trainers.append(pkg().trainer.HipTrainer(m, lr=1e-3, loss="bce"))
        metrics.append(M.VQAChallengeAccuracy())
    (a, b), (ta, tb) = models, trainers
    for s in range(2):
        images, ids, mask, _ = [t.to(DEV) for t in O.synthetic_batch(7, seed=300 + s, **SMALL_BATCH)]
        images = images[:3].contiguous()
        soft = _ST().answer_scores(_annotators(7, 10, 60 + s).to(DEV), 10)
        a.eval()
        with torch.no_grad():
            feats = a.encode_features(images)
        a.train()
        a.image_encoder.eval()
        la, lga = ta.step(feats, ids, mask, soft, metrics=metrics[0], image_index=index)
        lb, lgb = tb.step(images, ids, mask, soft, metrics=metrics[1], image_index=index)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(la).all())
        for u, v in ((la, lb), (lga, lgb), (a._flat.detach(), b._flat.detach()), (ta.m, tb.m), (ta.v, tb.v)):
            assert torch.equal(u, v), s
    ta.check(); tb.check()
    assert metrics[0]._read() == metrics[1]._read() and metrics[0].count == 14


def test_soft_target_bce_module_under_autograd():
    crit = _ST().SoftTargetBCEWithLogits()
    ST = _ST()
    for dtype, (B, N), K in ((torch.float32, (7, 10), 4), (torch.float32, (33, 2000), 10), (torch.bfloat16, (33, 2000), 10)):
        x, ids, w, ref, gref = _case(dtype, K, B, N)
        soft = ST.SoftTargets(ids.to(DEV), w.to(DEV))
        tol = 1e-6 if dtype == torch.float32 else 4e-3 * float(gref.abs().max())
        a = x.to(DEV).requires_grad_(True)
        loss = crit(a, soft)
        assert loss.dim() == 0 and loss.requires_grad and loss.dtype == torch.float32
        loss.backward()
        assert abs(loss.item() - ref) < 1e-5 * max(1.0, abs(ref))
        assert (a.grad.double().cpu() - gref).abs().max().item() < tol
        if dtype == torch.float32:                                         # a scaled loss scales the gradient
            b = x.to(DEV).requires_grad_(True)
            (crit(b, soft) * 3.0).backward()
            assert torch.allclose(b.grad, 3.0 * a.grad, rtol=1e-6, atol=0)
        with torch.no_grad():
            lv = crit(a, soft)
        assert not lv.requires_grad and torch.equal(lv, loss.detach())
    x, ids, w, _, _ = _case(torch.float32, 4, 7, 10)
    soft = ST.SoftTargets(ids.to(DEV), w.to(DEV))
    bad = ST.SoftTargets(soft.ids.clone(), soft.weights)
    bad.ids[1, 0] = 10
    with pytest.raises(IndexError):
        crit(x.to(DEV), bad)
    with pytest.raises(ValueError):
        crit(x.to(DEV)[:3], soft)
    with pytest.raises(RuntimeError):
        crit(x, soft)                                                       # host logits: there is no CPU path


def test_host_errors_come_before_any_launch():
    M = pkg().load_dropin_metrics()
    L = sub("_lib")
    HT = pkg().trainer.HipTrainer
    cfg = O.full_config(**SMALL)
    m = _model(cfg, O.init_state_dict(cfg, 1))
    m._ensure_engine()
    images, ids, mask, labels = [t.to(DEV) for t in O.synthetic_batch(2, seed=1, **SMALL_BATCH)]
    soft = _ST().answer_scores(_annotators(2, 10, 3).to(DEV), 10)
    seen, old = [], L._HOOK[0]
    L._HOOK[0] = lambda name, args: seen.append(name)
    try:
        for kw in (dict(loss="mse"), dict(loss="BCE"), dict(loss=None), dict(loss="bce", label_smoothing=0.1),
                   dict(loss="bce", class_weight=torch.ones(10)), dict(loss="bce", ignore_index=-100)):
            with pytest.raises(ValueError):
                HT(m, **kw)
        assert seen == []
        tr = HT(m, loss="bce")
        assert tr.loss_kind == "bce" and HT(m).loss_kind == "ce"
        del seen[:]                                                        # (the constructors may set up buffers; the steps below must not launch)
        with pytest.raises(TypeError, match=r"SoftTargets\(labels\.int\(\)\[:, None\], ones\)"):
            tr.step(images, ids, mask, labels)
        with pytest.raises(TypeError):
            tr.step(images, ids, mask, labels, metrics=M.VQAAccuracy())
        with pytest.raises(TypeError):
            tr.step(images, ids, mask, soft, metrics=M.VQAAccuracy())
        with pytest.raises(TypeError):
            tr.step(images, ids, mask, _ST().SoftTargets(soft.ids, soft.weights), metrics=M.VQAChallengeAccuracy())
    finally:
        L._HOOK[0] = old
    assert seen == [] and tr.calls == 0
    # hard labels wrapped as the message says: the step runs
    wrapped = _ST().SoftTargets(labels.int()[:, None].contiguous(), torch.ones(2, 1, device=DEV))
    loss, _ = tr.step(images, ids, mask, wrapped)
    torch.cuda.synchronize()
    tr.check()
    assert bool(torch.isfinite(loss).all())
