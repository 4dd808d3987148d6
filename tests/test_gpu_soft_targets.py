"""GPU: soft answer scores (ten annotator answers per question) through every layer -- vqa_answer_scores against a numpy
first-occurrence count on the fixture written by the reference's VQAChallengeAccuracy (tests/golden/soft_targets.npz),
vqa_cross_entropy_soft against F.cross_entropy with dense probability targets in fp64 (tolerances of
test_gpu_trainer.py::test_cross_entropy_kernel_matches_torch) and bit-equal to vqa_cross_entropy for K = 1, the challenge accuracy in
exact integer thirds, and HipTrainer.step / SoftTargetCrossEntropy / VQAChallengeAccuracy against the CPU oracle driven by autograd."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(dropout=0.0, answer_dropout=0.0, vocab_size=100, num_answers=10, embed_dim=32)
SMALL_BATCH = dict(image_size=64, seq_len=10, vocab=100, num_answers=10)


def _ST():
    return pkg().load_dropin_soft_targets()


def _model(cfg, sd, dtype="fp32"):
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _annotators(B, N, seed, A=10):
    """Seeded annotator ids [B, A]: each question draws from a pool of three answers (so 1 .. 10 votes occur), ~20 % of the entries
    are out of the vocabulary (-1), row 0 has no in-vocabulary answer at all when B > 2."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.randint(0, N, (B, 3), generator=g)
    pick = torch.randint(0, 3, (B, A), generator=g) * (torch.rand(B, A, generator=g) < 0.7)      # biased towards pool[:, 0]
    a = torch.gather(pool, 1, pick)
    a[torch.rand(B, A, generator=g) < 0.2] = -1
    if B > 2:
        a[0] = -1
    return a


def _dense(ids, weights, N):
    """t[b, c] = sum of weights[b, k] over ids[b, k] == c, on the CPU in fp64 (-1 slots skipped)."""
    ids, w = ids.cpu().long(), weights.cpu().double()
    return torch.zeros(ids.shape[0], N, dtype=torch.float64).scatter_add_(1, ids.clamp(min=0), w * (ids >= 0))


def _first_occurrence(row, N):
    ids, cnt = [], []
    for v in row:
        if 0 <= v < N:
            if v in ids:
                cnt[ids.index(v)] += 1
            else:
                ids.append(int(v)); cnt.append(1)
    return ids, cnt


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "soft_targets.npz"))
    return g, g["answers"].astype(np.int64), g["pred"].astype(np.int64), [int(n) for n in g["block_n"]]


def _soft_ce(L, dtype, logits, ids, w, ws=True, counts=None, acc=None, want_grad=True, err=None):
    B, N = logits.shape
    loss = torch.zeros(1, device=DEV)
    dl = torch.empty(B, N, device=DEV, dtype=dtype) if want_grad else None
    lf = torch.empty(B, N, device=DEV)
    wsb = torch.empty(B, device=DEV) if ws else None
    L.call("vqa_cross_entropy_soft", L.dt(dtype), logits.data_ptr(), ids.data_ptr(), w.data_ptr(), ids.shape[1], loss.data_ptr(),
           L.ptr(dl), lf.data_ptr(), B, N, 1.0, L.ptr(err), L.ptr(wsb), L.ptr(counts), L.ptr(acc))
    torch.cuda.synchronize()
    return loss, dl, lf


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("mode", [0, 1])
def test_answer_scores_on_the_fixture(golden_dir, mode):
    L = sub("_lib")
    _, answers, _, block_n = _golden(golden_dir)
    per = len(answers) // len(block_n)
    for b, N in enumerate(block_n):
        a = answers[b * per:(b + 1) * per].copy()
        a[5, 3], a[9, 0], a[9, 7], a[11, 9] = N, -2, N + 5, 1 << 40         # three offending rows (one of them twice)
        ad = torch.from_numpy(a).to(DEV)
        B, A = a.shape
        ids = torch.full((B, A), 77, device=DEV, dtype=torch.int32)
        w = torch.full((B, A), 77.0, device=DEV)
        cnt = torch.full((B, A), 77, device=DEV, dtype=torch.int32)
        err = torch.zeros(1, device=DEV, dtype=torch.int32)
        L.call("vqa_answer_scores", ad.data_ptr(), ids.data_ptr(), w.data_ptr(), cnt.data_ptr(), B, A, N, mode, err.data_ptr())
        torch.cuda.synchronize()
        assert int(err.item()) == 3                                        # rows, not entries; -1 is not an error
        ids, w, cnt = ids.cpu().numpy(), w.cpu().numpy(), cnt.cpu().numpy()
        for r in range(B):
            if r in (5, 9, 11):
                assert ids[r].tolist() == [N] + [-1] * (A - 1) and not w[r].any() and not cnt[r].any(), r
                continue
            ri, rc = _first_occurrence(a[r], N)
            pad = A - len(ri)
            assert ids[r].tolist() == ri + [-1] * pad and cnt[r].tolist() == rc + [0] * pad, r
            ref = np.minimum(np.float32(1), np.array(rc + [0] * pad, dtype=np.float32) / np.float32(3))
            if mode == 1 and ri:
                s = np.float32(0)
                for v in ref[:len(ri)]:
                    s = np.float32(s + v)
                ref = (ref / s).astype(np.float32)
            assert ref.dtype == np.float32 and w[r].tobytes() == ref.tobytes(), (r, w[r], ref)


def _random_soft(B, N, K, g):
    """ids with duplicates, -1 slots and all-empty rows; weights as the scores come: 1/3, 2/3, 1 in fp32."""
    ids = torch.randint(0, N, (B, K), generator=g)
    if K > 1:
        ids[:, K // 2] = ids[:, 0]                                         # a duplicate in every row: the weights add up
        ids[torch.rand(B, K, generator=g) < 0.25] = -1
    ids[torch.arange(B) % 5 == 3] = -1                                     # rows without any answer
    w = (torch.randint(1, 4, (B, K), generator=g).float() / 3.0).clamp(max=1.0)
    return ids.int(), w


@pytest.mark.parametrize("K", [1, 4, 10])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_soft_cross_entropy_kernel_matches_torch(dtype, K):
    L = sub("_lib")
    g = torch.Generator().manual_seed(3)
    for B, N in ((512, 1000), (7, 10), (33, 2000)):
        logits = (torch.randn(B, N, generator=g) * 3).to(dtype)
        ids, w = _random_soft(B, N, K, g)
        t = _dense(ids, w, N)
        ref_in = logits.double().requires_grad_(True)
        ref = F.cross_entropy(ref_in, t)
        ref.backward()
        err = torch.zeros(1, device=DEV, dtype=torch.int32)
        for ws in (True, False):
            loss, dl, lf = _soft_ce(L, dtype, logits.to(DEV), ids.to(DEV), w.to(DEV), ws=ws, err=err)
            d_loss = abs(loss.item() - ref.item())
            d_grad = (dl.double().cpu() - ref_in.grad).abs().max().item()
            tol = 1e-6 if dtype == torch.float32 else 4e-3 * float(ref_in.grad.abs().max())
            print(f"soft CE {dtype} K={K} B={B} N={N} ws={ws}: |loss - ref| = {d_loss:.3e} (ref {ref.item():.4f}), max|grad - ref| = {d_grad:.3e} (tol {tol:.3e})")
            assert d_loss < 1e-5 * max(1.0, abs(ref.item()))
            assert d_grad < tol
            assert torch.equal(lf.cpu(), logits.float())
            empty = (ids < 0).all(1)
            assert empty.any() and (dl.cpu()[empty] == 0).all()              # W = 0: a zero gradient row
        assert int(err.item()) == 0
        loss2, dl2, _ = _soft_ce(L, dtype, logits.to(DEV), ids.to(DEV), w.to(DEV), want_grad=False)     # validation: the loss alone
        assert dl2 is None and abs(loss2.item() - ref.item()) < 1e-5 * max(1.0, abs(ref.item()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_slot_of_weight_one_is_bit_equal_to_the_hard_kernel(dtype):
    L = sub("_lib")
    g = torch.Generator().manual_seed(4)
    for B, N in ((512, 1000), (7, 10), (33, 2000)):
        ld = (torch.randn(B, N, generator=g) * 3).to(dtype).to(DEV)
        tgt = torch.randint(0, N, (B,), generator=g).to(DEV)
        loss = torch.zeros(1, device=DEV)
        dl, lf, ws = torch.empty(B, N, device=DEV, dtype=dtype), torch.empty(B, N, device=DEV), torch.empty(B, device=DEV)
        L.call("vqa_cross_entropy", L.dt(dtype), ld.data_ptr(), tgt.data_ptr(), loss.data_ptr(), dl.data_ptr(), lf.data_ptr(), B, N, 1.0, None, ws.data_ptr())
        loss_s, dl_s, lf_s = _soft_ce(L, dtype, ld, tgt.int()[:, None].contiguous(), torch.ones(B, 1, device=DEV))
        assert torch.equal(loss, loss_s) and torch.equal(dl, dl_s) and torch.equal(lf, lf_s), (B, N)


def test_soft_cross_entropy_rejects_out_of_range_ids_without_reading_them():
    L = sub("_lib")
    B, N, K, PAD = 6, 10, 3, 64
    nan = float("nan")
    big = torch.full((PAD + B * N + PAD,), nan, device=DEV)                # NaN all around the logits: an out-of-bounds read poisons a good row
    logits = big[PAD:PAD + B * N].view(B, N)
    logits.copy_(torch.randn(B, N))
    ids = torch.tensor([[1, -1, -1], [10, 2, -1], [3, 3, -1], [-2, 1, 1], [9, -1, 0], [2, 1 << 30, -1]], device=DEV, dtype=torch.int32)
    w = torch.full((B, K), 1.0 / 3.0, device=DEV)
    outs = [torch.full((PAD + B * N + PAD,), 5.0, device=DEV) for _ in range(2)]
    dl, lf = (o[PAD:PAD + B * N].view(B, N) for o in outs)
    loss = torch.zeros(1, device=DEV)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    L.call("vqa_cross_entropy_soft", 0, logits.data_ptr(), ids.data_ptr(), w.data_ptr(), K, loss.data_ptr(), dl.data_ptr(), lf.data_ptr(), B, N, 1.0,
           err.data_ptr(), None, None, None)
    torch.cuda.synchronize()
    assert int(err.item()) == 3
    assert torch.isnan(loss).all()
    bad = torch.tensor([False, True, False, True, False, True])
    assert torch.isnan(dl.cpu()[bad]).all() and torch.isfinite(dl.cpu()[~bad]).all()
    assert torch.equal(lf, logits)
    for o in outs:                                                         # nothing written outside the rows
        assert (o[:PAD] == 5.0).all() and (o[PAD + B * N:] == 5.0).all()
    # the good rows alone: finite loss, equal to torch's
    good = (~bad).nonzero().flatten()
    loss_g, _, _ = _soft_ce(L, torch.float32, logits[good.to(DEV)].contiguous(), ids[good.to(DEV)].contiguous(), w[good.to(DEV)].contiguous())
    ref = F.cross_entropy(logits[good.to(DEV)].cpu().double(), _dense(ids.cpu()[good], w.cpu()[good], N))
    assert abs(loss_g.item() - ref.item()) < 1e-5 * max(1.0, abs(ref.item()))


def test_two_runs_with_a_workspace_are_bit_identical():
    L = sub("_lib")
    g = torch.Generator().manual_seed(6)
    B, N, K = 512, 1000, 10
    for dtype in (torch.float32, torch.bfloat16):
        ld = (torch.randn(B, N, generator=g) * 3).to(dtype).to(DEV)
        ids, w = _random_soft(B, N, K, g)
        a = _soft_ce(L, dtype, ld, ids.to(DEV), w.to(DEV))
        b = _soft_ce(L, dtype, ld, ids.to(DEV), w.to(DEV))
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def _logits_with_argmax(pred, N, seed, tie=True):
    """Random logits whose maximum sits at pred[b] -- and, again, at a HIGHER index when there is one (ties -> the lower index)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(len(pred), N, generator=g)
    p = torch.as_tensor(pred)
    x[torch.arange(len(pred)), p] = 9.0
    if tie:
        rows = (p < N - 1).nonzero().flatten()
        x[rows, p[rows] + 1 + (torch.arange(len(rows)) % (N - 1 - p[rows]))] = 9.0
    return x


def test_challenge_accuracy_fused_and_alone_equal_the_reference_thirds(golden_dir):
    L = sub("_lib")
    g, answers, pred, block_n = _golden(golden_dir)
    thirds = np.rint(g["scores"] * 3).astype(np.int64)
    assert np.abs(g["scores"] * 3 - thirds).max() < 1e-12
    per = len(pred) // len(block_n)
    acc_f = torch.zeros(2, device=DEV, dtype=torch.int64)
    acc_a = torch.zeros(2, device=DEV, dtype=torch.int64)
    for b, N in enumerate(block_n):
        sl = slice(b * per, (b + 1) * per)
        soft = _ST().answer_scores(torch.from_numpy(answers[sl]).to(DEV), N)
        x = _logits_with_argmax(pred[sl], N, seed=b).to(DEV)
        for dtype in (torch.float32, torch.bfloat16):
            before = acc_f.clone()
            _soft_ce(L, dtype, x.to(dtype), soft.ids, soft.weights, counts=soft.counts, acc=acc_f)
            assert (acc_f - before).tolist() == [int(thirds[sl].sum()), per], (b, dtype)
        L.call("vqa_challenge_accuracy_update", x.data_ptr(), soft.ids.data_ptr(), soft.counts.data_ptr(), soft.ids.shape[1], acc_a.data_ptr(), per, N)
    torch.cuda.synchronize()
    assert acc_a.tolist() == [int(thirds.sum()), len(pred)]
    assert acc_f.tolist() == [2 * int(thirds.sum()), 2 * len(pred)]
    # a tie between two logits resolves to the lower index: class 2 (one vote) wins over class 7 (three votes)
    x = torch.zeros(1, 10, device=DEV)
    x[0, 2] = x[0, 7] = 4.0
    ids = torch.tensor([[7, 2, -1]], device=DEV, dtype=torch.int32)
    cnt = torch.tensor([[3, 1, 0]], device=DEV, dtype=torch.int32)
    for fused in (False, True):
        acc = torch.zeros(2, device=DEV, dtype=torch.int64)
        if fused:
            _soft_ce(L, torch.float32, x, ids, torch.ones(1, 3, device=DEV), counts=cnt, acc=acc)
        else:
            L.call("vqa_challenge_accuracy_update", x.data_ptr(), ids.data_ptr(), cnt.data_ptr(), 3, acc.data_ptr(), 1, 10)
        assert acc.tolist() == [1, 1], fused


# ------------------------------------------------------------------------------------------------------------- whole step
@pytest.mark.parametrize("tag,cfgkw,seed,B,bkw", [
    ("full", dict(dropout=0.0, answer_dropout=0.0), 2, 4, dict(image_size=224, seq_len=20, vocab=1000, num_answers=1000)),
    ("small", SMALL, 3, 2, SMALL_BATCH),
])
def test_soft_step_matches_the_oracle_driven_by_autograd(tag, cfgkw, seed, B, bkw):
    """Bounds of test_gpu_trainer.py::test_hiptrainer_step_matches_reference_golden: logits 1e-3, loss 1e-4, clip norm 5e-3 relative,
    per-tensor update 2e-2 relative, BatchNorm buffers 1e-4."""
    cfg = O.full_config(**cfgkw)
    N = cfg["num_answers"]
    sd = O.init_state_dict(cfg, seed, jitter=True)
    m = _model(cfg, sd)
    tr = pkg().trainer.HipTrainer(m)
    ot = O.OracleTrainer(sd, cfg)
    images, ids, mask, _ = O.synthetic_batch(B, seed=seed + 100, **bkw)
    soft = _ST().answer_scores(_annotators(B, N, seed + 7).to(DEV), N)
    lo, lref, gno = ot.step(images, ids, mask, _dense(soft.ids, soft.weights, N).float())
    names = O.parameter_names(cfg)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    loss, logits = tr.step(images.to(DEV), ids.to(DEV), mask.to(DEV), soft)
    torch.cuda.synchronize()
    tr.check()
    d_logits = (logits.cpu() - lref).abs().max().item()
    d_loss = abs(float(loss.item()) - float(lo))
    d_norm = abs(float(tr.grad_norm().item()) - float(gno)) / float(gno)
    print(f"soft step {tag}: logits {d_logits:.3e}, loss {d_loss:.3e} (ref {float(lo):.4f}), clip norm rel {d_norm:.3e}")
    assert d_logits < 1e-3 and d_loss < 1e-4 and d_norm < 5e-3
    P = dict(m.named_parameters())
    delta = np.array([float((P[n].detach() - before[n]).double().norm()) for n in names])
    ref_delta = np.array([float((ot.sd[n].detach() - sd[n]).double().norm()) for n in names])
    np.testing.assert_allclose(delta, ref_delta, rtol=2e-2, atol=1e-7)
    st = m.state_dict()
    for k, v in ot.sd.items():
        if "running_" in k:
            assert (st[k].cpu() - v).abs().max().item() < 1e-4, k


def _state(m, tr):
    bn = [v.detach().clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k]
    return [m._flat.detach().clone(), tr.m.clone(), tr.v.clone(), tr.loss.clone()] + bn


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_slot_soft_step_is_bit_equal_to_the_hard_label_step(dtype):
    cfg = O.full_config(**SMALL)
    sd = O.init_state_dict(cfg, 31, jitter=True)
    batches = [[t.to(DEV) for t in O.synthetic_batch(4, seed=900 + s, **SMALL_BATCH)] for s in range(2)]
    out = []
    for soft in (False, True):
        m = _model(cfg, sd, dtype)
        tr = pkg().trainer.HipTrainer(m, lr=1e-3)
        for images, ids, mask, answers in batches:
            tgt = _ST().SoftTargets(answers.int()[:, None].contiguous(), torch.ones(4, 1, device=DEV)) if soft else answers
            _, logits = tr.step(images, ids, mask, tgt)
        torch.cuda.synchronize()
        tr.check()
        out.append(_state(m, tr) + [logits.clone()])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def _oracle_grouped(sd, cfg, images, ids, mask, t, index):
    names = set(O.parameter_names(cfg))
    sdr = {k: (v.clone().requires_grad_(True) if k in names else v.clone()) for k, v in sd.items()}
    nb = {}
    feat = O.image_encoder(images, sdr, True, nb)
    text, _ = O.text_encoder(ids, mask, sdr, cfg, True)
    fused, _ = O.fusion(feat[torch.as_tensor(index)], text, mask, sdr, cfg, True)
    logits = O.answer_head(fused, sdr, cfg, True)
    loss = F.cross_entropy(logits, t)
    loss.backward()
    return sdr, nb, logits.detach(), float(loss.detach())


def test_soft_step_with_an_image_index():
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0)
    N = cfg["num_answers"]
    sd = O.init_state_dict(cfg, 21, jitter=True)
    # identity index: the bits of the plain soft step
    images, ids, mask, _ = O.synthetic_batch(4, seed=31)
    soft = _ST().answer_scores(_annotators(4, N, 41).to(DEV), N)
    out = []
    for index in (None, torch.arange(4)):
        m = _model(cfg, sd)
        tr = pkg().trainer.HipTrainer(m)
        tr.step(images.to(DEV), ids.to(DEV), mask.to(DEV), soft, image_index=index)
        torch.cuda.synchronize()
        out.append(_state(m, tr) + [tr.G.clone()])
    for a, b in zip(*out):
        assert torch.equal(a, b)
    # two questions per image against the oracle composition (bounds of tests/test_gpu_grouped_train.py)
    index = [0, 0, 1, 1, 2, 2]
    images, _, _, _ = O.synthetic_batch(3, seed=51)
    _, ids, mask, _ = O.synthetic_batch(6, seed=52)
    mask[:, 0] = 1
    soft = _ST().answer_scores(_annotators(6, N, 53).to(DEV), N)
    m = _model(cfg, sd)
    tr = pkg().trainer.HipTrainer(m)
    loss, logits = tr.step(images.to(DEV), ids.to(DEV), mask.to(DEV), soft, image_index=torch.tensor(index))
    torch.cuda.synchronize()
    tr.check()
    sdr, nb, lref, sref = _oracle_grouped(sd, cfg, images, ids, mask, _dense(soft.ids, soft.weights, N).float(), index)
    assert (logits.cpu() - lref).abs().max().item() < 1e-3
    assert abs(loss.item() - sref) < 1e-4
    E, LY = m._engine.E, sub("layout")
    worst = (0.0, None)
    for n in O.parameter_names(cfg):
        gh, gr = LY.view_of(tr.G, E[n]).cpu().double().flatten(), sdr[n].grad.double().flatten()       # (conv weights are stored KRSC)
        if float(gr.norm()) < 1e-12:
            assert float(gh.norm()) < 1e-9, n
            continue
        rel = float((gh - gr).norm() / gr.norm())
        if rel > worst[0]:
            worst = (rel, n)
    assert worst[0] < 5e-2, worst
    st = m.state_dict()
    for k, v in nb.items():
        if "running_" in k:
            assert (st[k].cpu() - v).abs().max().item() < 1e-4, k


def test_soft_target_cross_entropy_module_under_autograd():
    cfg = O.full_config(**SMALL)
    N = cfg["num_answers"]
    sd = O.init_state_dict(cfg, 13, jitter=True)
    images, ids, mask, _ = [t.to(DEV) for t in O.synthetic_batch(4, seed=500, **SMALL_BATCH)]
    soft = _ST().answer_scores(_annotators(4, N, 17).to(DEV), N)
    crit = _ST().SoftTargetCrossEntropy()
    m = _model(cfg, sd)
    logits, _ = m(images, ids, mask)
    loss = crit(logits, soft)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    m2 = _model(cfg, sd)
    tr = pkg().trainer.HipTrainer(m2)
    tloss, tlogits = tr.step(images, ids, mask, soft)
    torch.cuda.synchronize()
    assert abs(loss.item() - tloss.item()) < 1e-6
    E, LY = m2._engine.E, sub("layout")
    for n, p in m.named_parameters():
        d = (p.grad - LY.view_of(tr.G, E[n])).abs().max().item()
        assert d < 1e-6, (n, d)
    # a scaled loss scales the gradient (the incoming gradient multiplies the kernel's d logits)
    x = tlogits.clone().requires_grad_(True)
    (crit(x, soft) * 3.0).backward()
    y = tlogits.clone().requires_grad_(True)
    crit(y, soft).backward()
    assert torch.allclose(x.grad, 3.0 * y.grad, rtol=1e-6, atol=0)
    ref = F.cross_entropy(tlogits.cpu().double(), _dense(soft.ids, soft.weights, N))
    with torch.no_grad():
        lv = crit(tlogits, soft)
    assert not lv.requires_grad and abs(lv.item() - ref.item()) < 1e-5 * max(1.0, abs(ref.item()))
    bad = _ST().SoftTargets(soft.ids.clone(), soft.weights, soft.counts)
    bad.ids[1, 0] = N
    with pytest.raises(IndexError):
        crit(tlogits, bad)
    with pytest.raises(ValueError):
        crit(tlogits[:3], soft)


def _skipped_step(force):
    """A soft step with an annotator id out of range: skipped (parameters, moments, Adam's step number untouched), check() raises."""
    cfg = O.full_config(**SMALL)
    N = cfg["num_answers"]
    m = _model(cfg, O.init_state_dict(cfg, 1))
    tr = pkg().trainer.HipTrainer(m, force_reducer=force)
    images, ids, mask, _ = [t.to(DEV) for t in O.synthetic_batch(2, seed=1, **SMALL_BATCH)]
    ann = _annotators(2, N, 3)
    tr.step(images, ids, mask, _ST().answer_scores(ann.to(DEV), N))
    torch.cuda.synchronize()
    tr.check()
    p0, m0, v0, t0 = m._flat.detach().clone(), tr.m.clone(), tr.v.clone(), tr.t
    ann[1, 4] = N
    tr.step(images, ids, mask, _ST().answer_scores(ann.to(DEV), N))
    torch.cuda.synchronize()
    res = dict(nan=bool(torch.isnan(tr.loss).all()), kept=torch.equal(m._flat.detach(), p0) and torch.equal(tr.m, m0) and torch.equal(tr.v, v0),
               t_kept=tr.t == t0 and tr.calls == t0 + 1, active=tr.reducer.active)
    try:
        tr.check()
        res["raised"] = False
    except IndexError as e:
        res["raised"] = "out of range" in str(e)
    tr.check()
    return res


def test_a_step_with_a_bad_annotator_id_is_skipped():
    r = _skipped_step(False)
    assert r["nan"] and r["kept"] and r["t_kept"] and r["raised"] and not r["active"], r


def _nccl1_worker(port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    q.put(_skipped_step(True))
    dist.destroy_process_group()


def test_a_step_with_a_bad_annotator_id_is_skipped_through_a_forced_reducer():
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")                                          # a fresh child process owns the RCCL group
    q = ctx.Queue()
    p = ctx.Process(target=_nccl1_worker, args=(port, q))
    p.start()
    try:
        r = q.get(timeout=300)
        p.join(timeout=120)
        assert p.exitcode == 0, p.exitcode
    finally:
        if p.is_alive():
            p.kill()
    assert r["nan"] and r["kept"] and r["t_kept"] and r["raised"] and r["active"], r


def test_the_fused_metric_costs_no_launch():
    L = sub("_lib")
    M = pkg().load_dropin_metrics()
    cfg = O.full_config(**SMALL)
    N = cfg["num_answers"]
    sd = O.init_state_dict(cfg, 5, jitter=True)
    images, ids, mask, answers = [t.to(DEV) for t in O.synthetic_batch(4, seed=300, **SMALL_BATCH)]
    soft = _ST().answer_scores(_annotators(4, N, 9).to(DEV), N)

    def entries(targets, metrics):
        m = _model(cfg, sd, "bf16")
        tr = pkg().trainer.HipTrainer(m)
        tr.step(images, ids, mask, targets, metrics=metrics)                # (the first step also casts the parameters)
        seen, old = [], L._HOOK[0]

        def hook(name, args):
            seen.append(name)
            return old(name, args) if old is not None else None
        L._HOOK[0] = hook
        try:
            _, logits = tr.step(images, ids, mask, targets, metrics=metrics)
        finally:
            L._HOOK[0] = old
        torch.cuda.synchronize()
        return seen, logits
    hard, _ = entries(answers, None)
    hard_m, _ = entries(answers, M.VQAAccuracy())
    ch = M.VQAChallengeAccuracy()
    soft_m, logits = entries(soft, ch)
    soft_p, _ = entries(soft, None)
    assert hard.count("vqa_cross_entropy") == 1 and "vqa_cross_entropy_soft" not in hard and "vqa_accuracy_update" not in hard
    assert hard_m == hard[:hard.index("vqa_cross_entropy") + 1] + ["vqa_accuracy_update"] + hard[hard.index("vqa_cross_entropy") + 1:]
    swapped = ["vqa_cross_entropy_soft" if n == "vqa_cross_entropy" else n for n in hard]
    assert soft_m == swapped and soft_p == swapped and len(soft_m) == len(hard_m) - 1
    # and the counters hold what the metric kernel alone finds on the returned logits of the two steps
    assert ch.count == 8
    alone = M.VQAChallengeAccuracy()
    alone.update(logits, soft)
    assert alone.count == 4 and 0 <= ch.total_score <= 8 and ch._read()[0] >= alone._read()[0] >= 0


def test_soft_step_with_a_frozen_cnn():
    cfg = O.full_config(**SMALL)
    N = cfg["num_answers"]
    m = _model(cfg, O.init_state_dict(cfg, 7, jitter=True))
    m.image_encoder.requires_grad_(False)
    m.image_encoder.eval()
    images, ids, mask, _ = [t.to(DEV) for t in O.synthetic_batch(4, seed=77, **SMALL_BATCH)]
    soft = _ST().answer_scores(_annotators(4, N, 19).to(DEV), N)
    with torch.no_grad():
        ref = _ST().SoftTargetCrossEntropy()(m(images, ids, mask)[0], soft)
    frozen = {n: p.detach().clone() for n, p in m.named_parameters() if not p.requires_grad}
    moving = {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}
    assert frozen and moving
    tr = pkg().trainer.HipTrainer(m, lr=1e-3)
    loss, _ = tr.step(images, ids, mask, soft)
    torch.cuda.synchronize()
    tr.check()
    assert abs(loss.item() - ref.item()) < 1e-6
    P = dict(m.named_parameters())
    for n, v in frozen.items():
        assert torch.equal(P[n].detach(), v), n
    assert any(not torch.equal(P[n].detach(), v) for n, v in moving.items())


def test_challenge_accuracy_metric_and_the_type_errors_of_step(golden_dir):
    g, answers, pred, block_n = _golden(golden_dir)
    M = pkg().load_dropin_metrics()
    per = len(pred) // len(block_n)
    by_ids, by_soft, by_index = M.VQAChallengeAccuracy(), M.VQAChallengeAccuracy(), M.VQAChallengeAccuracy()
    for b, N in enumerate(block_n):
        for lo in range(b * per, (b + 1) * per, 200):                      # batches of 200, 200, 112
            hi = min(lo + 200, (b + 1) * per)
            a = torch.from_numpy(answers[lo:hi]).to(DEV)
            x = _logits_with_argmax(pred[lo:hi], N, seed=lo).to(DEV)
            by_ids.update(x, a)
            by_soft.update(x.bfloat16(), _ST().answer_scores(a, N))
            by_index.update(torch.from_numpy(pred[lo:hi]).to(DEV), a)
    for m in (by_ids, by_soft, by_index):
        assert m.count == int(g["count"])
        assert abs(m.compute() - float(g["compute"])) < 1e-9
        assert abs(m.total_score - float(g["total_score"])) < 1e-9 * len(pred)
    by_ids.reset()
    assert by_ids.count == 0 and by_ids.compute() == 0.0
    with pytest.raises(TypeError):
        by_ids.update(x, _ST().SoftTargets(torch.zeros(len(x), 2, device=DEV, dtype=torch.int32), torch.zeros(len(x), 2, device=DEV)))
    # HipTrainer.step: a metric that does not fit the targets raises before anything is launched
    cfg = O.full_config(**SMALL)
    m = _model(cfg, O.init_state_dict(cfg, 1))
    tr = pkg().trainer.HipTrainer(m)
    images, ids, mask, labels = [t.to(DEV) for t in O.synthetic_batch(2, seed=1, **SMALL_BATCH)]
    soft = _ST().answer_scores(_annotators(2, 10, 3).to(DEV), 10)
    seen, L = [], sub("_lib")
    old = L._HOOK[0]
    L._HOOK[0] = lambda name, args: seen.append(name)
    try:
        with pytest.raises(TypeError):
            tr.step(images, ids, mask, soft, metrics=M.VQAAccuracy())
        with pytest.raises(TypeError):
            tr.step(images, ids, mask, labels, metrics=M.VQAChallengeAccuracy())
        with pytest.raises(TypeError):
            tr.step(images, ids, mask, _ST().SoftTargets(soft.ids, soft.weights), metrics=M.VQAChallengeAccuracy())
        with pytest.raises(ValueError):
            tr.step(images, ids, mask, _ST().SoftTargets(soft.ids[:1], soft.weights[:1], soft.counts[:1]))
    finally:
        L._HOOK[0] = old
    assert seen == [] and tr.calls == 0
    tr.step(images, ids, mask, _ST().SoftTargets(soft.ids, soft.weights))    # without counts and without a metric: fine
    torch.cuda.synchronize()
    tr.check()
