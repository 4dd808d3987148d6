"""GPU: inference path -- eval-mode Conv+BN folded into the implicit-GEMM epilogue (bias + ReLU, ReLU after the
residual addend).  Parity pin: the folded path is what `torch.no_grad()` evaluation runs, so tests/test_gpu_model.py's
eval goldens (logits within 1e-3 of the real reference) exercise it; here it is additionally compared with the unfolded
BN-as-a-pass path on the same weights and checked kernel by kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _foldref as R
from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(dtype):
    cfg = O.full_config()
    sd = O.init_state_dict(cfg, 1, jitter=True)          # jitter: non-trivial running_mean / running_var / gamma / beta
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.mark.parametrize("dtype,tol", [("fp32", 2e-4), ("bf16", 6e-2)])
def test_folded_eval_equals_unfolded_eval(dtype, tol):
    m = _model(dtype)
    images, ids, _, _ = O.synthetic_batch(6, seed=21)
    mask = (torch.arange(20)[None, :] < torch.tensor([20, 3, 9, 20, 1, 14])[:, None]).long()
    args = (images.to(DEV), ids.to(DEV), mask.to(DEV))
    with torch.no_grad():
        a, _ = m(*args)
        m._engine.fold_eval = False
        b, _ = m(*args)
        m._engine.fold_eval = True
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert (a - b).abs().max().item() < tol * max(1.0, b.abs().max().item())
    if dtype == "fp32":
        assert (a.argmax(-1) == b.argmax(-1)).all()


def test_folded_eval_leaves_bn_buffers_and_training_path_untouched():
    m = _model("fp32")
    before = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    images, ids, _, _ = O.synthetic_batch(2, seed=5)
    with torch.no_grad():
        m(images.to(DEV), ids.to(DEV), None)
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    # eval with autograd enabled still records a tape (unfolded path) and back-propagates
    lg, _ = m(images.to(DEV), ids.to(DEV), None)
    lg.sum().backward()
    assert dict(m.named_parameters())["answer_head.classifier.6.weight"].grad is not None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fold_kernel_and_relu_after_addend(dtype):
    """vqa_fold_bn_batch + vqa_igemm(relu=2) on one 3x3 conv against F.conv2d -> F.batch_norm(eval) -> + residual -> relu."""
    L, K = sub("_lib"), sub("kernels")
    B, C, H, N = 2, 64, 12, 128
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, C, H, H, generator=g)
    w = torch.randn(N, C, 3, 3, generator=g) * 0.05
    gamma, beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    rm, rv = torch.randn(N, generator=g) * 0.1, torch.rand(N, generator=g) + 0.5
    res = torch.randn(B, N, H, H, generator=g)
    rd = (lambda t: t.to(torch.bfloat16).float()) if dtype == torch.bfloat16 else (lambda t: t)
    ref = F.relu(F.batch_norm(F.conv2d(rd(x), w, None, 1, 1), rm, rv, gamma, beta, False, 0.0, 1e-5) + rd(res))
    flat = torch.cat([w.permute(0, 2, 3, 1).reshape(-1), gamma, beta]).to(DEV)          # [N][R][S][C] weight, then gamma, beta
    rmd, rvd = rm.to(DEV), rv.to(DEV)
    Kw = 9 * C
    desc = torch.tensor([[0, N * Kw, N * Kw + N, rmd.data_ptr(), rvd.data_ptr(), N, Kw, 0, 0, 0]], dtype=torch.int64).to(DEV)
    wout = torch.empty(N * Kw, device=DEV, dtype=dtype)
    bout = torch.empty(N, device=DEV)
    L.call("vqa_fold_bn_batch", int(dtype == torch.bfloat16), flat.data_ptr(), wout.data_ptr(), bout.data_ptr(), desc.data_ptr(), 1,
           (N * Kw + 255) // 256, 1e-5)
    # the fold itself, element by element within the counted bound of test_fold_bn_batch_multi_piece_against_fp64
    wref, bref, prod = R.fold(w.permute(0, 2, 3, 1).reshape(N, Kw), gamma, beta, rm, rv, 1e-5)
    assert R.error_in_bounds(wout.cpu().view(N, Kw), wref, R.fold_weight_tol(wref, dtype == torch.bfloat16)) <= 1.0
    assert R.error_in_bounds(bout.cpu(), bref, R.fold_bias_tol(bref, prod)) <= 1.0
    xa = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(DEV, dtype)
    ra = res.permute(0, 2, 3, 1).reshape(-1, N).contiguous().to(DEV, dtype)
    out, _, _ = K.igemm(xa, wout.view(N, Kw), B * H * H, N, Kw, (B, H, H, C, H, H, 3, 3, 1, 1), dtype=dtype, bias=bout, addend=ra, relu=2)
    torch.cuda.synchronize()
    got = out.float().cpu().view(B, H, H, N).permute(0, 3, 1, 2)
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    assert (got - ref).abs().max().item() < tol * max(1.0, ref.abs().max().item())
    assert (got >= 0).all()


# ------------------------------------------------------------------------------------------------ vqa_fold_bn_batch against fp64
# (N, K) of the pieces of one launch, in table order: a 3x3 64 -> 64 conv, a 1x1 64 -> 128 shortcut, two pieces whose N * K is no
# multiple of 256 (10 x 147: six workgroups with a ragged last one; 300 x 3: N > 256, so two workgroups write the bias), and a
# last piece of a single workgroup.  Gaps (elements) in front of each piece's weights / bias in the output buffers: every dst_off / bias_off is
# non-zero, none is a multiple of 256, and the gaps must keep the sentinel.
FOLD_PIECES = [(64, 576), (128, 64), (10, 147), (300, 3), (5, 9)]
FOLD_WGAP, FOLD_BGAP = [40, 8, 24, 3, 16], [8, 16, 5, 8, 24]
FOLD_EPS = 1e-5
FOLD_SENTINEL = -12352.0                    # a bf16 number far from every folded value
CH_VAR0, CH_NEG, CH_ZERO, CH_BIGMEAN, CH_CANCEL = 0, 1, 2, 3, 4     # the special channels of every piece


def _fold_table():
    """Operands of one vqa_fold_bn_batch launch laid out like engine._fold_bn's table: flat = every piece's weight | gamma | beta
    (with padding in between), one running_mean / running_var tensor PER PIECE, desc rows {w_off, gamma_off, beta_off, rm ptr,
    rv ptr, N, K, dst_off, bias_off, blk0}.  Channels 0..4 of every piece: running_var == 0 (only eps holds the denominator), a
    negative gamma, a zero gamma, |running_mean| = 50 against beta = 1e-3, and beta = running_mean * scale up to fp32 rounding
    (the bias cancels)."""
    g = torch.Generator().manual_seed(11)
    parts, rows, stats, off, woff, boff, blk = [], [], [], 0, 0, 0, 0
    for (N, Kw), wg, bg in zip(FOLD_PIECES, FOLD_WGAP, FOLD_BGAP):
        w = torch.randn(N, Kw, generator=g) * (2.0 / (9 * N)) ** 0.5
        gamma, beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.3
        rm, rv = torch.randn(N, generator=g) * 0.2, torch.rand(N, generator=g) + 0.5
        rv[CH_VAR0] = 0.0
        gamma[CH_NEG] = -0.8
        gamma[CH_ZERO] = 0.0
        rm[CH_BIGMEAN], beta[CH_BIGMEAN] = 50.0, 1e-3
        beta[CH_CANCEL] = (rm[CH_CANCEL].double() * gamma[CH_CANCEL].double() / (rv[CH_CANCEL].double() + FOLD_EPS).sqrt()).float()
        pad = torch.full((3,), float("nan"))                          # never read
        parts += [pad, w.reshape(-1), pad, gamma, pad, beta]
        w_off = off + 3
        g_off = w_off + N * Kw + 3
        b_off = g_off + N + 3
        off = b_off + N
        woff += wg
        boff += bg
        rows.append([w_off, g_off, b_off, None, None, N, Kw, woff, boff, blk])
        stats.append((rm, rv))
        woff += N * Kw
        boff += N
        blk += (N * Kw + 255) // 256
    return torch.cat(parts), rows, stats, woff + 32, boff + 32, blk


def _fold_ref(flat, rows, stats):
    """fp64 fold from the fp32 inputs, per piece: (w * scale, beta - rm * scale, |rm * scale|)."""
    return [R.fold(flat[w_off: w_off + N * Kw].view(N, Kw), flat[g_off: g_off + N], flat[b_off: b_off + N], rm, rv, FOLD_EPS)
            for (w_off, g_off, b_off, _, _, N, Kw, _, _, _), (rm, rv) in zip(rows, stats)]


def _run_fold(dtype, flat, rows, stats, wlen, blen, blocks):
    L = sub("_lib")
    flat_d = flat.to(DEV)
    keep = [(rm.to(DEV), rv.to(DEV)) for rm, rv in stats]
    desc = torch.tensor([r[:3] + [m.data_ptr(), v.data_ptr()] + r[5:] for r, (m, v) in zip(rows, keep)], dtype=torch.int64).to(DEV)
    wout = torch.full((wlen,), FOLD_SENTINEL, device=DEV, dtype=dtype)
    bout = torch.full((blen,), FOLD_SENTINEL, device=DEV)
    L.call("vqa_fold_bn_batch", int(dtype == torch.bfloat16), flat_d.data_ptr(), wout.data_ptr(), bout.data_ptr(), desc.data_ptr(),
           len(rows), blocks, FOLD_EPS)
    torch.cuda.synchronize()
    return wout.cpu(), bout.cpu()


def check_fold(wout, bout, flat, rows, stats, dtype, title):
    """Every element of every piece within the counted bound of the fp64 fold; everything outside the pieces still the sentinel.
    Returns the worst (weight, bias) error in units of its bound."""
    wseen, bseen = torch.zeros(wout.numel(), dtype=torch.bool), torch.zeros(bout.numel(), dtype=torch.bool)
    worst_w = worst_b = 0.0
    for (wref, bref, prod), r in zip(_fold_ref(flat, rows, stats), rows):
        N, Kw, wo, bo = r[5], r[6], r[7], r[8]
        worst_w = max(worst_w, R.error_in_bounds(wout[wo: wo + N * Kw].view(N, Kw), wref, R.fold_weight_tol(wref, dtype == torch.bfloat16)))
        worst_b = max(worst_b, R.error_in_bounds(bout[bo: bo + N], bref, R.fold_bias_tol(bref, prod)))
        wseen[wo: wo + N * Kw] = True
        bseen[bo: bo + N] = True
    print(f"{title}: worst error / bound: weights {worst_w:.3f}, bias {worst_b:.3f}")
    assert worst_w <= 1.0 and worst_b <= 1.0, (title, worst_w, worst_b)
    assert bool((~wseen).any()) and bool((~bseen).any())
    assert bool((wout[~wseen].float() == FOLD_SENTINEL).all()), "a weight was written outside every piece"
    assert bool((bout[~bseen] == FOLD_SENTINEL).all()), "a bias was written outside every piece"
    return worst_w, worst_b


def test_fold_bn_batch_multi_piece_against_fp64():
    """vqa_fold_bn_batch as the model calls it -- ONE launch over several pieces found through the blk0 column, non-zero dst_off /
    bias_off, running statistics in a tensor of their own per piece -- against w * gamma / sqrt(rv + eps) and beta - rm * scale in
    fp64 from the fp32 inputs, element by element.

    Bound (tests/_foldref.py: fold_weight_tol, fold_bias_tol), counted from fold_bn_batch_kernel.  u = 2^-24 is fp32's unit
    roundoff: half an ulp relative to the value, which is how a rounding of an intermediate carries into the result.
      weight  4 fp32 operations per element: rv + eps, sqrtf, gamma / ., w * .  -> 4 u |ref| (the sqrt halves the first one's share:
              3.5 u to first order, the rest covers the second-order terms).  bf16: plus ONE bf16 round-to-nearest half-ulp of the
              reference (2^(floor(log2 |ref|) - 8)), for the store.
      bias    5 operations: the same three for the scale, rm * scale, beta - .  The first four are relative to the PRODUCT rm * scale
              and only the subtraction is relative to the result: 4 u |rm * scale| + u |ref|.  (Five half-ulps of the result
              alone would be a mis-count where beta and rm * scale cancel: channel 4 of every piece.)  The bias is fp32 for both
              dtypes.
    A zero gamma has a zero bound: the folded weights must be exactly 0 and the bias exactly beta.
    Measured on gfx950, worst error / bound (1.0 = the bound): fp32 weights 0.647, bias 0.661; bf16 weights 1.000 to three
    places (the bf16 half-ulp itself: a value next to a tie; 0.99989 for fp32 arithmetic on the CPU), bias 0.661.
    Sentinels: every element of every piece is overwritten (the sentinel is far outside the bound), and every element of the gaps
    between the pieces, in front of the first and behind the last, keeps it.
    bf16 weight bits: the bf16 launch's weights equal RNE_bf16 of the fp32 launch's, bit for bit, and the two biases are identical:
    the store's rounding is pinned apart from the arithmetic."""
    flat, rows, stats, wlen, blen, blocks = _fold_table()
    assert [r[9] for r in rows] == [0, 144, 176, 182, 186] and blocks == 187
    assert any((r[5] * r[6]) % 256 for r in rows[:-1]) and rows[-1][5] * rows[-1][6] <= 256 and all(r[7] % 256 and r[8] for r in rows)
    ref = _fold_ref(flat, rows, stats)
    for wref, bref, prod in ref:                                     # the edges are what they claim to be (CPU side)
        assert bool((wref[CH_ZERO] == 0).all()) and float(wref[CH_NEG].abs().max()) > 0 and float(wref[CH_VAR0].abs().max()) > 0
        assert float(prod[CH_BIGMEAN]) > 1e4 * 1e-3 and float(bref[CH_CANCEL].abs()) < 1e-6 * float(prod[CH_CANCEL])
    w32, b32 = _run_fold(torch.float32, flat, rows, stats, wlen, blen, blocks)
    check_fold(w32, b32, flat, rows, stats, torch.float32, "fold fp32")
    w16, b16 = _run_fold(torch.bfloat16, flat, rows, stats, wlen, blen, blocks)
    check_fold(w16, b16, flat, rows, stats, torch.bfloat16, "fold bf16")
    assert torch.equal(w16.view(torch.int16), w32.to(torch.bfloat16).view(torch.int16))
    assert torch.equal(b16.view(torch.int32), b32.view(torch.int32))


def test_graphed_forward_replays_the_same_logits_for_new_inputs():
    """forward_graphed: the captured HIP graph must give the eager eval logits bit for bit, also for inputs other than the ones it
    was captured with (static buffers are refilled), and must refuse train mode."""
    m = _model("bf16")
    with torch.no_grad():
        for seed in (31, 32, 33):
            images, ids, _, _ = O.synthetic_batch(3, seed=seed)
            mask = (torch.arange(20)[None, :] < torch.tensor([20, 6, 11])[:, None]).long()
            a = m.forward_graphed(images.to(DEV), ids.to(DEV), mask.to(DEV)).clone()
            m.graph_inference = False                               # eager launches, kernel by kernel
            b, _ = m(images.to(DEV), ids.to(DEV), mask.to(DEV))
            m.graph_inference = True                                # the serving route: model(...) under no_grad replays the graph
            c, _ = m(images.to(DEV), ids.to(DEV), mask.to(DEV))
            torch.cuda.synchronize()
            assert torch.equal(a, b) and torch.equal(a, c), seed
    assert len(m._graphs) == 1
    m.train()
    with pytest.raises(RuntimeError):
        m.forward_graphed(images.to(DEV), ids.to(DEV), mask.to(DEV))


def test_graph_cache_is_lru_and_outputs_are_owned_by_the_caller():
    """api/inference.py:228,296 calls model(...) in eval mode under no_grad at small B: that route replays a captured HIP graph.
    The shape cache is LRU (a hit refreshes the entry), evicting a graph synchronises first, and forward() hands out a copy of
    the graph's static output (two results of the same shape must not alias)."""
    m = _model("bf16")
    m.graph_max_shapes = 2
    images, ids, _, _ = O.synthetic_batch(3, seed=41)
    im, idd = images.to(DEV), ids.to(DEV)
    with torch.no_grad():
        o1, _ = m(im[:1], idd[:1], None)
        o2, _ = m(im[1:2], idd[1:2], None)
        assert o1.data_ptr() != o2.data_ptr() and not torch.equal(o1, o2)     # same shape, same graph, two owned results
        k1 = next(iter(m._graphs))
        m(im[:2], idd[:2], None)                                  # second shape
        m(im[:1], idd[:1], None)                                  # hit on the first: it becomes the youngest
        assert list(m._graphs)[-1] == k1
        m(im[:3], idd[:3], None)                                  # third shape evicts the B=2 graph, not the B=1 one
        assert k1 in m._graphs and len(m._graphs) == 2
        o3, _ = m(im[:1], idd[:1], None)
    torch.cuda.synchronize()
    assert torch.equal(o3, o1)


def test_inference_stem_fusion_keeps_the_logits():
    """eval + no_grad forward with the one-launch stem (default) against the same model with it switched off: logits within the
    bf16 path's tolerance, identical top-1; the HIP-graph replay uses the fused stem too (same logits as the eager call)."""
    m = _model("bf16")
    torch.manual_seed(3)
    B = 8
    images = torch.randn(B, 3, 224, 224, device=DEV)
    ids = torch.randint(1, 900, (B, 20), device=DEV)
    mask = torch.ones(B, 20, dtype=torch.long, device=DEV)
    m.eval()
    with torch.no_grad():
        a, _ = m(images, ids, mask)
        eng = m._ensure_engine()
        assert eng.fuse_stem_eval
        eng.fuse_stem_eval = False
        m._graphs.clear() if hasattr(m, "_graphs") else None
        m.graph_inference = False
        b, _ = m(images, ids, mask)
        eng.fuse_stem_eval = True
        c, _ = m(images, ids, mask)                    # eager, fused stem
    torch.cuda.synchronize()
    assert (a - b).abs().max().item() < 6e-2 * max(1.0, float(b.abs().max()))
    assert torch.equal(a.argmax(-1), b.argmax(-1))
    assert torch.equal(a, c)
