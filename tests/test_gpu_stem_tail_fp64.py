"""GPU: the stem tail -- vqa_stem_pool_fwd (BatchNorm + ReLU + MaxPool 3x3/2), vqa_stem_bwd_apply, the routing forms of
csrc/stem_route.h that are compiled into a kernel (stem_route in vqa_stem_bwd_apply, stem_route_pair_buf in the fused stem
gradients; stem_route_buf is defined in the header but instantiated nowhere, so no entry point reaches it and nothing here covers
it), and the BatchNorm-backward sums taken from the pooled output -- against the float64 references of tests/_stemref.py
(validated without a GPU in test_stem_tail_ref_cpu.py), never against a sibling kernel.
(stem_route's `!((k >> 1) && oh_b == oh_a)` term can never fire: (h - 1) >> 1 and (h + 1) >> 1 differ for every h, and the
candidate that does not hold the pixel is rejected by the range check on r and s.  Dropping the term changes no result.)

1. pooling forward on operands whose results are exact: values bit-equal, argmax codes equal (11 % of the windows tie), one NaN.
2. pooling forward on random operands: |out - ref| <= 2^-23 (|y*scale| + |shift|) (largest of the window) [+ 2^-8 |ref| in bf16];
   a code may differ from torch's only where the two taps cannot be told apart within their bounds; at most 1 % of the windows.
3. vqa_stem_bwd_apply: bit-equal on exact operands with the pooling kernel's codes; on random operands and random codes 0..8
   (padding taps included) |dy - ref| <= 8 * 2^-24 (|bc0| sum|routed dpool| + |bc1 y| + |bc2|) [+ 2^-8 |ref|].
4. vqa_stem_wgrad_fused / vqa_stem_dgrad_fused (stem_route_pair_buf) against torch's fp64 conv gradients of the fp64 dy rounded
   to bf16 (the kernels stage dy in bf16).  Bound per case: 8x the max-norm error of torch's CPU fp32 result on the same operands,
   floor 1e-6 max|ref| (the convention of test_gpu_layernorm_fp64.py); the figures stand in the two tests' docstrings.
5. pool -> vqa_bn_bwd_reduce(y := pooled, coef := engine.stem_fcoef) -> vqa_bn_bwd_finalize -> vqa_stem_bwd_apply against fp64
   autograd of batch_norm -> relu -> max_pool2d on the same stored y; see test_bn_backward_sums_from_the_pooled_output."""
import pytest
import torch
import torch.nn.functional as Fn

import _stemref as R
from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5


def _coef4(scale, shift):
    C = scale.numel()
    return torch.cat([scale.float(), shift.float(), torch.zeros(2 * C)]).to(DEV)


def _pool(dtype, y, scale, shift):
    """vqa_stem_pool_fwd on an NCHW host tensor: (out NCHW on the host in `dtype`, codes NCHW uint8, device y, coef, out, idx)."""
    L = sub("_lib")
    B, C, H, W = y.shape
    Ho, Wo = R.pooled_hw(H, W)
    yd = R.nhwc(y).to(DEV, dtype)
    coef = _coef4(scale, shift)
    out = torch.full((B * Ho * Wo, C), 7.0, device=DEV, dtype=dtype)       # every element must be written
    idx = torch.full((B * Ho * Wo, C), 99, device=DEV, dtype=torch.uint8)
    L.call("vqa_stem_pool_fwd", L.dt(dtype), yd.data_ptr(), coef.data_ptr(), out.data_ptr(), idx.data_ptr(), B, H, W, C)
    torch.cuda.synchronize()
    return R.nchw(out.cpu(), B, Ho, Wo), R.nchw(idx.cpu(), B, Ho, Wo), yd, coef, out, idx


def _apply(dtype, dpool_d, idx_d, y_d, coef, bc, B, H, W, C):
    L = sub("_lib")
    dy = torch.full((B * H * W, C), 7.0, device=DEV, dtype=dtype)
    bcd = bc.float().contiguous().to(DEV)
    L.call("vqa_stem_bwd_apply", L.dt(dtype), dpool_d.data_ptr(), idx_d.data_ptr(), y_d.data_ptr(), coef.data_ptr(), bcd.data_ptr(),
           dy.data_ptr(), B, H, W, C)
    torch.cuda.synchronize()
    return R.nchw(dy.cpu(), B, H, W)


def _round(t, dtype):
    """fp64 -> the storage dtype, one rounding (the values are exact in fp32 where this is used for equality)"""
    return t.float().to(dtype)


# ------------------------------------------------------------------------------------------------------------- 1. forward, exact
@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.case_id)
def test_pool_forward_exact_operands_bit_equal(case):
    (B, H, W), d, C = case
    dtype = R.DT[d]
    op = R.exact_operands(B, H, W, C, R.seed_of(B, H, W, C, salt=2))
    ref, codes, _ = R.pool_ref(op["y"], op["scale"], op["shift"])
    out, idx, *_ = _pool(dtype, op["y"], op["scale"], op["shift"])
    print(f"pool exact {R.case_id(case)}: tie share {op['tie_share']:.3f}, codes differing {int((idx.long() != codes).sum())}, "
          f"values differing {int((out != _round(ref, dtype)).sum())}")
    assert torch.equal(out, _round(ref, dtype))
    assert torch.equal(idx.long(), codes)


@pytest.mark.parametrize("d", ["fp32", "bf16"])
def test_pool_forward_propagates_a_single_nan(d):
    """Every window over the NaN returns NaN and the code of the NaN's position (ATen: `val > max || isnan(val)`)."""
    B, H, W, C = 2, 8, 8, 64
    dtype = R.DT[d]
    op = R.exact_operands(B, H, W, C, R.seed_of(B, H, W, C, salt=3))
    y = op["y"].clone()
    b0, c0, h0, w0 = 1, 37, 3, 5                                         # odd row and column: four windows hold it
    y[b0, c0, h0, w0] = float("nan")
    ref, codes, _ = R.pool_ref(y, op["scale"], op["shift"])
    out, idx, *_ = _pool(dtype, y, op["scale"], op["shift"])
    want = torch.zeros_like(ref, dtype=torch.bool)
    for oh in ((h0 - 1) // 2, (h0 + 1) // 2):
        for ow in ((w0 - 1) // 2, (w0 + 1) // 2):
            want[b0, c0, oh, ow] = True
            assert int(idx[b0, c0, oh, ow]) == (h0 - (2 * oh - 1)) * 3 + (w0 - (2 * ow - 1))
    assert int(want.sum()) == 4 and torch.equal(ref.isnan(), want)        # the reference agrees with the hand count
    assert torch.equal(out.isnan(), want)
    assert torch.equal(out[~want], _round(ref, dtype)[~want])
    assert torch.equal(idx.long(), codes)


# ------------------------------------------------------------------------------------------------------------ 2. forward, random
@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.case_id)
def test_pool_forward_random_operands_within_fp32_rounding(case):
    (B, H, W), d, C = case
    dtype = R.DT[d]
    y, scale, shift = R.random_pool_operands(B, H, W, C, dtype, R.seed_of(B, H, W, C))
    ref, codes, v = R.pool_ref(y, scale, shift)
    e = R.fwd_bound(y, scale, shift)
    E = R.window_max(e)                                                   # |max fl(v_i) - max v_i| <= max_i |fl(v_i) - v_i|
    out, idx, *_ = _pool(dtype, y, scale, shift)
    bound = E + (2.0 ** -8 * ref.abs() if dtype == BF16 else 0)
    err = (out.double() - ref).abs()
    differ = idx.long() != codes
    print(f"pool random {R.case_id(case)}: worst err / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}, "
          f"codes differing {int(differ.sum())} of {differ.numel()}")
    assert bool((err <= bound).all())
    assert int(idx.max()) <= 8
    # a differing code: the kernel's tap lies inside the map and its value and the window maximum cannot be told apart -- each of
    # the two carries its own bound
    flat, inside = R.tap_index(idx, H, W)
    assert bool(inside.all())
    at = lambda t: t.reshape(B, C, -1).gather(2, flat.reshape(B, C, -1)).view_as(ref)
    flat_ref, _ = R.tap_index(codes, H, W)
    e_ref = e.reshape(B, C, -1).gather(2, flat_ref.reshape(B, C, -1)).view_as(ref)
    assert bool(((ref - at(v)) <= at(e) + e_ref)[differ].all())
    assert float(differ.double().mean()) <= 0.01


# ----------------------------------------------------------------------------------------------------------- 3. backward apply
@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.case_id)
def test_bwd_apply_exact_operands_bit_equal_on_the_pooling_kernels_codes(case):
    (B, H, W), d, C = case
    dtype = R.DT[d]
    Ho, Wo = R.pooled_hw(H, W)
    op = R.exact_operands(B, H, W, C, R.seed_of(B, H, W, C, salt=4))
    y, dpool, bc = op["y"], op["dpool"], op["bc"]
    _, idx, yd, coef, _, idx_d = _pool(dtype, y, op["scale"], op["shift"])
    dpd = R.nhwc(dpool).to(DEV, dtype)
    dy = _apply(dtype, dpd, idx_d, yd, coef, bc, B, H, W, C)
    _, pre = R.bn_relu(y, op["scale"], op["shift"])
    g = R.route_ref(dpool, idx, pre > 0, H, W)
    ref = R.dy_ref(bc, g, y)
    assert torch.equal(ref.float().double(), ref)                         # exact in fp32: one rounding to bf16
    print(f"apply exact {R.case_id(case)}: elements differing {int((dy != _round(ref, dtype)).sum())}")
    assert torch.equal(dy, _round(ref, dtype))
    # every pixel with v <= 0 has g = 0: dy == bc1*y + bc2 there -- also where a window's code names it (channel 0: v == 0 everywhere)
    dead = pre <= 0
    assert torch.equal(dy[dead], _round(R.dy_ref(bc, torch.zeros_like(g), y), dtype)[dead])
    named = R.scatter_windows(dpool.abs() * (R._chan(bc[0]) != 0), idx, H, W) > 0
    assert bool((named & (pre == 0)).any())


@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.case_id)
def test_bwd_apply_random_operands_and_codes_match_the_explicit_scatter(case):
    (B, H, W), d, C = case
    dtype = R.DT[d]
    y, dpool, codes, scale, shift, bc = R.random_bwd_operands(B, H, W, C, dtype, R.seed_of(B, H, W, C, salt=R.BWD_SALT[(B, H, W)]))
    _, pre = R.bn_relu(y, scale, shift)
    assert bool((pre.abs() > R.fwd_bound(y, scale, shift)).all())         # (no ReLU sign hangs on an fp32 rounding; CPU test)
    pos = pre > 0
    g = R.route_ref(dpool, codes, pos, H, W)
    ref = R.dy_ref(bc, g, y)
    bound = R.apply_bound(bc, R.route_ref(dpool.abs(), codes, pos, H, W), y) + (2.0 ** -8 * ref.abs() if dtype == BF16 else 0)
    dy = _apply(dtype, R.nhwc(dpool).to(DEV), R.nhwc(codes).to(DEV), R.nhwc(y).to(DEV), _coef4(scale, shift), bc, B, H, W, C)
    err = (dy.double() - ref).abs()
    print(f"apply random {R.case_id(case)}: worst err / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    # v <= 0: nothing is routed, the kernel's dy is bc1*y + bc2 within that expression's own rounding (+ the bf16 store)
    plain = R.dy_ref(bc, torch.zeros_like(g), y)
    lim = R.apply_bound(bc, torch.zeros_like(g), y) + (2.0 ** -8 * plain.abs() if dtype == BF16 else 0)
    assert bool(((dy.double() - plain).abs() <= lim)[~pos].all()) and bool((~pos).any())
    n = R.route_counts(codes, H, W) * pos
    if H >= 3 and W >= 3:
        assert bool((n == 2).any()) and bool((n == 4).any())
    _, inside = R.tap_index(codes, H, W)
    assert H * W == 1 or not bool(inside.all())                           # some code points into the padding


# ------------------------------------------------------------------------------------------------------------- 4. fused gradients
def _fused_operands(B, IH, IW, seed):
    """Exact stem-tail operands at the conv output size of a B x 3 x IH x IW image with the pooling kernel's codes: the device
    operands (y, dpool, idx, coef, bc) of the fused kernels, the fp64 dy rounded to bf16, and the generator for what else a case draws."""
    H, W = (IH - 1) // 2 + 1, (IW - 1) // 2 + 1
    op = R.exact_operands(B, H, W, 64, seed)
    _, idx, yd, coef, _, idx_d = _pool(BF16, op["y"], op["scale"], op["shift"])
    _, pre = R.bn_relu(op["y"], op["scale"], op["shift"])
    dy64 = R.dy_ref(op["bc"], R.route_ref(op["dpool"], idx, pre > 0, H, W), op["y"])
    dyb = dy64.float().bfloat16().double()                                # the kernels stage dy in bf16: the reference operand is rounded too
    g = torch.Generator().manual_seed(seed + 1)
    return (yd, R.nhwc(op["dpool"]).to(DEV, BF16), idx_d, coef, op["bc"].float().contiguous().to(DEV)), dyb, g


def _bound8(cpu32, ref):
    cpu = float((cpu32.double() - ref).abs().max())
    return cpu, max(8 * cpu, 1e-6 * float(ref.abs().max()))


@pytest.mark.parametrize("B,IH,IW", [(2, 32, 32), (1, 8, 64), (2, 24, 96)])
def test_fused_stem_wgrad_matches_fp64(B, IH, IW):
    """vqa_stem_wgrad_fused against torch.nn.grad.conv2d_weight in fp64 of the bf16-rounded image and the bf16-rounded fp64 dy.
    Images 2x32x32 / 1x8x64 / 2x24x96: CPU fp32 error (max-norm) 1.09e-5 / 4.77e-6 / 2.28e-5 -> bound 1.04e-4 (the floor) /
    6.11e-5 (the floor) / 1.83e-4 at max|ref| 104 / 61 / 151; measured on MI355X: 9.06e-6 / 4.77e-6 / 1.28e-5."""
    K, L = sub("kernels"), sub("_lib")
    (yd, dpd, idx_d, coef, bcd), dyb, g = _fused_operands(B, IH, IW, seed=IH + IW)
    img = torch.randn(B, 3, IH, IW, generator=g)
    imgb = img.bfloat16()
    ref = torch.nn.grad.conv2d_weight(imgb.double(), (64, 3, 7, 7), dyb, stride=2, padding=3).permute(0, 2, 3, 1).reshape(64, 147)
    cpu32 = torch.nn.grad.conv2d_weight(imgb.float(), (64, 3, 7, 7), dyb.float(), stride=2, padding=3).permute(0, 2, 3, 1).reshape(64, 147)
    cpu, bound = _bound8(cpu32, ref)
    imgd = img.to(DEV)
    dw = torch.zeros(64, 147, device=DEV)
    ws, wsf = K.stem_wgrad_scratch(DEV, B, IH, IW)
    L.call("vqa_stem_wgrad_fused", imgd.data_ptr(), yd.data_ptr(), dpd.data_ptr(), idx_d.data_ptr(), coef.data_ptr(), bcd.data_ptr(),
           dw.data_ptr(), B, IH, IW, ws.data_ptr(), wsf)
    torch.cuda.synchronize()
    err = float((dw.cpu().double() - ref).abs().max())
    print(f"fused wgrad {B}x{IH}x{IW}: cpu fp32 {cpu:.2e} bound {bound:.2e} max|ref| {float(ref.abs().max()):.2e} kernel {err:.2e}")
    assert err <= bound


@pytest.mark.parametrize("B,IH,IW", [(2, 32, 32), (1, 8, 64), (2, 24, 96), (2, 30, 36)])
def test_fused_stem_dgrad_matches_fp64(B, IH, IW):
    """vqa_stem_dgrad_fused against torch.nn.grad.conv2d_input in fp64 of the bf16-rounded fp64 dy and the bf16 weights the kernel
    contracts with.  2 x 30 x 36: Ho = 15 (odd), Wo = 18.  Images 2x32x32 / 1x8x64 / 2x24x96 / 2x30x36: CPU fp32 error (max-norm,
    it moves with the CPU's thread count) 8.1e-7 / 1.04e-6 / 1.31e-6 / 1.51e-6 -> bound 8.84e-6 (the floor) / 8.33e-6 / 1.27e-5
    (the floor) / 1.21e-5 at max|ref| 8.8 / 7.7 / 12.7 / 9.9; measured on MI355X: 1.33e-6 / 1.01e-6 / 1.49e-6 / 1.14e-6."""
    K = sub("kernels")
    (yd, dpd, idx_d, coef, bcd), dyb, g = _fused_operands(B, IH, IW, seed=IH + IW + 1)
    assert K.stem_dgrad_fused_ok(B, IH, IW)
    w = torch.randn(64, 7, 7, 3, generator=g) * 0.1                       # KRSC master
    wk = w.bfloat16().permute(0, 3, 1, 2)                                 # OIHW, the kernel's operand values
    ref = torch.nn.grad.conv2d_input((B, 3, IH, IW), wk.double(), dyb, stride=2, padding=3)
    cpu32 = torch.nn.grad.conv2d_input((B, 3, IH, IW), wk.float(), dyb.float(), stride=2, padding=3)
    cpu, bound = _bound8(cpu32, ref)
    wpk = K.stem_dgrad_pack(w.to(DEV), BF16)
    got = K.stem_dgrad_fused(yd, dpd, idx_d, coef, bcd, wpk, B, IH, IW)
    torch.cuda.synchronize()
    err = float((got.cpu().double() - ref).abs().max())
    print(f"fused dgrad {B}x{IH}x{IW}: cpu fp32 {cpu:.2e} bound {bound:.2e} max|ref| {float(ref.abs().max()):.2e} kernel {err:.2e}")
    assert err <= bound


# ------------------------------------------------------------------------------------- 5. BatchNorm-backward sums from the pooled output
def _units(err, unit, live):
    return float((err[live] / unit[live]).max())


def _bn_reference(y, dpool, gamma, beta, rm, rv, training, bf16):
    """fp64 side of the chain test: autograd results, the coefficient form, and the scales the bounds are stated in (per channel).
    U_b = sum |dpool| [pooled > 0] and U_g = sum |dpool| [pooled > 0] (|pooled| + |beta|) / |gamma| are the sums of the magnitudes
    of what the two reductions add; Hb = sum |dpool| [pooled > 0] 2^-9 |pooled| / |gamma| is the issue's bound for the bf16
    rounding of the stored pooled value (0 in fp32); u_bc scales the three apply coefficients.  The gamma == 0 channel is not
    `live`: its 1/gamma is taken as 0 here as in stem_fcoef, so its scales are 0."""
    B, C, H, W = y.shape
    rows = B * H * W
    r = {}
    r["dy"], r["dgamma"], r["dbeta"] = R.stem_bn_backward_ref(y, gamma, beta, dpool, training, EPS, rm, rv)
    scale, shift, mean, invstd = R.bn_coef_ref(y, gamma, beta, training, EPS, rm, rv)
    pooled, r["codes"], _ = R.pool_ref(y, scale, shift)
    _, pre = R.bn_relu(y, scale, shift)
    r["pos"] = pre > 0
    r["g"] = R.route_ref(dpool, r["codes"], r["pos"], H, W)
    r["bc"] = R.bc_ref(r["dbeta"], r["dgamma"], rows, gamma, mean, invstd, training)
    live = torch.ones(C, dtype=torch.bool)
    live[R.CH_ZERO_GAMMA] = False
    rg = torch.where(live, 1.0 / gamma.double(), torch.zeros(C, dtype=torch.float64))
    ad = dpool.double().abs() * (pooled > 0)
    r["live"], r["rg"] = live, rg
    r["U_b"] = ad.sum((0, 2, 3))
    r["U_g"] = (ad * (pooled.abs() + R._chan(beta).abs())).sum((0, 2, 3)) * rg.abs()
    r["Hb"] = (ad * 2.0 ** -9 * pooled.abs()).sum((0, 2, 3)) * rg.abs() if bf16 else torch.zeros(C, dtype=torch.float64)
    gi = (gamma.double() * invstd).abs()
    r["u_bc"] = torch.stack([gi, gi * invstd * r["U_g"] / rows, gi * ((mean * invstd).abs() * r["U_g"] + r["U_b"]) / rows])
    # what the pooled rounding adds to bc1 and bc2 through the mean of g*xhat (training mode)
    zero = torch.zeros(C, dtype=torch.float64)
    r["h_bc"] = torch.stack([zero, gi * invstd * r["Hb"] / rows, gi * (mean * invstd).abs() * r["Hb"] / rows]) if training else torch.stack([zero] * 3)
    return r


def _cpu_fp32_units(y, dpool, gamma, beta, rm, rv, training, ref):
    """The project's formulas in torch fp32 on the CPU -- statistics, BatchNorm + ReLU + MaxPool, sum dpool [pooled > 0],
    sum dpool [pooled > 0] (pooled - beta) (1/gamma), the apply coefficients of bn_bwd_finalize_kernel -- and their error against
    fp64 in the units of _bn_reference, worst live channel, floored at 2^-24 (half an ulp): (d beta, d gamma, [bc0, bc1, bc2])."""
    B, C, H, W = y.shape
    rows = B * H * W
    ch = lambda t: t.view(1, C, 1, 1)
    y32 = y.float()
    if training:
        mean, var = y32.mean((0, 2, 3)), y32.var((0, 2, 3), unbiased=False)
    else:
        mean, var = rm, rv
    inv = (var + EPS).rsqrt()
    gi = gamma * inv
    pooled = Fn.max_pool2d(torch.relu(y32 * ch(gi) + ch(beta - mean * gi)), 3, 2, 1)
    g = dpool.float() * (pooled > 0)
    sg, sx = g.sum((0, 2, 3)), (g * (pooled - ch(beta)) * ch(ref["rg"].float())).sum((0, 2, 3))
    if training:
        mg, mgx = sg / rows, sx / rows
        bc = torch.stack([gi, -gi * inv * mgx, gi * (mean * inv * mgx - mg)])
    else:
        bc = torch.stack([gi, torch.zeros(C), torch.zeros(C)])
    floor, live = 2.0 ** -24, ref["live"]
    worst = lambda got, want, unit: max(_units((got.double() - want).abs(), unit, live & (unit > 0)), floor)
    cpu_bc = [worst(bc[k], ref["bc"][k], ref["u_bc"][k]) if (training or k == 0) else 0.0 for k in range(3)]
    return worst(sg, ref["dbeta"], ref["U_b"]), worst(sx, ref["dgamma"], ref["U_g"]), cpu_bc


def _gpu_chain(y, dpool, gamma, beta, rm, rv, training, dtype):
    """pool -> reduce(y := pooled, coef := stem_fcoef) -> finalize -> apply on the device; host results (dy NCHW, codes NCHW,
    d gamma, d beta, bc, fcoef)."""
    K, L, E = sub("kernels"), sub("_lib"), sub("engine")
    B, C, H, W = y.shape
    Ho, Wo = R.pooled_hw(H, W)
    rows, rows_p = B * H * W, B * Ho * Wo
    yd, dpd = R.nhwc(y).to(DEV), R.nhwc(dpool).to(DEV)
    gam_d, bet_d = gamma.to(DEV), beta.to(DEV)
    if training:                                   # statistics slab [tiles][2][C]: per-tile sum and sum of squares, built by torch
        T = 5
        parts = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in R.nhwc(y).double().chunk(T)]).float().contiguous().to(DEV)
        assert parts.shape == (T, 2, C)
        coef = K.bn_train_coef(parts, T, C, rows, gam_d, bet_d, rm.clone().to(DEV), rv.clone().to(DEV),
                               torch.zeros((), device=DEV, dtype=torch.int64), eps=EPS)
    else:
        coef = K.bn_eval_coef(C, gam_d, bet_d, rm.to(DEV), rv.to(DEV), eps=EPS)
    pooled = torch.empty((rows_p, C), device=DEV, dtype=dtype)
    idx = torch.empty((rows_p, C), device=DEV, dtype=torch.uint8)
    L.call("vqa_stem_pool_fwd", L.dt(dtype), yd.data_ptr(), coef.data_ptr(), pooled.data_ptr(), idx.data_ptr(), B, H, W, C)
    fcoef = E.stem_fcoef(gam_d, bet_d)
    nb = L.count("vqa_bn_bwd_blocks", rows_p)
    slab = torch.empty((nb, 3, C), device=DEV, dtype=torch.float32)
    L.call("vqa_bn_bwd_reduce", L.dt(dtype), dpd.data_ptr(), pooled.data_ptr(), pooled.data_ptr(), fcoef.data_ptr(), None, None,
           slab.data_ptr(), rows_p, C, 0, 0)
    bc = torch.empty((3, C), device=DEV, dtype=torch.float32)
    dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    L.call("vqa_bn_bwd_finalize", slab.data_ptr(), nb, C, 1, float(rows), gam_d.data_ptr(), coef.data_ptr(), int(training),
           dgam.data_ptr(), dbet.data_ptr(), bc.data_ptr())
    dy = torch.empty((rows, C), device=DEV, dtype=dtype)
    L.call("vqa_stem_bwd_apply", L.dt(dtype), dpd.data_ptr(), idx.data_ptr(), yd.data_ptr(), coef.data_ptr(), bc.data_ptr(), dy.data_ptr(),
           B, H, W, C)
    torch.cuda.synchronize()
    return (R.nchw(dy.cpu(), B, H, W), R.nchw(idx.cpu(), B, Ho, Wo).long(), dgam.cpu().double(), dbet.cpu().double(), bc.cpu().double(),
            fcoef.cpu())


@pytest.mark.parametrize("training", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("d", ["fp32", "bf16"])
@pytest.mark.parametrize("B,H,W", R.BN_SHAPES)
def test_bn_backward_sums_from_the_pooled_output(B, H, W, d, training):
    """vqa_stem_pool_fwd -> vqa_bn_bwd_reduce(dout = dpool, outact = y = pooled, coef = stem_fcoef) -> vqa_bn_bwd_finalize ->
    vqa_stem_bwd_apply, coefficients from vqa_bn_stats_finalize (a statistics slab built from y by torch) or vqa_bn_eval_coef,
    against fp64 autograd of F.batch_norm -> relu -> max_pool2d on the same stored y.

    Bounds.  The sums: 8x the error of the SAME formulas in torch fp32 on the CPU (_cpu_fp32_units), in units of the sum of the
    magnitudes of what is added (the cancellation of pooled - beta is part of the formula), worst channel, floored at 2^-24.
    d gamma in bf16 adds the issue's bound for the rounding of the stored pooled value, sum |dpool| [pooled > 0] 2^-9 |pooled| /
    |gamma| per channel.  (Per term that rounding can reach 2^-8 |pooled| -- half a bf16 ulp at the bottom of a binade; the sum
    over signed gradients stays far inside the 2^-9 figure, see below.)  dy: the bound of the apply test with the reference's
    coefficients, plus |g|, |y| and 1 times what bc0, bc1, bc2 may be off by the same convention (in bf16 the pooled rounding
    enters bc1 and bc2 through the mean of g*xhat), plus 2^-8 |ref| in bf16.

    Measured on MI355X.  CPU fp32 error in those units: d beta and d gamma 6.0e-8 (the floor) in all eight cases, bc0 1.0e-7 ...
    1.5e-7 -> bounds 4.8e-7 resp. 8e-7 ... 1.2e-6 of the unit.  Kernel: d beta 1.6e-8 ... 2.0e-8 (fp32), 2.5e-9 ... 9.0e-9 (bf16);
    d gamma 1.4e-8 ... 3.2e-8 (fp32); in bf16 the worst channel's d gamma error is 0.14 ... 0.18 of its bound; dy worst
    error / bound 0.13 ... 0.16 (fp32), 0.90 ... 0.99 (bf16: the final rounding, which the 2^-8 |ref| term describes tightly).
    The beta/gamma = 30 channel (gamma = 0.1, beta = 3), error of d gamma relative to |d gamma|:
        3x15x29   fp32 train 6.4e-7   fp32 eval 5.5e-7   bf16 train 6.6e-5   bf16 eval 2.2e-2   (d gamma 32.9 / 30.9)
        2x16x32   fp32 train 9.1e-8   fp32 eval 1.8e-7   bf16 train 1.0e-1   bf16 eval 2.8e-2   (d gamma 5.4 / 7.9)
    i.e. in bf16 between nothing and 10 % of this channel's d gamma (absolute 2.2e-3 / 0.68 / 0.55 / 0.22 against hard bounds of
    17.7 / 17.6 / 12.8 / 13.1): rounding noise of (pooled - beta) / gamma, 360 resp. 256 windows, as large as the estimate of
    several per cent; in fp32 the cancellation costs nothing visible.

    The channel with gamma == 0: stem_fcoef maps 1/gamma to 0, so its d gamma is 0 by construction (autograd's is not: the
    documented deviation); its d beta is right, its dy is 0, and everything is finite."""
    dtype = R.DT[d]
    y, dpool, gamma, beta, rm, rv = R.bn_case_operands(B, H, W, dtype, R.seed_of(B, H, W, 64, salt=5))
    ref = _bn_reference(y, dpool, gamma, beta, rm, rv, training, dtype == BF16)
    cpu_b, cpu_g, cpu_bc = _cpu_fp32_units(y, dpool, gamma, beta, rm, rv, training, ref)
    dy, codes, dgam, dbet, bc, fcoef = _gpu_chain(y, dpool, gamma, beta, rm, rv, training, dtype)
    live, U_b, U_g, Hb = ref["live"], ref["U_b"], ref["U_g"], ref["Hb"]
    assert torch.equal(codes, ref["codes"])                               # (inputs decided far from rounding: CPU test)
    for t in (dy, dgam, dbet, bc, fcoef):
        assert bool(torch.isfinite(t.double()).all())
    # ---- the sums
    e_b, e_g = (dbet - ref["dbeta"]).abs(), (dgam - ref["dgamma"]).abs()
    tol_b, tol_g = 8 * cpu_b * U_b, 8 * cpu_g * U_g + Hb
    cn = R.CH_CANCEL
    tag = f"bn sums {B}x{H}x{W} {d} {'train' if training else 'eval'}"
    print(f"{tag}: cpu fp32 units dbeta {cpu_b:.2e} dgamma {cpu_g:.2e} bc {[f'{c:.2e}' for c in cpu_bc]}; kernel units "
          f"dbeta {_units(e_b, U_b, live & (U_b > 0)):.2e} dgamma (fp32 term only) {_units((e_g - Hb).clamp(min=0), U_g, live & (U_g > 0)):.2e}; "
          f"worst dgamma err / bound {float((e_g[live] / tol_g[live].clamp(min=1e-300)).max()):.3f}")
    print(f"{tag}: beta/gamma = 30 channel: dgamma {float(ref['dgamma'][cn]):.4f}, error {float(e_g[cn]):.3e} = "
          f"{float(e_g[cn] / ref['dgamma'][cn].abs()):.3e} of |dgamma|; bound {float(tol_g[cn]):.3e}")
    assert bool((e_b <= tol_b).all())                                      # every channel, gamma == 0 included
    assert bool((e_g[live] <= tol_g[live]).all())
    assert float(dgam[R.CH_ZERO_GAMMA]) == 0.0 and float(ref["dgamma"][R.CH_ZERO_GAMMA].abs()) > 0      # the documented deviation
    assert float(dgam[R.CH_DEAD]) == 0.0 and float(dbet[R.CH_DEAD]) == 0.0
    # ---- dy
    d_bc = torch.stack([8 * cpu_bc[k] * ref["u_bc"][k] for k in range(3)]) + ref["h_bc"]
    bound = (R.apply_bound(ref["bc"], R.route_ref(dpool.abs(), ref["codes"], ref["pos"], H, W), y)
             + R._chan(d_bc[0]) * ref["g"].abs() + R._chan(d_bc[1]) * y.double().abs() + R._chan(d_bc[2])
             + (2.0 ** -8 * ref["dy"].abs() if dtype == BF16 else 0))
    err = (dy.double() - ref["dy"]).abs()
    print(f"{tag}: dy worst err / bound {float((err[:, live] / bound[:, live].clamp(min=1e-300)).max()):.3f}")
    assert bool((err[:, live] <= bound[:, live]).all())
    assert bool((dy[:, R.CH_ZERO_GAMMA] == 0).all()) and bool((ref["dy"][:, R.CH_ZERO_GAMMA] == 0).all())
    assert bool((dy[:, R.CH_DEAD] == 0).all())
