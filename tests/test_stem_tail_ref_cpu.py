"""The fp64 references of tests/_stemref.py, validated without a GPU: the explicit scatter against autograd, the padding rule, the
BatchNorm-backward coefficient form against autograd, and -- on the reference alone -- everything the GPU tests of
test_gpu_stem_tail_fp64.py presuppose about their seeded inputs (near-tie share, no value at the ReLU threshold, coverage)."""
import pytest
import torch
import torch.nn.functional as F

import _stemref as R


def _autograd_route(pre, dpool):
    """d/d pre of max_pool2d(relu(pre), 3, 2, 1) . dpool"""
    p = pre.clone().requires_grad_(True)
    F.max_pool2d(torch.relu(p), 3, 2, 1).backward(dpool)
    return p.grad


@pytest.mark.parametrize("tied", [True, False], ids=["tied", "untied"])
@pytest.mark.parametrize("H,W", [(7, 9), (15, 29), (1, 1)])
def test_route_ref_equals_autograd_of_maxpool_relu(H, W, tied):
    B, C = 2, 8
    if tied:
        op = R.exact_operands(B, H, W, C, seed=H + W)
        y, scale, shift, dpool = op["y"], op["scale"], op["shift"], op["dpool"]
        assert H * W == 1 or op["tie_share"] >= 0.05
    else:
        y, scale, shift = R.random_pool_operands(B, H, W, C, torch.float32, seed=H + W)
        dpool = torch.randn(B, C, *R.pooled_hw(H, W), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    pooled, codes, v = R.pool_ref(y, scale, shift)
    _, pre = R.bn_relu(y, scale, shift)
    if not tied:
        assert bool((pooled.reshape(B, C, -1)[R.window_ties(v) > 1] == 0).all())   # the only ties: windows the ReLU zeroed
    got = R.route_ref(dpool, codes, pre > 0, H, W)
    assert torch.equal(got, _autograd_route(pre, dpool.double()))
    # the pooled value is the value at the tap the code names
    flat, inside = R.tap_index(codes, H, W)
    assert bool(inside.all())
    assert torch.equal(v.reshape(B, C, -1).gather(2, flat.reshape(B, C, -1)).view_as(pooled), pooled)


def test_codes_into_the_padding_contribute_nothing():
    # a single pixel: only the centre tap (code 4) lies inside
    for code in range(9):
        g = R.route_ref(torch.ones(1, 1, 1, 1), torch.full((1, 1, 1, 1), code), torch.ones(1, 1, 1, 1, dtype=torch.bool), 1, 1)
        assert float(g.sum()) == (1.0 if code == 4 else 0.0)
    # 4 x 5 map, windows 2 x 3: the top row's taps r = 0 and the left column's taps s = 0 are padding
    H, W = 4, 5
    dpool = torch.arange(1.0, 7.0, dtype=torch.float64).view(1, 1, 2, 3)
    for code in range(9):
        g = R.route_ref(dpool, torch.full((1, 1, 2, 3), code), torch.ones(1, 1, H, W, dtype=torch.bool), H, W)
        r, s = divmod(code, 3)
        want = sum(float(dpool[0, 0, oh, ow]) for oh in range(2) for ow in range(3)
                   if 0 <= 2 * oh - 1 + r < H and 0 <= 2 * ow - 1 + s < W)
        assert float(g.sum()) == want
        for oh in range(2):
            for ow in range(3):
                ih, iw = 2 * oh - 1 + r, 2 * ow - 1 + s
                if 0 <= ih < H and 0 <= iw < W:
                    assert float(g[0, 0, ih, iw]) == float(dpool[0, 0, oh, ow])
    # the ReLU mask drops what was routed
    g = R.route_ref(dpool, torch.full((1, 1, 2, 3), 4), torch.zeros(1, 1, H, W, dtype=torch.bool), H, W)
    assert float(g.abs().sum()) == 0.0


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,H,W", R.BN_SHAPES)
def test_bn_backward_ref_equals_the_coefficient_form(B, H, W, training):
    """autograd dy == bc0*g + bc1*y + bc2 with bc from the reference's own sums; dgamma = sum g*xhat, dbeta = sum g."""
    eps = 1e-5
    y, dpool, gamma, beta, rm, rv = R.bn_case_operands(B, H, W, torch.float32, R.seed_of(B, H, W, 64, salt=5))
    gamma = gamma.clone()
    gamma[R.CH_ZERO_GAMMA] = 0.3                                                    # (the form divides nothing by gamma; any value)
    dy, dgamma, dbeta = R.stem_bn_backward_ref(y, gamma, beta, dpool, training, eps, rm, rv)
    scale, shift, mean, invstd = R.bn_coef_ref(y, gamma, beta, training, eps, rm, rv)
    _, codes, _ = R.pool_ref(y, scale, shift)
    _, pre = R.bn_relu(y, scale, shift)
    g = R.route_ref(dpool, codes, pre > 0, H, W)
    xhat = (y.double() - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    sg, sgx = g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))
    assert torch.allclose(sg, dbeta, rtol=1e-12, atol=1e-12) and torch.allclose(sgx, dgamma, rtol=1e-12, atol=1e-12)
    bc = R.bc_ref(sg, sgx, B * H * W, gamma, mean, invstd, training)
    assert torch.allclose(R.dy_ref(bc, g, y), dy, rtol=1e-11, atol=1e-13)
    assert float(g[:, R.CH_DEAD].abs().max()) == 0.0 and float(dy[:, R.CH_DEAD].abs().max()) < 1e-15


@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.case_id)
def test_seeded_random_inputs_keep_what_the_gpu_tests_presuppose(case):
    (B, H, W), d, C = case
    dtype = R.DT[d]
    # pooling forward: at most 1 % of the windows have their two largest values closer than the forward bound allows to tell apart,
    # and no pre-ReLU value lies within its bound of zero
    y, scale, shift = R.random_pool_operands(B, H, W, C, dtype, R.seed_of(B, H, W, C))
    _, _, v = R.pool_ref(y, scale, shift)
    _, pre = R.bn_relu(y, scale, shift)
    e = R.fwd_bound(y, scale, shift)
    assert R.near_tie_share(v, e) <= 0.01
    assert bool((pre.abs() > e).all())
    # vqa_stem_bwd_apply on random codes: no value at the ReLU threshold; some pixel is named by two and some by four windows
    # whose gradient survives the mask
    y, dpool, codes, scale, shift, bc = R.random_bwd_operands(B, H, W, C, dtype, R.seed_of(B, H, W, C, salt=R.BWD_SALT[(B, H, W)]))
    _, pre = R.bn_relu(y, scale, shift)
    assert bool((pre.abs() > R.fwd_bound(y, scale, shift)).all())
    if H >= 3 and W >= 3:
        n = R.route_counts(codes, H, W) * (pre > 0)
        assert bool((n == 2).any()) and bool((n == 4).any())


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("d", ["fp32", "bf16"])
@pytest.mark.parametrize("B,H,W", R.BN_SHAPES)
def test_seeded_bn_inputs_are_decided_far_from_rounding(B, H, W, d, training):
    """The chain test compares dy element by element, so no ReLU sign and no pooling winner may hang on the fp32 rounding of the
    BatchNorm coefficients: every |pre-ReLU value| and every gap between a window's two largest distinct values exceeds 8x the
    forward bound.  The special channels are what they claim to be."""
    y, dpool, gamma, beta, rm, rv = R.bn_case_operands(B, H, W, R.DT[d], R.seed_of(B, H, W, 64, salt=5))
    scale, shift, mean, invstd = R.bn_coef_ref(y, gamma, beta, training, 1e-5, rm, rv)
    pooled, _, v = R.pool_ref(y, scale, shift)
    _, pre = R.bn_relu(y, scale, shift)
    e = 8 * R.fwd_bound(y, scale, shift)
    assert bool((pre.abs() > e).all())
    assert R.near_tie_share(v, e) == 0.0
    assert float(pooled[:, R.CH_DEAD].max()) == 0.0 and float(pre[:, R.CH_DEAD].max()) < 0
    assert float(pre[:, R.CH_CANCEL].min()) > 0 and float(pre[:, R.CH_ZERO_GAMMA].min()) == 0.5
    assert float(scale[R.CH_NEG_GAMMA]) < 0
