"""Bit-exact tests of the GEMM and convolution kernels on small-integer operands (tests/_exactint.py): with sum |a||b| below 2^24
every fp32 partial sum is an exact integer in any summation order, so a bf16 output must be RNE_bf16(exact integer) bit for bit, an
fp32 output the integer itself, and a fixed-point BatchNorm accumulator exactly 16 * sum in its hi plane and 0 in its lo plane.
Every comparison is torch.equal / integer equality: there is no tolerance in this file.  Each test asserts the reference-side bound
first (a condition on the inputs; tests/test_exactint_ref_cpu.py proves the same bounds and the tie shares without a GPU).

Rounding orders the kernels document, encoded here exactly:
  vqa_igemm         acc + bias, ReLU (relu = 1) in fp32 -> the compute dtype (first rounding) -> + addend * (addmask > 0) -> ReLU
                    (relu = 2: after the addend, the folded eval block) -> rounded again -> * (outmask > 0).  Slab / accumulator
                    statistics: bf16 sums the STORED (rounded) values, fp32 the accumulators.
  vqa_conv8p        same epilogue; statistics and the BatchNorm-backward sums are those of the STORED bf16 tile.
  vqa_conv3x3_c64p  same epilogue; statistics are those of the fp32 ACCUMULATORS; the BatchNorm-backward sums use the stored value.
  vqa_linear_dgrad_act   the value rounded to the compute dtype, masked by (outact > 0), times the keep scale, rounded.
What this family proves: no dropped, doubled or misplaced term anywhere in a reduction, round-to-nearest-even stores, exact
statistics.  It says nothing about accuracy on real-valued data: that stays with the tolerance tests of the other files."""
import pytest
import torch

import _exactint as X
from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
WIDE, NARROW = X.WIDE, X.NARROW
DTYPES = [F32, BF]


def dev(t, dtype):
    return t.to(dtype).contiguous().to(DEV)


def krsc(w):
    """[Cout][Cin][R][S] -> the fp32 master layout [Cout][R][S][Cin] on the device"""
    return X.nhwc(w).float().to(DEV)


def same(got, want):
    torch.cuda.synchronize()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    got = got.cpu()
    if not torch.equal(got, want):
        bad = (got.double() != want.double())
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} elements differ; first at {i}: got {float(got[tuple(i)])}, want {float(want[tuple(i)])}")


def words(k, c):
    return sub("_lib").count("vqa_bn_acc_words", k, c)


def acc_zero(k, c):
    return torch.zeros(words(k, c), device=DEV, dtype=torch.int64)


def assert_acc(acc, k, c, sums):
    """hi plane == 16 * sums as integers, lo plane == 0, flag == 0 (sums: fp64 [k][c], multiples of 1/16)"""
    torch.cuda.synchronize()
    hi, lo, flag = X.acc_decode_exact(acc, X.acc_replicas(c), k, c)
    want = (sums * 16).round().to(torch.int64)
    assert torch.equal(want.double(), sums * 16)
    assert flag == 0 and int(lo.abs().max()) == 0
    assert torch.equal(hi, want), f"{int((hi != want).sum())} accumulator sums differ"


def epilogue_cases(need_addend=False):
    out = [dict(addend=1), dict(addend=1, addmask=1), dict(outmask=1), dict(addend=1, addmask=1, outmask=1)]
    if need_addend:
        out[2] = dict(addend=1, outmask=1)
    return out


def epilogue_expect(base, kw, add, am, om, dtype):
    """(conv + addend * (addmask > 0)) re-rounded, then * (outmask > 0): base is the value after the first rounding"""
    e = base.double()
    if "addend" in kw:
        e = X.expect(e + (add * (am > 0) if "addmask" in kw else add), dtype).double()
    if "outmask" in kw:
        e = e * (om > 0)
    return X.expect(e, dtype)


# ------------------------------------------------------------------------------------------------ canary
@pytest.mark.parametrize("entry", ["vqa_gemm8p", "vqa_gemm4w"])
@pytest.mark.parametrize("M,N,K", X.GEMM_CANARY)
def test_canary_dense_gemm(M, N, K, entry):
    """If ONLY this dense product fails, exact MFMA accumulation of integers is what broke, not a kernel's indexing."""
    L = sub("_lib")
    d = X.gemm_case(M, N, K, WIDE)
    X.assert_exact_range(d["bound"])
    A, B = dev(d["A"], BF), dev(d["B"], BF)
    C = torch.full((M, N), float("nan"), device=DEV, dtype=BF)
    L.call(entry, A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K)
    same(C, X.rne_bf16(d["y"]))


# ------------------------------------------------------------------------------------------------ vqa_igemm
def _igemm_fwd(K, d, case, dtype, **kw):
    B, Cin, Cout, H, R, stride, pad = case[:7]
    Ho = (H + 2 * pad - R) // stride + 1
    M, Kw = B * Ho * Ho, R * R * Cin
    geom = (B, H, H, Cin, Ho, Ho, R, R, stride, pad)
    wp = K.pack_rows(krsc(d["w"]).view(Cout, Kw), dtype)
    return K.igemm(dev(X.nhwc(d["x"]), dtype), wp, M, Cout, Kw, geom, dtype=dtype, **kw), geom, M, Kw


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", X.IGEMM_CONV)
def test_igemm_conv_forward_dgrad_epilogues(case, dtype):
    K = sub("kernels")
    B, Cin, Cout, H, R, stride, pad, off = case
    d = X.conv_case(B, Cin, Cout, H, H, R, stride, pad, WIDE, off, want_dgrad=stride == 1)
    X.assert_exact_range(d["bound"])
    (y, _, _), geom, M, Kw = _igemm_fwd(K, d, case, dtype)
    same(y, X.expect(d["y"], dtype))
    if stride != 1:
        return
    # transposed = 1: the stride-1 data gradient through the [Cin][(tap, Cout)] pack, then the masked identity-path epilogues
    Ho, Md = geom[4], B * H * H
    add, am, om = X.epilogue_operands((Md, Cin), 100 + Cin)
    X.assert_exact_range(d["dbound"] + float(add.abs().max()))
    wt = K.pack_transpose(krsc(d["w"]).view(Cout, R * R, Cin), dtype)
    geom_d = (B, Ho, Ho, Cout, H, H, R, R, stride, pad)
    dy_d = dev(X.nhwc(d["dy"]), dtype)
    dx, _, _ = K.igemm(dy_d, wt, Md, Cin, R * R * Cout, geom_d, dtype=dtype, transposed=1)
    base = X.expect(d["dx"], dtype)
    same(dx, base)
    t = dict(addend=dev(add, dtype), addmask=dev(am, dtype), outmask=dev(om, dtype))
    for kw in epilogue_cases():
        got, _, _ = K.igemm(dy_d, wt, Md, Cin, R * R * Cout, geom_d, dtype=dtype, transposed=1, **{k: t[k] for k in kw})
        same(got, epilogue_expect(base, kw, add, am, om, dtype))


def _infer_operands(d, dtype):
    e = d["e"]
    return dev(e["bias"], F32), dev(e["add"], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", X.IGEMM_CONV)
def test_igemm_folded_block_conv1_and_conv2_forms(case, dtype):
    """The epilogues of the Conv+BN-folded eval block on every conv geometry: conv1 = bias + ReLU (relu = 1), conv2 = bias + residual
    addend + ReLU AFTER the addend (relu = 2).  About 15 % of the outputs have conv + bias > 0 and conv + bias + addend < 0 and as
    many the reverse (asserted on the reference in test_exactint_ref_cpu.py): a ReLU before the addend, a dropped bias or a single
    rounding in place of two all change stored bits."""
    K = sub("kernels")
    B, Cin, Cout, H, R, stride, pad, off = case
    d = X.conv_infer_case(B, Cin, Cout, H, H, R, stride, pad, WIDE, off)
    X.assert_exact_range(d["ibound"])
    bias, add = _infer_operands(d, dtype)
    (a1, _, _), _, _, _ = _igemm_fwd(K, d, case, dtype, bias=bias, relu=1)
    same(a1, X.conv1_expect(d["e"], dtype))
    (out, _, _), _, _, _ = _igemm_fwd(K, d, case, dtype, bias=bias, addend=add, relu=2)
    want = X.conv2_expect(d["e"], dtype)
    assert not torch.equal(want, X.relu_before_addend(d["e"], dtype))
    same(out, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", X.IGEMM_SHORTCUT, ids=["1x1s2", "1x1s1"])
def test_igemm_folded_block_shortcut_form(case, dtype):
    """The folded shortcut: 1x1 conv, pad 0, bias, no ReLU (negative values are stored as they are)."""
    K = sub("kernels")
    B, Cin, Cout, H, R, stride, pad, off = case
    d = X.conv_infer_case(B, Cin, Cout, H, H, R, stride, pad, WIDE, off)
    X.assert_exact_range(d["ibound"])
    bias, _ = _infer_operands(d, dtype)
    (res, _, _), _, _, _ = _igemm_fwd(K, d, case, dtype, bias=bias)
    want = X.shortcut_expect(d["e"], dtype)
    assert float(want.min()) < 0
    same(res, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_igemm_scalar_epilogue_relu_after_addend(dtype):
    """N = 10 is no multiple of the vector width: the epilogue's scalar branch, with bias + addend + relu = 2 and with bias + ReLU."""
    K = sub("kernels")
    M, Kin, N, off = X.LINEAR_SCALAR_RELU2
    d = X.linear_relu2_case(M, Kin, N, WIDE, off)
    X.assert_exact_range(d["ibound"])
    bias, add = _infer_operands(d, dtype)
    args = (dev(d["x"], dtype), K.pack_rows(dev(d["w"], F32), dtype), M, N, Kin, K.linear_geom(M, Kin))
    out, _, _ = K.igemm(*args, dtype=dtype, bias=bias, addend=add, relu=2)
    same(out, X.conv2_expect(d["e"], dtype))
    a1, _, _ = K.igemm(*args, dtype=dtype, bias=bias, relu=1)
    same(a1, X.conv1_expect(d["e"], dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", X.IGEMM_CONV)
def test_igemm_statistics_slab_and_accumulator(case, dtype):
    """Narrow range.  bf16: column sums of the STORED bf16 tile (the kernel sums the staged tile on the matrix cores); fp32: of the
    accumulators (which are the stored values).  Slab rows are exact integers, so their fp64 total is exact."""
    K = sub("kernels")
    B, Cin, Cout, H, R, stride, pad, _ = case
    d = X.conv_case(B, Cin, Cout, H, H, R, stride, pad, NARROW)
    X.assert_exact_range(d["bound"])
    summed = X.expect(d["y"], dtype).double()
    X.assert_resummed(summed)
    want = torch.stack([summed.sum(0), (summed * summed).sum(0)])
    (y, stats, mt), _, M, _ = _igemm_fwd(K, d, case, dtype, want_stats=True)
    same(y, X.expect(d["y"], dtype))
    assert stats.shape == (mt, 2, Cout) and mt > 0
    assert torch.equal(stats.double().sum(0).cpu(), want)
    acc = acc_zero(2, Cout)
    (y2, _, _), _, _, _ = _igemm_fwd(K, d, case, dtype, stats_acc=acc)
    same(y2, X.expect(d["y"], dtype))
    assert_acc(acc, 2, Cout, want)


@pytest.mark.parametrize("case", X.IGEMM_STAGES)
def test_igemm_window_loader_variants(case):
    """One case per window-loader instantiation the benchmark times, at the smallest batch that still selects it (bf16)."""
    K = sub("kernels")
    B, C, H, want = case
    geom = (B, H, H, C, H, H, 3, 3, 1, 1)
    M, Kw = B * H * H, 9 * C
    assert K.igemm_variant(BF, K.LOADER_NHWC, M, C, Kw, geom) == want
    assert K.igemm_variant(BF, K.LOADER_NHWC, (B - 1) * H * H, C, Kw, (B - 1,) + geom[1:]) != want        # the smallest such batch
    d = X.conv_case(B, C, C, H, H, 3, 1, 1, WIDE, want_dgrad=True)
    X.assert_exact_range(max(d["bound"], d["dbound"]))
    (y, _, _), _, _, _ = _igemm_fwd(K, d, (B, C, C, H, 3, 1, 1), BF)
    same(y, X.rne_bf16(d["y"]))
    # the folded eval block's conv1 form (bias + ReLU) through the same window loader
    X.with_infer_epilogue(d, X.infer_seed(B, C, C, H, 3, 1))
    X.assert_exact_range(d["ibound"])
    (a1, _, _), _, _, _ = _igemm_fwd(K, d, (B, C, C, H, 3, 1, 1), BF, bias=dev(d["e"]["bias"], F32), relu=1)
    same(a1, X.conv1_expect(d["e"], BF))
    wt = K.pack_transpose(krsc(d["w"]).view(C, 9, C), BF)
    dx, _, _ = K.igemm(dev(X.nhwc(d["dy"]), BF), wt, M, C, Kw, geom, dtype=BF, transposed=1)
    same(dx, X.rne_bf16(d["dx"]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_igemm_stem_loader(dtype):
    K = sub("kernels")
    B, H = 3, X.STEM_LOADER_HW
    d = X.stem_case(B, H, H, WIDE)
    X.assert_exact_range(d["bound"])
    Ho = (H + 6 - 7) // 2 + 1
    BK = 64 if dtype == BF else 32
    Kp = (147 + BK - 1) // BK * BK
    wp = K.pack_rows(krsc(d["w"]).view(64, 147), dtype, Kp)
    y, _, _ = K.igemm(dev(d["img"], F32), wp, B * Ho * Ho, 64, Kp, (B, H, H, 3, Ho, Ho, 7, 7, 2, 3), dtype=dtype, loader=K.LOADER_STEM)
    same(y, X.expect(d["y"], dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", X.LINEARS)
def test_igemm_linear_bias_relu_addend(case, dtype):
    """out = round(round(relu(x w^T + b)) + addend): bias and ReLU act on the fp32 accumulator, the addend on the rounded value."""
    K = sub("kernels")
    M, Kin, N, off = case
    d = X.linear_case(M, Kin, N, WIDE, off)
    X.assert_exact_range(d["bound"])
    out, _, _ = K.igemm(dev(d["x"], dtype), K.pack_rows(dev(d["w"], F32), dtype), M, N, Kin, K.linear_geom(M, Kin), dtype=dtype,
                        bias=dev(d["bias"], F32), relu=1, addend=dev(d["res"], dtype))
    same(out, X.expect(X.expect(d["pre"], dtype).double() + d["res"], dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("drop_p", [0.0, 0.5])
def test_linear_dgrad_act(drop_p, dtype):
    """(dz W) rounded to the compute dtype, * (outact > 0), * 1 / (1 - p) (2 is exact), rounded."""
    K = sub("kernels")
    M, Kin, N = X.LINEAR_DGRAD_ACT
    d = X.linear_dgrad_case(M, Kin, N, WIDE)
    X.assert_exact_range(d["bound"])
    wt = K.pack_transpose(dev(d["w"], F32).view(N, 1, Kin), dtype)
    got = K.linear_dgrad_act(dev(d["dz"], dtype), wt, M, Kin, N, dtype=dtype, outact=dev(d["h"], dtype), drop_p=drop_p)
    e = X.expect(d["y"], dtype).double() * (d["h"] > 0) * (1.0 / (1.0 - drop_p))
    same(got, X.expect(e, dtype))


# ------------------------------------------------------------------------------------------------ vqa_conv8p
def _c8_fwd_operands(d, N, C):
    return dev(X.rows(d["x"]), BF), dev(X.nhwc(d["w"]).reshape(N, 9 * C), BF)


@pytest.mark.parametrize("B,H,W,C,N,stride", [c + (1,) for c in X.CONV8P] + [c + (2,) for c in X.CONV8P_S2])
def test_conv8p_forward_and_statistics(B, H, W, C, N, stride):
    K = sub("kernels")
    assert K.conv8p_ok(B, H, W, C, N)
    d = X.conv_case(B, C, N, H, W, 3, stride, 1, WIDE)
    X.assert_exact_range(d["bound"])
    x, w = _c8_fwd_operands(d, N, C)
    same(K.conv8p(x, w, B, H, W, C, N, stride=stride), X.rne_bf16(d["y"]))
    # narrow range: the fixed-point statistics of the STORED bf16 tile
    n = X.conv_case(B, C, N, H, W, 3, stride, 1, NARROW)
    X.assert_exact_range(n["bound"])
    stored = X.rne_bf16(n["y"]).double()
    X.assert_resummed(stored)
    acc = acc_zero(2, N)
    x, w = _c8_fwd_operands(n, N, C)
    same(K.conv8p(x, w, B, H, W, C, N, stride=stride, stats_acc=acc), X.rne_bf16(n["y"]))
    assert_acc(acc, 2, N, torch.stack([stored.sum(0), (stored * stored).sum(0)]))


@pytest.mark.parametrize("B,H,W,C,N", X.CONV8P)
def test_conv8p_transposed_and_epilogues(B, H, W, C, N):
    K = sub("kernels")
    d = X.transposed8p_case(B, H, W, C, N, WIDE)
    add, am, om = X.epilogue_operands(d["y"].shape, 200 + N)
    X.assert_exact_range(d["bound"] + float(add.abs().max()))
    x = dev(X.rows(d["x"]), BF)
    wt = K.pack_transpose(dev(d["w"].reshape(C, 9, N), F32), BF).view(N, 9 * C)
    base = X.rne_bf16(d["y"])
    same(K.conv8p(x, wt, B, H, W, C, N, transposed=1), base)
    t = dict(addend=dev(add, BF), addmask=dev(am, BF), outmask=dev(om, BF))
    for kw in epilogue_cases():
        same(K.conv8p(x, wt, B, H, W, C, N, transposed=1, **{k: t[k] for k in kw}), epilogue_expect(base, kw, add, am, om, BF))


@pytest.mark.parametrize("B,H,W,C,N", X.CONV8P)
def test_conv8p_batchnorm_backward_sums(B, H, W, C, N):
    """bnred in its three forms, narrow range, exact coefficients (integer mean and shift, scale and invstd powers of two): the sums
    sum g | sum g xhat(y) | sum g xhat(y2) of the STORED tile are multiples of 1/2 and must sit in the hi plane exactly.
    self-mask: g = out * [y * scale + shift > 0]; already masked: g = out (after addend and outmask); dual: + the shortcut's row."""
    K = sub("kernels")
    d = X.bnred8p_case(B, H, W, C, N)
    X.assert_exact_range(d["bound"])
    x = dev(X.rows(d["x"]), BF)
    wt = K.pack_transpose(dev(d["w"].reshape(C, 9, N), F32), BF).view(N, 9 * C)
    y, coef = dev(d["bn_y"], BF), dev(d["coef"], F32)
    for form, (want, sums, bound) in d["forms"].items():
        X.assert_exact_range(bound)
        facc = acc_zero(3, N)
        if form == "self":
            out = K.conv8p(x, wt, B, H, W, C, N, transposed=1, bnred=(y, coef, facc))
        else:
            dual = form == "dual"
            out = K.conv8p(x, wt, B, H, W, C, N, transposed=1, addend=dev(d["add"], BF), outmask=dev(d["om"], BF),
                           bnred=(y, coef, facc, False, dev(d["bn_y2"], BF) if dual else None, dev(d["coef2"], F32) if dual else None))
        same(out, want)
        assert_acc(facc, 3, N, sums)


# ------------------------------------------------------------------------------------------------ vqa_conv3x3_c64p, _epi, _bnred
@pytest.mark.parametrize("B,H,W", X.C64P)
def test_conv3x3_c64p_forward_dgrad_epilogues(B, H, W):
    K = sub("kernels")
    assert K.c64p_blocks(B, H, W) > 0
    d = X.conv_case(B, 64, 64, H, W, 3, 1, 1, WIDE, want_dgrad=True)
    add, am, om = X.epilogue_operands(d["dx"].shape, 400 + H)
    X.assert_exact_range(max(d["bound"], d["dbound"]) + float(add.abs().max()))
    wk = krsc(d["w"])
    y, _, _ = K.conv3x3_c64p(dev(X.nhwc(d["x"]), BF), K.pack_rows(wk.view(64, 576), BF), B, H, W)
    same(y, X.rne_bf16(d["y"]))
    wflip = K.pack_transpose(wk.view(64, 9, 64), BF, flip=True)
    dy_d = dev(X.nhwc(d["dy"]), BF)
    dx, _, _ = K.conv3x3_c64p(dy_d, wflip, B, H, W)
    base = X.rne_bf16(d["dx"])
    same(dx, base)
    t = dict(addend=dev(add, BF), addmask=dev(am, BF), outmask=dev(om, BF))
    for kw in epilogue_cases(need_addend=True):
        same(K.conv3x3_c64p_epi(dy_d, wflip, B, H, W, **{k: t[k] for k in kw}), epilogue_expect(base, kw, add, am, om, BF))


@pytest.mark.parametrize("B,H,W", X.C64P)
def test_conv3x3_c64p_statistics_and_batchnorm_backward_sums(B, H, W):
    """Narrow range.  Both statistics modes (slab, fixed-point accumulator) hold the sums of the fp32 ACCUMULATORS (the kernel adds
    acc and acc^2 before the bf16 conversion): the exact integers y, not the rounded tile.  bnred: g = the STORED value * mask."""
    K = sub("kernels")
    d = X.c64p_narrow_case(B, H, W)
    X.assert_exact_range(max(d["bound"], d["dbound"]))
    X.assert_resummed(d["y"])
    want = torch.stack([d["y"].sum(0), (d["y"] * d["y"]).sum(0)])
    wk = krsc(d["w"])
    x, wp = dev(X.nhwc(d["x"]), BF), K.pack_rows(wk.view(64, 576), BF)
    y, stats, nb = K.conv3x3_c64p(x, wp, B, H, W, want_stats=True)
    same(y, X.rne_bf16(d["y"]))
    assert stats.shape == (nb, 2, 64) and torch.equal(stats.double().sum(0).cpu(), want)
    acc = acc_zero(2, 64)
    y2, _, _ = K.conv3x3_c64p(x, wp, B, H, W, stats_acc=acc)
    same(y2, X.rne_bf16(d["y"]))
    assert_acc(acc, 2, 64, want)
    # the data gradient that also leaves the BatchNorm-backward sums of relu(BatchNorm(yv)) (self mask; the third row stays zero)
    X.assert_exact_range(d["sums_bound"])
    facc = acc_zero(3, 64)
    wflip = K.pack_transpose(wk.view(64, 9, 64), BF, flip=True)
    out = K.conv3x3_c64p_bnred(dev(X.nhwc(d["dy"]), BF), wflip, B, H, W, dev(d["bn_y"], BF), dev(d["coef"], F32), facc)
    same(out, d["g"])
    assert_acc(facc, 3, 64, d["sums"])


# ------------------------------------------------------------------------------------------------ weight gradients (fp32, +=)
@pytest.mark.parametrize("case", X.WGRAD_PLAN, ids=["%dx%d-%d-r%ds%d" % (c[1], c[2], c[3], c[4], c[5]) for c in X.WGRAD_PLAN])
def test_wgrad_every_planner_kind(case):
    """vqa_wgrad at the smallest batch at which vqa_wgrad_plan still gives the kind and tiles of the B = 512 benchmark launch (and a
    split over M), narrow range, into a prefilled buffer: every element equal."""
    K = sub("kernels")
    B, Cin, Cout, H, R, stride, pad, expect = case
    Ho = (H + 2 * pad - R) // stride + 1
    M, Kw = B * Ho * Ho, R * R * Cin
    plan = K.wgrad_plan(BF, 0, M, Cout, Kw, B, H, H, Cin, R, R)
    bench = K.wgrad_plan(BF, 0, 512 * Ho * Ho, Cout, Kw, 512, H, H, Cin, R, R)
    assert plan[:3] == expect and bench[:3] == expect and plan[3] > 1, (plan, bench)
    d = X.wgrad_plan_case(case)
    X.assert_exact_range(d["bound"])
    dw = dev(d["dw0"], F32)
    K.wgrad(dev(X.nhwc(d["dy"]), BF), dev(X.nhwc(d["x"]), BF), dw, M, Cout, Kw, (B, H, H, Cin, Ho, Ho, R, R, stride, pad), dtype=BF)
    same(dw, (X.wgrad_ref(d["x"], d["dy"], (Cout, Cin, R, R), stride, pad) + d["dw0"]).float())


@pytest.mark.parametrize("B,H,W", X.WGRAD_C64)
def test_wgrad3x3_c64_and_its_batchnorm_prologue(B, H, W):
    """(20, 56, 56): 280 row blocks on the 256-workgroup persistent grid.  _bn: x = relu(y * scale + shift) with exact coefficients."""
    K = sub("kernels")
    assert K.c64w_blocks(B, H, W) > 0 and K.c64w_bn_ok(B, H, W)
    d = X.wgrad_c64_case(B, H, W)
    X.assert_exact_range(max(d["bound"], d["bound_bn"]))
    x, dy = dev(X.nhwc(d["x"]), BF), dev(X.nhwc(d["dy"]), BF)
    dw = dev(d["dw0"], F32)
    K.wgrad3x3_c64(x, dy, dw, B, H, W)
    same(dw, (X.wgrad_ref(d["x"], d["dy"], (64, 64, 3, 3), 1, 1) + d["dw0"]).float())
    dw = dev(d["dw0"], F32)
    K.wgrad3x3_c64_bn(x, dev(d["coef"], F32), dy, dw, B, H, W)
    same(dw, (X.wgrad_ref(d["xin"], d["dy"], (64, 64, 3, 3), 1, 1) + d["dw0"]).float())


@pytest.mark.parametrize("B", X.WGRAD_C128_B)
def test_wgrad3x3_c128(B):
    K = sub("kernels")
    H = W = 28
    assert K.c128_wgrad_blocks(B, H, W) > 0
    d = X.wgrad_c128_case(B)
    X.assert_exact_range(d["bound"])
    dw = dev(d["dw0"], F32)
    K.wgrad3x3_c128(dev(X.nhwc(d["x"]), BF), dev(X.nhwc(d["dy"]), BF), dw, B, H, W)
    same(dw, (X.wgrad_ref(d["x"], d["dy"], (128, 128, 3, 3), 1, 1) + d["dw0"]).float())


def test_wgrad_group_three_jobs():
    K = sub("kernels")
    jobs, wants = [], []
    for i, (M, N, Kw) in enumerate(X.WGRAD_GROUP):
        assert K.wgrad_group_ok(BF, M, N, Kw)
        d = X.wgrad_group_case(i)
        X.assert_exact_range(d["bound"])
        jobs.append((dev(d["dy"], BF), dev(d["x"], BF), dev(d["dw0"], F32), M, N, Kw))
        wants.append((d["dy"].t() @ d["x"] + d["dw0"]).float())
    K.wgrad_group(jobs, dtype=BF)
    for j, w in zip(jobs, wants):
        same(j[2], w)


@pytest.mark.parametrize("H,W", X.STEM_WGRAD_HW)
def test_stem_wgrad(H, W):
    K = sub("kernels")
    B = 3
    d = X.stem_wgrad_case(B, H, W)
    X.assert_exact_range(d["bound"])
    dw = dev(d["dw0"], F32)
    K.stem_wgrad(dev(d["img"], F32), dev(X.nhwc(d["dy"]), BF), dw, B, H, W)
    same(dw, (X.wgrad_ref(d["img"], d["dy"], (64, 3, 7, 7), 2, 3) + d["dw0"]).float())


# ------------------------------------------------------------------------------------------------ vqa_dgrad_s2
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", X.DGRAD_S2)
def test_dgrad_s2(case, dtype):
    K = sub("kernels")
    B, Cin, Cout, H, shortcut = case
    d = X.dgrad_s2_case(B, Cin, Cout, H, shortcut, WIDE)
    X.assert_exact_range(d["bound"])
    Ho = H // 2
    ktot = (10 if shortcut else 9) * Cout
    wt = torch.empty(Cin, ktot, device=DEV, dtype=dtype)
    K.pack_transpose(krsc(d["w1"]).view(Cout, 9, Cin), dtype, out=wt, ldo=ktot, col0=0)
    if shortcut:
        K.pack_transpose(krsc(d["wd"]).view(Cout, 1, Cin), dtype, out=wt, ldo=ktot, col0=9 * Cout)
    dx = K.dgrad_s2(dev(X.nhwc(d["dy"]), dtype), dev(X.nhwc(d["dyd"]), dtype) if shortcut else None, wt, B, Ho, Ho, Cout, H, H, Cin, 3, 1, dtype=dtype)
    same(dx, X.expect(d["dx"], dtype))


# ------------------------------------------------------------------------------------------------ stem
def _stem_pack(w):
    wst = torch.empty(64, 192, device=DEV, dtype=BF)
    sub("_lib").call("vqa_stem_pack", krsc(w).data_ptr(), wst.data_ptr())
    return wst


@pytest.mark.parametrize("H,W", X.STEM_CONV_HW)
def test_stem_conv(H, W):
    K = sub("kernels")
    B = 3
    assert K.stem_conv_blocks(B, H, W) > 0
    d = X.stem_case(B, H, W, WIDE)
    X.assert_exact_range(d["bound"])
    y, _, _ = K.stem_conv(dev(d["img"], F32), _stem_pack(d["w"]), B, H, W, False)
    same(y, X.rne_bf16(d["y"]))


@pytest.mark.parametrize("H,W", X.STEM_POOL_HW)
def test_stem_conv_pool(H, W):
    """vqa_stem_conv refuses 32 x 72 (conv width 36 is no multiple of 16); the inference kernel takes it: with scale a power of two and
    an integer shift, max-pool(relu(scale * acc + shift)) is exact and the one bf16 rounding of the result is all that is left."""
    K, L = sub("kernels"), sub("_lib")
    B = 3
    assert L.count("vqa_stem_conv_pool_ok", B, H, W) == 1
    d = X.stem_pool_case(B, H, W)
    X.assert_exact_range(d["bound"])
    coef = dev(torch.cat([d["scale"], d["shift"], torch.zeros(128, dtype=torch.float64)]), F32)
    got = K.stem_conv_pool(dev(d["img"], F32), _stem_pack(d["w"]), coef, B, H, W)
    same(got, X.rne_bf16(d["pooled"]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_stem_dgrad(dtype):
    K = sub("kernels")
    B = 2
    H, W = X.STEM_DGRAD_HW
    d = X.stem_dgrad_case(B, H, W)
    X.assert_exact_range(d["bound"])
    got = K.stem_dgrad(dev(X.rows(d["dy"]), dtype), K.stem_dgrad_pack(krsc(d["w"]), dtype), B, H, W)
    same(got, d["dimg"].float())
