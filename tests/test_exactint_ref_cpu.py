"""The exact-integer helper (tests/_exactint.py) checked on the reference alone, without a GPU: bf16 ties, the generators, the
accumulator decoder, and -- for every (shape, range) pair tests/test_gpu_exact_integer.py uses -- that the operands are inside the
exact range (bound below 2^24) and that the wide cases really land on bf16 ties and roundings (at least 5 % / 10 % of the outputs),
so the GPU comparisons cannot silently degenerate into trivially exact ones."""
import pytest
import torch

import _exactint as X

WIDE, NARROW = X.WIDE, X.NARROW


def test_rne_bf16_on_hand_picked_ties():
    for v, want in ((257, 256), (259, 260), (513, 512), (515, 516), (258, 258), (514, 512), (518, 520), (1028, 1024), (1036, 1040)):
        for s in (1, -1):
            got = X.rne_bf16(torch.tensor([float(s * v)], dtype=torch.float64))
            assert got.dtype == torch.bfloat16 and float(got) == float(s * want), (s * v, float(got))
    tie, changed = X.shares(torch.tensor([257.0, 258.0, 259.0, 513.0, 514.0, 100.0, -515.0, 0.0], dtype=torch.float64))
    assert tie == 3 / 8 and changed == 5 / 8                       # ties: 257, 259, 514 (between 512 and 516); 513 and -515 round but are no ties
    tie, changed = X.shares(torch.tensor([513.0, 515.0], dtype=torch.float64))
    assert tie == 0.0 and changed == 1.0


def test_generators_are_reproducible_and_stay_in_range():
    for amax in (1, 2, 3, 8):
        a, b = X.ints((64, 33), amax, 5), X.ints((64, 33), amax, 5)
        assert torch.equal(a, b) and a.dtype == torch.float64 and torch.equal(a, a.round())
        assert float(a.min()) == -amax and float(a.max()) == amax
        assert not torch.equal(a, X.ints((64, 33), amax, 6))
        o = X.ints((64, 33), amax, 5, offset=True)
        assert float(o.min()) == 0 and float(o.max()) == amax
        assert torch.equal(a, a.to(torch.bfloat16).double())          # exact in bf16
    p = X.pow2s(200, 3, signed=True)
    assert set(p.abs().tolist()) == {0.5, 1.0, 2.0} and float(p.min()) < 0
    c = X.bn_coef(64, 9)
    assert c.shape == (4, 64) and torch.equal(c[1:3], c[1:3].round()) and float(c[3].min()) >= 0.5


def test_assert_exact_range_fails_outside():
    X.assert_exact_range(float((1 << 24) - 1))
    with pytest.raises(AssertionError):
        X.assert_exact_range(float(1 << 24))
    with pytest.raises(AssertionError):
        X.assert_exact_range(torch.tensor([1.0, float(1 << 25)]))


def test_acc_decode_exact_on_a_hand_built_accumulator():
    R, K, C = 2, 3, 4
    n = R * K * C
    acc = torch.zeros(2 * n + 2, dtype=torch.int64)
    acc[(0 * K + 1) * C + 2] = 16 * 5                   # replica 0, row 1, channel 2: 5
    acc[(1 * K + 1) * C + 2] = -16 * 7 + 3              # replica 1: -7 + 3/16
    acc[(1 * K + 2) * C + 0] = (1 << 45)                # far beyond what a double-based decode of a sum keeps apart from +1
    acc[(0 * K + 2) * C + 0] = 1
    acc[n] = 2
    acc[n + 1 + (1 * K + 0) * C + 3] = -9
    hi, lo, flag = X.acc_decode_exact(acc, R, K, C)
    assert hi.dtype == torch.int64 and lo.dtype == torch.int64 and hi.shape == (K, C)
    assert int(hi[1, 2]) == -16 * 2 + 3 and int(hi[2, 0]) == (1 << 45) + 1 and int(lo[0, 3]) == -9 and flag == 2
    assert int(hi.abs().sum()) == 29 + (1 << 45) + 1 and int(lo.abs().sum()) == 9
    assert [X.acc_replicas(c) for c in (64, 128, 256, 512, 1024)] == [8, 4, 2, 1, 1]


# ---------------------------------------------------------------------------------------------- every case of the GPU file
@pytest.mark.parametrize("case", X.GEMM_CANARY)
def test_canary_cases(case):
    d = X.gemm_case(*case, WIDE)
    X.assert_exact_range(d["bound"])
    X.assert_wide_shares(d["y"])


@pytest.mark.parametrize("case", X.IGEMM_CONV + [(B, C, C, H, 3, 1, 1, False) for B, C, H, _ in X.IGEMM_STAGES])
def test_igemm_conv_cases(case):
    B, Cin, Cout, H, R, stride, pad, off = case
    d = X.conv_case(B, Cin, Cout, H, H, R, stride, pad, WIDE, off, want_dgrad=stride == 1)
    X.assert_exact_range(d["bound"])
    X.assert_wide_shares(d["y"])
    if stride == 1:
        X.assert_exact_range(d["dbound"] + 64)                      # (+ the epilogue addend)
        X.assert_wide_shares(d["dx"])
    # the folded eval block's epilogues on the same product: bias + ReLU, bias alone, bias + addend + ReLU after it
    i = X.with_infer_epilogue(d, X.infer_seed(B, Cin, Cout, H, R, stride))
    X.assert_exact_range(i["ibound"])
    assert i["ibound"] > d["bound"]
    X.assert_infer_epilogue(i["e"])
    if B >= 16:                                                    # (a window-loader stage case: stored outputs only, no statistics)
        return
    n = X.conv_case(B, Cin, Cout, H, H, R, stride, pad, NARROW, False)
    X.assert_exact_range(n["bound"])
    X.assert_resummed(n["y"])
    X.assert_resummed(X.rne_bf16(n["y"]).double())


@pytest.mark.parametrize("case", X.IGEMM_SHORTCUT)
def test_shortcut_cases(case):
    B, Cin, Cout, H, R, stride, pad, off = case
    assert R == 1 and pad == 0
    d = X.conv_infer_case(B, Cin, Cout, H, H, R, stride, pad, WIDE, off)
    X.assert_exact_range(d["ibound"])
    X.assert_infer_epilogue(d["e"])
    v = d["e"]["v"]
    X.assert_wide_shares(v)                                         # the shortcut stores v itself, negatives included
    assert float(v.min()) < -256 and float(d["e"]["bias"].min()) < 0 < float(d["e"]["bias"].max())


def test_infer_epilogue_orders_on_hand_picked_values():
    """The three expectations on values where each rounding and the ReLU's place can be read off by hand (bf16)."""
    v = torch.tensor([[257.0, 259.0, -300.0, 100.0, 513.0]], dtype=torch.float64)
    add = torch.tensor([[2.0, -400.0, 400.0, -100.0, -2.0]], dtype=torch.float64)
    e = dict(v=v, add=add)
    assert X.conv1_expect(e, X.BF).tolist() == [[256.0, 260.0, 0.0, 100.0, 512.0]]
    assert X.shortcut_expect(e, X.BF).tolist() == [[256.0, 260.0, -300.0, 100.0, 512.0]]
    # 257 -> 256, + 2 = 258 (exact); 259 -> 260, - 400 < 0 -> 0; -300 + 400 = 100 (a ReLU before the addend gives 400);
    # 100 - 100 = 0; 513 -> 512, - 2 = 510 (one rounding of 511 would give 512)
    assert X.conv2_expect(e, X.BF).tolist() == [[258.0, 0.0, 100.0, 0.0, 510.0]]
    assert X.relu_before_addend(e, X.BF).tolist() == [[258.0, -140.0, 400.0, 0.0, 510.0]]
    assert X.conv2_expect(e, torch.float32).tolist() == [[259.0, 0.0, 100.0, 0.0, 511.0]]
    assert X.sign_flip_shares(e) == (0.2, 0.2)


def test_linear_scalar_relu2_case():
    M, Kin, N, off = X.LINEAR_SCALAR_RELU2
    assert (M, Kin, N, off) in X.LINEARS and N % 8 != 0 and N % 4 != 0           # neither the bf16 nor the fp32 vector width divides N
    d = X.linear_relu2_case(M, Kin, N, WIDE, off)
    X.assert_exact_range(d["ibound"])
    X.assert_infer_epilogue(d["e"])


@pytest.mark.parametrize("case", X.LINEARS)
def test_linear_cases(case):
    M, Kin, N, off = case
    d = X.linear_case(M, Kin, N, WIDE, off)
    X.assert_exact_range(d["bound"])
    X.assert_wide_shares(d["pre"])
    assert float((d["pre"] == 0).double().mean()) >= 0.02 and float(d["bias"].min()) < 0        # ReLU clips, the bias has both signs


def test_stem_cases():
    for H, W in [(X.STEM_LOADER_HW,) * 2] + X.STEM_CONV_HW:
        d = X.stem_case(3, H, W, WIDE)
        X.assert_exact_range(d["bound"])
        X.assert_wide_shares(d["y"])
    for H, W in X.STEM_POOL_HW:                                       # the shares of the value that is compared: the pooled activation
        d = X.stem_pool_case(3, H, W)
        X.assert_exact_range(d["bound"])
        X.assert_wide_shares(d["pooled"])
        assert 0.1 <= float((d["pooled"] == 0).double().mean()) <= 0.7          # ReLU clips, and not everything
    for H, W in X.STEM_WGRAD_HW:
        X.assert_exact_range(X.stem_wgrad_case(3, H, W)["bound"])
    d = X.stem_dgrad_case(2, *X.STEM_DGRAD_HW)
    X.assert_exact_range(d["bound"])
    assert float(d["dimg"].abs().max()) <= d["bound"]


@pytest.mark.parametrize("case", X.CONV8P)
def test_conv8p_cases(case):
    B, H, W, C, N = case
    d = X.conv_case(B, C, N, H, W, 3, 1, 1, WIDE)
    t = X.transposed8p_case(B, H, W, C, N, WIDE)
    for v in (d, t):
        X.assert_exact_range(v["bound"] + 8 * WIDE[0])
        X.assert_wide_shares(v["y"])
    n = X.conv_case(B, C, N, H, W, 3, 1, 1, NARROW)
    X.assert_exact_range(n["bound"])
    X.assert_resummed(X.rne_bf16(n["y"]).double())
    r = X.bnred8p_case(B, H, W, C, N)
    X.assert_exact_range(r["bound"])
    for form, (g, sums, bound) in r["forms"].items():
        X.assert_exact_range(bound)
        assert torch.equal(sums * 2, (sums * 2).round()) and (form == "dual") == bool(sums[2].abs().max() > 0)


@pytest.mark.parametrize("case", X.CONV8P_S2)
def test_conv8p_stride2_cases(case):
    B, H, W, C, N = case
    d = X.conv_case(B, C, N, H, W, 3, 2, 1, WIDE)
    X.assert_exact_range(d["bound"])
    X.assert_wide_shares(d["y"])
    n = X.conv_case(B, C, N, H, W, 3, 2, 1, NARROW)
    X.assert_resummed(X.rne_bf16(n["y"]).double())


@pytest.mark.parametrize("case", X.C64P)
def test_c64p_cases(case):
    B, H, W = case
    d = X.conv_case(B, 64, 64, H, W, 3, 1, 1, WIDE, want_dgrad=True)
    X.assert_exact_range(d["bound"] + 8 * WIDE[0])
    X.assert_wide_shares(d["y"])
    X.assert_wide_shares(d["dx"])
    n = X.c64p_narrow_case(B, H, W)
    X.assert_exact_range(max(n["bound"], n["dbound"]))
    X.assert_resummed(n["y"])
    X.assert_exact_range(n["sums_bound"])


@pytest.mark.parametrize("case", X.WGRAD_PLAN, ids=["%dx%d-%d-r%ds%d" % (c[1], c[2], c[3], c[4], c[5]) for c in X.WGRAD_PLAN])
def test_wgrad_plan_cases(case):
    """dw += dy^T gather(x) over M rows, both operands in the narrow activation range, into a prefilled buffer."""
    d = X.wgrad_plan_case(case)
    X.assert_exact_range(d["bound"])
    assert float(d["dw0"].abs().max()) > 0


def test_other_weight_gradient_cases():
    for B, H, W in X.WGRAD_C64:
        d = X.wgrad_c64_case(B, H, W)
        X.assert_exact_range(max(d["bound"], d["bound_bn"]))
        assert torch.equal(d["xin"] * 2, (d["xin"] * 2).round()) and float(d["xin"].min()) == 0 and float(d["xin"].max()) > 2
    for B in X.WGRAD_C128_B:
        X.assert_exact_range(X.wgrad_c128_case(B)["bound"])
    for i in range(len(X.WGRAD_GROUP)):
        X.assert_exact_range(X.wgrad_group_case(i)["bound"])


@pytest.mark.parametrize("case", X.DGRAD_S2)
def test_dgrad_s2_cases(case):
    d = X.dgrad_s2_case(*case, WIDE)
    X.assert_exact_range(d["bound"])
    X.assert_wide_shares(d["dx"])


def test_linear_dgrad_act_case():
    d = X.linear_dgrad_case(*X.LINEAR_DGRAD_ACT, WIDE)
    X.assert_exact_range(d["bound"])
    X.assert_wide_shares(d["y"])
