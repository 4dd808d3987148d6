"""The fp64 references of tests/_bnref.py, validated without a GPU: the closed forms against torch fp64 autograd for the three
residual-block patterns, the accumulator encoder / decoder against exact integer arithmetic, the host mirrors of the launch
geometry, everything the GPU tests of test_gpu_batchnorm_fp64.py presuppose about their seeded inputs (self-mask margins, special
channels, grid coverage) -- and the teeth of the bounds: each of ten deliberately wrong formulas, evaluated in fp64 on the same
generated inputs, misses the bound it is held to by at least 10x in at least one case."""
import pytest
import torch

import _bnref as R

SMALL_CASES = [c for c in R.ROW_CASES if c[2] <= 300]


# ------------------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("pattern", ["res", "dual", "eval"])
@pytest.mark.parametrize("C,rows", [(8, 37), (64, 5), (16, 197)])
def test_closed_forms_equal_fp64_autograd(pattern, C, rows):
    o, _ = R.chain_operands(pattern, R.F32, C, rows)
    kw = R.block_kwargs(pattern, o)
    a, c = R.block_autograd(pattern, **kw), R.block_closed_form(pattern, **kw)
    keys = ["out", "dy", "dgamma", "dbeta"] + {"res": ["dres"], "dual": ["dy2", "dgamma2", "dbeta2"], "eval": []}[pattern]
    for k in keys:
        scale = float(a[k].abs().max()) + 1e-300
        assert float((a[k] - c[k]).abs().max()) <= 1e-11 * scale + 1e-13, k
    assert bool((c["g"] == 0).any()) and bool((c["g"] != 0).any())              # the mask masks


@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=R.case_id)
def test_chain_operands_keep_every_relu_sign_far_from_rounding(case):
    pattern, d, C = case
    o, margin = R.chain_operands(pattern, R.DT[d], C)
    assert margin > 64
    kw = R.block_kwargs(pattern, o)
    c = R.block_closed_form(pattern, **kw)
    share = float((c["out"] > 0).double().mean())
    assert 0.2 < share < 0.8


# ------------------------------------------------------------------------------------------------------------ launch geometry
def test_row_cases_cover_the_lane_splits_replicas_and_grid_caps():
    lr = {R.lanes_r(C, R.DT[d]) for d, C, _ in R.ROW_CASES}
    assert {256, 32, 16, 4, 2, 1} <= lr
    assert {R.replicas(C) for _, C, _ in R.ROW_CASES} == {8, 4, 2, 1}
    grid = lambda rows, l: (rows + l - 1) // l
    passes = lambda d, C, rows, cap: grid(rows, R.lanes_r(C, R.DT[d])) > cap
    assert passes("fp32", 512, 16387, 8192) and passes("bf16", 2048, 8195, 8192)            # row_grid of bn_apply / bn_bwd_apply
    assert ("fp32", 512, 16387) in R.ROW_CASES and ("bf16", 2048, 8195) in R.ROW_CASES
    assert passes("bf16", 64, 65541, 1024) and passes("bf16", 64, 65541, 512)               # bn_apply_acc / bn_bwd_apply_acc
    assert R.bwd_blocks(8229) == 129 and R.bwd_blocks(65541) == 512 and R.bwd_blocks(65535) == 256
    assert 129 * 32 < 8229 and 512 * 32 < 65541                                              # bn_bwd_reduce strides at both
    assert ("bf16", 64, 8229) in R.ROW_CASES and ("bf16", 64, 65541) in R.ROW_CASES
    for d, C, rows in R.ROW_CASES:
        assert rows * C * (2 if d == "bf16" else 4) <= 34 * 2 ** 20
    for d, C, B, HW in R.pool_cases():
        assert B * HW * C * (2 if d == "bf16" else 4) <= 34 * 2 ** 20
    ch = {R.pool_chunks(HW, C, R.DT[d]) for d, C, B, HW in R.pool_cases()}
    assert 1 in ch and max(ch) >= 14
    assert R.acc_words(2, 64) == 2 * 8 * 2 * 64 + 2 and R.acc_words(3, 2048) == 2 * 3 * 2048 + 2
    G = [min(64, (t + 63) // 64) for t in R.STATS_TILES]
    assert {1, 2, 5, 64} <= set(G)


# ---------------------------------------------------------------------------------------------------------------- accumulator
def _acc_parts(kind, P, K, C, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":                      # both signs, |v| from 2^-20 up: every value a multiple of 2^-50
        v = (torch.randn(P, K, C, generator=g) * 10.0 ** torch.randint(-3, 4, (P, K, C), generator=g).float()).float()
        v = torch.where(v.abs() < 2.0 ** -20, torch.full_like(v, -0.37), v)
    elif kind == "lo_zero":                   # multiples of 1/16: the lo plane stays empty
        v = torch.randint(-2 ** 20, 2 ** 20, (P, K, C), generator=g).float() / 16
    elif kind == "dyadic":                    # k / 2^12: hi and lo both used, every partial sum exact in fp64
        v = torch.randint(-2 ** 22, 2 ** 22, (P, K, C), generator=g).float() / 4096
    else:                                     # just under the range limit 2^41, both signs, and small values among them
        big = 2.0 ** 41 * (1 - 2.0 ** -24)
        v = torch.where(torch.rand(P, K, C, generator=g) < 0.5, torch.tensor(big), torch.tensor(-big))
        v[::3] = torch.randn(v[::3].shape, generator=g)
        v = torch.where(v.abs() < 2.0 ** -20, torch.full_like(v, 0.61), v)
        v[0, 0, 0], v[1 % P, 0, 0] = big, big
    return v.contiguous()


@pytest.mark.parametrize("kind", ["random", "lo_zero", "dyadic", "limit"])
@pytest.mark.parametrize("K,C,P", [(2, 8, 1), (2, 64, 37), (3, 512, 5), (3, 2048, 3), (2, 100, 64)])
def test_accumulator_round_trip_is_exact(kind, K, C, P):
    parts = _acc_parts(kind, P, K, C, seed=K * C + P)
    assert bool((parts.abs() < 2.0 ** 41).all())
    rep = R.uneven_replicas(P, C, seed=P)
    acc = R.acc_encode(parts, rep, K, C)
    assert acc.numel() == R.acc_words(K, C)
    hi, lo, flag = R.acc_planes(acc, K, C)
    assert flag == 0
    assert R.acc_total_exact(acc, K, C) == R.parts_total_exact(parts)            # integers: exactly the sum of the partials
    if kind == "lo_zero":
        assert int(lo.abs().sum()) == 0
    else:
        assert int(lo.abs().sum()) > 0
    if P * K * C > 8:
        assert bool((hi < 0).any())                                              # two's-complement negatives in the planes
    dec, _ = R.acc_decode(acc, K, C)
    want = parts.double().sum(0)
    if kind in ("lo_zero", "dyadic"):
        assert torch.equal(dec, want)                                            # the fp64 sum is exact here, and so is the decode
    else:                                                                        # > 53 bits: both round, each at most once or twice
        exact = torch.tensor([float(t) for t in R.parts_total_exact(parts)], dtype=torch.float64).view(K, C) / 2.0 ** 50
        assert bool(((dec - exact).abs() <= 2.0 ** -51 * parts.double().abs().sum(0)).all())


def test_accumulator_flag_word_counts_what_leaves_the_range():
    parts = torch.tensor([1.5, 2.0 ** 41, float("nan"), float("-inf"), -2.0 ** 40]).view(5, 1, 1).repeat(1, 2, 8)
    acc = R.acc_encode(parts, torch.zeros(5, dtype=torch.long), 2, 8)
    dec, flag = R.acc_decode(acc, 2, 8)
    assert flag == 3 * 16
    assert torch.equal(dec, torch.full((2, 8), 1.5 - 2.0 ** 40, dtype=torch.float64))


# ------------------------------------------------------------------------------------- what the GPU tests presuppose about inputs
@pytest.mark.parametrize("case", R.ROW_CASES, ids=R.case_id)
def test_self_mask_preactivations_lie_outside_the_forward_bound(case):
    d, C, rows = case
    op = R.bwd_operands(R.DT[d], C, rows, R.seed_of("bwd", d, C, rows))
    assert R.self_margin(op) > 1.0
    oa = op["outact"]
    assert float(oa[0, 0]) == 0.0 and float(oa[0, 1]) == R.FLT_MIN and float(oa[0, 1]) > 0
    assert float(oa[-1, -1]) == 0.0 and bool(torch.signbit(oa[-1, -1]))          # -0.0 survived the storage dtype
    assert float(oa.min()) >= 0.0
    if rows * C >= 64:
        assert bool((oa == 0).any()) and bool((oa > 0).any())


@pytest.mark.parametrize("tiles", R.STATS_TILES)
def test_stats_operands_hold_their_special_channels(tiles):
    part, count, gamma, beta, rm, rv = R.stats_operands(tiles, 64, R.seed_of("stats", tiles, 64))
    (s, q), (d_s, d_q) = zip(*[R.slab_sums(part[:, k]) for k in (0, 1)])
    ref, bnd = R.coef_ref(s, q, d_s, d_q, count, gamma, beta, rm, rv)
    mean, inv = ref["coef"][2], ref["coef"][3]
    assert float(ref["var"][0]) == 0.0 and abs(float(inv[0]) - R.EPS ** -0.5) < 1e-9 * R.EPS ** -0.5
    if count > 2:
        assert 300 < float(mean[1].abs() * inv[1]) < 3000
    assert float(ref["coef"][0][2]) == 0.0 and float(gamma[2]) == 0.0 and float(beta[3]) == 0.0
    assert bool((bnd["coef"] < 1e-3 * ref["coef"].abs() + 1e-4).all())           # the bounds stay rounding-sized


# --------------------------------------------------------------------------------------------------------------------- mutants
def _worst(err, bound):
    return float((err / bound.clamp(min=1e-300)).max())


def test_mutant_shortcut_shift_dropped():
    worst = 0.0
    for d, C, rows in SMALL_CASES:
        op = R.fwd_operands(R.DT[d], C, rows, R.seed_of("fwd", d, C, rows))
        a = (op["y"], op["coef"][0], op["coef"][1], op["res"], op["rcoef"][0], op["rcoef"][1])
        ref, _ = R.apply_ref(*a)
        bad, _ = R.apply_ref(*a, drop_rshift=True)
        worst = max(worst, _worst((bad - ref).abs(), R.store_bound(R.apply_bound(*a), ref, R.DT[d])))
    assert worst >= 10


def _reduce_bound(op, mode, dual):
    g = R.bwd_g(op, mode)
    s, a = R.bwd_sums(g, op, dual)
    tol = torch.stack([R.units_bound(R.bwd_sums_fp32(op, mode, dual)[k], s[k], a[k])[0] for k in range(3)])
    return s, tol


def test_mutant_mask_greater_or_equal():
    worst = 0.0
    for d, C, rows in SMALL_CASES:
        op = R.bwd_operands(R.DT[d], C, rows, R.seed_of("bwd", d, C, rows))
        s, tol = _reduce_bound(op, "outact", False)
        bad, _ = R.bwd_sums(R.bwd_g(op, "outact", ge=True), op, False)
        worst = max(worst, _worst((bad - s).abs()[:2], tol[:2]))
    assert worst >= 10


def test_mutants_last_row_and_last_channel_vector_skipped():
    w_row = w_vec = 0.0
    for d, C, rows in SMALL_CASES:
        op = R.bwd_operands(R.DT[d], C, rows, R.seed_of("bwd", d, C, rows))
        s, tol = _reduce_bound(op, "none", True)
        g = R.bwd_g(op, "none")
        w_row = max(w_row, _worst((R.bwd_sums(g, op, True, skip_last_row=True)[0] - s).abs(), tol))
        w_vec = max(w_vec, _worst((R.bwd_sums(g, op, True, skip_last_vec=R.VEC[R.DT[d]])[0] - s).abs(), tol))
        # the forward: an element never written keeps the sentinel
        fo = R.fwd_operands(R.DT[d], C, rows, R.seed_of("fwd", d, C, rows))
        ref, _ = R.apply_ref(fo["y"], fo["coef"][0], fo["coef"][1])
        bound = R.store_bound(R.apply_bound(fo["y"], fo["coef"][0], fo["coef"][1]), ref, R.DT[d])
        assert _worst((ref[-1] - R.SENT).abs(), bound[-1]) >= 10 and _worst((ref[:, -1] - R.SENT).abs(), bound[:, -1]) >= 10
    assert w_row >= 10 and w_vec >= 10


def test_mutants_of_the_backward_coefficients():
    """which 1 / 2 swapped, the -mg term of bcoef[2] dropped, count - 1 for count"""
    w_swap = w_mg = w_cnt = 0.0
    for nblk in R.FINALIZE_NBLK:
        C = 64
        slab, gamma, coef = R.slab_operands(nblk, C, R.seed_of("slab", nblk, C))
        s, d_s = R.slab_sums(slab)
        count = float(nblk * 7 + 2)
        for which in (1, 2):
            ref, bnd = R.bc_ref(s[0], s[which], count, gamma, coef, True), R.bc_bound(s[0], s[which], count, gamma, coef, True, d_s[0], d_s[which])
            other = R.bc_ref(s[0], s[3 - which], count, gamma, coef, True)
            w_swap = max(w_swap, _worst((other - ref).abs()[1:], bnd[1:]),
                         _worst((s[3 - which] - s[which]).abs(), R.grad_add_bound(s[which], 0.5, d_s[which])))
            w_mg = max(w_mg, _worst((R.bc_ref(s[0], s[which], count, gamma, coef, True, drop_mg=True) - ref).abs()[2], bnd[2]))
            w_cnt = max(w_cnt, _worst((R.bc_ref(s[0], s[which], count, gamma, coef, True, count_off=1) - ref).abs()[1:], bnd[1:]))
    assert w_swap >= 10 and w_mg >= 10 and w_cnt >= 10


def test_mutant_biased_running_variance():
    worst = 0.0
    for tiles in R.STATS_TILES:
        part, count, gamma, beta, rm, rv = R.stats_operands(tiles, 64, R.seed_of("stats", tiles, 64))
        (s, q), (d_s, d_q) = zip(*[R.slab_sums(part[:, k]) for k in (0, 1)])
        ref, bnd = R.coef_ref(s, q, d_s, d_q, count, gamma, beta, rm, rv)
        bad, _ = R.coef_ref(s, q, d_s, d_q, count, gamma, beta, rm, rv, unbiased=False)
        worst = max(worst, _worst((bad["rv"] - ref["rv"]).abs(), bnd["rv"]))
    assert worst >= 10


def test_mutants_of_the_decoder():
    """one replica ignored, the lo plane ignored: judged by the bound of the statistics the decoded sums feed (exact sums:
    d_s = d_q = 0, so what remains is the fp32 rounding of the coefficients)"""
    w_rep = w_lo = 0.0
    for d, C, rows in [("bf16", 64, 197), ("fp32", 512, 37), ("bf16", 8, 257)]:
        y = R.fwd_operands(R.DT[d], C, rows, R.seed_of("fwd", d, C, rows))["y"]
        parts = R.stat_partials(y, 9)
        acc = R.acc_encode(parts, R.uneven_replicas(parts.shape[0], C, 3), 2, C)
        gamma, beta, zero = torch.ones(C), torch.zeros(C), torch.zeros(C, dtype=torch.float64)
        (s, q), _ = R.acc_decode(acc, 2, C)
        ref, bnd = R.coef_ref(s, q, zero, zero, float(rows), gamma, beta, acc=True)
        for kw, name in (({"skip_replica": R.replicas(C) - 1}, "rep"), ({"use_lo": False}, "lo")):
            (s1, q1), _ = R.acc_decode(acc, 2, C, **kw)
            bad, _ = R.coef_ref(s1, q1, zero, zero, float(rows), gamma, beta, acc=True)
            w = _worst((bad["coef"] - ref["coef"]).abs(), bnd["coef"])
            if name == "rep":
                w_rep = max(w_rep, w)
            else:
                w_lo = max(w_lo, w)
    assert w_rep >= 10 and w_lo >= 10
