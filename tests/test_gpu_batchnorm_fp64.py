"""GPU: the BatchNorm kernels of the residual blocks -- vqa_bn_stats_finalize, vqa_bn_eval_coef, vqa_bn_apply, vqa_bn_apply_pool,
vqa_bn_apply_acc (bn_acc_coef and the fixed-point accumulator of csrc/common.h), vqa_bn_bwd_reduce (slab and accumulator),
vqa_bn_bwd_finalize, vqa_bn_bwd_apply, vqa_bn_bwd_apply_acc -- through the C ABI against the float64 references of
tests/_bnref.py (validated without a GPU in test_bn_ref_cpu.py), never against a sibling kernel.  The bounds are those of
_bnref's docstring: per element / per channel, counted from the kernels' own expressions; reductions 8x the fp32 CPU error in units
of the sum of magnitudes, floor 2^-24.  Every output buffer is pre-filled with a sentinel and carries a guard row: every element
must be written and nothing past the end.  Accumulators are fed from the host encoder (partials spread unevenly over the replicas)
and what vqa_bn_bwd_reduce(acc_mode = 1) wrote is decoded on the host, so no producer kernel stands between a kernel and fp64."""
import pytest
import torch

import _bnref as R
from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
EARG = 1000


def _d(t):
    return None if t is None else t.contiguous().to(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


_KEEP = []


def K(t):
    """device pointer of a host tensor's device copy (None -> NULL); the copy lives until the test ends"""
    if t is None:
        return None
    _KEEP.append(_d(t))
    return _KEEP[-1].data_ptr()


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                       # a faulted device: start nothing more on it
        pytest.exit(f"the GPU reported an error, nothing more is started: {e}", returncode=3)
    _KEEP.clear()


def _guarded(rows, C, dtype=F32, fill=R.SENT):
    return torch.full((rows + 1, C), fill, device=DEV, dtype=dtype)


def _written(buf, rows, what=""):
    """host copy of the first `rows` rows: all of them written, the guard row untouched"""
    torch.cuda.synchronize()
    h = buf.cpu()
    assert bool((h[rows:] == R.SENT).all()), f"{what}: written past the end"
    assert bool((h[:rows] != R.SENT).all()), f"{what}: {int((h[:rows] == R.SENT).sum())} elements never written"
    return h[:rows]


def _untouched(buf):
    torch.cuda.synchronize()
    return bool((buf.cpu() == R.SENT).all())


def _rc(name, *args):
    """status of an entry point (no exception)"""
    L = sub("_lib")
    return getattr(L.lib(), name)(*args, L.stream())


def _ratio(err, bound):
    return float((err / bound.clamp(min=1e-300)).max())


def _check(tag, got, ref, bound):
    """every entry within its bound -> the worst err / bound.  The fp64 evaluation of reference and bound carries its own rounding
    (it moves with the CPU's thread count): bound (1 + 2^-30) + 2^-45 |ref|, five orders below one fp32 rounding."""
    bound = bound * (1 + 2.0 ** -30) + 2.0 ** -45 * ref.abs()
    err = (got.double() - ref).abs()
    r = _ratio(err, bound)
    assert bool((err <= bound).all()), f"{tag}: worst err / bound {r:.3f} at {int((err / bound.clamp(min=1e-300)).argmax())}"
    return r


def test_host_mirrors_of_the_launch_geometry_match_the_library():
    L = sub("_lib")
    for d, C, rows in R.ROW_CASES:
        assert L.count("vqa_bn_bwd_blocks", rows) == R.bwd_blocks(rows)
        for K in (2, 3):
            assert L.count("vqa_bn_acc_words", K, C) == R.acc_words(K, C)
    for d, C, B, HW in R.pool_cases():
        assert L.count("vqa_bn_apply_pool_chunks", L.dt(R.DT[d]), HW, C) == R.pool_chunks(HW, C, R.DT[d])
    assert L.count("vqa_bn_apply_pool_chunks", 1, 49, 96) == 0


# ------------------------------------------------------------------------------------------------------------------ statistics
def _stats_finalize(part, count, gamma, beta, rm, rv):
    L = sub("_lib")
    T, _, C = part.shape
    coef, scratch = _guarded(4, C), torch.empty(64 * 2 * C, device=DEV, dtype=torch.float64)
    run = _guarded(2, C)
    nbt = torch.tensor([41, 7], device=DEV, dtype=torch.int64)
    if rm is not None:
        run[0], run[1] = _d(rm), _d(rv)
    L.call("vqa_bn_stats_finalize", K(part), T, C, count, K(gamma), K(beta),
           run[0].data_ptr() if rm is not None else None, run[1].data_ptr() if rm is not None else None,
           nbt.data_ptr() if rm is not None else None, 0.1, 1e-5, scratch.data_ptr(), coef.data_ptr())
    coef_h = _written(coef, 4, "coef")
    return coef_h, (_written(run, 2, "running") if rm is not None else run), nbt.cpu().tolist()


def _stats_reference(part, count, gamma, beta, rm, rv):
    (s, q), (d_s, d_q) = zip(*[R.slab_sums(part[:, k]) for k in (0, 1)])
    return R.coef_ref(s, q, d_s, d_q, count, gamma, beta, rm, rv)


@pytest.mark.parametrize("C", R.STATS_CHANNELS)
@pytest.mark.parametrize("tiles", R.STATS_TILES)
def test_stats_finalize_matches_fp64(tiles, C):
    """Measured on MI355X: worst err / bound over the 28 cases coef 0.60 ... 0.99, running statistics 0.34 ... 0.74."""
    part, count, gamma, beta, rm, rv = R.stats_operands(tiles, C, R.seed_of("stats", tiles, C))
    ref, bnd = _stats_reference(part, count, gamma, beta, rm, rv)
    coef, run, nbt = _stats_finalize(part, count, gamma, beta, rm, rv)
    r1 = _check("coef", coef, ref["coef"], bnd["coef"])
    r2 = max(_check("running mean", run[0], ref["rm"], bnd["rm"]), _check("running var", run[1], ref["rv"], bnd["rv"]))
    assert nbt == [42, 7]
    assert float(coef[0][2]) == 0.0                                        # gamma == 0: scale exactly 0
    # all running-statistics pointers NULL: the same coefficients, nothing else written
    coef0, run0, nbt0 = _stats_finalize(part, count, gamma, beta, None, None)
    assert torch.equal(coef0, coef) and _untouched(run0) and nbt0 == [41, 7]
    print(f"stats tiles {tiles} C {C}: worst err / bound coef {r1:.3f} running {r2:.3f}")


@pytest.mark.parametrize("C", [8, 100])
def test_stats_finalize_at_count_one_keeps_the_biased_variance(C):
    """count = 1: var = 0 in every channel, invstd = eps^-1/2, unbiased factor 1 (no division by count - 1 = 0).
    Measured on MI355X: worst err / bound 0.70 (C = 8), 0.81 (C = 100)."""
    part, count, gamma, beta, rm, rv = R.stats_operands(1, C, R.seed_of("stats1", C), per_tile=1)
    assert count == 1.0
    ref, bnd = _stats_reference(part, count, gamma, beta, rm, rv)
    coef, run, nbt = _stats_finalize(part, count, gamma, beta, rm, rv)
    assert bool(torch.isfinite(coef).all()) and bool(torch.isfinite(run).all())
    r = max(_check("coef", coef, ref["coef"], bnd["coef"]), _check("running mean", run[0], ref["rm"], bnd["rm"]),
            _check("running var", run[1], ref["rv"], bnd["rv"]))
    print(f"stats count 1 C {C}: worst err / bound {r:.3f}")


@pytest.mark.parametrize("C", R.STATS_CHANNELS)
def test_eval_coef_matches_fp64(C):
    """Measured on MI355X: worst err / bound 0.34 ... 0.52."""
    L = sub("_lib")
    _, _, gamma, beta, rm, rv = R.stats_operands(3, C, R.seed_of("eval", C))
    rv[0], rv[1], rm[1] = 0.0, 1e-6, 1000.0                                  # running_var = 0; a large mean over a small variance
    ref, bnd = R.eval_coef_ref(gamma, beta, rm, rv)
    coef = _guarded(4, C)
    L.call("vqa_bn_eval_coef", C, K(gamma), K(beta), K(rm), K(rv), 1e-5, coef.data_ptr())
    got = _written(coef, 4, "coef")
    r = _check("eval coef", got, ref, bnd)
    assert float(got[0][2]) == 0.0 and torch.equal(got[2], rm)
    print(f"eval coef C {C}: worst err / bound {r:.3f}")


# --------------------------------------------------------------------------------------------------------------------- forward
def _apply(dtype, op, mode, relu, rows, C):
    L = sub("_lib")
    res, rs, _ = R.fwd_mode_args(op, mode)
    out = _guarded(rows, C, dtype)
    L.call("vqa_bn_apply", L.dt(dtype), K(op["y"]), K(op["coef"]), K(res),
           K(op["rcoef"]) if rs is not None else None, out.data_ptr(), rows * C, C, relu)
    return _written(out, rows, f"out {mode}")


def _fwd_reference(op, mode, relu, dtype):
    res, rs, rh = R.fwd_mode_args(op, mode)
    ref, _ = R.apply_ref(op["y"], op["coef"][0], op["coef"][1], res, rs, rh, relu)
    return ref, R.store_bound(R.apply_bound(op["y"], op["coef"][0], op["coef"][1], res, rs, rh), ref, dtype)


@pytest.mark.parametrize("case", R.ROW_CASES, ids=R.case_id)
def test_apply_matches_fp64_in_every_mode(case):
    """vqa_bn_apply, rcoef in fp32: exact operands bit-equal, random operands within the bound, three residual modes x relu on / off
    (two combinations at the rows past the grid cap).  Measured on MI355X, random operands: worst err / bound 0.23 ... 0.64
    (fp32), 0.92 ... 0.996 (bf16: the final rounding, which 2^-8 |ref| describes tightly)."""
    d, C, rows = case
    dtype = R.DT[d]
    big = rows * C > 2 ** 20
    combos = [("bn", 1), ("add", 0)] if big else [(m, r) for m in R.RES_MODES for r in (1, 0)]
    worst = 0.0
    for exact in (True, False):
        op = R.fwd_operands(dtype, C, rows, R.seed_of("fwd", d, C, rows), exact=exact)
        for mode, relu in combos[:1] if (big and exact) else combos:
            out = _apply(dtype, op, mode, relu, rows, C)
            ref, bound = _fwd_reference(op, mode, relu, dtype)
            if exact:
                assert torch.equal(ref.float().double(), ref)
                assert torch.equal(out, R.stored(ref, dtype)), f"exact {mode} relu {relu}: {int((out != R.stored(ref, dtype)).sum())} differ"
            else:
                worst = max(worst, _check(f"apply {mode} relu {relu}", out, ref, bound))
    print(f"apply {R.case_id(case)}: worst err / bound {worst:.3f}")


def _acc_of(y, C, seed, P=9):
    parts = R.stat_partials(y, min(P, y.shape[0]))
    acc = R.acc_encode(parts, R.uneven_replicas(parts.shape[0], C, seed), 2, C)
    (s, q), flag = R.acc_decode(acc, 2, C)
    assert flag == 0
    return acc, s, q


def _apply_acc(dtype, y, acc, gamma, beta, rm, rv, res, racc, rgamma, rbeta, rrm, rrv, B, HW, C, relu, pool=False):
    """vqa_bn_apply_acc on host operands -> dict of host results"""
    L = sub("_lib")
    rows = B * HW
    out, coef, rcoef, run, rrun = _guarded(rows, C, dtype), _guarded(4, C), _guarded(4, C), _guarded(2, C), _guarded(2, C)
    run[0], run[1] = _d(rm), _d(rv)
    nbt = torch.tensor([41, 7, 13], device=DEV, dtype=torch.int64)
    if racc is not None:
        rrun[0], rrun[1] = _d(rrm), _d(rrv)
    chunks = R.pool_chunks(HW, C, dtype)
    part = _guarded(B * chunks, C) if pool else None
    a = K
    two = racc is not None
    L.call("vqa_bn_apply_acc", L.dt(dtype), a(y), a(acc), a(gamma), a(beta), run[0].data_ptr(), run[1].data_ptr(), nbt[0:].data_ptr(),
           coef.data_ptr(), a(res), a(racc), a(rgamma) if two else None, a(rbeta) if two else None,
           rrun[0].data_ptr() if two else None, rrun[1].data_ptr() if two else None, nbt[1:].data_ptr() if two else None,
           rcoef.data_ptr() if two else None, out.data_ptr(), B, HW, C, relu, float(rows), 0.1, 1e-5, _p(part))
    r = {"out": _written(out, rows, "out"), "coef": _written(coef, 4, "coef_out"), "run": _written(run, 2, "running")}
    if two:
        r["rcoef"], r["rrun"] = _written(rcoef, 4, "rcoef_out"), _written(rrun, 2, "shortcut running")
    else:
        assert _untouched(rcoef) and _untouched(rrun)
    if pool:
        r["part"] = _written(part, B * chunks, "pool part").view(B, chunks, C)
    r["nbt"] = nbt.cpu().tolist()
    return r


def _partial_rounding(y, P):
    """what the sums of P fp32 partials may differ by from the tensor's exact sums: half an ulp of every partial"""
    pa = R.stat_partials(y, min(P, y.shape[0])).double().abs().sum(0)
    return 2.0 ** -25 * pa[0], 2.0 ** -25 * pa[1]


def _acc_stats(y, C, gamma, beta, rm, rv, seed, of_tensor=False):
    """host-encoded accumulator of y's partial sums, reference and bound of the coefficients.  The reference takes the decoded sums
    (exactly what the kernel reads); of_tensor: the tensor's own fp64 sums instead, the partials' rounding in the bound."""
    acc, s, q = _acc_of(y, C, seed)
    d_s, d_q = 2.0 ** -52 * s.abs(), 2.0 ** -52 * q.abs()
    if of_tensor:
        r_s, r_q = _partial_rounding(y, 9)
        s, q, d_s, d_q = y.double().sum(0), (y.double() ** 2).sum(0), d_s + r_s, d_q + r_q
    ref, bnd = R.coef_ref(s, q, d_s, d_q, float(y.shape[0]), gamma, beta, rm, rv, acc=True)
    return acc, ref, bnd


def _acc_operands(dtype, C, rows, seed):
    op = R.fwd_operands(dtype, C, rows, seed)
    g = torch.Generator().manual_seed(seed + 1)
    y = (op["y"].float() * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g) * 0.5).to(dtype)
    v = lambda s=1.0: torch.randn(C, generator=g) * s
    p = {"y": y, "res": op["res"], "gamma": torch.rand(C, generator=g) + 0.5, "beta": v(0.3), "rgamma": -(torch.rand(C, generator=g) + 0.5),
         "rbeta": v(0.3), "rm": v(0.2), "rv": torch.rand(C, generator=g) + 0.5, "rrm": v(0.2), "rrv": torch.rand(C, generator=g) + 0.5}
    p["gamma"][2] = 0.0
    return p


@pytest.mark.parametrize("case", R.ROW_CASES, ids=R.case_id)
def test_apply_acc_matches_fp64_from_host_encoded_accumulators(case):
    """vqa_bn_apply_acc: the statistics arrive as fixed-point accumulators encoded on the host from fp32 partial sums of y (and of
    res for the shortcut BatchNorm), spread unevenly over the replicas; coefficients, running statistics, num_batches_tracked and
    the output against fp64.  The gamma == 0 channel's scale is exactly 0 and its shift exactly beta.
    Measured on MI355X: worst err / bound out 0.81 ... 0.996 (bf16) / 0.06 ... 0.47 (fp32), coefficients 0.34 ... 1.000 (at 3 rows of
    C = 512 in fp32 the stored mean of one channel: a single rounding of almost half an ulp just above a power of two), running statistics 0.30 ... 0.73."""
    d, C, rows = case
    dtype = R.DT[d]
    p = _acc_operands(dtype, C, rows, R.seed_of("acc", d, C, rows))
    acc, ref, bnd = _acc_stats(p["y"], C, p["gamma"], p["beta"], p["rm"], p["rv"], 5)
    racc, rref, rbnd = _acc_stats(p["res"], C, p["rgamma"], p["rbeta"], p["rrm"], p["rrv"], 6)
    big = rows * C > 2 ** 20
    w_out = w_coef = w_run = 0.0
    for mode, relu in ([("bn", 1), ("none", 0)] if big else [(m, r) for m in R.RES_MODES for r in (1, 0)]):
        two = mode == "bn"
        res = None if mode == "none" else p["res"]
        got = _apply_acc(dtype, p["y"], acc, p["gamma"], p["beta"], p["rm"], p["rv"], res, racc if two else None, p["rgamma"],
                         p["rbeta"], p["rrm"], p["rrv"], 1, rows, C, relu)
        w_coef = max(w_coef, _check("coef_out", got["coef"], ref["coef"], bnd["coef"]))
        w_run = max(w_run, _check("running mean", got["run"][0], ref["rm"], bnd["rm"]), _check("running var", got["run"][1], ref["rv"], bnd["rv"]))
        assert float(got["coef"][0][2]) == 0.0 and float(got["coef"][1][2]) == float(p["beta"][2])
        assert got["nbt"] == ([42, 8, 13] if two else [42, 7, 13])
        sc, sh = ref["coef"][0], ref["coef"][1]
        if two:
            w_coef = max(w_coef, _check("rcoef_out", got["rcoef"], rref["coef"], rbnd["coef"]))
            w_run = max(w_run, _check("shortcut running mean", got["rrun"][0], rref["rm"], rbnd["rm"]),
                        _check("shortcut running var", got["rrun"][1], rref["rv"], rbnd["rv"]))
            a = (p["y"], sc, sh, res, rref["coef"][0], rref["coef"][1])
            e = R.apply_bound(*a, d=bnd["coef"][:2], dr=rbnd["coef"][:2])
        else:
            a = (p["y"], sc, sh, res, None, None)
            e = R.apply_bound(*a, d=bnd["coef"][:2])
        want, _ = R.apply_ref(*a, relu=relu)
        w_out = max(w_out, _check(f"out {mode} relu {relu}", got["out"], want, R.store_bound(e, want, dtype)))
        if mode == "none":                                                   # gamma == 0: out = [relu](beta), exactly
            b2 = p["beta"][2].double()
            assert bool((got["out"][:, 2] == R.stored(b2.clamp(min=0) if relu else b2, dtype)).all())
    print(f"apply_acc {R.case_id(case)}: worst err / bound out {w_out:.3f} coef {w_coef:.3f} running {w_run:.3f}")


@pytest.mark.parametrize("case", R.pool_cases(), ids=R.case_id)
def test_apply_pool_writes_the_column_sums_of_what_it_stored(case):
    """vqa_bn_apply_pool and vqa_bn_apply_acc(pool_part): the output as vqa_bn_apply's, and part[b][chunk][c] = the sum of the
    STORED outputs of rows [chunk rpc, (chunk + 1) rpc) of sample b -- bit-equal on exact operands, within the reduction bound on
    random ones.  Measured on MI355X: worst err / bound out 0.63 ... 0.996 (bf16) / 0.36 ... 0.64 (fp32), pooling sums 0 ... 0.37."""
    L = sub("_lib")
    d, C, B, HW = case
    dtype = R.DT[d]
    rows, chunks = B * HW, R.pool_chunks(HW, C, dtype)
    w_out = w_sum = 0.0
    for exact in (True, False):
        op = R.fwd_operands(dtype, C, rows, R.seed_of("pool", d, C, B, HW), exact=exact)
        for mode, relu in [("none", 1), ("add", 1), ("bn", 1), ("bn", 0)]:
            res, rs, _ = R.fwd_mode_args(op, mode)
            out, part = _guarded(rows, C, dtype), _guarded(B * chunks, C)
            L.call("vqa_bn_apply_pool", L.dt(dtype), K(op["y"]), K(op["coef"]), K(res),
                   K(op["rcoef"]) if rs is not None else None, out.data_ptr(), B, HW, C, relu, part.data_ptr())
            out_h, part_h = _written(out, rows, "out"), _written(part, B * chunks, "part").view(B, chunks, C)
            ref, bound = _fwd_reference(op, mode, relu, dtype)
            if exact:
                assert torch.equal(out_h, R.stored(ref, dtype))
                sums, _, _ = R.pool_ref(R.stored(ref, dtype), B, HW, C, dtype)
                assert torch.equal(part_h.double(), sums)
            else:
                w_out = max(w_out, _check(f"pool out {mode}", out_h, ref, bound))
                sums, mags, cpu32 = R.pool_ref(out_h, B, HW, C, dtype)
                tol, _ = R.units_bound(cpu32, sums, mags)
                w_sum = max(w_sum, _check(f"pool sums {mode}", part_h, sums, tol.clamp(min=1e-300)))
    # the accumulator-fed variant: same geometry, coefficients from host-encoded statistics
    p = _acc_operands(dtype, C, rows, R.seed_of("accpool", d, C, B, HW))
    acc, ref, bnd = _acc_stats(p["y"], C, p["gamma"], p["beta"], p["rm"], p["rv"], 7)
    for mode in ("none", "add"):
        res = None if mode == "none" else p["res"]
        got = _apply_acc(dtype, p["y"], acc, p["gamma"], p["beta"], p["rm"], p["rv"], res, None, None, None, None, None, B, HW, C, 1, pool=True)
        a = (p["y"], ref["coef"][0], ref["coef"][1], res, None, None)
        want, _ = R.apply_ref(*a)
        w_out = max(w_out, _check(f"acc pool out {mode}", got["out"], want, R.store_bound(R.apply_bound(*a, d=bnd["coef"][:2]), want, dtype)))
        sums, mags, cpu32 = R.pool_ref(got["out"], B, HW, C, dtype)
        tol, _ = R.units_bound(cpu32, sums, mags)
        w_sum = max(w_sum, _check(f"acc pool sums {mode}", got["part"], sums, tol.clamp(min=1e-300)))
    print(f"apply_pool {R.case_id(case)}: chunks {chunks}, worst err / bound out {w_out:.3f} sums {w_sum:.3f}")


@pytest.mark.parametrize("d", ["fp32", "bf16"])
def test_a_single_nan_reaches_its_element_and_its_chunk_only(d):
    L = sub("_lib")
    dtype, C, B, HW = R.DT[d], 512, 3, 197
    rows, chunks = B * HW, R.pool_chunks(HW, C, dtype)
    rpc = 14 * R.lanes_r(C, dtype)
    b0, r0, c0 = 1, 100, 37
    assert chunks >= 3
    op = R.fwd_operands(dtype, C, rows, R.seed_of("nan", d), exact=True)
    clean_y = op["y"].clone()
    op["y"][b0 * HW + r0, c0] = float("nan")
    want = torch.zeros(rows, C, dtype=torch.bool)
    want[b0 * HW + r0, c0] = True
    wantp = torch.zeros(B, chunks, C, dtype=torch.bool)
    wantp[b0, r0 // rpc, c0] = True
    for mode in R.RES_MODES:
        ref, _ = _fwd_reference(op, mode, 1, dtype)
        assert torch.equal(ref.isnan(), want)
        out = _apply(dtype, op, mode, 1, rows, C)
        assert torch.equal(out.isnan(), want) and torch.equal(out[~want], R.stored(ref, dtype)[~want])
        res, rs, _ = R.fwd_mode_args(op, mode)
        outp, part = _guarded(rows, C, dtype), _guarded(B * chunks, C)
        L.call("vqa_bn_apply_pool", L.dt(dtype), K(op["y"]), K(op["coef"]), K(res),
               K(op["rcoef"]) if rs is not None else None, outp.data_ptr(), B, HW, C, 1, part.data_ptr())
        outp_h, part_h = _written(outp, rows, "out"), _written(part, B * chunks, "part").view(B, chunks, C)
        assert torch.equal(outp_h.isnan(), want) and torch.equal(part_h.isnan(), wantp)
        sums, _, _ = R.pool_ref(R.stored(ref, dtype), B, HW, C, dtype)
        assert torch.equal(part_h.double()[~wantp], sums[~wantp])
    # accumulator-fed pooling variant: statistics of the clean tensor, the NaN only in what the kernel streams
    p = _acc_operands(dtype, C, rows, R.seed_of("nanacc", d))
    acc, _, _ = _acc_stats(clean_y, C, p["gamma"], p["beta"], p["rm"], p["rv"], 8)
    got = _apply_acc(dtype, op["y"], acc, p["gamma"], p["beta"], p["rm"], p["rv"], None, None, None, None, None, None, B, HW, C, 1, pool=True)
    want[:, 2] = False                                                        # gamma == 0 there: channel 2 is not the NaN's channel anyway
    assert torch.equal(got["out"].isnan(), want) and torch.equal(got["part"].isnan(), wantp)
    assert bool(torch.isfinite(got["coef"]).all()) and bool(torch.isfinite(got["run"]).all())


@pytest.mark.parametrize("d", ["fp32", "bf16"])
def test_apply_acc_with_a_raised_flag_word_turns_mean_shift_and_output_into_nan(d):
    """What the code does, pinned: a non-zero flag word makes the MEAN NaN.  scale and invstd (from the variance of the planes as
    they are) stay finite and equal to the unflagged launch's; shift, coef_out's mean, the running mean and every output are NaN;
    the running variance is updated as without the flag and num_batches_tracked still counts the step."""
    dtype, C, rows = R.DT[d], 64, 33
    p = _acc_operands(dtype, C, rows, R.seed_of("flag", d))
    acc, ref, bnd = _acc_stats(p["y"], C, p["gamma"], p["beta"], p["rm"], p["rv"], 9)
    clean = _apply_acc(dtype, p["y"], acc, p["gamma"], p["beta"], p["rm"], p["rv"], None, None, None, None, None, None, 1, rows, C, 1)
    flagged = acc.clone()
    flagged[R.replicas(C) * 2 * C] = 1
    got = _apply_acc(dtype, p["y"], flagged, p["gamma"], p["beta"], p["rm"], p["rv"], None, None, None, None, None, None, 1, rows, C, 1)
    assert bool(got["out"].isnan().all()) and bool(got["coef"][1].isnan().all()) and bool(got["coef"][2].isnan().all())
    assert torch.equal(got["coef"][0], clean["coef"][0]) and torch.equal(got["coef"][3], clean["coef"][3])
    assert bool(got["run"][0].isnan().all()) and torch.equal(got["run"][1], clean["run"][1])
    assert got["nbt"] == [42, 7, 13] and clean["nbt"] == [42, 7, 13]
    _check("clean coef", clean["coef"], ref["coef"], bnd["coef"])


def test_apply_acc_refuses_a_shortcut_accumulator_with_pooling_or_without_res():
    dtype, C, B, HW = BF16, 64, 2, 49
    rows = B * HW
    p = _acc_operands(dtype, C, rows, 11)
    acc, _, _ = _acc_stats(p["y"], C, p["gamma"], p["beta"], p["rm"], p["rv"], 1)
    t = {k: _d(v) for k, v in p.items()}
    accd = _d(acc)
    out, coef, rcoef, run, rrun, part = (_guarded(rows, C, dtype), _guarded(4, C), _guarded(4, C), _guarded(2, C), _guarded(2, C),
                                         _guarded(B * R.pool_chunks(HW, C, dtype), C))
    nbt = torch.tensor([41, 7], device=DEV, dtype=torch.int64)

    def status(res, pool):
        return _rc("vqa_bn_apply_acc", 1, t["y"].data_ptr(), accd.data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), run[0].data_ptr(),
                   run[1].data_ptr(), nbt.data_ptr(), coef.data_ptr(), _p(res), accd.data_ptr(), t["rgamma"].data_ptr(), t["rbeta"].data_ptr(),
                   rrun[0].data_ptr(), rrun[1].data_ptr(), nbt[1:].data_ptr(), rcoef.data_ptr(), out.data_ptr(), B, HW, C, 1, float(rows),
                   0.1, 1e-5, _p(part) if pool else None)
    assert status(t["res"], True) == EARG
    assert status(None, False) == EARG
    for buf in (out, coef, rcoef, run, rrun, part):
        assert _untouched(buf)
    assert nbt.cpu().tolist() == [41, 7]


# -------------------------------------------------------------------------------------------------------------------- backward
def _bwd_modes(rows, C):
    """all four mask modes; past a million elements the two that read the most (every mode's own code runs at the small row counts)"""
    return ("self", "dual") if rows * C > 2 ** 20 else R.BWD_MODES


def _mode_ptrs(op, mode):
    """device (outact, y2, coef2) of a mask mode and the self_mask switch"""
    return (_d(op["outact"]) if mode in ("outact", "dual") else None, _d(op["y2"]) if mode == "dual" else None,
            _d(op["coef2"]) if mode == "dual" else None, int(mode == "self"))


def _reduce(dtype, op, mode, rows, C, acc_mode):
    """vqa_bn_bwd_reduce -> fp64 [3][C]: the slab summed on the host in fp64, or the accumulator decoded on the host"""
    L = sub("_lib")
    oa, y2, c2, self_mask = _mode_ptrs(op, mode)
    nb = R.bwd_blocks(rows)
    if acc_mode:
        words = R.acc_words(3, C)
        buf = torch.zeros(words + 2, device=DEV, dtype=torch.int64)
        buf[words:] = 0x5A5A5A5A
    else:
        buf = _guarded(nb * 3, C)
    L.call("vqa_bn_bwd_reduce", L.dt(dtype), K(op["dout"]), _p(oa), K(op["y"]), K(op["coef"]), _p(y2), _p(c2),
           buf.data_ptr(), rows, C, self_mask, acc_mode)
    if acc_mode:
        torch.cuda.synchronize()
        h = buf.cpu()
        assert h[words:].tolist() == [0x5A5A5A5A] * 2
        s, flag = R.acc_decode(h[:words], 3, C)
        assert flag == 0
        hi, lo, _ = R.acc_planes(h[:words], 3, C)
        if mode != "dual":
            assert int(hi[:, 2].abs().sum()) == 0 and int(lo[:, 2].abs().sum()) == 0
        if nb >= R.replicas(C) and rows * C >= 4096:
            assert bool((hi[:, :2].abs().sum((1, 2)) > 0).all()) and bool((hi < 0).any())     # every replica took part, negatives occur
        return s
    slab = _written(buf, nb * 3, "slab").view(nb, 3, C)
    if mode != "dual":
        assert float(slab[:, 2].abs().max()) == 0.0
    return slab.double().sum(0)


@pytest.mark.parametrize("case", R.ROW_CASES, ids=R.case_id)
def test_bwd_reduce_sums_match_fp64_as_slab_and_as_accumulator(case):
    """sum g, sum g xhat, sum g xhat2 in the four mask modes; the accumulator of acc_mode = 1 is decoded on the host (acc_add_fixed:
    sign handling, replica blockIdx.x % R, both planes) and held to the same bound as the slab.
    Measured on MI355X: worst err / bound 0.009 ... 0.22, the same figure for slab and accumulator in every case; CPU fp32 error
    6.0e-8 (the floor) ... 1.6e-7 of the unit."""
    d, C, rows = case
    dtype = R.DT[d]
    op = R.bwd_operands(dtype, C, rows, R.seed_of("bwd", d, C, rows))
    assert R.self_margin(op) > 1.0
    w_slab = w_acc = w_cpu = 0.0
    for mode in _bwd_modes(rows, C):
        dual = mode == "dual"
        s, a = R.bwd_sums(R.bwd_g(op, "outact" if dual else mode), op, dual)
        cpu32 = R.bwd_sums_fp32(op, mode, dual)
        tw = [R.units_bound(cpu32[k], s[k], a[k]) for k in range(3)]
        tol, w_cpu = torch.stack([t for t, _ in tw]).clamp(min=1e-300), max([w_cpu] + [w for _, w in tw])
        w_slab = max(w_slab, _check(f"slab {mode}", _reduce(dtype, op, mode, rows, C, 0), s, tol))
        w_acc = max(w_acc, _check(f"acc {mode}", _reduce(dtype, op, mode, rows, C, 1), s, tol))
    print(f"bwd_reduce {R.case_id(case)}: blocks {R.bwd_blocks(rows)}, cpu fp32 units {w_cpu:.2e}, worst err / bound slab {w_slab:.3f} acc {w_acc:.3f}")


@pytest.mark.parametrize("C", [64, 100])
@pytest.mark.parametrize("nblk", R.FINALIZE_NBLK)
def test_bwd_finalize_matches_fp64_for_both_batchnorms_in_train_and_eval(nblk, C):
    """vqa_bn_bwd_finalize on a hand-built slab: which = 1 and 2, training 1 and 0; d gamma / d beta are ADDED into buffers holding
    0.5.  Measured on MI355X: worst err / bound bcoef 0.72 ... 0.97, gradients 0.48 ... 1.000 (the cancelling channel: its sum is
    2^-25, 0.5 + 2^-25 is a tie that rounds to 0.5, and that half ulp is the bound)."""
    L = sub("_lib")
    slab, gamma, coef = R.slab_operands(nblk, C, R.seed_of("slab", nblk, C))
    s, d_s = R.slab_sums(slab)
    count = float(nblk * 7 + 2)
    slab_d, gamma_d, coef_d = _d(slab), _d(gamma), _d(coef)
    w_bc = w_g = 0.0
    for which in (1, 2):
        for training in (1, 0):
            bc, grads = _guarded(3, C), _guarded(2, C)
            grads[:2] = 0.5
            L.call("vqa_bn_bwd_finalize", slab_d.data_ptr(), nblk, C, which, count, gamma_d.data_ptr(), coef_d.data_ptr(), training,
                   grads[0].data_ptr(), grads[1].data_ptr(), bc.data_ptr())
            bc_h, g_h = _written(bc, 3, "bcoef"), _written(grads, 2, "gradients")
            w_bc = max(w_bc, _check(f"bcoef which {which} training {training}", bc_h, R.bc_ref(s[0], s[which], count, gamma, coef, training),
                                    R.bc_bound(s[0], s[which], count, gamma, coef, training, d_s[0], d_s[which])))
            w_g = max(w_g, _check("dgamma", g_h[0], 0.5 + s[which], R.grad_add_bound(s[which], 0.5, d_s[which])),
                      _check("dbeta", g_h[1], 0.5 + s[0], R.grad_add_bound(s[0], 0.5, d_s[0])))
            if not training:
                assert float(bc_h[1:].abs().max()) == 0.0
    print(f"bwd_finalize nblk {nblk} C {C}: worst err / bound bcoef {w_bc:.3f} gradients {w_g:.3f}")


@pytest.mark.parametrize("case", R.ROW_CASES, ids=R.case_id)
def test_bwd_apply_matches_fp64_in_every_mask_mode(case):
    """vqa_bn_bwd_apply with given coefficients: dy, and dy2 of the shortcut BatchNorm.
    Measured on MI355X: worst err / bound 0.43 ... 0.71 (fp32), 0.73 ... 0.996 (bf16, the final rounding)."""
    L = sub("_lib")
    d, C, rows = case
    dtype = R.DT[d]
    op = R.bwd_operands(dtype, C, rows, R.seed_of("bwd", d, C, rows))
    worst = 0.0
    for mode in _bwd_modes(rows, C):
        oa, y2, _, self_mask = _mode_ptrs(op, mode)
        dual = mode == "dual"
        dy, dy2 = _guarded(rows, C, dtype), _guarded(rows, C, dtype)
        L.call("vqa_bn_bwd_apply", L.dt(dtype), K(op["dout"]), _p(oa), K(op["y"]), K(op["bc"]), dy.data_ptr(),
               _p(y2), K(op["bc2"]) if dual else None, dy2.data_ptr() if dual else None, rows * C, C,
               K(op["coef"]) if self_mask else None)
        g = R.bwd_g(op, "outact" if dual else mode)
        ref = R.dy_ref(op["bc"], g, op["y"])
        worst = max(worst, _check(f"dy {mode}", _written(dy, rows, "dy"), ref, R.store_bound(R.dy_bound(op["bc"], g, op["y"]), ref, dtype)))
        if dual:
            ref2 = R.dy_ref(op["bc2"], g, op["y2"])
            worst = max(worst, _check("dy2", _written(dy2, rows, "dy2"), ref2, R.store_bound(R.dy_bound(op["bc2"], g, op["y2"]), ref2, dtype)))
        else:
            assert _untouched(dy2)
    print(f"bwd_apply {R.case_id(case)}: worst err / bound {worst:.3f}")


def _bwd_apply_acc(dtype, op, mode, facc, rows, C):
    L = sub("_lib")
    oa, y2, c2, self_mask = _mode_ptrs(op, mode)
    dual = mode == "dual"
    dy, dy2, grads = _guarded(rows, C, dtype), _guarded(rows, C, dtype), _guarded(4, C)
    grads[:4] = 0.5
    L.call("vqa_bn_bwd_apply_acc", L.dt(dtype), K(op["dout"]), _p(oa), K(op["y"]), K(facc),
           K(op["gamma"]), K(op["coef"]), grads[0].data_ptr(), grads[1].data_ptr(), dy.data_ptr(), _p(y2),
           K(op["gamma2"]) if dual else None, _p(c2), grads[2].data_ptr() if dual else None, grads[3].data_ptr() if dual else None,
           dy2.data_ptr() if dual else None, rows * C, C, float(rows), self_mask)
    g_h = _written(grads, 4, "gradients")
    if not dual:
        assert _untouched(dy2) and bool((g_h[2:] == 0.5).all())
    return _written(dy, rows, "dy"), (_written(dy2, rows, "dy2") if dual else None), g_h


@pytest.mark.parametrize("case", R.ROW_CASES, ids=R.case_id)
def test_bwd_apply_acc_matches_fp64_from_host_encoded_accumulators(case):
    """vqa_bn_bwd_apply_acc: the three column sums arrive as an accumulator encoded on the host (partials of uneven row chunks,
    spread unevenly over the replicas); d gamma / d beta (and the shortcut's) are added into buffers holding 0.5, dy / dy2 against
    fp64 with the coefficient bound.  Measured on MI355X: worst err / bound dy 0.73 ... 0.996 (bf16) / 0.08 ... 0.73 (fp32), gradients 0.36 ... 1.000."""
    d, C, rows = case
    dtype = R.DT[d]
    op = R.bwd_operands(dtype, C, rows, R.seed_of("bwd", d, C, rows))
    w_dy = w_g = 0.0
    for mode in _bwd_modes(rows, C):
        dual = mode == "dual"
        g = R.bwd_g(op, "outact" if dual else mode)
        parts = R.sum_partials(g, op, dual, min(rows, 11))
        facc = R.acc_encode(parts, R.uneven_replicas(parts.shape[0], C, 4), 3, C)
        s, flag = R.acc_decode(facc, 3, C)
        assert flag == 0
        d_s = 2.0 ** -51 * s.abs()
        dy, dy2, grads = _bwd_apply_acc(dtype, op, mode, facc, rows, C)
        pairs = [(op["gamma"], op["coef"], 1, op["y"], dy, 0)] + ([(op["gamma2"], op["coef2"], 2, op["y2"], dy2, 2)] if dual else [])
        for gamma, coef, k, yy, got, slot in pairs:
            bc = R.bc_ref(s[0], s[k], float(rows), gamma, coef, True)
            d_bc = R.bc_bound(s[0], s[k], float(rows), gamma, coef, True, d_s[0], d_s[k])
            ref = R.dy_ref(bc, g, yy)
            w_dy = max(w_dy, _check(f"dy{k} {mode}", got, ref, R.store_bound(R.dy_bound(bc, g, yy, d_bc), ref, dtype)))
            w_g = max(w_g, _check(f"dgamma{k}", grads[slot], 0.5 + s[k], R.grad_add_bound(s[k], 0.5, d_s[k])),
                      _check(f"dbeta{k}", grads[slot + 1], 0.5 + s[0], R.grad_add_bound(s[0], 0.5, d_s[0])))
    print(f"bwd_apply_acc {R.case_id(case)}: worst err / bound dy {w_dy:.3f} gradients {w_g:.3f}")


def test_entries_refuse_self_mask_with_a_second_input_and_channel_counts_that_do_not_divide_a_workgroup():
    """self_mask together with y2 or outact, and C = 96 in bf16 (12 channel vectors: 256 % 12 != 0): VQA_EARG from every entry that
    checks it, nothing written."""
    rows, C = 5, 64
    op = R.bwd_operands(BF16, C, rows, 3)
    t = {k: _d(v) for k, v in op.items()}
    dy, dy2, grads, slab = _guarded(rows, C, BF16), _guarded(rows, C, BF16), _guarded(4, C), _guarded(3, C)
    facc = torch.zeros(R.acc_words(3, C), device=DEV, dtype=torch.int64)
    P = lambda k: t[k].data_ptr()

    def reduce_(C_, oa, y2, self_mask):
        return _rc("vqa_bn_bwd_reduce", 1, P("dout"), oa, P("y"), P("coef"), y2, P("coef2") if y2 else None, slab.data_ptr(), rows, C_, self_mask, 0)

    def apply_(C_, oa, y2, mask):
        return _rc("vqa_bn_bwd_apply", 1, P("dout"), oa, P("y"), P("bc"), dy.data_ptr(), y2, P("bc2") if y2 else None,
                   dy2.data_ptr() if y2 else None, rows * C_, C_, mask)

    def apply_acc_(C_, oa, y2, self_mask):
        two = y2 is not None
        return _rc("vqa_bn_bwd_apply_acc", 1, P("dout"), oa, P("y"), facc.data_ptr(), P("gamma"), P("coef"), grads[0].data_ptr(),
                   grads[1].data_ptr(), dy.data_ptr(), y2, P("gamma2") if two else None, P("coef2") if two else None,
                   grads[2].data_ptr() if two else None, grads[3].data_ptr() if two else None, dy2.data_ptr() if two else None,
                   rows * C_, C_, float(rows), self_mask)
    for fn, mask in ((reduce_, 1), (apply_, P("coef")), (apply_acc_, 1)):
        assert fn(C, P("outact"), None, mask) == EARG
        assert fn(C, None, P("y2"), mask) == EARG
        assert fn(96, None, None, 0 if mask == 1 else None) == EARG
    out, part, coef, run = _guarded(rows, 96, BF16), _guarded(1, 96), _guarded(4, 96), _guarded(2, 96)
    nbt = torch.tensor([41], device=DEV, dtype=torch.int64)
    assert _rc("vqa_bn_apply", 1, P("y"), P("coef"), None, None, out.data_ptr(), rows * 96, 96, 1) == EARG
    assert _rc("vqa_bn_apply_pool", 1, P("y"), P("coef"), None, None, out.data_ptr(), 1, rows, 96, 1, part.data_ptr()) == EARG
    assert _rc("vqa_bn_apply_acc", 1, P("y"), facc.data_ptr(), P("gamma"), P("gamma"), run[0].data_ptr(), run[1].data_ptr(), nbt.data_ptr(),
               coef.data_ptr(), None, None, None, None, None, None, None, None, out.data_ptr(), 1, rows, 96, 1, float(rows), 0.1, 1e-5, None) == EARG
    for buf in (dy, dy2, grads, slab, out, part, coef, run):
        assert _untouched(buf)
    assert nbt.cpu().tolist() == [41] and int(facc.abs().sum()) == 0


# ----------------------------------------------------------------------------------------------------------------------- chain
def _chain_coef(o, key_y, key_g, key_b, C, seed):
    """vqa_bn_stats_finalize on a partial slab of the tensor's own sums -> (device coef, ref, bound)"""
    L = sub("_lib")
    y = o[key_y]
    part = R.stat_partials(y, 5)
    (_, d_s), (_, d_q) = R.slab_sums(part[:, 0]), R.slab_sums(part[:, 1])
    r_s, r_q = _partial_rounding(y, 5)                                     # the reference: the tensor's own sums, as autograd's
    ref, bnd = R.coef_ref(y.double().sum(0), (y.double() ** 2).sum(0), d_s + r_s, d_q + r_q, float(y.shape[0]), o[key_g], o[key_b])
    coef, scratch = _guarded(4, C), torch.empty(64 * 2 * C, device=DEV, dtype=torch.float64)
    L.call("vqa_bn_stats_finalize", K(part), part.shape[0], C, float(y.shape[0]), K(o[key_g]), K(o[key_b]),
           None, None, None, 0.1, 1e-5, scratch.data_ptr(), coef.data_ptr())
    _written(coef, 4, "coef")
    return coef, ref["coef"], bnd["coef"]


def _chain_tolerances(pattern, o, ag, cf, refs, d_coefs, dtype):
    """per-channel tolerances of the sums and the coefficient errors behind dy: (tol [3][C], d_bc, d_bc2)"""
    rows = o["y"].shape[0]
    dual = pattern == "dual"
    g = cf["g"]
    op = {"dout": o["dout"], "y": o["y"], "y2": o["y2"], "coef": refs[0], "coef2": refs[1]}
    s, a = R.bwd_sums(g, op, dual)
    # the same formulas in fp32: the mask of the fp64 output, xhat from fp32 coefficients
    g32 = o["dout"].float() * (cf["out"] > 0)
    x32 = lambda y, c: g32 * (y.float() - c[2].float()) * c[3].float()
    cpu32 = torch.stack([g32.sum(0), x32(o["y"], refs[0]).sum(0), x32(o["y2"], refs[1]).sum(0) if dual else torch.zeros_like(s[0])])
    tol = torch.stack([R.units_bound(cpu32[k], s[k], a[k])[0] for k in range(3)])
    # d gamma also moves with the kernel's own mean / invstd
    for k, (c, dc) in enumerate(zip(refs, d_coefs)):
        if c is not None and (k == 0 or dual):
            tol[k + 1] = tol[k + 1] + a[0] * c[3] * dc[2] + a[k + 1] / c[3] * dc[3]
    training = pattern != "eval"
    d_bcs = []
    for k, gam in ((1, o["gamma"]), (2, o["gamma2"])):
        if k == 2 and not dual:
            d_bcs.append(None)
            continue
        c, dc = refs[k - 1], d_coefs[k - 1]
        d_bcs.append(R.bc_bound(s[0], s[k], float(rows), gam, c, training, tol[0], tol[k]) + R.bc_sens(s[0], s[k], float(rows), gam, c, dc, training))
    return s, tol, d_bcs


@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=R.case_id)
def test_block_chain_matches_fp64_autograd(case):
    """A whole block on coefficients that really are the statistics of y: vqa_bn_stats_finalize (or vqa_bn_eval_coef) -> vqa_bn_apply
    -> vqa_bn_bwd_reduce (slab) -> vqa_bn_bwd_finalize -> vqa_bn_bwd_apply, and for the training patterns the accumulator route
    vqa_bn_apply_acc -> vqa_bn_bwd_reduce(acc_mode = 1) -> vqa_bn_bwd_apply_acc, against torch fp64 autograd of
    relu(bn(y) + res) / relu(bn(y) + bn(y2)) / relu(bn_eval(y)).  The mask is the kernels' own output (outact) for the training
    patterns and self_mask for the eval pattern.
    Measured on MI355X (slab and accumulator routes alike): worst err / bound out 0.98 ... 0.996 (bf16) / 0.23 ... 0.48 (fp32),
    d gamma / d beta 0.06 ... 0.12, dy 0.98 ... 0.995 (bf16) / 0.26 ... 0.40 (fp32)."""
    L = sub("_lib")
    pattern, d, C = case
    dtype = R.DT[d]
    o, margin = R.chain_operands(pattern, dtype, C)
    rows = o["y"].shape[0]
    kw = R.block_kwargs(pattern, o)
    ag, cf = R.block_autograd(pattern, **kw), R.block_closed_form(pattern, **kw)
    dual, training = pattern == "dual", pattern != "eval"
    dv = {k: _d(v) for k, v in o.items()}
    zero_c = torch.zeros(C, dtype=torch.float64)

    def judge(route, out_h, coefs_ref, d_coefs, dy_h, dy2_h, grads_h):
        res = o["res"] if pattern == "res" else (o["y2"] if dual else None)
        a = (o["y"], coefs_ref[0][0], coefs_ref[0][1], res, coefs_ref[1][0] if dual else None, coefs_ref[1][1] if dual else None)
        e = R.apply_bound(*a, d=d_coefs[0][:2], dr=d_coefs[1][:2] if dual else None)
        w_out = _check(f"{route} out", out_h, ag["out"], R.store_bound(e, ag["out"], dtype))
        assert torch.equal(out_h > 0, ag["out"] > 0)
        s, tol, d_bcs = _chain_tolerances(pattern, o, ag, cf, coefs_ref, d_coefs, dtype)
        add = lambda k: R.grad_add_bound(s[k], 0.5, tol[k])
        w_g = max(_check(f"{route} dgamma", grads_h[0], 0.5 + ag["dgamma"], add(1)), _check(f"{route} dbeta", grads_h[1], 0.5 + ag["dbeta"], add(0)))
        bc = R.bc_ref(s[0], s[1], float(rows), o["gamma"], coefs_ref[0], training)
        w_dy = _check(f"{route} dy", dy_h, ag["dy"], R.store_bound(R.dy_bound(bc, cf["g"], o["y"], d_bcs[0]), ag["dy"], dtype))
        if dual:
            w_g = max(w_g, _check(f"{route} dgamma2", grads_h[2], 0.5 + ag["dgamma2"], add(2)), _check(f"{route} dbeta2", grads_h[3], 0.5 + ag["dbeta2"], add(0)))
            bc2 = R.bc_ref(s[0], s[2], float(rows), o["gamma2"], coefs_ref[1], True)
            w_dy = max(w_dy, _check(f"{route} dy2", dy2_h, ag["dy2"], R.store_bound(R.dy_bound(bc2, cf["g"], o["y2"], d_bcs[1]), ag["dy2"], dtype)))
        print(f"chain {R.case_id(case)} {route}: margin {margin:.0f}, worst err / bound out {w_out:.3f} gradients {w_g:.3f} dy {w_dy:.3f}")

    # ---- slab route
    if training:
        coef, c_ref, c_bnd = _chain_coef(o, "y", "gamma", "beta", C, 1)
    else:
        c_ref, c_bnd = R.eval_coef_ref(o["gamma"], o["beta"], o["rm"], o["rv"])
        coef = _guarded(4, C)
        L.call("vqa_bn_eval_coef", C, dv["gamma"].data_ptr(), dv["beta"].data_ptr(), dv["rm"].data_ptr(), dv["rv"].data_ptr(), 1e-5, coef.data_ptr())
    coef2, c2_ref, c2_bnd = _chain_coef(o, "y2", "gamma2", "beta2", C, 2) if dual else (None, None, None)
    out = _guarded(rows, C, dtype)
    res_d = dv["res"] if pattern == "res" else (dv["y2"] if dual else None)
    L.call("vqa_bn_apply", L.dt(dtype), dv["y"].data_ptr(), coef.data_ptr(), _p(res_d), _p(coef2), out.data_ptr(), rows * C, C, 1)
    out_h = _written(out, rows, "out")
    nb = R.bwd_blocks(rows)
    slab, bc, bc2, grads = _guarded(nb * 3, C), _guarded(3, C), _guarded(3, C), _guarded(4, C)
    grads[:4] = 0.5
    self_mask = int(not training)
    L.call("vqa_bn_bwd_reduce", L.dt(dtype), dv["dout"].data_ptr(), None if self_mask else out.data_ptr(), dv["y"].data_ptr(), coef.data_ptr(),
           dv["y2"].data_ptr() if dual else None, _p(coef2), slab.data_ptr(), rows, C, self_mask, 0)
    L.call("vqa_bn_bwd_finalize", slab.data_ptr(), nb, C, 1, float(rows), dv["gamma"].data_ptr(), coef.data_ptr(), int(training),
           grads[0].data_ptr(), grads[1].data_ptr(), bc.data_ptr())
    if dual:
        L.call("vqa_bn_bwd_finalize", slab.data_ptr(), nb, C, 2, float(rows), dv["gamma2"].data_ptr(), coef2.data_ptr(), 1,
               grads[2].data_ptr(), grads[3].data_ptr(), bc2.data_ptr())
    dy, dy2 = _guarded(rows, C, dtype), _guarded(rows, C, dtype)
    L.call("vqa_bn_bwd_apply", L.dt(dtype), dv["dout"].data_ptr(), None if self_mask else out.data_ptr(), dv["y"].data_ptr(), bc.data_ptr(),
           dy.data_ptr(), dv["y2"].data_ptr() if dual else None, bc2.data_ptr() if dual else None, dy2.data_ptr() if dual else None,
           rows * C, C, coef.data_ptr() if self_mask else None)
    judge("slab", out_h, (c_ref, c2_ref), (c_bnd, c2_bnd), _written(dy, rows, "dy"), _written(dy2, rows, "dy2") if dual else None,
          _written(grads, 4, "gradients"))
    if not training:
        return
    # ---- accumulator route
    acc, a_ref, a_bnd = _acc_stats(o["y"], C, o["gamma"], o["beta"], o["rm"], o["rv"], 1, of_tensor=True)
    racc, ra_ref, ra_bnd = _acc_stats(o["y2"], C, o["gamma2"], o["beta2"], o["rm"], o["rv"], 2, of_tensor=True) if dual else (None, None, None)
    outa, coefa, coefa2, run, run2 = _guarded(rows, C, dtype), _guarded(4, C), _guarded(4, C), _guarded(2, C), _guarded(2, C)
    run[:2], run2[:2] = 0.25, 0.25
    nbt = torch.zeros(2, device=DEV, dtype=torch.int64)
    L.call("vqa_bn_apply_acc", L.dt(dtype), dv["y"].data_ptr(), K(acc), dv["gamma"].data_ptr(), dv["beta"].data_ptr(),
           run[0].data_ptr(), run[1].data_ptr(), nbt.data_ptr(), coefa.data_ptr(), _p(res_d), K(racc),
           dv["gamma2"].data_ptr() if dual else None, dv["beta2"].data_ptr() if dual else None, run2[0].data_ptr() if dual else None,
           run2[1].data_ptr() if dual else None, nbt[1:].data_ptr() if dual else None, coefa2.data_ptr() if dual else None,
           outa.data_ptr(), 1, rows, C, 1, float(rows), 0.1, 1e-5, None)
    outa_h = _written(outa, rows, "out")
    words = R.acc_words(3, C)
    facc = torch.zeros(words, device=DEV, dtype=torch.int64)
    L.call("vqa_bn_bwd_reduce", L.dt(dtype), dv["dout"].data_ptr(), outa.data_ptr(), dv["y"].data_ptr(), coefa.data_ptr(),
           dv["y2"].data_ptr() if dual else None, coefa2.data_ptr() if dual else None, facc.data_ptr(), rows, C, 0, 1)
    dya, dya2, gradsa = _guarded(rows, C, dtype), _guarded(rows, C, dtype), _guarded(4, C)
    gradsa[:4] = 0.5
    L.call("vqa_bn_bwd_apply_acc", L.dt(dtype), dv["dout"].data_ptr(), outa.data_ptr(), dv["y"].data_ptr(), facc.data_ptr(), dv["gamma"].data_ptr(),
           coefa.data_ptr(), gradsa[0].data_ptr(), gradsa[1].data_ptr(), dya.data_ptr(), dv["y2"].data_ptr() if dual else None,
           dv["gamma2"].data_ptr() if dual else None, coefa2.data_ptr() if dual else None, gradsa[2].data_ptr() if dual else None,
           gradsa[3].data_ptr() if dual else None, dya2.data_ptr() if dual else None, rows * C, C, float(rows), 0)
    judge("acc", outa_h, (a_ref["coef"], ra_ref["coef"] if dual else None), (a_bnd["coef"], ra_bnd["coef"] if dual else None),
          _written(dya, rows, "dy"), _written(dya2, rows, "dy2") if dual else None, _written(gradsa, 4, "gradients"))
