"""GPU: the LayerNorm kernels of csrc/token_ops.hip against float64, kernel by kernel.

Forward (vqa_layernorm_fwd): output AND statistics against fp64 F.layer_norm computed from the same (already rounded) inputs, for
every bf16 instantiation (D = 64 / 128 / 256 / 512 -> layernorm_fwd_bf16v_kernel<8|16|32|64>), the generic kernel in fp32 and bf16,
row counts that leave a wave partly empty, and more rows than the capped grid carries in one trip.  The fp32 bound is 8x the error of
torch's own fp32 layer_norm on the CPU on the same inputs (measured in the test, in units of 1 + |ref|); bf16 adds half an ulp of the
output.  The dropout / addrow forms are checked against  fp64 LN * keep / (1 - p) + addrow[row % period]  with the numpy restatement
of the generator -- never against the kernel's own plain output.
Backward (vqa_layernorm_bwd): dx, dgamma, dbeta, dadd against fp64 autograd of that formula (+ addend on dx), with and without the
fixed-order scratch, on top of pre-filled accumulators (the += contract) and a pre-filled dx (which must be overwritten)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _dropmask import keep_mask
from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = float(np.float32(1e-5))                                       # the entry takes eps as a float
F32, BF16 = torch.float32, torch.bfloat16
HALF_ULP_F32 = 2.0 ** -24

FWD_SHAPES = [(37, 64), (37, 128), (37, 256), (37, 512),           # the four bf16v instantiations, rows % (64 / LPR) != 0
              (1, 64), (3, 128),                                    # fewer rows than one wave carries
              (37, 8), (37, 40), (37, 96), (37, 320), (5, 500),     # generic kernel: D < 64, D % 64 != 0, D % 8 != 0
              (8195, 512)]                                          # > 2048 blocks x 4 waves: the grid-stride loop's second trip


def _inputs(rows, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g) * 2 + 0.7
    const = rows // 2 if rows > 1 else None                         # one constant row (a lone row stays random: it must test something)
    if const is not None:
        x[const] = 1.5                                              # exactly representable, sums exact for D <= 512
    gam, bet = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    return x.to(dtype), gam, bet, const, g


def _ref_ln(x, gam, bet):
    """fp64 output, mean, rstd from the rounded inputs."""
    xd = x.double()
    mean = xd.mean(1)
    rstd = (xd.var(1, unbiased=False) + EPS).rsqrt()
    return F.layer_norm(xd, (x.shape[1],), gam.double(), bet.double(), EPS), mean, rstd


def _units(a, ref):
    """worst |a - ref| in units of (1 + |ref|)"""
    return float(((a.double() - ref).abs() / (1 + ref.abs())).max())


def _fp32_bound(cpu_fp32, ref):
    """8 x the error of the same formula in torch fp32 on the CPU (different summation tree, rsqrtf's couple of ulps).  The CPU figure
    is floored at half an ulp of fp32: below that it only says the inputs were lucky."""
    cpu = max(_units(cpu_fp32, ref), HALF_ULP_F32)
    return cpu, 8 * cpu


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,D", FWD_SHAPES)
def test_layernorm_forward_output_and_stats_match_fp64(rows, D, dtype):
    K = sub("kernels")
    x, gam, bet, const, _ = _inputs(rows, D, dtype, 1000 * D + rows)
    ref, mean, rstd = _ref_ln(x, gam, bet)
    out, st = K.layernorm_fwd(x.to(DEV), gam.to(DEV), bet.to(DEV), eps=EPS)
    torch.cuda.synchronize()
    out, st = out.cpu(), st.cpu().double()
    # measured on the CPU with these inputs: torch fp32 layer_norm is 1.1e-7 (3 x 128) ... 3.5e-7 (37 x 512) ... 4.6e-7 (8195 x 512) of
    # (1 + |ref|) from fp64 on fp32 inputs, 6.0e-8 (floor) ... 4.4e-7 on bf16-rounded inputs -> the kernel is allowed
    # 8.6e-7 ... 3.7e-6 resp. 4.8e-7 ... 3.5e-6 (8x, per case, recomputed here from the same inputs)
    cpu, bound = _fp32_bound(F.layer_norm(x.float(), (D,), gam, bet, EPS), ref)
    err = ((out.double() - ref).abs() - (2.0 ** -8 * ref.abs() if dtype == BF16 else 0)) / (1 + ref.abs())
    print(f"LN fwd {rows}x{D} {dtype}: cpu fp32 {cpu:.2e} bound {bound:.2e} kernel {float(err.max()):.2e}")
    assert float(err.max()) <= bound
    # mean: an fp32 sum is accurate relative to the sum of magnitudes (|mean| itself can cancel to nothing); rstd: plainly relative
    scale = x.double().abs().mean(1)
    e_mean, e_rstd = float(((st[:, 0] - mean).abs() / scale).max()), float(((st[:, 1] - rstd).abs() / rstd).max())
    print(f"   stats: mean {e_mean:.2e} rstd {e_rstd:.2e}")
    assert e_mean <= bound and e_rstd <= bound
    if const is not None:
        assert torch.equal(out[const], bet.to(dtype)) and float(st[const, 0]) == 1.5


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [64, 96, 512])                        # bf16v, generic, widest: each kernel forms the flat dropout index itself
def test_layernorm_forward_dropout_and_addrow_match_fp64(D, dtype):
    K = sub("kernels")
    period, p, seed = 7, 0.1, 4711
    rows = 3 * period + 2                                           # row % period wraps mid-tensor and ends mid-period
    x, gam, bet, const, g = _inputs(rows, D, dtype, 77 + D)
    pos = torch.randn(period, D, generator=g)
    keep = torch.from_numpy(keep_mask(seed, rows * D, p)).view(rows, D)
    addrow = pos[torch.arange(rows) % period]
    p32 = float(np.float32(p))
    ln, _, _ = _ref_ln(x, gam, bet)
    ref = ln * keep / (1 - p32) + addrow.double()
    out, _ = K.layernorm_fwd(x.to(DEV), gam.to(DEV), bet.to(DEV), eps=EPS, drop_p=p, seed=seed, addrow=pos.to(DEV), period=period)
    torch.cuda.synchronize()
    out = out.cpu()
    # the same formula in torch fp32 on the CPU: 2.2e-7 ... 3.6e-7 of (1 + |ref|) over these six cases -> bound 1.7e-6 ... 2.9e-6
    cpu, bound = _fp32_bound(F.layer_norm(x.float(), (D,), gam, bet, EPS) * keep / np.float32(1 - p32) + addrow, ref)
    err = ((out.double() - ref).abs() - (2.0 ** -8 * ref.abs() if dtype == BF16 else 0)) / (1 + ref.abs())
    print(f"LN fwd dropout {rows}x{D} {dtype}: cpu fp32 {cpu:.2e} bound {bound:.2e} kernel {float(err.max()):.2e}")
    assert float(err.max()) <= bound
    assert 0 < int((~keep).sum()) < rows * D
    if dtype == F32:
        assert torch.equal(out[~keep], addrow[~keep])               # dropped: exactly the addend


# ---------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------
def _bwd_case(rows, D, dtype, fixed_order, *, p=0.0, addend=False, period=0, seed=0):
    L, K = sub("_lib"), sub("kernels")
    x, gam, bet, _, g = _inputs(rows, D, dtype, 31 * D + rows)
    dout = torch.randn(rows, D, generator=g).to(dtype)
    add = torch.randn(rows, D, generator=g).to(dtype) if addend else None
    keep = torch.from_numpy(keep_mask(seed, rows * D, p)).view(rows, D) if p > 0 else torch.ones(rows, D, dtype=torch.bool)
    p32 = float(np.float32(p))
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, gam, bet))
    y = F.layer_norm(xr, (D,), gr, br, EPS) * keep / (1 - p32)
    pr = None
    if period:
        pr = torch.zeros(period, D, dtype=torch.float64, requires_grad=True)
        y = y + pr[torch.arange(rows) % period]
    y.backward(dout.double())
    dx_ref = xr.grad + (add.double() if addend else 0)

    xd, gd, dd = x.to(DEV), gam.to(DEV), dout.to(DEV)
    _, st = K.layernorm_fwd(xd, gd, bet.to(DEV), eps=EPS)
    dx = torch.full_like(xd, 7.0)                                   # must be overwritten, whatever it held
    dgam, dbet = torch.full((D,), 0.25, device=DEV), torch.full((D,), 0.25, device=DEV)       # += contract
    dpos = torch.full((period, D), 0.25, device=DEV) if period else None
    addd = add.to(DEV) if addend else None
    ws = None
    if fixed_order:
        ws = torch.empty(K.reduce_ws("vqa_layernorm_bwd_ws", L.dt(dtype), rows, D, period), device=DEV)
    L.call("vqa_layernorm_bwd", L.dt(dtype), dd.data_ptr(), xd.data_ptr(), gd.data_ptr(), st.data_ptr(), L.ptr(addd), dx.data_ptr(),
           dgam.data_ptr(), dbet.data_ptr(), rows, D, float(p), seed, L.ptr(dpos), max(period, 1), L.ptr(ws), 0)
    torch.cuda.synchronize()
    rel = lambda a, b: float((a.double().cpu() - b).abs().max() / b.abs().max())
    bound = 2e-4 if dtype == F32 else 1.5e-2                        # the project's bounds (test_gpu_reproducible.py)
    errs = {"dx": rel(dx, dx_ref), "dgamma": rel(dgam - 0.25, gr.grad), "dbeta": rel(dbet - 0.25, br.grad)}
    if period:
        errs["dadd"] = rel(dpos - 0.25, pr.grad)
    print(f"LN bwd {rows}x{D} {dtype} fixed={fixed_order} p={p} addend={addend} period={period}: {errs}")
    for k, e in errs.items():
        assert e < bound, (k, e)


BWD_WIDTHS = [64, 128, 256, 512, 8, 40, 96, 320, 500]


@pytest.mark.parametrize("fixed_order", [True, False], ids=["fold", "atomics"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("i,D", list(enumerate(BWD_WIDTHS)))
def test_layernorm_backward_matches_fp64_autograd(i, D, dtype, fixed_order):
    _bwd_case(37, D, dtype, fixed_order, p=0.1 if i % 3 != 2 else 0.0, addend=i % 2 == 0, seed=900 + i)


@pytest.mark.parametrize("fixed_order", [True, False], ids=["fold", "atomics"])
def test_layernorm_backward_above_the_grid_cap(fixed_order):
    _bwd_case(16400, 64, BF16, fixed_order, p=0.1, addend=fixed_order, seed=5)       # > 1024 blocks x 16 rows


@pytest.mark.parametrize("fixed_order", [True, False], ids=["fold", "atomics"])
@pytest.mark.parametrize("dtype,D", [(F32, 96), (BF16, 64), (BF16, 500), (F32, 500)], ids=["fp32-96", "bf16-64", "bf16-500", "fp32-500"])
@pytest.mark.parametrize("rows", [50, 49])
def test_layernorm_backward_addrow_gradient(rows, dtype, D, fixed_order):
    """rows = 50, period = 7: rows % period != 0 sends dadd through the in-kernel atomics; rows = 49 takes the column-sum pass
    (when period * D is a whole number of 16-byte groups: 7 * 500 bf16 elements are not)."""
    _bwd_case(rows, D, dtype, fixed_order, p=0.1, addend=rows == 50, period=7, seed=rows + D)


def test_layernorm_refusals():
    L = sub("_lib")
    rows, D = 4, 520                                                # D > 512: no kernel holds such a row
    x = torch.zeros(rows, D, device=DEV)
    v = torch.ones(D, device=DEV)
    out, st = torch.full_like(x, 3.0), torch.full((rows, 2), 3.0, device=DEV)
    with pytest.raises(RuntimeError):
        L.call("vqa_layernorm_fwd", 0, x.data_ptr(), v.data_ptr(), v.data_ptr(), out.data_ptr(), st.data_ptr(), rows, D, EPS, 0.0, 0, None, 1)
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    with pytest.raises(RuntimeError):
        L.call("vqa_layernorm_bwd", 0, x.data_ptr(), x.data_ptr(), v.data_ptr(), st.data_ptr(), None, out.data_ptr(), dg.data_ptr(),
               db.data_ptr(), rows, D, 0.0, 0, None, 1, None, 0)
    torch.cuda.synchronize()
    assert (out == 3.0).all() and (st == 3.0).all() and (dg == 0).all() and (db == 0).all()      # nothing was launched
    assert L.count("vqa_layernorm_bwd_ws", 0, rows, D, 0) == 0 and L.count("vqa_layernorm_bwd_ws", 1, rows, D, 0) == 0
    D = 64
    x = torch.zeros(rows, D, device=DEV)
    v = torch.ones(D, device=DEV)
    st = torch.ones(rows, 2, device=DEV)
    dx = torch.full_like(x, 3.0)
    with pytest.raises(RuntimeError):                               # a deferred fold needs the scratch it folds
        L.call("vqa_layernorm_bwd", 0, x.data_ptr(), x.data_ptr(), v.data_ptr(), st.data_ptr(), None, dx.data_ptr(), dg.data_ptr(),
               db.data_ptr(), rows, D, 0.0, 0, None, 1, None, 1)
    torch.cuda.synchronize()
    assert (dx == 3.0).all()
