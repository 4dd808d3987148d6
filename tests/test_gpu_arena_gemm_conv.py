"""GPU: WHERE the GEMM, convolution and stem kernels read and write (gemm_conv.hip, gemm8p.hip, conv_c64.hip, stem_conv.hip,
stem_dgrad.hip, mxfp8.hip).  Every operand of every call sits in its own allocation [64 KiB moat | 16-byte skew | payload | 64 KiB
moat] (tests/_arena.py): the moats hold NaN in every float view (0xFF for byte operands: a NaN through the test's own byte table and
the NaN E8M0 scale), outputs and scratch are NaN-prefilled, scratch has exactly the size the matching query reports, and the
payload starts 16 bytes past a 512-byte boundary -- the least alignment layout.py promises.

Each test asserts (1) the outputs equal the exact-integer fp64 reference of tests/_exactint.py bit for bit -- a single stray NaN term
breaks that --, (2) arena.check(): no moat byte changed, inputs bit-identical, every output element overwritten, and (3) the same
call on plain exact-size buffers gives the same bits.  There is no tolerance in this file.

The premise -- a NaN term cannot hide behind a zero weight -- is tested in contract at the end: one case per MFMA family plants a
NaN at a pixel whose every weight is zero and wants exactly that pixel's receptive field NaN.

COVERED / EXEMPT are read by tests/test_arena_cpu.py: a new pointer-taking entry in one of the six sources without a case here
fails there, on the CPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _arena as A
import _exactint as X
import _mxfp8 as MX
import test_gpu_exact_integer as E
from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, U8, I64 = torch.bfloat16, torch.float32, torch.uint8, torch.int64
WIDE, NARROW = X.WIDE, X.NARROW
UNIT = (1, 1)                 # activations and weights in [-1, 1]: for statistics over tens of thousands of rows
DTYPES = [F32, BF]

COVERED = {
    "vqa_igemm", "vqa_linear_dgrad_act", "vqa_dgrad_s2", "vqa_pack_rows", "vqa_pack_transpose", "vqa_pack_transpose_batch",
    "vqa_gemm8p", "vqa_gemm4w", "vqa_conv8p",
    "vqa_conv3x3_c64p", "vqa_conv3x3_c64p_epi", "vqa_conv3x3_c64p_bnred", "vqa_conv3x3_c64p_bn",
    "vqa_wgrad3x3_c64", "vqa_wgrad3x3_c64_bn", "vqa_wgrad3x3_c128", "vqa_wgrad", "vqa_wgrad_group", "vqa_slab_reduce",
    "vqa_stem_pack", "vqa_stem_conv", "vqa_stem_conv_u8", "vqa_stem_conv_pool", "vqa_stem_conv_pool_u8",
    "vqa_stem_wgrad", "vqa_stem_wgrad_u8", "vqa_stem_wgrad_fused", "vqa_stem_wgrad_fused_u8",
    "vqa_stem_dgrad_pack", "vqa_stem_dgrad", "vqa_stem_dgrad_fused",
    "vqa_mx_quant", "vqa_conv_mxfp8", "vqa_fold_bn_mxfp8", "vqa_fold_bn_batch", "vqa_u8_norm_table",
}
EXEMPT = {}            # entry -> one-line reason; empty: every pointer-taking entry of the six sources has an arena case


# ------------------------------------------------------------------------------------------------ running one call twice
def run(entry, **kw):
    """call `entry` with its parameters BY NAME (include/vqa_hip.h through _lib.ARGNAMES); pointers not given are NULL"""
    L = sub("_lib")
    args = []
    for n, t in zip(L.ARGNAMES[entry], L.SIGNATURES[entry]):
        if t is L.P:
            v = kw.pop(n, None)
            args.append(v.data_ptr() if torch.is_tensor(v) else v)
        else:
            args.append(kw.pop(n))
    assert not kw, (entry, sorted(kw))
    L.call(entry, *args)


def _plain_out(shape, dtype):
    """an exact-size buffer holding the arena's fill pattern, so that untouched elements compare equal between the two runs"""
    n = 1
    for s in shape:
        n *= int(s)
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    return A.fill_bytes((nbytes + 3) // 4 * 4, dtype == U8)[:nbytes].clone().to(DEV).view(dtype).view(tuple(shape))


def both(entry, ins, outs, **scal):
    """Run `entry` on plain exact-size buffers and then inside an arena.  ins: name -> CPU tensor in its final dtype (None: NULL).
    outs: name -> ("out", shape, dtype[, may_stay]) | ("acc", cpu tensor) | ("scratch", floats).  Asserts arena.check() and the
    bit equality of the two runs; returns {name: CPU tensor} of the arena run's out / acc operands."""
    res = []
    for arena in (None, A.Arena(DEV)):
        kw, o = {}, {}
        for n, t in ins.items():
            if t is not None:
                kw[n] = t.contiguous().to(DEV) if arena is None else arena.put(t, name=f"{entry}.{n}")
        for n, spec in outs.items():
            nm = f"{entry}.{n}"
            if spec[0] == "out":
                o[n] = _plain_out(spec[1], spec[2]) if arena is None else \
                    arena.out(spec[1], spec[2], name=nm, may_stay=spec[3] if len(spec) > 3 else None)
            elif spec[0] == "acc":
                o[n] = spec[1].contiguous().to(DEV) if arena is None else arena.acc(spec[1], name=nm)
            else:
                o[n] = (_plain_out((spec[1],), F32) if arena is None else arena.scratch(spec[1], name=nm)) if spec[1] else None
        run(entry, **kw, **o, **scal)
        if arena is not None:
            arena.check()
        torch.cuda.synchronize()
        res.append({n: t.cpu() for n, t in o.items() if outs[n][0] != "scratch"})
    for n in res[0]:
        assert torch.equal(A.bits(res[0][n]), A.bits(res[1][n])), f"{entry}.{n}: the arena run and the plain run differ"
    return res[1]


def c(t, dtype):
    """fp64 reference operand -> the CPU tensor a kernel is handed"""
    return t.to(dtype).contiguous()


def krsc(w):
    """[Cout][Cin][R][S] fp64 -> the fp32 master layout [Cout][R][S][Cin] (CPU)"""
    return X.nhwc(w).float()


def zacc(k, ch):
    return ("acc", torch.zeros(E.words(k, ch), dtype=I64))


def packed_rows(w2d, dtype, kp=None):
    """vqa_pack_rows in an arena: [N][K] -> [N][Kp] in dtype, zero padded; checked against the cast"""
    n, k = w2d.shape
    kp = k if kp is None else kp
    got = both("vqa_pack_rows", {"in": c(w2d, F32)}, {"out": ("out", (n, kp), dtype)}, dtype=int(dtype == BF), N=n, K=k, Kp=kp)["out"]
    E.same(got, F.pad(w2d.to(dtype), (0, kp - k)))
    return got


def packed_t(w3d, dtype, flip=False):
    """vqa_pack_transpose in an arena: [N][T][C] -> [C][T*N] in dtype (taps reversed with flip)"""
    n, t, ch = w3d.shape
    got = both("vqa_pack_transpose", {"in": c(w3d, F32)}, {"out": ("out", (ch, t * n), dtype)}, dtype=int(dtype == BF), N=n, T=t, C=ch,
               ldo=t * n, col0=0, flip=int(flip))["out"]
    E.same(got, (w3d.flip(1) if flip else w3d).permute(2, 1, 0).reshape(ch, t * n).to(dtype))
    return got


def igemm(dtype, a, w, M, N, Kw, geom, *, loader=0, bias=None, addend=None, addmask=None, outmask=None, stats=None, transposed=0, relu=0):
    """vqa_igemm twice; stats: None | "slab" ([mtiles][2][N] as an out(): the moat behind it is the canary) | "acc".
    Returns (out, stats)."""
    B, H, W, C, Ho, Wo, R, S, stride, pad = geom
    outs = {"out": ("out", (M, N), dtype)}
    if stats == "slab":
        outs["stats"] = ("out", (sub("_lib").count("vqa_igemm_mtiles", M, N, loader), 2, N), F32)
    elif stats == "acc":
        outs["stats"] = zacc(2, N)
    r = both("vqa_igemm", dict(a=a, w=w, bias=bias, addend=addend, addmask=addmask, outmask=outmask), outs, dtype=int(dtype == BF),
             loader=loader, M=M, N=N, Kw=Kw, B=B, H=H, W=W, C=C, Ho=Ho, Wo=Wo, R=R, S=S, stride=stride, pad=pad, transposed=transposed,
             relu=relu, drop_p=0.0, drop_seed=0, stats_mode=int(stats == "acc"))
    return r["out"], r.get("stats")


def stats_of(summed):
    X.assert_resummed(summed)
    return torch.stack([summed.sum(0), (summed * summed).sum(0)])


# ------------------------------------------------------------------------------------------------ vqa_igemm
ARENA_IGEMM_CONV = [X.IGEMM_CONV[0], X.IGEMM_CONV[1], X.IGEMM_CONV[3]]


def _conv_geom(case):
    B, Cin, Cout, H, R, stride, pad = case[:7]
    Ho = (H + 2 * pad - R) // stride + 1
    return (B, H, H, Cin, Ho, Ho, R, R, stride, pad), B * Ho * Ho, R * R * Cin


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ARENA_IGEMM_CONV)
def test_igemm_conv_forward_bias_statistics(case, dtype):
    B, Cin, Cout, H, R, stride, pad, off = case
    geom, M, Kw = _conv_geom(case)
    d = X.cached("conv_infer_case", B, Cin, Cout, H, H, R, stride, pad, WIDE, off)
    X.assert_exact_range(d["ibound"])
    a, wp = c(X.nhwc(d["x"]), dtype), packed_rows(krsc(d["w"]).view(Cout, Kw).double(), dtype)
    y, _ = igemm(dtype, a, wp, M, Cout, Kw, geom)
    E.same(y, X.expect(d["y"], dtype))
    e = d["e"]
    a1, _ = igemm(dtype, a, wp, M, Cout, Kw, geom, bias=c(e["bias"], F32), relu=1)
    E.same(a1, X.conv1_expect(e, dtype))
    o2, _ = igemm(dtype, a, wp, M, Cout, Kw, geom, bias=c(e["bias"], F32), addend=c(e["add"], dtype), relu=2)
    E.same(o2, X.conv2_expect(e, dtype))
    # narrow range: the statistics slab (its high moat is the canary behind it) and the fixed-point accumulator
    n = X.cached("conv_case", B, Cin, Cout, H, H, R, stride, pad, NARROW)
    X.assert_exact_range(n["bound"])
    want = stats_of(X.expect(n["y"], dtype).double())
    a, wp = c(X.nhwc(n["x"]), dtype), c(krsc(n["w"]).view(Cout, Kw), dtype)
    y, slab = igemm(dtype, a, wp, M, Cout, Kw, geom, stats="slab")
    E.same(y, X.expect(n["y"], dtype))
    assert slab.shape[0] > 0 and torch.equal(slab.double().sum(0), want)
    y, acc = igemm(dtype, a, wp, M, Cout, Kw, geom, stats="acc")
    E.same(y, X.expect(n["y"], dtype))
    E.assert_acc(acc, 2, Cout, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_igemm_transposed_with_every_epilogue_operand(dtype):
    case = X.IGEMM_CONV[0]
    B, Cin, Cout, H, R, stride, pad, off = case
    geom, M, Kw = _conv_geom(case)
    d = X.cached("conv_case", B, Cin, Cout, H, H, R, stride, pad, WIDE, off, True)
    Md = B * H * H
    add, am, om = X.epilogue_operands((Md, Cin), 100 + Cin)
    X.assert_exact_range(d["dbound"] + float(add.abs().max()))
    wt = packed_t(krsc(d["w"]).view(Cout, R * R, Cin).double(), dtype)
    geom_d = (B, geom[4], geom[4], Cout, H, H, R, R, stride, pad)
    dy = c(X.nhwc(d["dy"]), dtype)
    base = X.expect(d["dx"], dtype)
    dx, _ = igemm(dtype, dy, wt, Md, Cin, R * R * Cout, geom_d, transposed=1)
    E.same(dx, base)
    t = dict(addend=c(add, dtype), addmask=c(am, dtype), outmask=c(om, dtype))
    for kw in E.epilogue_cases():
        got, _ = igemm(dtype, dy, wt, Md, Cin, R * R * Cout, geom_d, transposed=1, **{k: t[k] for k in kw})
        E.same(got, E.epilogue_expect(base, kw, add, am, om, dtype))


def test_igemm_window_loader_variant():
    K = sub("kernels")
    B, C, H, want = X.IGEMM_STAGES[0]
    geom = (B, H, H, C, H, H, 3, 3, 1, 1)
    M, Kw = B * H * H, 9 * C
    assert K.igemm_variant(BF, K.LOADER_NHWC, M, C, Kw, geom) == want
    d = X.cached("conv_case", B, C, C, H, H, 3, 1, 1, WIDE, False, True)
    X.assert_exact_range(max(d["bound"], d["dbound"]))
    a, wp = c(X.nhwc(d["x"]), BF), c(krsc(d["w"]).view(C, Kw), BF)
    y, _ = igemm(BF, a, wp, M, C, Kw, geom)
    E.same(y, X.rne_bf16(d["y"]))
    # the folded eval block's conv1 form (bias + ReLU) through the same window loader
    e = X.infer_epilogue(d["y"], X.infer_seed(B, C, C, H, 3, 1))
    X.assert_exact_range(d["bound"] + e["ebound"])
    a1, _ = igemm(BF, a, wp, M, C, Kw, geom, bias=c(e["bias"], F32), relu=1)
    E.same(a1, X.conv1_expect(e, BF))
    wt = packed_t(krsc(d["w"]).view(C, 9, C).double(), BF)
    dx, _ = igemm(BF, c(X.nhwc(d["dy"]), BF), wt, M, C, Kw, geom, transposed=1)
    E.same(dx, X.rne_bf16(d["dx"]))
    # statistics over the 392 M tiles of this instantiation.  50176 rows are summed per column, so the operands are drawn from
    # [-1, 1]: sum y^2 stays below 2^24 (asserted by stats_of) and every y is an integer below 256, exact in bf16
    n = X.cached("conv_case", B, C, C, H, H, 3, 1, 1, UNIT)
    X.assert_exact_range(n["bound"])
    assert torch.equal(X.rne_bf16(n["y"]).double(), n["y"])
    want = stats_of(n["y"])
    a, wp = c(X.nhwc(n["x"]), BF), c(krsc(n["w"]).view(C, Kw), BF)
    y, slab = igemm(BF, a, wp, M, C, Kw, geom, stats="slab")
    E.same(y, X.rne_bf16(n["y"]))
    assert slab.shape[0] == (M + 127) // 128 and torch.equal(slab.double().sum(0), want)
    y, acc = igemm(BF, a, wp, M, C, Kw, geom, stats="acc")
    E.same(y, X.rne_bf16(n["y"]))
    E.assert_acc(acc, 2, C, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_igemm_stem_loader(dtype):
    """the NCHW fp32 image in a NaN moat; K tail 147 -> the padded K (zero columns of the packed weight meet whatever the loader fetched)"""
    K = sub("kernels")
    B, H = 3, X.STEM_LOADER_HW
    Ho = (H + 6 - 7) // 2 + 1
    BK = 64 if dtype == BF else 32
    Kp = (147 + BK - 1) // BK * BK
    geom, M = (B, H, H, 3, Ho, Ho, 7, 7, 2, 3), B * Ho * Ho
    d = X.cached("stem_case", B, H, H, WIDE)
    X.assert_exact_range(d["bound"])
    wp = packed_rows(krsc(d["w"]).view(64, 147).double(), dtype, Kp)
    bias = X.ints((64,), 256, 77)
    y, _ = igemm(dtype, c(d["img"], F32), wp, M, 64, Kp, geom, loader=K.LOADER_STEM, bias=c(bias, F32))
    E.same(y, X.expect(d["y"] + bias, dtype))
    n = X.cached("stem_case", B, H, H, NARROW)
    want = stats_of(X.expect(n["y"], dtype).double())
    wp = c(F.pad(krsc(n["w"]).view(64, 147), (0, Kp - 147)), dtype)
    y, slab = igemm(dtype, c(n["img"], F32), wp, M, 64, Kp, geom, loader=K.LOADER_STEM, stats="slab")
    E.same(y, X.expect(n["y"], dtype))
    assert torch.equal(slab.double().sum(0), want)
    y, acc = igemm(dtype, c(n["img"], F32), wp, M, 64, Kp, geom, loader=K.LOADER_STEM, stats="acc")
    E.same(y, X.expect(n["y"], dtype))
    E.assert_acc(acc, 2, 64, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [X.LINEARS[1], X.LINEARS[0]], ids=["33x32x10", "17x1024x256"])
def test_igemm_linear(case, dtype):
    """(33, 32, 10): N below the tile, K below BK and N % VEC != 0 -- weight rows, bias and addend are read next to their end"""
    K = sub("kernels")
    M, Kin, N, off = case
    d = X.cached("linear_case", M, Kin, N, WIDE, off)
    X.assert_exact_range(d["bound"])
    geom = K.linear_geom(M, Kin)
    x, wp = c(d["x"], dtype), packed_rows(d["w"], dtype)
    out, _ = igemm(dtype, x, wp, M, N, Kin, geom, bias=c(d["bias"], F32), relu=1, addend=c(d["res"], dtype))
    E.same(out, X.expect(X.expect(d["pre"], dtype).double() + d["res"], dtype))
    if case == X.LINEAR_SCALAR_RELU2:
        r2 = X.cached("linear_relu2_case", M, Kin, N, WIDE, off)
        X.assert_exact_range(r2["ibound"])
        o2, _ = igemm(dtype, c(r2["x"], dtype), c(r2["w"], dtype), M, N, Kin, geom, bias=c(r2["e"]["bias"], F32),
                      addend=c(r2["e"]["add"], dtype), relu=2)
        E.same(o2, X.conv2_expect(r2["e"], dtype))
    n = X.cached("linear_case", M, Kin, N, NARROW, off)
    yn = n["x"] @ n["w"].t()
    X.assert_exact_range(n["bound"])
    want = stats_of(X.expect(yn, dtype).double())
    y, slab = igemm(dtype, c(n["x"], dtype), c(n["w"], dtype), M, N, Kin, geom, stats="slab")
    E.same(y, X.expect(yn, dtype))
    assert torch.equal(slab.double().sum(0), want)
    y, acc = igemm(dtype, c(n["x"], dtype), c(n["w"], dtype), M, N, Kin, geom, stats="acc")
    E.same(y, X.expect(yn, dtype))
    E.assert_acc(acc, 2, N, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("drop_p", [0.0, 0.5])
def test_linear_dgrad_act(drop_p, dtype):
    M, Kin, N = X.LINEAR_DGRAD_ACT
    d = X.cached("linear_dgrad_case", M, Kin, N, WIDE)
    X.assert_exact_range(d["bound"])
    wt = packed_t(d["w"].view(N, 1, Kin), dtype)
    add = X.ints((M, Kin), 64, 7100)
    for addend in (None, add):
        got = both("vqa_linear_dgrad_act", dict(dz=c(d["dz"], dtype), wt=wt, addend=None if addend is None else c(addend, dtype),
                                                outact=c(d["h"], dtype)), {"dx": ("out", (M, Kin), dtype)},
                   dtype=int(dtype == BF), drop_p=drop_p, M=M, Kin=Kin, N=N)["dx"]
        v = X.expect(d["y"], dtype).double()
        if addend is not None:
            v = X.expect(v + addend, dtype).double()
        E.same(got, X.expect(v * (d["h"] > 0) * (1.0 / (1.0 - drop_p)), dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", X.DGRAD_S2[:2], ids=["shortcut", "plain"])
def test_dgrad_s2(case, dtype):
    B, Cin, Cout, H, shortcut = case
    d = X.cached("dgrad_s2_case", B, Cin, Cout, H, shortcut, WIDE)
    X.assert_exact_range(d["bound"])
    Ho = H // 2
    ktot = (10 if shortcut else 9) * Cout
    # the operand [Cin][ktot]: the 3x3 pack at column 0 and the shortcut's 1x1 pack behind it, each launch leaving the other's columns
    w1, wd = krsc(d["w1"]).view(Cout, 9, Cin), krsc(d["wd"]).view(Cout, 1, Cin)
    want = torch.cat([w1.permute(2, 1, 0).reshape(Cin, 9 * Cout)] + ([wd.permute(2, 1, 0).reshape(Cin, Cout)] if shortcut else []), 1).to(dtype)
    cols = torch.arange(ktot)[None, :].expand(Cin, ktot)
    g1 = both("vqa_pack_transpose", {"in": w1}, {"out": ("out", (Cin, ktot), dtype, cols >= 9 * Cout)}, dtype=int(dtype == BF), N=Cout, T=9,
              C=Cin, ldo=ktot, col0=0, flip=0)["out"]
    E.same(g1[:, :9 * Cout].contiguous(), want[:, :9 * Cout].contiguous())
    if shortcut:
        g2 = both("vqa_pack_transpose", {"in": wd}, {"out": ("out", (Cin, ktot), dtype, cols < 9 * Cout)}, dtype=int(dtype == BF), N=Cout,
                  T=1, C=Cin, ldo=ktot, col0=9 * Cout, flip=0)["out"]
        E.same(g2[:, 9 * Cout:].contiguous(), want[:, 9 * Cout:].contiguous())
    dx = both("vqa_dgrad_s2", dict(dy=c(X.nhwc(d["dy"]), dtype), dyd=c(X.nhwc(d["dyd"]), dtype) if shortcut else None, wt=want),
              {"out": ("out", (B * H * H, Cin), dtype)}, dtype=int(dtype == BF), B=B, H=Ho, W=Ho, C=Cout, Ho=H, Wo=H, N=Cin, R=3, pad=1)["out"]
    E.same(dx, X.expect(d["dx"], dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_transpose_batch(dtype):
    """two pieces of one flat fp32 buffer (a flipped 3x3 pack and a 1x1 pack at a column offset) in one launch"""
    g = [(64, 9, 64, True), (40, 1, 24, False)]                      # N, T, C, flip
    srcs = [X.ints((n, t, ch), 100, 8000 + i) for i, (n, t, ch, _) in enumerate(g)]
    flat = torch.cat([s.reshape(-1) for s in srcs])
    ld1 = 48
    total = 64 * 9 * 64 + 24 * ld1
    rows, blk, soff = [], 0, 0
    for i, (n, t, ch, flip) in enumerate(g):
        rows.append([soff, 0 if i == 0 else 64 * 9 * 64, n, t, ch, t * n if i == 0 else ld1, 0 if i == 0 else 5, int(flip), blk, 0])
        blk += t * ((n + 31) // 32) * ((ch + 31) // 32)
        soff += n * t * ch
    want = torch.zeros(total, dtype=torch.float64)
    stay = torch.ones(total, dtype=torch.bool)
    want[:64 * 9 * 64] = srcs[0].flip(1).permute(2, 1, 0).reshape(-1)
    stay[:64 * 9 * 64] = False
    piece = want[64 * 9 * 64:].view(24, ld1)
    piece[:, 5:45] = srcs[1].permute(2, 1, 0).reshape(24, 40)
    stay[64 * 9 * 64:].view(24, ld1)[:, 5:45] = False
    got = both("vqa_pack_transpose_batch", dict(flat=c(flat, F32), desc=torch.tensor(rows, dtype=I64)), {"out": ("out", (total,), dtype, stay)},
               dtype=int(dtype == BF), nd=2, total_blocks=blk)["out"]
    E.same(got[~stay], want[~stay].to(dtype))


# ------------------------------------------------------------------------------------------------ gemm8p.hip
@pytest.mark.parametrize("entry", ["vqa_gemm8p", "vqa_gemm4w"])
def test_dense_gemm(entry):
    M, N, K = X.GEMM_CANARY[0]
    d = X.cached("gemm_case", M, N, K, WIDE)
    X.assert_exact_range(d["bound"])
    got = both(entry, dict(A=c(d["A"], BF), B=c(d["B"], BF)), {"C": ("out", (M, N), BF)}, M=M, N=N, K=K)["C"]
    E.same(got, X.rne_bf16(d["y"]))


def conv8p(x, w, B, H, W, C, N, *, transposed=0, stride=1, stats=False, addend=None, addmask=None, outmask=None, bnred=None):
    """vqa_conv8p twice.  bnred: (bn_y, bn_coef, selfmask, bn_y2 | None, bn_coef2 | None).  Returns (out, stats acc | None, bn_facc | None)."""
    Mo = B * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    ins = dict(x=x, w=w, addend=addend, addmask=addmask, outmask=outmask)
    outs = {"out": ("out", (Mo, N), BF)}
    if stats:
        outs["stats"] = zacc(2, N)
    selfmask = 1
    if bnred is not None:
        ins.update(bn_y=bnred[0], bn_coef=bnred[1], bn_y2=bnred[3], bn_coef2=bnred[4])
        selfmask = int(bnred[2])
        outs["bn_facc"] = zacc(3, N)
    r = both("vqa_conv8p", ins, outs, bn_selfmask=selfmask, B=B, H=H, W=W, C=C, N=N, transposed=transposed, stride=stride)
    return r["out"], r.get("stats"), r.get("bn_facc")


ARENA_CONV8P = [X.CONV8P[2], X.CONV8P[3], X.CONV8P[4]]


@pytest.mark.parametrize("B,H,W,C,N,stride", [k + (1,) for k in ARENA_CONV8P] + [X.CONV8P_S2[0] + (2,)])
def test_conv8p_forward_and_statistics(B, H, W, C, N, stride):
    """The kernel's descriptors start 4 KB below x and w, so the hardware bound no longer covers their low side.  At (1, 5, 9, 64, 256)
    and (1, 6, 10, 64, 128) one image row is 1152 / 1280 bytes: the left / top halo taps of the first pixels lie 128 .. 1408 bytes
    below x, inside that window, and read the low moat unless the per-tap range test drops them"""
    assert sub("kernels").conv8p_ok(B, H, W, C, N)
    d = X.cached("conv_case", B, C, N, H, W, 3, stride, 1, WIDE)
    X.assert_exact_range(d["bound"])
    y, _, _ = conv8p(c(X.rows(d["x"]), BF), c(X.nhwc(d["w"]).reshape(N, 9 * C), BF), B, H, W, C, N, stride=stride)
    E.same(y, X.rne_bf16(d["y"]))
    n = X.cached("conv_case", B, C, N, H, W, 3, stride, 1, NARROW)
    X.assert_exact_range(n["bound"])
    y, acc, _ = conv8p(c(X.rows(n["x"]), BF), c(X.nhwc(n["w"]).reshape(N, 9 * C), BF), B, H, W, C, N, stride=stride, stats=True)
    E.same(y, X.rne_bf16(n["y"]))
    E.assert_acc(acc, 2, N, stats_of(X.rne_bf16(n["y"]).double()))


@pytest.mark.parametrize("B,H,W,C,N", ARENA_CONV8P)
def test_conv8p_transposed_with_every_epilogue_operand(B, H, W, C, N):
    d = X.cached("transposed8p_case", B, H, W, C, N, WIDE)
    add, am, om = X.epilogue_operands(d["y"].shape, 200 + N)
    X.assert_exact_range(d["bound"] + float(add.abs().max()))
    x = c(X.rows(d["x"]), BF)
    wt = packed_t(d["w"].reshape(C, 9, N), BF).view(N, 9 * C)
    base = X.rne_bf16(d["y"])
    E.same(conv8p(x, wt, B, H, W, C, N, transposed=1)[0], base)
    t = dict(addend=c(add, BF), addmask=c(am, BF), outmask=c(om, BF))
    for kw in E.epilogue_cases():
        E.same(conv8p(x, wt, B, H, W, C, N, transposed=1, **{k: t[k] for k in kw})[0], E.epilogue_expect(base, kw, add, am, om, BF))


@pytest.mark.parametrize("B,H,W,C,N", ARENA_CONV8P)
def test_conv8p_batchnorm_backward_sums(B, H, W, C, N):
    """bn_y, bn_coef, bn_facc, bn_y2, bn_coef2 each in an arena of its own, in the self-masked, the masked and the dual form"""
    d = X.cached("bnred8p_case", B, H, W, C, N)
    X.assert_exact_range(d["bound"])
    x = c(X.rows(d["x"]), BF)
    wt = c(d["w"].reshape(C, 9, N).permute(2, 1, 0).reshape(N, 9 * C), BF)           # (the pack itself: tested above)
    y, coef = c(d["bn_y"], BF), c(d["coef"], F32)
    for form, (want, sums, bound) in d["forms"].items():
        X.assert_exact_range(bound)
        if form == "self":
            out, _, facc = conv8p(x, wt, B, H, W, C, N, transposed=1, bnred=(y, coef, True, None, None))
        else:
            dual = form == "dual"
            out, _, facc = conv8p(x, wt, B, H, W, C, N, transposed=1, addend=c(d["add"], BF), outmask=c(d["om"], BF),
                                  bnred=(y, coef, False, c(d["bn_y2"], BF) if dual else None, c(d["coef2"], F32) if dual else None))
        E.same(out, want)
        E.assert_acc(facc, 3, N, sums)


# ------------------------------------------------------------------------------------------------ conv_c64.hip
ARENA_C64P = X.C64P[:2]


def c64p(x, w, B, H, W, stats=None):
    outs = {"out": ("out", (B * H * W, 64), BF)}
    if stats == "slab":
        outs["stats"] = ("out", (sub("kernels").c64p_blocks(B, H, W), 2, 64), F32)
    elif stats == "acc":
        outs["stats"] = zacc(2, 64)
    r = both("vqa_conv3x3_c64p", dict(x=x, w=w), outs, B=B, H=H, W=W, stats_mode=int(stats == "acc"))
    return r["out"], r.get("stats")


@pytest.mark.parametrize("B,H,W", ARENA_C64P)
def test_conv3x3_c64p_forward_dgrad_epilogues(B, H, W):
    assert sub("kernels").c64p_blocks(B, H, W) > 0
    d = X.cached("conv_case", B, 64, 64, H, W, 3, 1, 1, WIDE, False, True)
    add, am, om = X.epilogue_operands(d["dx"].shape, 400 + H)
    X.assert_exact_range(max(d["bound"], d["dbound"]) + float(add.abs().max()))
    wk = krsc(d["w"])
    y, _ = c64p(c(X.nhwc(d["x"]), BF), c(wk.view(64, 576), BF), B, H, W)
    E.same(y, X.rne_bf16(d["y"]))
    wflip = packed_t(wk.view(64, 9, 64).double(), BF, flip=True)
    dy = c(X.nhwc(d["dy"]), BF)
    base = X.rne_bf16(d["dx"])
    E.same(c64p(dy, wflip, B, H, W)[0], base)
    t = dict(addend=c(add, BF), addmask=c(am, BF), outmask=c(om, BF))
    for kw in E.epilogue_cases(need_addend=True):
        got = both("vqa_conv3x3_c64p_epi", dict(x=dy, w=wflip, addend=t["addend"], addmask=t["addmask"] if "addmask" in kw else None,
                                                outmask=t["outmask"] if "outmask" in kw else None),
                   {"out": ("out", (B * H * W, 64), BF)}, B=B, H=H, W=W)["out"]
        E.same(got, E.epilogue_expect(base, kw, add, am, om, BF))


@pytest.mark.parametrize("B,H,W", ARENA_C64P)
def test_conv3x3_c64p_statistics_and_batchnorm_backward_sums(B, H, W):
    d = X.cached("c64p_narrow_case", B, H, W)
    X.assert_exact_range(max(d["bound"], d["dbound"]))
    want = stats_of(d["y"])
    wk = krsc(d["w"])
    x, wp = c(X.nhwc(d["x"]), BF), c(wk.view(64, 576), BF)
    y, slab = c64p(x, wp, B, H, W, stats="slab")
    E.same(y, X.rne_bf16(d["y"]))
    assert torch.equal(slab.double().sum(0), want)
    y, acc = c64p(x, wp, B, H, W, stats="acc")
    E.same(y, X.rne_bf16(d["y"]))
    E.assert_acc(acc, 2, 64, want)
    X.assert_exact_range(d["sums_bound"])
    wflip = c(wk.view(64, 9, 64).flip(1).permute(2, 1, 0).reshape(64, 576), BF)
    r = both("vqa_conv3x3_c64p_bnred", dict(x=c(X.nhwc(d["dy"]), BF), w=wflip, bn_y=c(d["bn_y"], BF), bn_coef=c(d["coef"], F32)),
             {"out": ("out", (B * H * W, 64), BF), "bn_facc": zacc(3, 64)}, B=B, H=H, W=W)
    E.same(r["out"], d["g"])
    E.assert_acc(r["bn_facc"], 3, 64, d["sums"])


@pytest.mark.parametrize("B,H,W", ARENA_C64P)
def test_conv3x3_c64p_bn_and_its_weight_gradient(B, H, W):
    """vqa_conv3x3_c64p_bn finalizes BatchNorm coefficients from statistics in fp64 (no exact-integer form): its reference is the pair
    the suite proves bit-equal (tests/test_gpu_cnn_fused.py), vqa_bn_apply_acc then vqa_conv3x3_c64p, on plain buffers."""
    K = sub("kernels")
    d = X.cached("c64p_narrow_case", B, H, W)
    wk = krsc(d["w"])
    x, w1 = c(X.nhwc(d["x"]), BF), c(wk.view(64, 576), BF)
    w2 = c(krsc(X.ints((64, 64, 3, 3), 1, 4242)).view(64, 576), BF)
    y1, acc1 = c64p(x, w1, B, H, W, stats="acc")
    gamma, beta = c(X.pow2s(64, 31), F32), c(X.ints((64,), 2, 32) / 4, F32)
    bnp = (gamma.to(DEV), beta.to(DEV), torch.zeros(64, device=DEV), torch.ones(64, device=DEV), torch.zeros((), device=DEV, dtype=I64))
    a1, coef_ref, _, _, _ = K.bn_apply_acc(y1.to(DEV), acc1.to(DEV), bnp, 64, True, B, H * W, B * H * W)
    y2_ref, _, _ = K.conv3x3_c64p(a1, w2.to(DEV), B, H, W)
    for stats in ("slab", "acc"):
        outs = {"out": ("out", (B * H * W, 64), BF), "coef_out": ("out", (4, 64), F32), "running_mean": ("acc", torch.zeros(64)),
                "running_var": ("acc", torch.ones(64)), "num_batches_tracked": ("acc", torch.zeros(1, dtype=I64)),
                "stats": ("out", (K.c64p_blocks(B, H, W), 2, 64), F32) if stats == "slab" else zacc(2, 64)}
        r = both("vqa_conv3x3_c64p_bn", dict(y=y1, acc=acc1, gamma=gamma, beta=beta, w=w2), outs, B=B, H=H, W=W,
                 stats_mode=int(stats == "acc"), count=float(B * H * W), momentum=0.1, eps=1e-5)
        E.same(r["out"], y2_ref.cpu())
        E.same(r["coef_out"], coef_ref.cpu().view(4, 64))
        assert torch.equal(r["running_mean"], bnp[2].cpu()) and torch.equal(r["running_var"], bnp[3].cpu()) and int(r["num_batches_tracked"]) == 1
    # the matching weight gradient: dw += dy^T gather(relu(y1 * coef[0] + coef[1])) == vqa_wgrad3x3_c64 on the materialised a1
    assert K.c64w_bn_ok(B, H, W)
    dy, dw0 = c(X.nhwc(d["dy"]), BF), X.prefill((64, 576), 702)
    dw_ref = dw0.float().to(DEV)
    K.wgrad3x3_c64(a1, dy.to(DEV), dw_ref, B, H, W)
    wsf = K.c64w_blocks(B, H, W) * 64 * 576
    r = both("vqa_wgrad3x3_c64_bn", dict(y=y1, coef=coef_ref.cpu(), dy=dy), {"dw": ("acc", dw0.float()), "ws": ("scratch", wsf)},
             B=B, H=H, W=W, ws_floats=wsf)
    E.same(r["dw"], dw_ref.cpu())


# ------------------------------------------------------------------------------------------------ weight gradients (fp32, +=)
@pytest.mark.parametrize("B,H,W", X.WGRAD_C64[:2])
def test_wgrad3x3_c64_and_its_batchnorm_prologue(B, H, W):
    """dw through acc() with a non-zero exact prefill, ws NaN-filled and of exactly the reported size; then ws = NULL (atomics)"""
    K = sub("kernels")
    assert K.c64w_blocks(B, H, W) > 0 and K.c64w_bn_ok(B, H, W)
    d = X.cached("wgrad_c64_case", B, H, W)
    X.assert_exact_range(max(d["bound"], d["bound_bn"]))
    x, dy, dw0 = c(X.nhwc(d["x"]), BF), c(X.nhwc(d["dy"]), BF), d["dw0"].float()
    wsf = K.c64w_blocks(B, H, W) * 64 * 576
    want = (X.wgrad_ref(d["x"], d["dy"], (64, 64, 3, 3), 1, 1) + d["dw0"]).float()
    for n in (wsf, 0):
        r = both("vqa_wgrad3x3_c64", dict(x=x, dy=dy), {"dw": ("acc", dw0), "ws": ("scratch", n)}, B=B, H=H, W=W, ws_floats=n)
        E.same(r["dw"], want)
    r = both("vqa_wgrad3x3_c64_bn", dict(y=x, coef=c(d["coef"], F32), dy=dy), {"dw": ("acc", dw0), "ws": ("scratch", wsf)}, B=B, H=H, W=W,
             ws_floats=wsf)
    E.same(r["dw"], (X.wgrad_ref(d["xin"], d["dy"], (64, 64, 3, 3), 1, 1) + d["dw0"]).float())


def test_wgrad3x3_c128():
    K = sub("kernels")
    B, H, W = X.WGRAD_C128_B[0], 28, 28
    wsf = K.c128_wgrad_blocks(B, H, W) * 128 * 576
    assert wsf > 0
    d = X.cached("wgrad_c128_case", B)
    X.assert_exact_range(d["bound"])
    r = both("vqa_wgrad3x3_c128", dict(x=c(X.nhwc(d["x"]), BF), dy=c(X.nhwc(d["dy"]), BF)), {"dw": ("acc", d["dw0"].float()), "ws": ("scratch", wsf)},
             B=B, H=H, W=W, ws_floats=wsf)
    E.same(r["dw"], (X.wgrad_ref(d["x"], d["dy"], (128, 128, 3, 3), 1, 1) + d["dw0"]).float())


@pytest.mark.parametrize("case,atomics", [(X.WGRAD_PLAN[0], False), (X.WGRAD_PLAN[0], True), (X.WGRAD_PLAN[1], False)],
                         ids=["kind0", "kind0-atomics", "kind1"])
def test_wgrad_planner_kinds(case, atomics):
    """the first case of each planner kind (4-wave split kernel, 8-wave LDS-DMA kernel) with the workspace at exactly the planned
    size, and the 4-wave case once more with ws = NULL: fp32 atomics (exact on integers in any order)"""
    K = sub("kernels")
    B, Cin, Cout, H, R, stride, pad, expect = case
    geom, M, Kw = _conv_geom(case)
    plan = K.wgrad_plan(BF, 0, M, Cout, Kw, B, H, H, Cin, R, R)
    assert plan[:3] == expect and plan[3] > 1 and plan[4] > 0, plan
    d = X.cached("wgrad_plan_case", case)
    X.assert_exact_range(d["bound"])
    wsf = 0 if atomics else plan[4]
    r = both("vqa_wgrad", dict(dy=c(X.nhwc(d["dy"]), BF), x=c(X.nhwc(d["x"]), BF)), {"dw": ("acc", d["dw0"].float()), "ws": ("scratch", wsf)},
             dtype=1, loader=0, M=M, N=Cout, Kw=Kw, B=B, H=H, W=H, C=Cin, Ho=geom[4], Wo=geom[5], R=R, S=R, stride=stride, pad=pad, ws_floats=wsf)
    want = (X.wgrad_ref(d["x"], d["dy"], (Cout, Cin, R, R), stride, pad) + d["dw0"]).float()
    X.cached.cache_clear()                                  # (the kind-1 case is about 600 MB of fp64)
    E.same(r["dw"], want)


def test_wgrad_group_three_jobs():
    """host arrays of device pointers: every dy, x and dw in an arena of its own, the shared workspace at exactly vqa_wgrad_group_ws"""
    L = sub("_lib")
    n = len(X.WGRAD_GROUP)
    IA, VP = ctypes.c_int * n, ctypes.c_void_p * n
    Ms, Ns, Ks = (IA(*[g[i] for g in X.WGRAD_GROUP]) for i in range(3))
    wsf = L.count("vqa_wgrad_group_ws", 1, n, Ms, Ns, Ks)
    assert wsf > 0
    cases = [X.wgrad_group_case(i) for i in range(n)]
    got = []
    for use_arena in (False, True):
        ar = A.Arena(DEV)
        if use_arena:
            dy = [ar.put(d["dy"], BF, name=f"dy{i}") for i, d in enumerate(cases)]
            x = [ar.put(d["x"], BF, name=f"x{i}") for i, d in enumerate(cases)]
            dw = [ar.acc(d["dw0"], F32, name=f"dw{i}") for i, d in enumerate(cases)]
            ws = ar.scratch(wsf, name="ws")
        else:
            dy, x = [c(d["dy"], BF).to(DEV) for d in cases], [c(d["x"], BF).to(DEV) for d in cases]
            dw, ws = [c(d["dw0"], F32).to(DEV) for d in cases], _plain_out((wsf,), F32)
        L.call("vqa_wgrad_group", 1, n, VP(*[t.data_ptr() for t in dy]), VP(*[t.data_ptr() for t in x]), VP(*[t.data_ptr() for t in dw]),
               Ms, Ns, Ks, ws.data_ptr(), wsf)
        ar.check()
        got.append([t.cpu() for t in dw])
    for i, d in enumerate(cases):
        X.assert_exact_range(d["bound"])
        E.same(got[1][i], (d["dy"].t() @ d["x"] + d["dw0"]).float())
        assert torch.equal(got[0][i], got[1][i])


@pytest.mark.parametrize("nslabs,n", [(3, 64 * 576), (33, 64 * 147 + 0), (40, 20)], ids=["reduce", "reduce2", "reduce2-one-vector-row"])
def test_slab_reduce(nslabs, n):
    """both reduce kernels (few slabs | >= 32 slabs over 16 thread groups); the workspace is an INPUT here: it must come back unchanged"""
    ws, dw0 = X.ints((nslabs, n), 64, 9000 + n), X.prefill((n,), 9001)
    r = both("vqa_slab_reduce", dict(ws=c(ws, F32)), {"dw": ("acc", dw0.float())}, nslabs=nslabs, n=n)
    E.same(r["dw"], (ws.sum(0) + dw0).float())


# ------------------------------------------------------------------------------------------------ stem
def byte_table():
    """the test's own [3][256] bf16 table: table[c][v] = v for v < 255 (exact in bf16) and NaN at 255 -- a stray moat byte is a NaN,
    and the fp32 entry fed the same integers is the reference"""
    t = torch.arange(256.0).repeat(3, 1)
    t[:, 255] = float("nan")
    assert torch.equal(t[:, :255].to(BF).float(), t[:, :255])
    return t.to(BF)


def test_u8_norm_table():
    import _bytesref as R
    mean, std = R.ODD
    names = ("mean0", "mean1", "mean2", "std0", "std1", "std2")
    got = both("vqa_u8_norm_table", {}, {"table": ("out", (3, 256), BF)}, **dict(zip(names, [float(v) for v in (*mean, *std)])))["table"]
    assert torch.equal(got.view(torch.int16), R.table(mean, std).view(torch.int16))


def hwc_bytes(img):
    """integer NCHW image (0 .. 254) -> the uint8 [B][H][W][3] batch"""
    assert float(img.min()) >= 0 and float(img.max()) < 255
    return img.permute(0, 2, 3, 1).contiguous().to(U8)


def stem_packed(w):
    """vqa_stem_pack in an arena (the [64][192] bf16 layout is the kernel's own: pinned by the exact conv results that use it)"""
    return both("vqa_stem_pack", dict(w_krsc=krsc(w)), {"wstem": ("out", (64, 192), BF)})["wstem"]


def _img_ins(img, u8):
    return dict(img_hwc=hwc_bytes(img), table=byte_table()) if u8 else dict(img=c(img, F32))


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
def test_stem_conv(u8):
    K = sub("kernels")
    B, (H, W) = 3, X.STEM_CONV_HW[0]
    nb = K.stem_conv_blocks(B, H, W)
    assert nb > 0
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    d = X.cached("stem_case", B, H, W, WIDE)
    X.assert_exact_range(d["bound"])
    entry = "vqa_stem_conv_u8" if u8 else "vqa_stem_conv"
    r = both(entry, dict(wstem=stem_packed(d["w"]), **_img_ins(d["img"], u8)), {"out": ("out", (B * Ho * Wo, 64), BF)}, B=B, H=H, W=W)
    E.same(r["out"], X.rne_bf16(d["y"]))
    # the statistics slab [blocks][2][64]: column sums and sums of squares of the fp32 ACCUMULATORS (the kernel adds v and v * v
    # before the bf16 conversion).  Narrow signed weights, the image shifted to 0 .. 4 (bytes are unsigned; the padding stays 0)
    n = X.cached("stem_case", B, H, W, NARROW, False)
    img = n["img"] + 2
    X.assert_exact_range(X.reduction_bound(147, img, n["w"]))
    yn = X.rows(X.conv_ref(img, n["w"], 2, 3))
    want = stats_of(yn)
    r = both(entry, dict(wstem=stem_packed(n["w"]), **_img_ins(img, u8)),
             {"out": ("out", (B * Ho * Wo, 64), BF), "stats": ("out", (nb, 2, 64), F32)}, B=B, H=H, W=W)
    E.same(r["out"], X.rne_bf16(yn))
    assert torch.equal(r["stats"].double().sum(0), want)


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
def test_stem_conv_pool(u8):
    L = sub("_lib")
    B, (H, W) = 3, X.STEM_POOL_HW[1]
    assert L.count("vqa_stem_conv_pool_ok", B, H, W) == 1
    d = X.cached("stem_pool_case", B, H, W)
    X.assert_exact_range(d["bound"])
    coef = c(torch.cat([d["scale"], d["shift"], torch.zeros(128, dtype=torch.float64)]), F32)
    entry = "vqa_stem_conv_pool_u8" if u8 else "vqa_stem_conv_pool"
    r = both(entry, dict(wstem=stem_packed(d["w"]), coef=coef, **_img_ins(d["img"], u8)), {"out": ("out", tuple(d["pooled"].shape), BF)}, B=B, H=H, W=W)
    E.same(r["out"], X.rne_bf16(d["pooled"]))


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
def test_stem_wgrad(u8):
    L = sub("_lib")
    B, (H, W) = 3, X.STEM_WGRAD_HW[0]
    d = X.cached("stem_wgrad_case", B, H, W)
    X.assert_exact_range(d["bound"])
    img = d["img"] + 2                                   # bytes are unsigned: shift the narrow range to 0 .. 4, the bound grows by the same 2
    X.assert_exact_range(X.reduction_bound(d["dy"].shape[0] * d["dy"].shape[2] * d["dy"].shape[3], img, d["dy"], d["dw0"]))
    wsf = L.count("vqa_stem_wgrad_blocks", B, H, W) * 64 * 147
    assert wsf > 0
    entry = "vqa_stem_wgrad_u8" if u8 else "vqa_stem_wgrad"
    want = (X.wgrad_ref(img, d["dy"], (64, 3, 7, 7), 2, 3) + d["dw0"]).float()
    for n in (wsf, 0):
        r = both(entry, dict(dy=c(X.nhwc(d["dy"]), BF), **_img_ins(img, u8)), {"dw": ("acc", d["dw0"].float()), "ws": ("scratch", n)},
                 B=B, H=H, W=W, ws_floats=n)
        E.same(r["dw"], want)


def _fused_case(B, H, W, seed):
    """exact stem-tail operands (tests/_stemref.exact_operands) with the pooling kernel's own codes, as CPU tensors, and dy: the fp64
    BatchNorm / ReLU / MaxPool backward of them rounded to bf16 -- exactly what the fused kernels rebuild per row"""
    import test_gpu_stem_tail_fp64 as T
    (yd, dpd, idx_d, coef, bcd), dyb, _ = T._fused_operands(B, H, W, seed)
    return dict(y=yd.cpu(), dpool=dpd.cpu(), idx=idx_d.cpu(), coef=coef.cpu(), bcoef=bcd.cpu()), dyb


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
def test_stem_wgrad_fused(u8):
    """dy is a multiple of 2^-6 and the image an integer in 0 .. 4: every partial sum is exact, the reference is fp64"""
    L = sub("_lib")
    B, (H, W) = 2, X.STEM_WGRAD_HW[0]
    ops, dyb = _fused_case(B, H, W, 71)
    img, dw0 = X.ints((B, 3, H, W), 4, 72, True), X.prefill((64, 147), 73)
    assert torch.equal((dyb * 64).round(), dyb * 64)
    X.assert_exact_range(64 * (dyb.shape[0] * dyb.shape[2] * dyb.shape[3] * 4 * float(dyb.abs().max()) + 64))
    wsf = L.count("vqa_stem_wgrad_blocks", B, H, W) * 64 * 147
    want = (X.wgrad_ref(img, dyb, (64, 3, 7, 7), 2, 3) + dw0).float()
    r = both("vqa_stem_wgrad_fused_u8" if u8 else "vqa_stem_wgrad_fused", dict(**ops, **_img_ins(img, u8)),
             {"dw": ("acc", dw0.float()), "ws": ("scratch", wsf)}, B=B, H=H, W=W, ws_floats=wsf)
    E.same(r["dw"], want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_stem_dgrad(dtype):
    B, (H, W) = 2, X.STEM_DGRAD_HW
    d = X.cached("stem_dgrad_case", B, H, W)
    X.assert_exact_range(d["bound"])
    wpk = both("vqa_stem_dgrad_pack", dict(w_krsc=krsc(d["w"])), {"wpk": ("out", (16 * 1024,), dtype)}, dtype=int(dtype == BF))["wpk"]
    r = both("vqa_stem_dgrad", dict(dy=c(X.rows(d["dy"]), dtype), wpk=wpk), {"dimg": ("out", (B, 3, H, W), F32)}, dtype=int(dtype == BF), B=B, H=H, W=W)
    E.same(r["dimg"], d["dimg"].float())


def test_stem_dgrad_fused():
    K = sub("kernels")
    B, (H, W) = 2, X.STEM_DGRAD_HW
    assert K.stem_dgrad_fused_ok(B, H, W)
    ops, dyb = _fused_case(B, H, W, 81)
    w = X.ints((64, 3, 7, 7), WIDE[1], 82)
    assert torch.equal((dyb * 64).round(), dyb * 64)
    X.assert_exact_range(64 * 16 * 64 * float(dyb.abs().max()) * WIDE[1])
    wpk = both("vqa_stem_dgrad_pack", dict(w_krsc=krsc(w)), {"wpk": ("out", (16 * 1024,), BF)}, dtype=1)["wpk"]
    r = both("vqa_stem_dgrad_fused", dict(wpk=wpk, **ops), {"dimg": ("out", (B, 3, H, W), F32)}, B=B, H=H, W=W)
    E.same(r["dimg"], X.dgrad_ref(dyb, w, 2, 3, (H, W)).float())


# ------------------------------------------------------------------------------------------------ mxfp8.hip
MX_CASES = [(2, 56, 64, 64, 3, 1), (3, 14, 256, 512, 1, 2)]          # B, H, Cin, Cout, R, stride: test_gpu_mxfp8.SHAPES' smallest 3x3 and its 1x1 / 2


def _mx_operands(B, H, C, N, R):
    """integers times per-block powers of two: exact e4m3 values with block scales that differ, every partial sum exact in fp32"""
    g = torch.Generator().manual_seed(B + H + C + N + R)
    xi, wi = X.ints((B * H * H, C), 4, 9100 + C), X.ints((N, R * R * C), 4, 9101 + C)
    xe = torch.randint(-2, 3, (B * H * H, C // 32), generator=g).double()
    we = torch.randint(-2, 3, (N, R * R * C // 32), generator=g).double()
    x, w = xi * torch.exp2(xe).repeat_interleave(32, 1), wi * torch.exp2(we).repeat_interleave(32, 1)
    X.assert_exact_range(64 * (R * R * C * 16 * 16 + 1024))                        # in units of 2^-4, bias and addend included
    return x, w


@pytest.mark.parametrize("B,H,C,N,R,stride", MX_CASES, ids=["3x3", "1x1s2"])
def test_mxfp8_quantizer_and_conv(B, H, C, N, R, stride):
    """codes and scale codes in 0xFF moats: a stray scale byte is the NaN scale, a stray code byte is an e4m3 NaN"""
    pad = 1 if R == 3 else 0
    Ho = (H + 2 * pad - R) // stride + 1
    M = B * Ho * Ho
    x, w = _mx_operands(B, H, C, N, R)
    for dtype in DTYPES:
        r = both("vqa_mx_quant", {"in": c(x, dtype)}, {"q": ("out", tuple(x.shape), U8), "s": ("out", (x.shape[0], C // 32), U8)},
                 dtype=int(dtype == BF), M=x.shape[0], C=C)
        xq = MX.quant(c(x, dtype))
        assert torch.equal(r["q"], xq[0]) and torch.equal(r["s"], xq[1])
    wq = MX.quant(w.float())
    assert torch.equal(MX.dequant(*xq), x) and torch.equal(MX.dequant(*wq), w)
    bias, add = X.ints((N,), 64, 9200), X.ints((M, N), 64, 9201)
    y = F.conv2d(x.view(B, H, H, C).permute(0, 3, 1, 2), w.view(N, R, R, C).permute(0, 3, 1, 2), stride=stride, padding=pad)
    y = X.rows(y) + bias
    want = X.rne_bf16(torch.relu(X.rne_bf16(y).double() + add))
    r = both("vqa_conv_mxfp8", {"a": xq[0], "as": xq[1], "w": wq[0], "ws": wq[1], "bias": c(bias, F32), "addend": c(add, BF)},
             {"out": ("out", (M, N), BF), "oq": ("out", (M, N), U8), "os": ("out", (M, N // 32), U8)},
             M=M, N=N, B=B, H=H, W=H, C=C, Ho=Ho, Wo=Ho, R=R, S=R, stride=stride, pad=pad, relu=2)
    E.same(r["out"], want)
    oq = MX.quant(want)
    assert torch.equal(r["oq"], oq[0]) and torch.equal(r["os"], oq[1])


FOLD_PIECES = [(64, 576), (48, 64)]                                   # N, K of two convs folded in one launch


@pytest.mark.parametrize("form", ["fp32", "bf16", "mxfp8"])
def test_fold_bn_batch_and_its_mxfp8_form(form):
    """Eval Conv+BN fold over a device table that holds the DEVICE POINTERS of the running statistics: the table is built per run,
    after they are placed.  eps = 0, running_var in {1/4, 1, 4} and gamma a power of two make the scale an exact power of two, so the
    folded integer weights, their e4m3 codes and the bias are exact.  A gap of 32 elements between the pieces must stay untouched."""
    L = sub("_lib")
    flat, rows, rm, rv, want_w, want_b = [], [], [], [], [], []
    foff = woff = boff = blk = 0
    stay_w, stay_b = [], []
    for i, (n, k) in enumerate(FOLD_PIECES):
        w, gamma, beta = X.ints((n, k), 4, 9300 + i), X.pow2s(n, 9310 + i, signed=True), X.ints((n,), 8, 9320 + i)
        m, v = X.ints((n,), 4, 9330 + i), X.pow2s(n, 9340 + i) ** 2
        flat += [w.reshape(-1), gamma, beta]
        rm.append(m), rv.append(v)
        sc = gamma / v.sqrt()
        want_w.append(torch.cat([(w * sc[:, None]).reshape(-1), torch.zeros(32, dtype=torch.float64)]))
        want_b.append(torch.cat([beta - m * sc, torch.zeros(8, dtype=torch.float64)]))
        stay_w.append(torch.cat([torch.zeros(n * k, dtype=torch.bool), torch.ones(32, dtype=torch.bool)]))
        stay_b.append(torch.cat([torch.zeros(n, dtype=torch.bool), torch.ones(8, dtype=torch.bool)]))
        rows.append([foff, foff + n * k, foff + n * k + n, None, None, n, k, woff, boff, blk])
        foff, woff, boff, blk = foff + n * k + 2 * n, woff + n * k + 32, boff + n + 8, blk + (n * k + 255) // 256
    flat, want_w, want_b, stay_w, stay_b = (torch.cat(t) for t in (flat, want_w, want_b, stay_w, stay_b))
    wdt = {"fp32": F32, "bf16": BF, "mxfp8": U8}[form]
    got = []
    for use_arena in (False, True):
        ar = A.Arena(DEV)
        put = (lambda t, dt, nm: ar.put(t, dt, name=nm)) if use_arena else (lambda t, dt, nm: c(t, dt).to(DEV))
        out = (lambda shape, dt, nm, stay: ar.out(shape, dt, name=nm, may_stay=stay)) if use_arena else (lambda shape, dt, nm, stay: _plain_out(shape, dt))
        fl = put(flat, F32, "flat")
        ms, vs = [put(t, F32, f"running_mean{i}") for i, t in enumerate(rm)], [put(t, F32, f"running_var{i}") for i, t in enumerate(rv)]
        table = put(torch.tensor([r[:3] + [ms[i].data_ptr(), vs[i].data_ptr()] + r[5:] for i, r in enumerate(rows)], dtype=I64), I64, "desc")
        wout, bout = out((woff,), wdt, "wout", stay_w), out((boff,), F32, "bout", stay_b)
        if form == "mxfp8":
            sout = out((woff // 32,), U8, "ws", stay_w.view(-1, 32).all(1))
            L.call("vqa_fold_bn_mxfp8", fl.data_ptr(), wout.data_ptr(), sout.data_ptr(), bout.data_ptr(), table.data_ptr(), len(rows), blk, 0.0)
        else:
            sout = None
            L.call("vqa_fold_bn_batch", int(form == "bf16"), fl.data_ptr(), wout.data_ptr(), bout.data_ptr(), table.data_ptr(), len(rows), blk, 0.0)
        ar.check()
        torch.cuda.synchronize()
        got.append([t.cpu() for t in (wout, bout, sout) if t is not None])
    for a, b in zip(*got):
        assert torch.equal(A.bits(a), A.bits(b))
    wout, bout = got[1][0], got[1][1]
    E.same(bout[~stay_b], want_b[~stay_b].float())
    if form == "mxfp8":
        q, s = MX.quant(want_w.float().view(-1, 32))
        keep = ~stay_w.view(-1, 32).all(1)
        assert torch.equal(MX.dequant(q, s)[keep], want_w.view(-1, 32)[keep])
        assert torch.equal(wout.view(-1, 32)[keep], q[keep]) and torch.equal(got[1][2][keep], s.view(-1)[keep])
    else:
        assert torch.equal(want_w.to(wdt).double(), want_w)
        E.same(wout[~stay_w], want_w[~stay_w].to(wdt))


# ------------------------------------------------------------------------------------------------ the premise, in contract
def _field(B, H, W, Ho, Wo, b, ph, pw, R, stride, pad):
    """[B*Ho*Wo] bool: the outputs whose R x R window (stride, pad) holds input pixel (b, ph, pw)"""
    hit = torch.zeros(B, Ho, Wo, dtype=torch.bool)
    for ho in range(Ho):
        for wo in range(Wo):
            hit[b, ho, wo] = 0 <= ph - (ho * stride - pad) < R and 0 <= pw - (wo * stride - pad) < R
    assert 0 < int(hit.sum()) < hit.numel()
    return hit.view(-1)


def _assert_poisoned_exactly(got, want, hit, nan_inside=True):
    got, want = got.view(hit.numel(), -1), want.view(hit.numel(), -1)
    if nan_inside:
        assert bool(torch.isnan(got[hit].float()).all()), "a NaN operand met zero weights and vanished: the file's premise does not hold"
    bad = ((got.float() != want.float()) | torch.isnan(got.float())).any(1) & ~hit
    assert not bool(bad.any()), f"{int(bad.sum())} outputs outside the pixel's receptive field changed; first rows {bad.nonzero().view(-1)[:8].tolist()}"


@pytest.mark.parametrize("family", ["igemm-bf16", "igemm-fp32", "conv8p", "c64p", "stem-conv", "stem-conv-pool"])
def test_a_nan_behind_zero_weights_reaches_exactly_its_receptive_field(family):
    """One NaN pixel (every channel) in the activation and ALL weights zero: 0 x NaN is NaN in the MFMA and nowhere masked away, so
    exactly the outputs whose window holds the pixel are NaN and every other output is the exact zero.  With that, a stray moat
    element cannot hide behind a zero weight, a zero-padded K column or a masked tap in any test above.
    The stem kernels contract over (c, r, s8) with s padded 7 -> 8: the eighth value is the pixel right of the window and meets a zero
    weight.  The kernels mask that operand word: unmasked, a NaN at pixel column 42 reaches conv column 19, whose window ends at 41."""
    K = sub("kernels")
    if family.startswith("stem-conv"):
        # column 42: the conv column 19, whose window ends at pixel 41, lies in no pooling window that a true hit (20 .. 22) shares
        B, H, W, b, ph, pw = 3, 64, 64, 1, 21, 42
        Ho, Wo = 32, 32
        img = X.ints((B, 3, H, W), 8, 1, True)
        img[b, :, ph, pw] = float("nan")
        ins = dict(img=c(img, F32), wstem=torch.zeros(64, 192, dtype=BF))
        hit = _field(B, H, W, Ho, Wo, b, ph, pw, 7, 2, 3)
        if family == "stem-conv":
            r = both("vqa_stem_conv", ins, {"out": ("out", (B * Ho * Wo, 64), BF)}, B=B, H=H, W=W)
            return _assert_poisoned_exactly(r["out"], torch.zeros(B * Ho * Wo, 64, dtype=BF), hit)
        # the one-launch inference stem: conv = 0, so every pooled value is relu(shift); what its max does with a NaN is the kernel's
        # own business, but outside the pooling windows over the pixel's receptive field nothing may change
        shift = X.ints((64,), 4, 3)
        coef = c(torch.cat([torch.ones(64, dtype=torch.float64), shift, torch.zeros(128, dtype=torch.float64)]), F32)
        Hp, Wp = Ho // 2, Wo // 2
        phit = F.max_pool2d(hit.view(B, 1, Ho, Wo).float(), 3, 2, 1).bool().view(-1)
        assert int(phit.sum()) == 6 and not bool(phit.view(B, Hp, Wp)[b, :, 9].any())          # pooled column 9 holds conv column 19
        r = both("vqa_stem_conv_pool", dict(coef=coef, **ins), {"out": ("out", (B * Hp * Wp, 64), BF)}, B=B, H=H, W=W)
        return _assert_poisoned_exactly(r["out"], torch.relu(shift).to(BF).expand(B * Hp * Wp, 64), phit, nan_inside=False)
    if family.startswith("igemm"):
        dtype = BF if family.endswith("bf16") else F32
        B, H, W, C, N, b, ph, pw = 2, 12, 12, 64, 64, 1, 0, 11
    else:
        dtype = BF
        B, H, W, C, N, b, ph, pw = (5, 7, 7, 128, 384, 4, 6, 6) if family == "conv8p" else (3, 16, 24, 64, 64, 2, 15, 0)
    x = X.ints((B, H, W, C), 8, 2)
    x[b, ph, pw, :] = float("nan")
    x2d, w0, M = c(x.view(-1, C), dtype), torch.zeros(N, 9 * C, dtype=dtype), B * H * W
    if family.startswith("igemm"):
        got, _ = igemm(dtype, x2d, w0, M, N, 9 * C, (B, H, W, C, H, W, 3, 3, 1, 1))
    elif family == "conv8p":
        got = conv8p(x2d, w0, B, H, W, C, N)[0]
    else:
        got = c64p(x2d, w0, B, H, W)[0]
    _assert_poisoned_exactly(got, torch.zeros(M, N, dtype=dtype), _field(B, H, W, H, W, b, ph, pw, 3, 1, 1))
