"""float64 references of the residual blocks' BatchNorm kernels (csrc/batchnorm.hip: bn_reduce_partials / bn_finalize / bn_eval_coef /
bn_fwd in its plain, pool and accumulator forms / bn_bwd_reduce / bn_bwd_finalize / bn_bwd_apply with and without accumulators, and
bn_acc_coef with the fixed-point accumulator helpers of csrc/common.h), their operand generators, their bounds, and a host encoder / decoder of the
accumulator format.  Plain torch on the CPU, nothing of the package.  test_bn_ref_cpu.py validates all of it without a GPU
(autograd, exact round trips, sign margins, mutants); test_gpu_batchnorm_fp64.py judges the kernels against it.

Layout: activations [rows][C] (NHWC flattened) in the storage dtype, per-channel vectors fp32; references take the STORED operand
values (bf16 / fp32 tensors, fp32 coefficients) and compute in fp64.

Bounds.  u = 2^-24 (one fp32 rounding of a result r costs at most u |r|), one bf16 store costs 2^-8 |ref| (the project's figure; the
fp32 error e in front of it is carried as e (1 + 2^-8)).  Every bound is per element or per channel.
  forward (apply_bound):  n u M, M = |y scale| + |shift| [+ |res| | + |res rscale| + |rshift|] the sum of the magnitudes the
    expression adds, n = 2 / 3 / 5 the roundings of  y*scale + shift  [+ res | + (res*rscale + rshift)]  counted in bn_fwd_kernel;
    plus |y| d_scale + d_shift (+ |res| d_rscale + d_rshift) where the kernel derived the coefficients itself (vqa_bn_apply_acc).
  statistics (coef_ref): with s, q the fp64 sums of the fp32 partials (d_s, d_q = 2 T 2^-53 sum|partial| for a T-term fp64
    sum done twice, by the kernel and by torch; 0 for the integer accumulators),
      d_mean = d_s / count + 2^-52 |mean|
      d_var  = d_q / count + 2 |mean| d_mean + 1.5 * 2^-52 (q / count + mean^2)      three fp64 roundings of q/count - mean*mean
      d_inv  = inv^3 d_var / 2 + inv (2^-24 + 3 * 2^-53)                             slab path: (float)(1.0 / sqrt(var + eps))
      d_inv  = inv^3 d_var / 2 + inv (2^-24 + 2^-23)                                 accumulator path: rsqrtf((float)var + eps), the
                                                       cast and the sum halved by the root, the hardware instruction's 1 ulp
      d_scale = |gamma| d_inv + u |scale|
      d_shift = |scale| (d_mean + u |mean|) + |mean| d_scale + 2 u (|beta| + |mean scale|)
      running mean: momentum (d_mean + u |mean|) + u (3 |(1 - m) rm| + 2 |m mean|);  running var likewise from var * unbias.
  eval coefficients: invstd = 1.0f / sqrtf(rv + eps): 3 u invstd (sum halved by the root, root, division); scale, shift as above.
  backward coefficients (bc_bound): gi = gamma invstd, mg = (float)(sg / count), mgx = (float)(sx / count), t = mean invstd mgx:
      bc0 u |gi|;  bc1 4 u |bc1|;  bc2 8 u |gi| (|t| + |mg|);  with d gamma = (float) sx added into a buffer holding p:
      u (|sx| + |p + sx|), all plus what the sums themselves may be off (d_sg, d_sx passed in).
  backward apply (dy_bound): 4 u (|a g| + |b y| + |c|) for a*g + b*y + c, plus |g| d_a + |y| d_b + d_c.
  reductions (d beta, d gamma, d gamma2, pooling sums): 8x the error of the same formula in torch fp32 on the CPU, in units of the
    sum of the magnitudes of what is added, worst channel, floor 2^-24 (units_bound); applied per channel (per chunk and channel).
The GPU file adds the fp64 evaluation's own rounding to every bound: bound (1 + 2^-30) + 2^-45 |ref|."""
import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16
DT = {"fp32": F32, "bf16": BF16}
VEC = {F32: 4, BF16: 8}
U = 2.0 ** -24
BF = 2.0 ** -8
EPS = float(torch.tensor(1e-5, dtype=F32))        # the fp32 values the entry points receive
MOM = float(torch.tensor(0.1, dtype=F32))
SENT = -8192.0                                    # sentinel of every output buffer (a bf16 number no case produces)
FLT_MIN = 2.0 ** -126                             # smallest positive normal of fp32 and of bf16

CHANNELS = {"bf16": [8, 64, 128, 256, 512, 2048], "fp32": [4, 64, 512, 1024]}
BIG_ROWS = {("fp32", 512): [16384 + 3], ("bf16", 2048): [8192 + 3], ("bf16", 64): [8192 + 37, 65536 + 5]}
STATS_TILES = [1, 3, 63, 64, 65, 257, 4100]
STATS_CHANNELS = [8, 64, 100, 512]
FINALIZE_NBLK = [1, 15, 16, 17, 112, 113, 129, 512]
POOL_HW = [1, 49, 196, 197, 3136]
POOL_CHANNELS = [("bf16", 8), ("bf16", 64), ("bf16", 512), ("bf16", 2048), ("fp32", 64), ("fp32", 1024)]
CHAIN_CASES = [(p, d, C) for p in ("res", "dual", "eval") for d in ("fp32", "bf16") for C in (64, 512)]
CHAIN_ROWS = 197


# ------------------------------------------------------------------------------------------------- launch geometry (host mirrors)
def lanes_r(C, dtype):
    return 256 // (C // VEC[dtype])


def replicas(C):
    return min(8, max(1, 512 // C))


def acc_words(K, C):
    return (2 * replicas(C) * K * C + 1 + 1) // 2 * 2


def bwd_blocks(rows):
    return max(1, min((rows + 63) // 64, 256 if rows < 65536 else 512))


def pool_chunks(HW, C, dtype):
    rpc = 14 * lanes_r(C, dtype)
    return (HW + rpc - 1) // rpc


def row_cases():
    """(dtype name, C, rows): rows 1, lanes_r - 1, lanes_r + 1 at every C, and the odd counts past the launchers' grid caps."""
    out = []
    for d, Cs in CHANNELS.items():
        for C in Cs:
            lr = lanes_r(C, DT[d])
            rows = [1] + ([lr - 1] if lr - 1 > 1 else []) + [lr + 1] + BIG_ROWS.get((d, C), [])
            out += [(d, C, r) for r in dict.fromkeys(rows)]
    return out


ROW_CASES = row_cases()


def pool_cases():
    """(dtype name, C, B, HW), no tensor above 34 MB"""
    return [(d, C, B, HW) for d, C in POOL_CHANNELS for HW in POOL_HW for B in (1, 3) if not (HW == 3136 and C > 64)]


def case_id(c):
    return "-".join(str(x) for x in c)


def seed_of(*k):
    s = 17
    for x in k:
        s = (s * 1000003 + (sum(map(ord, x)) if isinstance(x, str) else int(x))) % (2 ** 31 - 1)
    return s


def cv(t):
    return t.double().view(1, -1)


def store_bound(e, ref, dtype):
    return e * (1 + BF) + BF * ref.abs() if dtype == BF16 else e


def stored(t, dtype):
    """fp64 -> the storage dtype, one rounding"""
    return t.to(dtype)


def units_bound(cpu32, ref, unit):
    """8 x the worst (error of the fp32 CPU evaluation / unit), floored at 2^-24, times each entry's unit"""
    live = unit > 0
    w = float(((cpu32.double() - ref).abs()[live] / unit[live]).max()) if bool(live.any()) else 0.0
    w = max(w, U)
    return 8 * w * unit, w


# --------------------------------------------------------------------------------------------------------- accumulator format
def acc_encode(parts, replica, K, C):
    """parts [P][K][C] fp32 partial sums, replica [P] the copy each one is added to -> int64 [acc_words(K, C)], the image of
    acc_add_fixed: hi plane rint(16 v) | flag word (partials outside |v| < 2^41 or not finite) | lo plane (v - hi/16) 2^50."""
    R = replicas(C)
    n = R * K * C
    v = parts.double()
    ok = v.abs() < 2.0 ** 41
    v = torch.where(ok, v, torch.zeros_like(v))
    hi = torch.round(v * 16)                                    # half to even, as rintf; 16 v is exact
    lo = torch.round((v - hi / 16) * 2.0 ** 50)                 # v - hi/16 is exact; __float2ll_rn
    planes = [torch.zeros(R, K, C, dtype=torch.int64).index_add_(0, replica.long(), t.long()) for t in (hi, lo)]
    acc = torch.zeros(acc_words(K, C), dtype=torch.int64)
    acc[:n], acc[n], acc[n + 1:2 * n + 1] = planes[0].flatten(), int((~ok).sum()), planes[1].flatten()
    return acc


def acc_planes(acc, K, C):
    R = replicas(C)
    n = R * K * C
    return acc[:n].view(R, K, C), acc[n + 1:2 * n + 1].view(R, K, C), int(acc[n])


def acc_decode(acc, K, C, skip_replica=None, use_lo=True):
    """acc_read_fixed for every (k, c): integer sums over the replicas, then (double)hi / 16 + (double)lo / 2^50 -> ([K][C], flag).
    skip_replica / use_lo = False: the two wrong decoders of the mutant checks."""
    hi, lo, flag = acc_planes(acc, K, C)
    if skip_replica is not None:
        keep = [r for r in range(hi.shape[0]) if r != skip_replica]
        hi, lo = hi[keep], lo[keep]
    th, tl = hi.sum(0), lo.sum(0)
    return th.double() / 16 + (tl.double() / 2.0 ** 50 if use_lo else 0), flag


def acc_total_exact(acc, K, C):
    """the totals as Python integers in units of 2^-50"""
    hi, lo, _ = acc_planes(acc, K, C)
    th, tl = hi.sum(0).flatten().tolist(), lo.sum(0).flatten().tolist()
    return [h * 2 ** 46 + l for h, l in zip(th, tl)]


def parts_total_exact(parts):
    """sum over the partials as Python integers in units of 2^-50 (every partial must be a multiple of 2^-50)"""
    P = parts.shape[0]
    scaled = (parts.double() * 2.0 ** 50).reshape(P, -1)
    assert torch.equal(scaled, scaled.round())
    cols = scaled.t().tolist()
    return [sum(int(x) for x in col) for col in cols]


def uneven_replicas(P, C, seed):
    """replica of each of P partials: skewed (replica 0 gets about half), every replica used when P allows"""
    R = replicas(C)
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, R, (P,), generator=g)
    r[torch.rand(P, generator=g) < 0.5] = 0
    r[:min(P, R)] = torch.arange(min(P, R))
    return r


def stat_partials(y, P):
    """[P][2][C] fp32: sum y and sum y^2 of P uneven row chunks (fp64 sums rounded once, as a producer's fp32 partial)"""
    rows = y.shape[0]
    cuts = sorted({0, rows} | {(rows * (2 * i + 1)) // (2 * P + 1) for i in range(1, P)})
    yd = y.double()
    ps = [torch.stack([yd[a:b].sum(0), (yd[a:b] ** 2).sum(0)]) for a, b in zip(cuts[:-1], cuts[1:])]
    return torch.stack(ps).float()


# ------------------------------------------------------------------------------------------------------------------ statistics
def slab_sums(part):
    """fp64 sums of a partial slab [T][K][C] and what two T-term fp64 summations may differ by"""
    T = part.shape[0]
    pd = part.double()
    return pd.sum(0), 2 * T * 2.0 ** -53 * pd.abs().sum(0)


def coef_ref(s, q, d_s, d_q, count, gamma, beta, rm=None, rv=None, acc=False, unbiased=True):
    """(ref, bound) dicts of coef [4][C] = scale | shift | mean | invstd and the updated running statistics; formulas of
    bn_finalize_kernel (acc = False) / bn_acc_coef (acc = True), bounds of the module docstring."""
    g, b = gamma.double(), beta.double()
    mean = s / count
    ex2 = q / count
    var = (ex2 - mean * mean).clamp(min=0)
    inv = 1 / (var + EPS).sqrt()
    sc = g * inv
    sh = b - mean * sc
    d_mean = d_s / count + 2.0 ** -52 * mean.abs()
    d_var = d_q / count + 2 * mean.abs() * d_mean + 1.5 * 2.0 ** -52 * (ex2.abs() + mean * mean)
    d_inv = inv ** 3 * d_var / 2 + inv * ((U + 2.0 ** -23) if acc else (U + 3 * 2.0 ** -53))
    d_sc = g.abs() * d_inv + U * sc.abs()
    d_meanf = d_mean + U * mean.abs()
    d_sh = sc.abs() * d_meanf + mean.abs() * d_sc + 2 * U * (b.abs() + (mean * sc).abs())
    ref = {"coef": torch.stack([sc, sh, mean, inv]), "var": var}
    bnd = {"coef": torch.stack([d_sc, d_sh, d_meanf, d_inv])}
    if rm is not None:
        unb = var * (count / (count - 1) if (count > 1 and unbiased) else 1.0)
        keep = 1.0 - MOM
        ref["rm"], ref["rv"] = keep * rm.double() + MOM * mean, keep * rv.double() + MOM * unb
        d_unb = (count / (count - 1) if count > 1 else 1.0) * d_var + (U + 2.0 ** -51) * unb.abs()
        bnd["rm"] = MOM * d_meanf + U * (3 * (keep * rm.double()).abs() + 2 * (MOM * mean).abs())
        bnd["rv"] = MOM * d_unb + U * (3 * (keep * rv.double()).abs() + 2 * (MOM * unb).abs())
    return ref, bnd


def eval_coef_ref(gamma, beta, rm, rv):
    g, b, m = gamma.double(), beta.double(), rm.double()
    inv = 1 / (rv.double() + EPS).sqrt()
    sc = g * inv
    d_inv = 3 * U * inv
    d_sc = g.abs() * d_inv + U * sc.abs()
    d_sh = m.abs() * d_sc + 2 * U * (b.abs() + (m * sc).abs())
    return torch.stack([sc, b - m * sc, m, inv]), torch.stack([d_sc, d_sh, torch.zeros_like(m), d_inv])


def stats_operands(tiles, C, seed, per_tile=3):
    """A hand-built partial slab [tiles][2][C] (per-tile sum and sum of squares of `per_tile` values, rounded to fp32) with the
    special channels: 0 constant (var clamps to 0), 1 |mean| / std ~ 1e3, 2 gamma = 0, 3 beta = 0.  count = tiles * per_tile."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(tiles, per_tile, C, generator=g, dtype=torch.float64) * (torch.rand(C, generator=g, dtype=torch.float64) + 0.5) \
        + torch.randn(C, generator=g, dtype=torch.float64) * 0.5
    x[:, :, 0] = 3.0
    x[:, :, 1] = 1000.0 + torch.randn(tiles, per_tile, generator=g, dtype=torch.float64)
    part = torch.stack([x.sum(1), (x * x).sum(1)], 1).float().contiguous()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    gamma[5 % C] = -0.8
    gamma[2], beta[3] = 0.0, 0.0
    rm, rv = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
    return part, float(tiles * per_tile), gamma, beta, rm, rv


# --------------------------------------------------------------------------------------------------------------------- forward
def apply_ref(y, sc, sh, res=None, rs=None, rh=None, relu=True, drop_rshift=False):
    """(out, pre) fp64: out = [relu](y scale + shift [+ res | + res rscale + rshift]); a NaN stays a NaN (`x < 0 ? 0 : x`)."""
    pre = y.double() * cv(sc) + cv(sh)
    if res is not None:
        pre = pre + (res.double() if rs is None else res.double() * cv(rs) + (0 if drop_rshift else cv(rh)))
    return (torch.where(pre < 0, torch.zeros_like(pre), pre) if relu else pre), pre


def apply_bound(y, sc, sh, res=None, rs=None, rh=None, d=None, dr=None):
    """fp32 part of the forward bound; d / dr = (d_scale, d_shift) of coefficients the kernel derived itself"""
    M = (y.double() * cv(sc)).abs() + cv(sh).abs()
    n = 2
    if res is not None and rs is None:
        M, n = M + res.double().abs(), 3
    elif res is not None:
        M, n = M + (res.double() * cv(rs)).abs() + cv(rh).abs(), 5
    e = n * U * M
    if d is not None:
        e = e + y.double().abs() * cv(d[0]) + cv(d[1])
    if dr is not None:
        e = e + res.double().abs() * cv(dr[0]) + cv(dr[1])
    return e


def fwd_operands(dtype, C, rows, seed, exact=False):
    """y, res (storage dtype) and coef / rcoef [4][C] fp32 (scale | shift | 0 | 0).  exact: small dyadic values whose results are
    exact in fp32 with or without fma contraction (y, res = k/8, scales +-0.5 .. 2, shifts k/4)."""
    g = torch.Generator().manual_seed(seed)
    if exact:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        pick = lambda vals: torch.tensor(vals)[torch.randint(0, len(vals), (C,), generator=g)]
        y, res = (ri(-32, 32, rows, C) / 8).to(dtype), (ri(-32, 32, rows, C) / 8).to(dtype)
        sc, sh = pick([0.5, -0.5, 1.0, -1.0, 2.0, -2.0]), ri(-8, 8, C) / 4
        rs, rh = pick([0.5, -0.5, 1.0, -1.0]), ri(-8, 8, C) / 4
    else:
        sign = lambda: (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
        y, res = torch.randn(rows, C, generator=g).to(dtype), torch.randn(rows, C, generator=g).to(dtype)
        sc, sh = (torch.rand(C, generator=g) + 0.5) * sign(), torch.randn(C, generator=g) * 0.3
        rs, rh = (torch.rand(C, generator=g) + 0.5) * sign(), torch.randn(C, generator=g) * 0.3
    z = torch.zeros(2 * C)
    return {"y": y, "res": res, "coef": torch.cat([sc, sh, z]).view(4, C), "rcoef": torch.cat([rs, rh, z]).view(4, C)}


RES_MODES = ("none", "add", "bn")


def fwd_mode_args(op, mode):
    """(res, rscale, rshift) of a residual mode"""
    if mode == "none":
        return None, None, None
    return (op["res"], None, None) if mode == "add" else (op["res"], op["rcoef"][0], op["rcoef"][1])


def pool_ref(out, B, HW, C, dtype):
    """column sums of the stored outputs per (sample, chunk) -> ([B][chunks][C] fp64 sums, sums of magnitudes, fp32 CPU sums)"""
    rpc, ch = 14 * lanes_r(C, dtype), pool_chunks(HW, C, dtype)
    o = out.view(B, HW, C)
    segs = [o[:, k * rpc:min(HW, (k + 1) * rpc)] for k in range(ch)]
    return (torch.stack([s.double().sum(1) for s in segs], 1), torch.stack([s.double().abs().sum(1) for s in segs], 1),
            torch.stack([s.float().sum(1) for s in segs], 1))


# -------------------------------------------------------------------------------------------------------------------- backward
BWD_MODES = ("none", "outact", "self", "dual")


def bwd_operands(dtype, C, rows, seed):
    """dout, y, y2, outact (storage dtype), coef / coef2 [4][C] fp32 (scale | shift | mean | invstd), gamma / gamma2, bc / bc2
    [3][C].  outact is a ReLU output holding exact zeros, one -0.0 and one smallest positive normal; y is moved where its
    self-mask pre-activation y scale + shift would lie within 4x the forward bound of zero."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    sign = lambda: (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    dout, y, y2 = rn(rows, C).to(dtype), (rn(rows, C) * 1.5 + 0.3).to(dtype), (rn(rows, C) * 0.7 - 0.2).to(dtype)
    outact = torch.relu(rn(rows, C)).to(dtype)
    outact[0, 0], outact[-1, -1], outact[0, 1] = 0.0, -0.0, FLT_MIN
    outact[-1, 2] = 1.0                                                             # the last row counts in channel 2
    mk = lambda: torch.stack([(torch.rand(C, generator=g) + 0.5) * sign(), rn(C) * 0.3, rn(C) * 0.3, torch.rand(C, generator=g) + 0.5])
    coef, coef2 = mk(), mk()
    gamma, gamma2 = (torch.rand(C, generator=g) + 0.5) * sign(), (torch.rand(C, generator=g) + 0.5) * sign()
    scl = torch.tensor([1.0, 0.1, 0.01])[:, None]
    bc, bc2 = (rn(3, C) * scl).contiguous(), (rn(3, C) * scl).contiguous()
    for _ in range(4):
        pre = y.double() * cv(coef[0]) + cv(coef[1])
        bad = pre.abs() <= 4 * apply_bound(y, coef[0], coef[1])
        if not bool(bad.any()):
            break
        y = torch.where(bad, (y.float() + 1.0).to(dtype), y)
    return {"dout": dout, "y": y, "y2": y2, "outact": outact, "coef": coef, "coef2": coef2, "gamma": gamma, "gamma2": gamma2,
            "bc": bc, "bc2": bc2}


def self_margin(op):
    """smallest |pre-activation| / forward bound over the tensor (must exceed 1 for the self_mask cases)"""
    pre = op["y"].double() * cv(op["coef"][0]) + cv(op["coef"][1])
    return float((pre.abs() / apply_bound(op["y"], op["coef"][0], op["coef"][1])).min())


def bwd_g(op, mode, ge=False):
    """g = dout [outact > 0] | dout | dout [y scale + shift > 0]   (ge: the wrong mask `>=`)"""
    d = op["dout"].double()
    if mode in ("none",):
        return d
    z = op["y"].double() * cv(op["coef"][0]) + cv(op["coef"][1]) if mode == "self" else op["outact"].double()
    return d * ((z >= 0) if ge else (z > 0))


def xhat(y, coef):
    return (y.double() - cv(coef[2])) * cv(coef[3])


def bwd_sums(g, op, dual, skip_last_row=False, skip_last_vec=0):
    """([3][C] sums: sum g | sum g xhat | sum g xhat2 (0 without the second BatchNorm), [3][C] sums of magnitudes)"""
    t = [g, g * xhat(op["y"], op["coef"]), g * xhat(op["y2"], op["coef2"]) if dual else torch.zeros_like(g)]
    if skip_last_row:
        t = [x[:-1] for x in t]
    s, a = torch.stack([x.sum(0) for x in t]), torch.stack([x.abs().sum(0) for x in t])
    if skip_last_vec:
        s[:, -skip_last_vec:] = 0
    return s, a


def bwd_sums_fp32(op, mode, dual):
    """the same sums by the same formulas in torch fp32"""
    d = op["dout"].float()
    if mode == "self":
        d = d * (op["y"].float() * op["coef"][0] + op["coef"][1] > 0)
    elif mode != "none":
        d = d * (op["outact"].float() > 0)
    x1 = d * (op["y"].float() - op["coef"][2]) * op["coef"][3]
    x2 = d * (op["y2"].float() - op["coef2"][2]) * op["coef2"][3] if dual else torch.zeros_like(d)
    return torch.stack([d.sum(0), x1.sum(0), x2.sum(0)])


def bc_ref(sg, sx, count, gamma, coef, training, drop_mg=False, count_off=0):
    """bcoef [3][C] of bn_bwd_finalize_kernel: dy = bc0 g + bc1 y + bc2   (drop_mg / count_off: mutants)"""
    mean, inv = coef[2].double(), coef[3].double()
    gi = gamma.double() * inv
    if not training:
        return torch.stack([gi, torch.zeros_like(gi), torch.zeros_like(gi)])
    mg, mgx = sg / (count - count_off), sx / (count - count_off)
    return torch.stack([gi, -gi * inv * mgx, gi * (mean * inv * mgx - (0 if drop_mg else mg))])


def bc_bound(sg, sx, count, gamma, coef, training, d_sg=0.0, d_sx=0.0):
    mean, inv = coef[2].double(), coef[3].double()
    gi = (gamma.double() * inv).abs()
    if not training:
        return torch.stack([U * gi, torch.zeros_like(gi), torch.zeros_like(gi)])
    mg, mgx, dmg, dmgx = (sg / count).abs(), (sx / count).abs(), d_sg / count, d_sx / count
    t = (mean * inv).abs() * mgx
    return torch.stack([U * gi, 4 * U * gi * inv * mgx + gi * inv * dmgx,
                        8 * U * gi * (t + mg) + gi * ((mean * inv).abs() * dmgx + dmg)])


def bc_sens(sg, sx, count, gamma, coef, d_coef, training):
    """what bcoef moves by when mean / invstd (coef rows 2, 3) are off by d_coef rows 2, 3: first-order terms of bc_ref"""
    mean, inv, g = coef[2].double().abs(), coef[3].double(), gamma.double().abs()
    d_mean, d_inv = d_coef[2], d_coef[3]
    if not training:
        return torch.stack([g * d_inv, torch.zeros_like(g), torch.zeros_like(g)])
    mg, mgx = (sg / count).abs(), (sx / count).abs()
    return torch.stack([g * d_inv, 2 * g * inv * d_inv * mgx,
                        g * d_inv * (mean * inv * mgx + mg) + g * inv * mgx * (d_mean * inv + mean * d_inv)])


def grad_add_bound(s, prefill, d_s=0.0):
    """(float) s added into a buffer holding `prefill`"""
    return U * (s.abs() + (prefill + s).abs()) + d_s


def dy_ref(bc, g, y):
    return cv(bc[0]) * g + cv(bc[1]) * y.double() + cv(bc[2])


def dy_bound(bc, g, y, d_bc=None):
    e = 4 * U * ((cv(bc[0]) * g).abs() + (cv(bc[1]) * y.double()).abs() + cv(bc[2]).abs())
    if d_bc is not None:
        e = e + g.abs() * cv(d_bc[0]) + y.double().abs() * cv(d_bc[1]) + cv(d_bc[2])
    return e


def sum_partials(g, op, dual, P):
    """[P][3][C] fp32 partial sums over P uneven row chunks (what P producer workgroups would add to an accumulator)"""
    rows = g.shape[0]
    cuts = sorted({0, rows} | {(rows * (2 * i + 1)) // (2 * P + 1) for i in range(1, P)})
    t = [g, g * xhat(op["y"], op["coef"]), g * xhat(op["y2"], op["coef2"]) if dual else torch.zeros_like(g)]
    return torch.stack([torch.stack([x[a:b].sum(0) for x in t]) for a, b in zip(cuts[:-1], cuts[1:])]).float()


def slab_operands(nblk, C, seed):
    """a hand-built backward slab [nblk][3][C] fp32, gamma, coef [4][C]; channel 1 sums to about zero (cancellation)"""
    g = torch.Generator().manual_seed(seed)
    slab = torch.randn(nblk, 3, C, generator=g) * torch.tensor([4.0, 2.0, 3.0])[None, :, None] + torch.randn(3, C, generator=g)[None]
    if nblk > 1:
        slab[-1, :, 1] = -slab[:-1, :, 1].double().sum(0).float()
    sign = (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    coef = torch.stack([torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5,
                        torch.rand(C, generator=g) + 0.5])
    return slab.contiguous(), (torch.rand(C, generator=g) + 0.5) * sign, coef


# ------------------------------------------------------------------------------------------------------------- whole block, autograd
def block_autograd(pattern, y, gamma, beta, dout, res=None, y2=None, gamma2=None, beta2=None, rm=None, rv=None):
    """fp64 autograd of   res: relu(bn_train(y) + res)   dual: relu(bn_train(y) + bn_train(y2))   eval: relu(bn_eval(y; rm, rv))
    on [rows][C] operands -> dict out, dy, dgamma, dbeta (, dres | dy2, dgamma2, dbeta2)"""
    leaf = lambda t: t.double().clone().requires_grad_(True)
    yl, gl, bl = leaf(y), leaf(gamma), leaf(beta)
    if pattern == "eval":
        pre = F.batch_norm(yl, rm.double(), rv.double(), gl, bl, False, 0.1, EPS)
        extra = {}
    elif pattern == "res":
        rl = leaf(res)
        pre = F.batch_norm(yl, None, None, gl, bl, True, 0.1, EPS) + rl
        extra = {"dres": rl}
    else:
        y2l, g2l, b2l = leaf(y2), leaf(gamma2), leaf(beta2)
        pre = F.batch_norm(yl, None, None, gl, bl, True, 0.1, EPS) + F.batch_norm(y2l, None, None, g2l, b2l, True, 0.1, EPS)
        extra = {"dy2": y2l, "dgamma2": g2l, "dbeta2": b2l}
    out = torch.relu(pre)
    out.backward(dout.double())
    r = {"out": out.detach(), "pre": pre.detach(), "dy": yl.grad, "dgamma": gl.grad, "dbeta": bl.grad}
    r.update({k: v.grad for k, v in extra.items()})
    return r


def exact_coef(y, gamma, beta, rm=None, rv=None):
    """fp64 coef [4][C] of y's own batch statistics (or of rm / rv)"""
    yd = y.double()
    mean, var = (yd.mean(0), yd.var(0, unbiased=False)) if rm is None else (rm.double(), rv.double())
    inv = 1 / (var + EPS).sqrt()
    sc = gamma.double() * inv
    return torch.stack([sc, beta.double() - mean * sc, mean, inv])


def block_closed_form(pattern, y, gamma, beta, dout, res=None, y2=None, gamma2=None, beta2=None, rm=None, rv=None):
    """the same through this module's closed forms: apply_ref, the mask out > 0, bwd sums, bc_ref, dy_ref"""
    rows = y.shape[0]
    c1 = exact_coef(y, gamma, beta, rm, rv)
    op = {"dout": dout, "y": y, "coef": c1, "y2": y2, "coef2": None}
    if pattern == "dual":
        c2 = exact_coef(y2, gamma2, beta2)
        op["coef2"] = c2
        out, pre = apply_ref(y, c1[0], c1[1], y2, c2[0], c2[1])
    else:
        out, pre = apply_ref(y, c1[0], c1[1], res if pattern == "res" else None)
    g = dout.double() * (out > 0)
    s, _ = bwd_sums(g, op, pattern == "dual")
    bc = bc_ref(s[0], s[1], rows, gamma, c1, pattern != "eval")
    r = {"out": out, "pre": pre, "g": g, "dy": dy_ref(bc, g, y), "dgamma": s[1], "dbeta": s[0], "coef": c1, "bc": bc}
    if pattern == "res":
        r["dres"] = g
    if pattern == "dual":
        bc2 = bc_ref(s[0], s[2], rows, gamma2, c2, True)
        r.update({"dy2": dy_ref(bc2, g, y2), "dgamma2": s[2], "dbeta2": s[0], "coef2": c2, "bc2": bc2})
    return r


def chain_operands(pattern, dtype, C, rows=CHAIN_ROWS, seed=None):
    """Operands of a whole-block chain whose coefficients really are the statistics of y.  The seed is the first for which every
    pre-activation of the block's ReLU lies farther from zero than 64x the forward bound with the exact coefficients (the kernels'
    own coefficients are off by their rounding): no mask hangs on a rounding.  Returns (operands, smallest |pre| / bound)."""
    for salt in range(64):
        g = torch.Generator().manual_seed(seed_of(pattern, str(dtype), C, rows, salt) if seed is None else seed + salt)
        rn = lambda *s: torch.randn(*s, generator=g)
        sign = lambda: (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
        o = {"y": (rn(rows, C) * (torch.rand(C, generator=g) + 0.5) + rn(C) * 0.5).to(dtype),
             "y2": (rn(rows, C) * 0.8 + rn(C) * 0.3).to(dtype), "res": torch.relu(rn(rows, C)).to(dtype), "dout": rn(rows, C).to(dtype),
             "gamma": (torch.rand(C, generator=g) + 0.5) * sign(), "beta": rn(C) * 0.3,
             "gamma2": (torch.rand(C, generator=g) + 0.5) * sign(), "beta2": rn(C) * 0.3,
             "rm": rn(C) * 0.2, "rv": torch.rand(C, generator=g) + 0.5}
        kw = block_kwargs(pattern, o)
        c1 = exact_coef(o["y"], o["gamma"], o["beta"], kw.get("rm"), kw.get("rv"))
        if pattern == "dual":
            c2 = exact_coef(o["y2"], o["gamma2"], o["beta2"])
            _, pre = apply_ref(o["y"], c1[0], c1[1], o["y2"], c2[0], c2[1])
            e = apply_bound(o["y"], c1[0], c1[1], o["y2"], c2[0], c2[1])
        else:
            r = o["res"] if pattern == "res" else None
            _, pre = apply_ref(o["y"], c1[0], c1[1], r)
            e = apply_bound(o["y"], c1[0], c1[1], r)
        margin = float((pre.abs() / e).min())
        if margin > 64:
            return o, margin
    raise AssertionError("no seed keeps the pre-activations away from zero")


def block_kwargs(pattern, o):
    kw = {"y": o["y"], "gamma": o["gamma"], "beta": o["beta"], "dout": o["dout"]}
    if pattern == "res":
        kw["res"] = o["res"]
    elif pattern == "dual":
        kw.update({"y2": o["y2"], "gamma2": o["gamma2"], "beta2": o["beta2"]})
    else:
        kw.update({"rm": o["rm"], "rv": o["rv"]})
    return kw
