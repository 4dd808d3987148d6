"""Exact-integer operands and fp64 references for the GEMM / convolution kernels.  CPU only: nothing here touches the GPU.

Every product of two small integers is exact in fp32, and as long as the sum of |a||b| over a whole reduction stays below 2^24
every fp32 partial sum is an integer below 2^24, hence exact IN ANY SUMMATION ORDER (tiles, split-K, slabs, atomics).  A bf16
output must then equal RNE_bf16(exact integer) bit for bit and an fp32 output the integer itself.

Two operand ranges:
  WIDE    activations in [-8, 8], weights in [-3, 3]: outputs reach |y| ~ 1000..3000, a good share of them exactly on a bf16 tie
          (odd integers in [256, 512), 2 mod 4 in [512, 1024), ...).  For stored outputs.
  NARROW  activations in [-2, 2], weights in [-1, 1]: |y| stays small enough that sums OF outputs (BatchNorm statistics, the fused
          BatchNorm-backward sums, += weight gradients over many rows) stay below 2^24 too.
`offset=True` draws from the non-negative half of the same range: short reductions (K = 32 .. 256) then still land where bf16
rounds (mean K * 4 * 1.5 instead of 0); the values stay inside the range.

The case tables at the bottom are shared by tests/test_exactint_ref_cpu.py (which proves, on the reference alone, that every
operand set is inside the exact range and that the wide cases really exercise the rounding) and tests/test_gpu_exact_integer.py."""
import functools

import torch
import torch.nn.functional as F

LIMIT = float(1 << 24)
WIDE = (8, 3)
NARROW = (2, 1)
BF = torch.bfloat16


def ints(shape, amax, seed, offset=False):
    """Seeded integers in [-amax, amax] ([0, amax] with offset) as fp64 (exact in bf16 and fp32 for the ranges used here)."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(0 if offset else -amax, amax + 1, tuple(shape), generator=g, dtype=torch.int64).double()


def pow2s(n, seed, signed=False):
    """n values from {1/2, 1, 2} (and their negatives with signed): exact scale factors."""
    g = torch.Generator().manual_seed(int(seed))
    v = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n,), generator=g)]
    return v * (torch.randint(0, 2, (n,), generator=g).double() * 2 - 1) if signed else v


def rne_bf16(t):
    """fp64 -> fp32 -> bf16.  The first step is exact for |integer| < 2^24, the second is torch's round-to-nearest-even."""
    return t.double().float().to(BF)


def expect(t, dtype):
    """What a kernel of compute dtype `dtype` must store for the exact value t."""
    return rne_bf16(t) if dtype == BF else t.double().float()


def assert_exact_range(abs_bound):
    """A condition on the INPUTS: the reference-side bound (sum |a||b|, sum |y|, sum y^2 ...) is below 2^24.  It fails the test."""
    b = float(abs_bound.max()) if torch.is_tensor(abs_bound) else float(abs_bound)
    assert b < LIMIT, f"operands leave the exact range: bound {b:.0f} >= 2^24"


def reduction_bound(kred, a, b, *extra):
    """Upper bound of sum |a||b| over a reduction of length kred (+ |extra| terms added afterwards, e.g. bias, addend, prefill)."""
    return kred * float(a.abs().max()) * float(b.abs().max()) + sum(float(e.abs().max()) for e in extra)


def assert_resummed(y):
    """Column sums of outputs [rows][C] that a kernel sums again: sum |y| and sum y^2 per column below 2^24."""
    assert_exact_range(y.abs().sum(0))
    assert_exact_range((y * y).sum(0))


def shares(y):
    """(share of exact bf16 ties, share changed by the bf16 rounding) among the exact fp64 values y."""
    bits = y.double().float().contiguous().view(torch.int32) & 0xFFFF
    tie = (bits == 0x8000).double().mean().item()
    changed = (rne_bf16(y).double() != y.double()).double().mean().item()
    return tie, changed


def assert_wide_shares(y):
    tie, changed = shares(y)
    assert tie >= 0.05 and changed >= 0.10, f"degenerate wide case: {tie:.3f} ties, {changed:.3f} changed by rounding"


def acc_decode_exact(acc, R, K, C):
    """Fixed-point accumulator (common.h: hi plane [R][K][C] in units of 2^-4 | flag | lo plane in units of 2^-50) ->
    (int64 hi sums [K][C], int64 lo sums [K][C], flag) by integer addition over the replicas only."""
    acc = acc.detach().cpu()
    assert acc.dtype == torch.int64
    n = R * K * C
    return acc[:n].view(R, K, C).sum(0), acc[n + 1: 2 * n + 1].view(R, K, C).sum(0), int(acc[n])


def acc_replicas(C):
    return max(1, min(8, 512 // C))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rows(t):
    """NCHW -> [B*H*W][C]"""
    return nhwc(t).reshape(-1, t.shape[1])


# ------------------------------------------------------------------------------------------------ fp64 references
def conv_ref(x, w, stride, pad):
    return F.conv2d(x.double(), w.double(), None, stride=stride, padding=pad)


def dgrad_ref(dy, w, stride, pad, hw):
    """Data gradient of conv2d(x [.., H, W], w, stride, pad) for the upstream gradient dy."""
    H, W = hw
    R, S = w.shape[2], w.shape[3]
    op = (H + 2 * pad - R - (dy.shape[2] - 1) * stride, W + 2 * pad - S - (dy.shape[3] - 1) * stride)
    return F.conv_transpose2d(dy.double(), w.double(), None, stride=stride, padding=pad, output_padding=op)


def wgrad_ref(x, dy, wshape, stride, pad):
    """Weight gradient as [Cout][R*S*Cin] (the KRSC master layout)."""
    dw = torch.nn.grad.conv2d_weight(x.double(), tuple(wshape), dy.double(), stride=stride, padding=pad)
    return dw.permute(0, 2, 3, 1).reshape(wshape[0], -1)


def conv_operands(B, Cin, Cout, H, W, R, stride, pad, rng, seed, offset=False):
    """x [B][Cin][H][W], w [Cout][Cin][R][R], dy [B][Cout][Ho][Wo] (drawn like an activation)."""
    a, b = rng
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    return (ints((B, Cin, H, W), a, seed, offset), ints((Cout, Cin, R, R), b, seed + 1, offset),
            ints((B, Cout, Ho, Wo), a, seed + 2, offset))


def bn_coef(N, seed, signed=True):
    """coef [4][N] = scale | shift | mean | invstd with exact arithmetic: powers of two and small integers."""
    return torch.stack([pow2s(N, seed, signed), ints((N,), 2, seed + 1), ints((N,), 1, seed + 2), pow2s(N, seed + 3)])


def bnred_sums(g, y, coef, self_mask, y2=None, coef2=None):
    """Rows sum g | sum g xhat(y) | sum g xhat(y2) (zeros without y2), g masked by [y * scale + shift > 0] with self_mask.
    Returns (sums [3][N], bound on the sums of absolute values)."""
    g = g.double()
    if self_mask:
        g = g * ((y * coef[0] + coef[1]) > 0)
    t = [g, g * (y - coef[2]) * coef[3], g * (y2 - coef2[2]) * coef2[3] if y2 is not None else torch.zeros_like(g)]
    return torch.stack([v.sum(0) for v in t]), max(float(v.abs().sum(0).max()) for v in t)


# ------------------------------------------------------------------------------------------------ shared case tables
# vqa_igemm convolutions: B, Cin, Cout, H, R, stride, pad, offset generator (short reductions only)
IGEMM_CONV = [
    (2, 64, 64, 12, 3, 1, 1, False),
    (3, 64, 128, 14, 3, 2, 1, False),
    (2, 128, 256, 9, 3, 1, 1, False),
    (2, 64, 128, 14, 1, 2, 0, True),
    (1, 256, 512, 7, 3, 2, 1, False),
]
# one case per window-loader variant of test_gpu_bigtile.STAGES at the smallest batch that still selects it: B, C, H, variant id
IGEMM_STAGES = [
    (16, 64, 56, 128 * 10000 + 64 * 10 + 1),
    (63, 128, 28, 128 * 10000 + 128 * 10 + 1),
    (125, 256, 14, 128 * 10000 + 128 * 10 + 1),
    (249, 512, 7, 128 * 10000 + 128 * 10 + 1),
]
LINEARS = [(17, 1024, 256, False), (33, 32, 10, True), (196, 512, 256, True)]          # M, Kin, N, offset
# the folded eval block's shortcut: 1x1 / stride 2 / pad 0 (the IGEMM_CONV geometry) and 1x1 / stride 1
IGEMM_SHORTCUT = [(2, 64, 128, 14, 1, 2, 0, True), (2, 64, 128, 14, 1, 1, 0, True)]
LINEAR_SCALAR_RELU2 = (33, 32, 10, True)                                                   # N % VEC != 0: the scalar epilogue branch
MIN_SIGN_FLIPS = 0.05         # least share of outputs on either side of the ReLU-placement test (see infer_epilogue)
STEM_LOADER_HW = 40
CONV8P = [(3, 14, 14, 256, 256), (5, 7, 7, 512, 512), (1, 5, 9, 64, 256), (1, 6, 10, 64, 128), (5, 7, 7, 128, 384)]   # B, H, W, C, N
CONV8P_S2 = [(3, 9, 11, 64, 256), (4, 28, 28, 128, 256)]
C64P = [(1, 8, 8), (3, 16, 24), (2, 12, 16), (5, 24, 16)]                                 # B, H, W
# vqa_wgrad: test_gpu_bigtile.WGRAD with the batch shrunk as far as the planner keeps (kind, tile_n, tile_k) and more than one split
WGRAD_PLAN = [  # B, Cin, Cout, H, R, stride, pad, (kind, tile_n, tile_k)
    (2, 128, 128, 28, 3, 1, 1, (0, 128, 128)),
    (260, 64, 128, 56, 3, 2, 1, (1, 128, 256)),
    (3, 64, 128, 56, 1, 2, 0, (0, 128, 64)),
    (130, 256, 256, 14, 3, 1, 1, (1, 256, 256)),
    (130, 512, 512, 7, 3, 1, 1, (1, 256, 256)),
    (260, 128, 256, 28, 3, 2, 1, (1, 256, 256)),
    (11, 128, 256, 28, 1, 2, 0, (0, 128, 128)),
]
WGRAD_C64 = [(1, 8, 8), (3, 16, 24), (20, 56, 56)]
WGRAD_C128_B = [1, 3]
WGRAD_GROUP = [(300, 256, 256), (4100, 256, 256), (1000, 256, 512)]                       # M, N, Kw: one split, three splits, one split
STEM_WGRAD_HW = [(64, 64), (96, 160)]
DGRAD_S2 = [(2, 64, 128, 16, True), (2, 64, 128, 16, False), (2, 256, 512, 14, True), (2, 256, 512, 14, False)]   # B, Cin, Cout, H, shortcut
STEM_CONV_HW = [(64, 64), (96, 160)]
STEM_POOL_HW = [(64, 64), (32, 72)]
STEM_DGRAD_HW = (64, 64)
LINEAR_DGRAD_ACT = (17, 512, 256)                                                          # M, Kin, N
GEMM_CANARY = [(256, 256, 64), (512, 256, 192)]


# ------------------------------------------------------------------------------------------------ shared case builders (CPU, fp64)
def conv_case(B, Cin, Cout, H, W, R, stride, pad, rng, offset=False, want_dgrad=False):
    """Operands, the exact forward output y [M][Cout], optionally the exact data gradient dx [B*H*W][Cin], and the bounds."""
    x, w, dy = conv_operands(B, Cin, Cout, H, W, R, stride, pad, rng, 1000 + 7 * B + Cin + 3 * Cout + H + W + R + stride, offset)
    d = dict(x=x, w=w, dy=dy, y=rows(conv_ref(x, w, stride, pad)), bound=reduction_bound(R * R * Cin, x, w))
    if want_dgrad:
        d["dx"] = rows(dgrad_ref(dy, w, stride, pad, (H, W)))
        d["dbound"] = reduction_bound(R * R * Cout, dy, w)
    return d


def infer_epilogue(y, seed):
    """Integer bias [N] and residual addend [M][N] for the epilogues of the folded eval block on the exact product y [M][N], and
    v = y + bias.  The bias is minus the rounded mean of y plus an integer in [-768, 768] per column: ReLU clips about half of v
    whichever generator drew y, and a short reduction (|y - mean| ~ 60 at K = 64) still reaches the zone where bf16 rounds
    (|v| >= 256).  The addend is 4 * [-256, 256] (exact in bf16, as wide as v itself), so that
    a fair share of outputs has v > 0 with v + addend < 0 and as many the reverse: there relu(v) + a, relu(v + a) and v + a all
    differ, and a ReLU on the wrong side of the addend changes bits."""
    N = y.shape[1]
    bias = ints((N,), 768, seed) - y.mean().round()
    add = 4 * ints(tuple(y.shape), 256, seed + 1)
    return dict(bias=bias, add=add, v=y + bias, ebound=float(bias.abs().max()) + float(add.abs().max()))


def conv1_expect(e, dtype):
    """relu = 1: relu(acc + bias) in fp32, then the compute dtype"""
    return expect(torch.relu(e["v"]), dtype)


def shortcut_expect(e, dtype):
    return expect(e["v"], dtype)


def conv2_expect(e, dtype):
    """relu = 2: acc + bias in fp32 -> the compute dtype -> + addend -> ReLU -> rounded again"""
    return expect(torch.relu(expect(e["v"], dtype).double() + e["add"]), dtype)


def relu_before_addend(e, dtype):
    """what a kernel with the ReLU on the wrong side of the addend would store"""
    return expect(torch.relu(expect(e["v"], dtype).double()) + e["add"], dtype)


def sign_flip_shares(e):
    """(share with v > 0 and v + addend < 0, share with v < 0 and v + addend > 0)"""
    v, s = e["v"], e["v"] + e["add"]
    return float(((v > 0) & (s < 0)).double().mean()), float(((v < 0) & (s > 0)).double().mean())


def assert_infer_epilogue(e):
    """The conditions on the reference that make the three forms worth running: ReLU clips a real share of v and keeps one, the
    kept values land on bf16 ties and roundings, both sign flips reach MIN_SIGN_FLIPS, and moving the ReLU changes stored values."""
    v = e["v"]
    clipped = float((v <= 0).double().mean())
    assert 0.2 <= clipped <= 0.8, clipped
    assert_wide_shares(v[v > 0])
    down, up = sign_flip_shares(e)
    assert down >= MIN_SIGN_FLIPS and up >= MIN_SIGN_FLIPS, (down, up)
    for dtype in (torch.float32, BF):
        moved = float((conv2_expect(e, dtype).double() != relu_before_addend(e, dtype).double()).double().mean())
        assert moved >= MIN_SIGN_FLIPS, (dtype, moved)
        assert float((conv2_expect(e, dtype) == 0).double().mean()) >= 0.2


def conv_infer_case(B, Cin, Cout, H, W, R, stride, pad, rng, offset=False):
    """conv_case plus the folded eval block's epilogue operands (key "e") and the bound that includes them."""
    return with_infer_epilogue(conv_case(B, Cin, Cout, H, W, R, stride, pad, rng, offset), infer_seed(B, Cin, Cout, H, R, stride))


def infer_seed(B, Cin, Cout, H, R, stride):
    return 1500 + B + Cin + Cout + H + R + stride


def with_infer_epilogue(d, seed):
    """adds the epilogue operands to a case that holds the exact product d["y"] and its bound"""
    d["e"] = infer_epilogue(d["y"], seed)
    d["ibound"] = d["bound"] + d["e"]["ebound"]
    return d


def linear_relu2_case(M, Kin, N, rng, offset=False):
    """x [M][Kin], w [N][Kin] and the same epilogue operands on y = x w^T (the scalar epilogue branch when N % VEC != 0)."""
    a, b = rng
    seed = 2500 + M + Kin + N
    x, w = ints((M, Kin), a, seed, offset), ints((N, Kin), b, seed + 1, offset)
    return with_infer_epilogue(dict(x=x, w=w, y=x @ w.t(), bound=reduction_bound(Kin, x, w)), seed + 2)


def linear_case(M, Kin, N, rng, offset=False):
    """x [M][Kin], w [N][Kin], integer bias and addend; pre = relu(x w^T + b) is the value of the first rounding.
    With the offset generator x w^T sits around Kin * 4 * 1.5: the bias then moves every column to about 768 (the densest bf16 tie
    zone) and every eighth column to about 0, so that ReLU still clips there."""
    a, b = rng
    seed = 2000 + M + Kin + N
    x, w = ints((M, Kin), a, seed, offset), ints((N, Kin), b, seed + 1, offset)
    bias, res = ints((N,), 256, seed + 2), ints((M, N), 8 * a, seed + 3)
    if offset:
        bias = bias - (Kin * 6 - 768)
        bias[::8] -= 768
    return dict(x=x, w=w, bias=bias, res=res, pre=torch.relu(x @ w.t() + bias), bound=reduction_bound(Kin, x, w, bias, res))


def transposed8p_case(B, H, W, C, N, rng):
    """conv8p transposed=1: x [B][C][H][W] is the upstream gradient, w [C][3][3][N] the forward weight (KRSC), out [B*H*W][N]."""
    a, b = rng
    seed = 3000 + 5 * B + H + W + C + N
    x, w = ints((B, C, H, W), a, seed), ints((C, 3, 3, N), b, seed + 1)
    y = rows(F.conv_transpose2d(x, w.permute(0, 3, 1, 2), padding=1))
    return dict(x=x, w=w, y=y, bound=reduction_bound(9 * C, x, w))


def dgrad_s2_case(B, Cin, Cout, H, shortcut, rng):
    a, b = rng
    seed = 4000 + Cin + H + int(shortcut)
    Ho = H // 2
    off = Cout < 256                                                # (one to four taps of Cout channels reach a pixel: a short reduction)
    w1, wd = ints((Cout, Cin, 3, 3), b, seed, off), ints((Cout, Cin, 1, 1), b, seed + 1, off)
    dy, dyd = ints((B, Cout, Ho, Ho), a, seed + 2, off), ints((B, Cout, Ho, Ho), a, seed + 3, off)
    dx = dgrad_ref(dy, w1, 2, 1, (H, H))
    if shortcut:
        dx = dx + dgrad_ref(dyd, wd, 2, 0, (H, H))
    return dict(w1=w1, wd=wd, dy=dy, dyd=dyd, dx=rows(dx), bound=reduction_bound((10 if shortcut else 9) * Cout, dy, w1))


def stem_case(B, H, W, rng, offset=True):
    """Integer image [B][3][H][W], stem weight [64][3][7][7], y = conv7x7/2/pad 3 as [B*Ho*Wo][64]."""
    a, b = rng
    seed = 5000 + B + H + W
    img, w = ints((B, 3, H, W), a, seed, offset), ints((64, 3, 7, 7), b, seed + 1, offset)
    y = conv_ref(img, w, 2, 3)
    return dict(img=img, w=w, y4=y, y=rows(y), bound=reduction_bound(147, img, w))


def gemm_case(M, N, K, rng):
    a, b = rng
    A, Bm = ints((M, K), a, 6000 + M + N + K, True), ints((N, K), b, 6001 + M + N + K, True)      # (K = 64, 192: short)
    return dict(A=A, B=Bm, y=A @ Bm.t(), bound=reduction_bound(K, A, Bm))


def linear_dgrad_case(M, Kin, N, rng):
    a, b = rng
    dz, w = ints((M, N), a, 7000, True), ints((N, Kin), b, 7001, True)
    h = ints((M, Kin), 2, 7002)                                     # out > 0 keeps: zeros and negatives drop
    return dict(dz=dz, w=w, h=h, y=dz @ w, bound=2 * reduction_bound(N, dz, w))


def epilogue_operands(shape, seed, addmax=64):
    """integer addend, masks in [-2, 2]: zeros and negatives both drop"""
    return ints(shape, addmax, seed), ints(shape, 2, seed + 1), ints(shape, 2, seed + 2)


def masked_epilogue(base, add, om, dtype=BF):
    """(base + addend) re-rounded, then * (outmask > 0): base is the value after the first rounding"""
    return expect(expect(base.double() + add, dtype).double() * (om > 0), dtype)


def bnred8p_case(B, H, W, C, N):
    """conv8p transposed=1 with the fused BatchNorm-backward sums, narrow range: the operands, the stored tiles (plain `base`, and
    `masked` = after a +-4 addend and the outmask) and per form (self | masked | dual) the tile it sums, the exact sums and their bound."""
    d = transposed8p_case(B, H, W, C, N, NARROW)
    shape = d["y"].shape
    add, _, om = epilogue_operands(shape, 300 + N, addmax=4)
    y, y2 = ints(shape, 2, 310 + N), ints(shape, 2, 311 + N)
    coef, coef2 = bn_coef(N, 320 + N), bn_coef(N, 330 + N)
    base = rne_bf16(d["y"])
    masked = masked_epilogue(base, add, om)
    d.update(add=add, om=om, bn_y=y, bn_y2=y2, coef=coef, coef2=coef2, base=base, masked=masked, bound=d["bound"] + 4)
    d["forms"] = {"self": (base,) + bnred_sums(base, y, coef, True), "masked": (masked,) + bnred_sums(masked, y, coef, False),
                  "dual": (masked,) + bnred_sums(masked, y, coef, False, y2, coef2)}
    return d


def c64p_narrow_case(B, H, W):
    """conv3x3_c64p in the narrow range: forward (statistics of the accumulators) and the data gradient with the self-masked sums."""
    d = conv_case(B, 64, 64, H, W, 3, 1, 1, NARROW, want_dgrad=True)
    yv, coef = ints(d["dx"].shape, 2, 500 + H), bn_coef(64, 510 + H)
    g = rne_bf16(d["dx"])
    sums, bound = bnred_sums(g, yv, coef, True)
    d.update(bn_y=yv, coef=coef, g=g, sums=sums, sums_bound=bound)
    return d


def prefill(shape, seed):
    """the nonzero integer pattern a weight-gradient buffer holds before the += launch"""
    return ints(shape, 64, seed)


def wgrad_plan_case(case):
    B, Cin, Cout, H, R, stride, pad, _ = case
    Ho = (H + 2 * pad - R) // stride + 1
    x, dy = ints((B, Cin, H, H), NARROW[0], 600 + Cin + H), ints((B, Cout, Ho, Ho), NARROW[0], 601 + Cin + H)
    dw0 = prefill((Cout, R * R * Cin), 602)
    return dict(x=x, dy=dy, dw0=dw0, bound=reduction_bound(B * Ho * Ho, x, dy, dw0))


def wgrad_c64_case(B, H, W):
    """+ the BatchNorm-prologue form: xin = relu(x * scale + shift), multiples of 1/2 (hence twice the bound)"""
    x, dy = ints((B, 64, H, W), NARROW[0], 700 + H), ints((B, 64, H, W), NARROW[0], 701 + H)
    dw0, coef = prefill((64, 576), 702), bn_coef(64, 710 + H)
    xin = torch.relu(x * coef[0][None, :, None, None] + coef[1][None, :, None, None])
    return dict(x=x, dy=dy, dw0=dw0, coef=coef, xin=xin, bound=reduction_bound(B * H * W, x, dy, dw0),
                bound_bn=2 * reduction_bound(B * H * W, xin, dy, dw0))


def wgrad_c128_case(B):
    x, dy = ints((B, 128, 28, 28), NARROW[0], 800 + B), ints((B, 128, 28, 28), NARROW[0], 801 + B)
    dw0 = prefill((128, 1152), 802)
    return dict(x=x, dy=dy, dw0=dw0, bound=reduction_bound(B * 28 * 28, x, dy, dw0))


def wgrad_group_case(i):
    M, N, Kw = WGRAD_GROUP[i]
    dy, x, dw0 = ints((M, N), NARROW[0], 900 + i), ints((M, Kw), NARROW[0], 910 + i), prefill((N, Kw), 920 + i)
    return dict(x=x, dy=dy, dw0=dw0, bound=reduction_bound(M, x, dy, dw0))


def stem_wgrad_case(B, H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img, dy = ints((B, 3, H, W), NARROW[0], 1000 + W), ints((B, 64, Ho, Wo), NARROW[0], 1001 + W)
    dw0 = prefill((64, 147), 1002)
    return dict(img=img, dy=dy, dw0=dw0, bound=reduction_bound(B * Ho * Wo, img, dy, dw0))


def stem_pool_case(B, H, W):
    """conv7x7/2 -> scale * y + shift (power of two, integer) -> ReLU -> MaxPool3x3/2/pad 1, all exact: `pooled` [B*Hp*Wp][64]"""
    d = stem_case(B, H, W, WIDE)
    scale, shift = pow2s(64, 1100 + W, signed=True), ints((64,), 64, 1101 + W)
    ref = F.max_pool2d(torch.relu(d["y4"] * scale[None, :, None, None] + shift[None, :, None, None]), 3, 2, 1)
    d.update(scale=scale, shift=shift, pooled=rows(ref), bound=2 * d["bound"] + 64)
    return d


def stem_dgrad_case(B, H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy, w = ints((B, 64, Ho, Wo), WIDE[0], 1200), ints((64, 3, 7, 7), WIDE[1], 1201)
    # at most 4 x 4 taps of 64 channels reach one pixel
    return dict(dy=dy, w=w, dimg=dgrad_ref(dy, w, 2, 3, (H, W)), bound=reduction_bound(16 * 64, dy, w))


# ------------------------------------------------------------------------------------------------ kept references
@functools.lru_cache(maxsize=4)
def cached(builder, *args):
    """builder(*args), kept for the last four argument lists: the several launches of one test in tests/test_gpu_arena_gemm_conv.py
    (plain buffers and arenas, one epilogue after the other) share one reference.  It wraps the builders by NAME instead of decorating
    them because some of them extend the dict another builder returned (with_infer_epilogue, bnred8p_case, c64p_narrow_case): behind
    a cache of their own the inner dict would be extended again on every call of the outer one.  The result is shared: do not modify
    it.  After a large case (the kind-1 weight gradient holds about 600 MB of fp64) call cached.cache_clear()."""
    return globals()[builder](*args)
