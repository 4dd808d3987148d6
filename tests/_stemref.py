"""float64 references of the stem tail (BatchNorm -> ReLU -> MaxPool 3x3 / stride 2 / pad 1) and of its backward, in plain torch
on the CPU.  No GPU, nothing of the package: the kernels in csrc/cnn_ops.hip (stem_pool_fwd_kernel, stem_bwd_apply_kernel), the
routing forms of csrc/stem_route.h and the fused stem gradients are judged against these, never against each other.

Layouts: the references work in NCHW float64; the kernels take NHWC [B*H*W, C] (nhwc / nchw convert).
Argmax code of a pooling window (oh, ow): r*3 + s, the window's tap (r, s) at pixel (2*oh - 1 + r, 2*ow - 1 + s)."""
import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16

# The pooling kernel's input sizes (B, H, W) and the branch each one reaches
POOL_SHAPES = [(2, 8, 8),       # plain
               (1, 7, 9),       # odd H and W: the last pair has `two == false`, the last window row is half outside
               (3, 15, 29),     # Wo = 15 -> Wp = 8, not a multiple of 7; Ho = 8
               (2, 16, 30),     # Ho = 8 with trows = 4 and trows = 2
               (1, 1, 1),       # a single pixel
               (2, 3, 57)]      # Wo = 29: five column tiles, a ragged last one
# (dtype name, C) at every shape, and the two extra channel counts at one shape each
POOL_CASES = [(s, d, 64) for s in POOL_SHAPES for d in ("fp32", "bf16")] + [((3, 15, 29), "bf16", 128), ((3, 15, 29), "fp32", 32)]
BN_SHAPES = [(3, 15, 29), (2, 16, 32)]
DT = {"fp32": F32, "bf16": BF16}


def case_id(case):
    (B, H, W), d, C = case
    return f"{B}x{H}x{W}-{d}-C{C}"


def seed_of(B, H, W, C, salt=0):
    """One fixed seed per case; test_stem_tail_ref_cpu.py checks on the reference alone that these seeds keep what the GPU tests
    presuppose (near-tie share, no value at the ReLU threshold, coverage)."""
    return 1000 * H + 10 * W + B + 7 * C + 100003 * salt


# salt of the random-codes case per shape: the first for which some pixel is named by four windows (one chance in 9^4 per pixel)
BWD_SALT = {(2, 8, 8): 2, (1, 7, 9): 31, (3, 15, 29): 1, (2, 16, 30): 6, (1, 1, 1): 1, (2, 3, 57): 5}


def pooled_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def nhwc(t):
    """NCHW -> the kernels' [B*H*W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def nchw(t, B, H, W):
    """[B*H*W, C] -> NCHW"""
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def _chan(t):
    return t.double().view(1, -1, 1, 1)


def bn_relu(y, scale, shift):
    """v = relu(y*scale + shift) and the pre-ReLU value, fp64.  A NaN stays a NaN (the kernel's `v < 0 ? 0 : v`)."""
    pre = y.double() * _chan(scale) + _chan(shift)
    return torch.where(pre < 0, torch.zeros_like(pre), pre), pre


def codes_of(flat, H, W):
    """torch's flat argmax ih*W + iw -> window code r*3 + s"""
    Ho, Wo = flat.shape[-2:]
    oh = torch.arange(Ho).view(1, 1, Ho, 1)
    ow = torch.arange(Wo).view(1, 1, 1, Wo)
    r = flat // W - (2 * oh - 1)
    s = flat % W - (2 * ow - 1)
    assert bool(((r >= 0) & (r <= 2) & (s >= 0) & (s <= 2)).all())
    return r * 3 + s


def pool_ref(y, scale, shift):
    """(pooled, codes, v): max_pool2d(relu(y*scale + shift), 3, 2, 1) in fp64 with the argmax as window codes.  ATen's CPU kernel
    takes the FIRST maximum in row-major window order and the LAST NaN (`val > maxval || isnan(val)`), the rule
    stem_pool_fwd_kernel states for itself."""
    v, _ = bn_relu(y, scale, shift)
    out, flat = F.max_pool2d(v, 3, 2, 1, return_indices=True)
    return out, codes_of(flat, y.shape[2], y.shape[3]), v


def tap_index(codes, H, W):
    """(flat pixel index ih*W + iw clamped into the map, inside) of the tap every window's code names"""
    Ho, Wo = codes.shape[-2:]
    oh = torch.arange(Ho).view(1, 1, Ho, 1)
    ow = torch.arange(Wo).view(1, 1, 1, Wo)
    c = codes.long()
    ih, iw = 2 * oh - 1 + c // 3, 2 * ow - 1 + c % 3
    inside = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
    return ih.clamp(0, H - 1) * W + iw.clamp(0, W - 1), inside


def scatter_windows(dpool, codes, H, W):
    """Every window adds its dpool to the pixel its code names, if that pixel lies inside the map, else to nothing.  fp64 NCHW."""
    B, C = dpool.shape[:2]
    flat, inside = tap_index(codes, H, W)
    g = torch.zeros(B, C, H * W, dtype=torch.float64)
    g.scatter_add_(2, flat.reshape(B, C, -1), (dpool.double() * inside).reshape(B, C, -1))
    return g.view(B, C, H, W)


def route_ref(dpool, codes, v_pos, H, W):
    """Gradient at the post-ReLU activation routed through the argmax codes (any code 0..8, also one pointing into the padding)
    and the ReLU mask v_pos = (y*scale + shift > 0)."""
    return scatter_windows(dpool, codes, H, W) * v_pos


def route_counts(codes, H, W):
    """How many windows name each pixel"""
    return scatter_windows(torch.ones(codes.shape, dtype=torch.float64), codes, H, W)


def dy_ref(bc, g, y):
    """dy = bc0*g + bc1*y + bc2 (bc [3][C])"""
    return _chan(bc[0]) * g + _chan(bc[1]) * y.double() + _chan(bc[2])


def bn_coef_ref(y, gamma, beta, training, eps, rm=None, rv=None):
    """fp64 (scale, shift, mean, invstd) of BatchNorm on y (batch statistics, biased variance, when training)."""
    yd = y.double()
    if training:
        mean, var = yd.mean((0, 2, 3)), yd.var((0, 2, 3), unbiased=False)
    else:
        mean, var = rm.double(), rv.double()
    invstd = (var + eps).rsqrt()
    scale = gamma.double() * invstd
    return scale, beta.double() - mean * scale, mean, invstd


def stem_bn_backward_ref(y, gamma, beta, dpool, training, eps, rm=None, rv=None):
    """fp64 autograd through F.batch_norm(y, ..., training) -> ReLU -> max_pool2d(3, 2, 1).  Returns dy, dgamma, dbeta."""
    yl, gl, bl = (t.double().clone().requires_grad_(True) for t in (y, gamma, beta))
    B, C, H, W = y.shape
    rmd = rm.double().clone() if rm is not None else torch.zeros(C, dtype=torch.float64)
    rvd = rv.double().clone() if rv is not None else torch.ones(C, dtype=torch.float64)
    out = F.max_pool2d(torch.relu(F.batch_norm(yl, rmd, rvd, gl, bl, bool(training), 0.1, eps)), 3, 2, 1)
    out.backward(dpool.double())
    return yl.grad, gl.grad, bl.grad


def bc_ref(sum_g, sum_gx, count, gamma, mean, invstd, training):
    """The apply coefficients of BatchNorm backward from its two sums (sum g, sum g*xhat): dy = bc0*g + bc1*y + bc2."""
    gi = gamma.double() * invstd
    if not training:
        return torch.stack([gi, torch.zeros_like(gi), torch.zeros_like(gi)])
    mg, mgx = sum_g / count, sum_gx / count
    return torch.stack([gi, -gi * invstd * mgx, gi * (mean * invstd * mgx - mg)])


# ------------------------------------------------------------------------------------------------------------------ operands
def window_ties(v):
    """per window: how many of its taps hold the window maximum (padding never does)"""
    B, C, H, W = v.shape
    u = F.unfold(F.pad(v, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(B, C, 9, -1)
    return (u == u.max(2, keepdim=True).values).sum(2)


def exact_operands(B, H, W, C, seed):
    """Operands whose results are exact in fp32 whether or not the compiler contracts a*b + c to an fma, and exactly representable
    in bf16 where the kernels store bf16: y = k/8 (|k| <= 32), scale in {+-0.5, +-1, +-2}, shift = k/4 (|k| <= 8),
    dpool = k/4 (|k| <= 8), bc0 in {0.5, 1, 2, -1}, bc1 in {0, +-1/8}, bc2 = k/16 (|k| <= 8).  Channel 0 is y = 2, scale = 1,
    shift = -2: its BatchNorm output is exactly 0 everywhere, so every window ties on zero and routes into a pixel whose gradient
    the ReLU mask (v > 0, not >= 0) must drop.  Returns a dict of fp64 NCHW tensors / fp64 channel vectors."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = pooled_hw(H, W)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).double()
    pick = lambda vals, n: torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (n,), generator=g)]
    y = ri(-32, 32, B, C, H, W) / 8
    scale, shift = pick([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], C), ri(-8, 8, C) / 4
    y[:, 0], scale[0], shift[0] = 2.0, 1.0, -2.0
    dpool = ri(-8, 8, B, C, Ho, Wo) / 4
    bc = torch.stack([pick([0.5, 1.0, 2.0, -1.0], C), pick([0.0, 0.125, -0.125], C), ri(-8, 8, C) / 16])
    v, _ = bn_relu(y, scale, shift)
    assert torch.equal(v.bfloat16().double(), v)                     # every BatchNorm + ReLU output is a bf16 number
    assert torch.equal(y.bfloat16().double(), y) and torch.equal(dpool.bfloat16().double(), dpool)
    ties = window_ties(v) > 1                                        # the maximum is >= 0 after the ReLU: a tie on a positive value or on zero
    if H * W > 1:                                                    # (a single pixel: one tap per window, nothing to tie)
        assert float(ties.double().mean()) >= 0.05, float(ties.double().mean())
    return {"y": y, "scale": scale, "shift": shift, "dpool": dpool, "bc": bc, "v": v, "tie_share": float(ties.double().mean())}


def random_pool_operands(B, H, W, C, dtype, seed):
    """Random normal y (rounded to the storage dtype), random scales of both signs, random shifts."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, C, H, W, generator=g).to(dtype)
    scale = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    shift = torch.randn(C, generator=g) * 0.3
    return y, scale, shift


def fwd_bound(y, scale, shift):
    """per pixel: 2^-23 * (|y*scale| + |shift|) -- two fp32 roundings of y*scale + shift (one with an fma)"""
    return 2.0 ** -23 * ((y.double() * _chan(scale)).abs() + _chan(shift).abs())


def window_max(t, pad_value=0.0):
    return F.max_pool2d(F.pad(t, (1, 1, 1, 1), value=pad_value), 3, 2, 0)


def near_tie_share(v, e):
    """Share of the windows whose two largest DISTINCT-position values differ by less than the two values' bounds together (each
    carries its own rounding error: the kernel may then pick the other tap), exact ties excluded -- those are decided by the rule,
    not by rounding.  Conservative: the larger bound of the window is taken for both."""
    B, C, H, W = v.shape
    u = F.unfold(F.pad(v, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(B, C, 9, -1)
    m = u.max(2, keepdim=True).values
    gap = torch.where(u < m, m - u, torch.full_like(u, float("inf"))).min(2).values
    E = window_max(e).reshape(B, C, -1)
    return float((gap < 2 * E).double().mean())


def random_bwd_operands(B, H, W, C, dtype, seed):
    """Random y, pooled gradient, argmax codes 0..8 (padding taps included), coefficients: the distributions of _stem_operands in
    test_gpu_input_grad.py, y and dpool rounded to the storage dtype."""
    Ho, Wo = pooled_hw(H, W)
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, C, H, W, generator=g).to(dtype)
    dpool = torch.randn(B, C, Ho, Wo, generator=g).to(dtype)
    codes = torch.randint(0, 9, (B, C, Ho, Wo), generator=g, dtype=torch.uint8)
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    bc = (torch.randn(3, C, generator=g) * torch.tensor([1.0, 0.1, 0.01])[:, None]).contiguous()
    return y, dpool, codes, scale, shift, bc


def apply_bound(bc, routed_abs, y):
    """8 * 2^-24 * (|bc0| * sum|routed dpool| + |bc1*y| + |bc2|): at most 3 fp32 additions in the routed sum, two products and two
    additions (or two fmas) in bc0*g + bc1*y + bc2 -- 7 roundings of partial results no larger than the bracket."""
    return 8 * 2.0 ** -24 * (_chan(bc[0]).abs() * routed_abs + (_chan(bc[1]) * y.double()).abs() + _chan(bc[2]).abs())


# the special channels of the BatchNorm-backward cases
CH_NEG_GAMMA, CH_DEAD, CH_CANCEL, CH_ZERO_GAMMA = 1, 2, 3, 4


def bn_case_operands(B, H, W, dtype, seed, C=64):
    """y, dpool (storage dtype), gamma, beta, running mean / var for the chain pool -> reduce -> finalize -> apply.
    gamma > 0 except: channel 1 negative; channel 2 gamma = 0.05, beta = -10: BatchNorm output negative everywhere (g = 0);
    channel 3 gamma = 0.1, beta = 3: beta / gamma = 30, (pooled - beta) / gamma cancels; channel 4 gamma = 0 exactly, beta = 0.5."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = pooled_hw(H, W)
    y = (torch.randn(B, C, H, W, generator=g) * (torch.rand(C, generator=g) + 0.5).view(1, C, 1, 1)
         + (torch.randn(C, generator=g) * 0.3).view(1, C, 1, 1)).to(dtype)
    dpool = torch.randn(B, C, Ho, Wo, generator=g).to(dtype)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    gamma[CH_NEG_GAMMA] = -0.8
    gamma[CH_DEAD], beta[CH_DEAD] = 0.05, -10.0
    gamma[CH_CANCEL], beta[CH_CANCEL] = 0.1, 3.0
    gamma[CH_ZERO_GAMMA], beta[CH_ZERO_GAMMA] = 0.0, 0.5
    rm, rv = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
    return y, dpool, gamma, beta, rm, rv
