"""GPU: kernel-level fp64 checks of the attention modules' HIP entry points, called through the C ABI.

  vqa_spatial_fwd / vqa_spatial_bwd   SpatialAttention (oracle/vqa_oracle.py spatial_attention): channel max / mean pool with the
                                      argmax channel, 7x7 conv + sigmoid, x * amap; backward dx and the accumulated conv-weight grad
  vqa_gate_fwd / vqa_gate_bwd         the fusion gate: fused = g*att + (1-g)*txt with g = sigmoid(z)
  vqa_se_bwd                          SEAttention backward at bottlenecks other than C / 16 (se_reduction is a constructor argument)

Every reference is fp64 on the CPU, built from the exact values the kernel read (bf16 inputs are upcast, never redrawn), so the
bounds cover only the kernel's own fp32 arithmetic and the rounding of what it stores.  Errors are max-abs relative to the
reference's max-abs.  The spatial max ignores NaN (a NaN channel never wins `f > mx`) while torch.max propagates it; that
difference is not exercised here."""
import pytest
import torch
import torch.nn.functional as F

from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["fp32", "bf16"]
EW = {torch.float32: 2e-5, torch.bfloat16: 1e-2}     # elementwise outputs, stored in the input dtype
RED = 1e-4                                           # fp32 reductions (dw, dz2, dh, dpool, dw1, dw2)


def _L():
    return sub("_lib")


def rel(a, r):
    r = r.double().cpu()
    return (a.double().cpu() - r).abs().max().item() / max(1e-6, r.abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------------------
# spatial attention
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, H, W, C): the 224-px stage outputs, the 384-px stage-4 map, maps at or below the 7 x 7 window (4 x 4 x 256 and 2 x 2 x 512
# are the 64-px model's stages 3 / 4), and B*H*W = 37632 > 32768 = 8192 workgroups x 4 waves: the pooling grid-stride loop and
# every spatial_wgrad_kernel slice (16 x 256 pixels per trip) loop.
SPATIAL_SHAPES = [(2, 56, 56, 64), (2, 28, 28, 128), (3, 14, 14, 256), (4, 7, 7, 512), (2, 12, 12, 512),
                  (3, 1, 1, 64), (3, 2, 2, 512), (2, 3, 5, 128), (3, 4, 4, 256), (2, 5, 9, 64), (12, 56, 56, 64)]


def _spatial_ref(x, w):
    """fp64 SpatialAttention on NHWC x: (pooled2 [B,H,W,2], amax [B,H,W], amap [B,H,W], out [B,H,W,C])."""
    xn = x.permute(0, 3, 1, 2)
    mx, am = torch.max(xn, 1, keepdim=True)
    av = xn.mean(1, keepdim=True)
    amap = torch.sigmoid(F.conv2d(torch.cat([mx, av], 1), w, None, padding=3))
    out = (xn * amap).permute(0, 2, 3, 1)
    return torch.cat([mx, av], 1).permute(0, 2, 3, 1), am[:, 0], amap[:, 0], out


def _spatial_fwd(x, w):
    L = _L()
    B, H, W, C = x.shape
    pooled2 = torch.full((B, H, W, 2), float("nan"), device=DEV)
    amax = torch.full((B, H, W), -7, device=DEV, dtype=torch.int32)
    amap = torch.full((B, H, W), float("nan"), device=DEV)
    out = torch.full_like(x, float("nan"))
    L.call("vqa_spatial_fwd", L.dt(x), x.data_ptr(), w.data_ptr(), pooled2.data_ptr(), amax.data_ptr(), amap.data_ptr(), out.data_ptr(),
           B, H, W, C)
    torch.cuda.synchronize()
    return pooled2, amax, amap, out


def _spatial_bwd(dout, x, w, pooled2, amax, amap, dw0):
    L = _L()
    B, H, W, C = x.shape
    scratch = torch.full((L.count("vqa_spatial_bwd_scratch", B, H, W),), float("nan"), device=DEV)
    dx = torch.full_like(x, float("nan"))
    dw = dw0.clone()
    L.call("vqa_spatial_bwd", L.dt(x), dout.data_ptr(), x.data_ptr(), w.data_ptr(), pooled2.data_ptr(), amax.data_ptr(), amap.data_ptr(),
           scratch.data_ptr(), dx.data_ptr(), dw.data_ptr(), B, H, W, C)
    torch.cuda.synchronize()
    npix = B * H * W
    return dx, dw, scratch[npix:3 * npix].view(B, H, W, 2)          # dpool2 (d max, d mean) per pixel


def _spatial_bwd_ref(x, w, dout):
    """fp64 autograd of the same formula (torch.max(dim=1) routes the max-gradient to the first maximal channel)."""
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    out = _spatial_ref(xr, wr)[3]
    (out * dout).sum().backward()
    return xr.grad, wr.grad


def _check_spatial(x, w, dout):
    """Forward and backward of one input against fp64; returns the fp64 reference argmax for extra checks."""
    dtype = x.dtype
    xd, wd, dd = x.double().cpu(), w.double().cpu(), dout.double().cpu()
    p_ref, am_ref, amap_ref, out_ref = _spatial_ref(xd, wd)
    pooled2, amax, amap, out = _spatial_fwd(x, w)
    assert torch.equal(pooled2[..., 0].double().cpu(), p_ref[..., 0])               # the max of stored values is exact
    assert torch.equal(amax.long().cpu(), am_ref)                                    # first maximal channel
    assert rel(pooled2[..., 1], p_ref[..., 1]) <= EW[torch.float32]
    assert rel(amap, amap_ref) <= EW[torch.float32]
    assert rel(out, out_ref) <= EW[dtype]
    # backward: dw accumulates into what is there
    dxr, dwr = _spatial_bwd_ref(xd, wd, dd)
    g = torch.Generator().manual_seed(5)
    dw0 = (torch.randn(1, 2, 7, 7, generator=g) * dwr.abs().max().item()).float().to(DEV)
    dx, dw, dpool2 = _spatial_bwd(dout, x, w, pooled2, amax, amap, dw0)
    assert rel(dx, dxr) <= EW[dtype], rel(dx, dxr)
    assert (dw.double().cpu() - dw0.double().cpu() - dwr).abs().max().item() <= RED * dwr.abs().max().item()
    dx2, dw2, _ = _spatial_bwd(dout, x, w, pooled2, amax, amap, dw0)               # fixed summation order: the same bits again
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2)
    return am_ref, dx, dpool2, amap


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SPATIAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spatial_attention_forward_and_backward_match_fp64(shape, dtype):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(B * 1000 + H * W + C)
    x = torch.randn(B, H, W, C, generator=g).to(DEV, dtype)
    w = (torch.randn(1, 2, 7, 7, generator=g) * 0.15).to(DEV)
    dout = torch.randn(B, H, W, C, generator=g).to(DEV, dtype)
    _check_spatial(x, w, dout)


def _tie_inputs(case, dtype, g):
    """Inputs whose channel maximum is shared; the expected argmax is the lowest such channel."""
    VEC = 8 if dtype == torch.bfloat16 else 4
    if case == "relu_zero_pixels":                   # post-ReLU map with whole pixels at zero: every channel ties, amax = 0
        B, H, W, C = 3, 7, 7, 512
        x = torch.relu(torch.randn(B, H, W, C, generator=g))
        x.view(-1, C)[::3] = 0.0
        x.view(-1, C)[1::3] = -torch.rand(x.view(-1, C)[1::3].shape, generator=g)     # all negative: the max is not 0
        return x
    B, H, W, C = 2, 6, 5, (512 if case == "bf16_dup_512" else 256)
    x = torch.randn(B, H, W, C, generator=g)
    flat = x.view(-1, C)
    n = flat.shape[0]
    top = flat.abs().max(1)[0] + 1.0
    if case == "same_vector":                        # two maxima inside one thread's 16-byte vector (c0 = lane * VEC)
        base = (torch.randint(0, C // VEC, (n,), generator=g) * VEC)
        i0 = base + torch.randint(0, VEC // 2, (n,), generator=g)
        i1 = base + VEC // 2 + torch.randint(0, VEC // 2, (n,), generator=g)
    elif case == "same_thread_next_trip":            # channel c and c + 64*VEC: one lane, two trips of its channel loop
        C2 = 64 * VEC
        x = torch.randn(B, H, W, 2 * C2, generator=g)
        flat = x.view(-1, 2 * C2)
        top = flat.abs().max(1)[0] + 1.0
        i0 = torch.randint(0, C2, (n,), generator=g)
        i1 = i0 + C2
    elif case == "different_lanes":                  # maxima in different lanes, resolved by the shuffle tie-break.  C = 128 * VEC:
        C2 = 64 * VEC                                 # every lane makes two trips.  Even pixels: lanes l0 < l1, first trip; odd
        x = torch.randn(B, H, W, 2 * C2, generator=g)  # pixels: the later channel sits in the LOWER lane (second trip of l1 < l0)
        flat = x.view(-1, 2 * C2)
        top = flat.abs().max(1)[0] + 1.0
        l0 = 1 + torch.randint(0, 62, (n,), generator=g)
        hi = l0 + 1 + (torch.rand(n, generator=g) * (63 - l0).float()).long()
        lo = (torch.rand(n, generator=g) * l0.float()).long()
        odd = torch.arange(n) % 2 == 1
        i0 = l0 * VEC + torch.randint(0, VEC, (n,), generator=g)
        i1 = torch.where(odd, C2 + lo * VEC, hi * VEC) + torch.randint(0, VEC, (n,), generator=g)
    elif case == "bf16_dup_512":                     # coarse values: duplicated (often triplicated) maxima at C = 512
        return torch.randn(B, H, W, C, generator=g).round()
    else:
        raise AssertionError(case)
    rows = torch.arange(n)
    flat[rows, i0] = top
    flat[rows, i1] = top
    return x


TIE_CASES = [("relu_zero_pixels", torch.float32), ("relu_zero_pixels", torch.bfloat16), ("same_vector", torch.float32),
             ("same_vector", torch.bfloat16), ("same_thread_next_trip", torch.float32), ("same_thread_next_trip", torch.bfloat16),
             ("different_lanes", torch.float32), ("different_lanes", torch.bfloat16), ("bf16_dup_512", torch.bfloat16),
             ("bf16_dup_512", torch.float32)]


@pytest.mark.parametrize("case,dtype", TIE_CASES, ids=[f"{c}-{str(d)[6:]}" for c, d in TIE_CASES])
def test_spatial_argmax_ties_pick_the_first_channel_and_route_the_gradient_there(case, dtype):
    g = torch.Generator().manual_seed(len(case) * 7 + (dtype == torch.bfloat16))
    x = _tie_inputs(case, dtype, g).to(DEV, dtype)
    B, H, W, C = x.shape
    xd = x.double().cpu()
    ntie = (xd == xd.max(-1, keepdim=True)[0]).sum(-1)
    assert int((ntie >= 2).sum()) >= B * H * W // 3                                  # the inputs do tie (after rounding to dtype)
    w = (torch.randn(1, 2, 7, 7, generator=g) * 0.3).to(DEV)
    dout = torch.randn(B, H, W, C, generator=g).to(DEV, dtype)
    am_ref, dx, dpool2, amap = _check_spatial(x, w, dout)
    # the max-gradient lands on the reference argmax channel and on no other: dx minus the mean / scale terms the kernel used
    base = dout.double() * amap.double()[..., None] + dpool2[..., 1:2].double() / C
    res = (dx.double() - base).cpu()
    dm = dpool2[..., 0].double().cpu()
    onehot = F.one_hot(am_ref, C).bool()
    tol = EW[dtype] * max(1e-6, dx.double().abs().max().item())
    assert (res[onehot] - dm.reshape(-1)).abs().max().item() <= tol
    assert res[~onehot].abs().max().item() <= tol
    assert dm.abs().max().item() > 20 * tol                                          # the routed term is visible above the bound


@pytest.mark.parametrize("dtype,C", [(torch.float32, 1028), (torch.float32, 96), (torch.bfloat16, 96)])
def test_spatial_calls_refused_for_the_channel_count_write_nothing(dtype, C):
    """C / VEC must divide 256 (the apply kernels' lane layout): refused with VQA_EARG before any launch."""
    L = _L()
    B, H, W = 2, 3, 3
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, H, W, C, generator=g).to(DEV, dtype)
    w = torch.randn(1, 2, 7, 7, generator=g).to(DEV)
    pooled2 = torch.full((B, H, W, 2), float("nan"), device=DEV)
    amax = torch.full((B, H, W), -7, device=DEV, dtype=torch.int32)
    amap = torch.full((B, H, W), float("nan"), device=DEV)
    out = torch.full_like(x, float("nan"))
    with pytest.raises(RuntimeError, match="argument/shape"):
        L.call("vqa_spatial_fwd", L.dt(dtype), x.data_ptr(), w.data_ptr(), pooled2.data_ptr(), amax.data_ptr(), amap.data_ptr(),
               out.data_ptr(), B, H, W, C)
    scratch = torch.full((L.count("vqa_spatial_bwd_scratch", B, H, W),), float("nan"), device=DEV)
    dx = torch.full_like(x, float("nan"))
    dw = torch.full((1, 2, 7, 7), float("nan"), device=DEV)
    amap_in = torch.rand(B, H, W, generator=g).to(DEV)
    p2_in = torch.randn(B, H, W, 2, generator=g).to(DEV)
    am_in = torch.zeros(B, H, W, device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="argument/shape"):
        L.call("vqa_spatial_bwd", L.dt(dtype), x.data_ptr(), x.data_ptr(), w.data_ptr(), p2_in.data_ptr(), am_in.data_ptr(),
               amap_in.data_ptr(), scratch.data_ptr(), dx.data_ptr(), dw.data_ptr(), B, H, W, C)
    torch.cuda.synchronize()
    for t in (pooled2, amap, out, scratch, dx, dw):
        assert torch.isnan(t.float()).all()
    assert bool((amax == -7).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# fusion gate
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,D", [(1, 64), (5, 256), (512, 512)])
def test_gate_forward_and_backward_match_fp64(B, D, dtype):
    L = _L()
    g = torch.Generator().manual_seed(B * 7 + D)
    z = torch.randn(B, D, generator=g) * 3
    z.view(-1)[::5] = torch.linspace(-30, 30, z.view(-1)[::5].numel())             # saturated sigmoid: g(1-g) underflows in fp32
    z = z.to(DEV, dtype)
    cat = torch.randn(B, 2 * D, generator=g).to(DEV, dtype)
    dfused = torch.randn(B, D, generator=g).to(DEV, dtype)
    fused = torch.full((B, D), float("nan"), device=DEV, dtype=dtype)
    dz = torch.full((B, D), float("nan"), device=DEV, dtype=dtype)
    dcat = torch.full((B, 2 * D), float("nan"), device=DEV, dtype=dtype)
    L.call("vqa_gate_fwd", L.dt(dtype), z.data_ptr(), cat.data_ptr(), fused.data_ptr(), B, D)
    L.call("vqa_gate_bwd", L.dt(dtype), dfused.data_ptr(), z.data_ptr(), cat.data_ptr(), dz.data_ptr(), dcat.data_ptr(), B, D)
    torch.cuda.synchronize()
    zd, cd, dfd = z.double().cpu(), cat.double().cpu(), dfused.double().cpu()
    gd = torch.sigmoid(zd)
    a, t = cd[:, :D], cd[:, D:]
    assert rel(fused, gd * a + (1 - gd) * t) <= EW[dtype]
    assert rel(dz, dfd * (a - t) * gd * (1 - gd)) <= EW[dtype]
    assert rel(dcat[:, :D], dfd * gd) <= EW[dtype]
    assert rel(dcat[:, D:], dfd * (1 - gd)) <= EW[dtype]


# ---------------------------------------------------------------------------------------------------------------------------------
# SE backward at non-default bottlenecks
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, HW, C, Cr).  vqa_se_bwd runs 256 threads per sample on small maps (HW * C / VEC below 2048 bf16 / 4096 fp32), 1024 otherwise:
# Cr = C at HW = 1 / 4 is Cr > NT (each thread owns several reduced channels), at 7 x 7 x 512 Cr < NT = 1024.  C / 3 does not divide
# the thread count.  bf16 C = 2048 over 36 pixels parks the most vectors in LDS (6 x 16 KB) next to the widest scratch; at Cr = C
# they no longer fit beside it in the 160 KB of a CU and fewer are parked.
SE_CASES = [(3, 49, 512, 1), (4, 196, 256, 1), (3, 49, 512, 170), (3, 196, 256, 85), (3, 1, 512, 512), (2, 4, 512, 512),
            (3, 4, 256, 256), (2, 49, 512, 512), (3, 196, 256, 40), (2, 36, 2048, 128), (2, 36, 2048, 2048)]


SE_PARAMS = [(c, d) for c in SE_CASES for d in DTYPES if d == torch.bfloat16 or c[2] <= 1024]      # fp32 takes C <= 1024


def _acc_decode(acc, R, K, C):
    """common.h layout: hi plane [R][K][C] (units of 2^-4) | flag | lo plane [R][K][C] (units of 2^-50)."""
    n = R * K * C
    hi = acc[:n].view(R, K, C).sum(0).double().cpu() / 16.0
    lo = acc[n + 1: 2 * n + 1].view(R, K, C).sum(0).double().cpu() / float(1 << 50)
    return hi + lo, int(acc[n])


@pytest.mark.parametrize("case,dtype", SE_PARAMS, ids=["B{}_HW{}_C{}_Cr{}-{}".format(*c, str(d)[6:]) for c, d in SE_PARAMS])
def test_se_backward_at_any_bottleneck_matches_fp64(case, dtype):
    L = _L()
    B, HW, C, Cr = case
    g = torch.Generator().manual_seed(B * 131 + HW * 17 + C + Cr)
    x = torch.relu(torch.randn(B * HW, C, generator=g)).to(DEV, dtype)             # SE input = a post-ReLU activation
    dout = torch.randn(B * HW, C, generator=g).to(DEV, dtype)
    y2 = torch.randn(B * HW, C, generator=g).to(DEV, dtype)
    coef = torch.stack([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.2,
                        torch.rand(C, generator=g) + 0.5]).to(DEV)
    w1 = torch.randn(Cr, C, generator=g) * (2.0 / C) ** 0.5
    if Cr == 1:
        w1 = w1.abs()                                                              # keep the single hidden unit alive
    w1 = w1.to(DEV)
    w2 = (torch.randn(C, Cr, generator=g) * (1.0 / Cr) ** 0.5).to(DEV)
    pooled = x.float().view(B, HW, C).mean(1).contiguous()
    hidden = torch.relu(pooled @ w1.t()).contiguous()
    scale = torch.sigmoid(hidden @ w2.t()).contiguous()
    assert float((hidden > 0).float().mean()) > 0.2
    dw1_0 = torch.randn(Cr, C, generator=g).to(DEV) * 0.1
    dw2_0 = torch.randn(C, Cr, generator=g).to(DEV) * 0.1

    def run(bn, mask_out=1):
        """bn: None (per-sample fused) | "slab" (per-sample reduce + grid-wide apply) | "acc" (fused, fixed-point BN sums)."""
        scratch = torch.full((L.count("vqa_se_bwd_scratch", L.dt(dtype), B, HW, C, Cr),), float("nan"), device=DEV)
        dx = torch.full_like(x, float("nan"))
        dw1, dw2 = dw1_0.clone(), dw2_0.clone()
        slab = None
        if bn == "slab":
            slab = torch.full((L.count("vqa_se_bwd_blocks", L.dt(dtype), B, HW, C), 3, C), float("nan"), device=DEV)
        elif bn == "acc":
            slab = torch.zeros(L.count("vqa_bn_acc_words", 3, C), device=DEV, dtype=torch.int64)
        L.call("vqa_se_bwd", L.dt(dtype), dout.data_ptr(), x.data_ptr(), w1.data_ptr(), w2.data_ptr(), pooled.data_ptr(), hidden.data_ptr(),
               scale.data_ptr(), scratch.data_ptr(), dx.data_ptr(), dw1.data_ptr(), dw2.data_ptr(), B, HW, C, Cr, mask_out,
               y2.data_ptr() if bn else None, coef.data_ptr() if bn else None, slab.data_ptr() if bn else None, int(bn == "acc"))
        torch.cuda.synchronize()
        dz2, dh, dpool = scratch[:B * C].view(B, C), scratch[B * C:B * (C + Cr)].view(B, Cr), scratch[B * (C + Cr):].view(B, C)
        return dict(dx=dx, dw1=dw1, dw2=dw2, dz2=dz2, dh=dh, dpool=dpool, slab=slab)

    # closed form in fp64 (the same as test_gpu_cnn_fused.test_se_backward_leaves_the_batchnorm_backward_sums)
    xd, dd = x.double().cpu().view(B, HW, C), dout.double().cpu().view(B, HW, C)
    sd, hd, pd = scale.double().cpu(), hidden.double().cpu(), pooled.double().cpu()
    dz2r = (dd * xd).sum(1) * sd * (1 - sd)
    dhr = (dz2r @ w2.double().cpu()) * (hd > 0)
    dpoolr = dhr @ w1.double().cpu()
    dxr_nomask = (dd * sd[:, None, :] + dpoolr[:, None, :] / HW).view(B * HW, C)
    dxr = dxr_nomask * (x.double().cpu() > 0)
    dw2r, dw1r = dz2r.t() @ hd, dhr.t() @ pd

    def check(o, dx_ref):
        assert rel(o["dz2"], dz2r) <= RED, ("dz2", rel(o["dz2"], dz2r))
        assert rel(o["dh"], dhr) <= RED, ("dh", rel(o["dh"], dhr))
        assert rel(o["dpool"], dpoolr) <= RED, ("dpool", rel(o["dpool"], dpoolr))
        assert rel(o["dx"], dx_ref) <= EW[dtype], ("dx", rel(o["dx"], dx_ref))
        e1 = (o["dw1"].double().cpu() - dw1_0.double().cpu() - dw1r).abs().max().item() / max(1e-6, dw1r.abs().max().item())
        e2 = (o["dw2"].double().cpu() - dw2_0.double().cpu() - dw2r).abs().max().item() / max(1e-6, dw2r.abs().max().item())
        assert e1 <= RED and e2 <= RED, ("dw1 / dw2", e1, e2)

    plain = run(None)
    check(plain, dxr)
    again = run(None)
    assert all(torch.equal(plain[k], again[k]) for k in ("dx", "dw1", "dw2", "dh"))
    check(run(None, mask_out=0), dxr_nomask)
    for bn in ("slab", "acc"):
        o = run(bn)
        check(o, dxr)
        gq = o["dx"].double().cpu()
        r0 = gq.sum(0)
        r1 = (gq * (y2.double().cpu() - coef[2].double().cpu()) * coef[3].double().cpu()).sum(0)
        if bn == "slab":
            s = o["slab"].double().cpu().sum(0)
        else:
            sums, flag = _acc_decode(o["slab"], max(1, min(8, 512 // C)), 3, C)
            assert flag == 0
            s = sums.double()
        tol = lambda r: 2e-4 * float(r.abs().max()) + 1e-4
        assert (s[0] - r0).abs().max().item() < tol(r0) and (s[1] - r1).abs().max().item() < tol(r1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_se_calls_refuse_a_bottleneck_wider_than_the_channels(dtype):
    L = _L()
    B, HW, C, Cr = 2, 4, 512, 513
    x = torch.zeros(B * HW, C, device=DEV, dtype=dtype)
    f = torch.zeros(2 * Cr * C, device=DEV)               # large enough for every operand of that shape
    with pytest.raises(RuntimeError, match="argument/shape"):
        L.call("vqa_se_fwd", L.dt(dtype), x.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), x.data_ptr(),
               B, HW, C, Cr, None, 0)
    with pytest.raises(RuntimeError, match="argument/shape"):
        L.call("vqa_se_bwd", L.dt(dtype), x.data_ptr(), x.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(),
               f.data_ptr(), x.data_ptr(), f.data_ptr(), f.data_ptr(), B, HW, C, Cr, 1, None, None, None, 0)
