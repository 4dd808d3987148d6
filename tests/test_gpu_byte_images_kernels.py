"""GPU: the uint8 stem entries through the C ABI against their fp32 siblings, torch.equal throughout.

vqa_u8_norm_table is compared with the CPU table of tests/_bytesref.py (pinned by tests/test_byte_images_cpu.py); each of
vqa_stem_conv_u8 / vqa_stem_conv_pool_u8 / vqa_stem_wgrad_u8 / vqa_stem_wgrad_fused_u8 reads the uint8 HWC batch and must give
the bits its sibling gives on ByteImages.to_float() of the same batch (vqa_image_normalize, or the torch expression at an odd
width).  The images (_bytesref.images) have zero borders with 0 / 255 corners and hold every byte value in every channel: padding
with table[c][0] instead of 0.0, or a read one byte past a row, cannot pass."""
import pytest
import torch

import _bytesref as R
from _pkg import pkg, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
NORMS = [R.IMAGENET, R.ODD]
_CACHE = {}


def _L():
    return sub("_lib")


def _out_hw(H, W):
    return (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1


def _table(mean, std):
    t = torch.empty((3, 256), device=DEV, dtype=torch.bfloat16)
    _L().call("vqa_u8_norm_table", *mean, *std, t.data_ptr())
    return t


def _inputs(B, H, W, norm=0):
    """(uint8 HWC batch, its float NCHW form, the device table, packed stem weights) of a shape, made once."""
    key = (B, H, W, norm)
    if key not in _CACHE:
        mean, std = NORMS[norm]
        u8 = R.images(B, H, W).to(DEV)
        f32 = pkg().load_dropin_byte_images().ByteImages(u8, mean, std).to_float()
        assert f32.shape == (B, 3, H, W) and f32.dtype == torch.float32 and f32.is_contiguous()
        g = torch.Generator().manual_seed(11)
        w = (torch.randn(64, 7, 7, 3, generator=g) * 0.1).to(DEV)
        wst = torch.empty((64, 192), device=DEV, dtype=torch.bfloat16)
        _L().call("vqa_stem_pack", w.data_ptr(), wst.data_ptr())
        _CACHE[key] = (u8, f32, _table(mean, std), wst)
    return _CACHE[key]


@pytest.mark.parametrize("norm", [0, 1])
def test_norm_table_equals_the_cpu_table(norm):
    mean, std = NORMS[norm]
    dev = _table(mean, std).cpu()
    assert torch.equal(dev.view(torch.int16), R.table(mean, std).view(torch.int16))


def test_to_float_is_the_normalize_kernel_and_the_torch_expression():
    """W % 4 == 0 goes through vqa_image_normalize, other widths through torch: the same float32 bits as the CPU expression."""
    BI = pkg().load_dropin_byte_images()
    for (B, H, W), (mean, std) in (((2, 8, 32), R.IMAGENET), ((2, 16, 31), R.ODD)):
        u8 = R.images(B, H, W)
        x = u8.permute(0, 3, 1, 2).float() / 255
        ref = torch.stack([(x[:, c] - mean[c]) / std[c] for c in range(3)], 1)
        assert torch.equal(BI.ByteImages(u8.to(DEV), mean, std).to_float().cpu(), ref)


def _conv(u8, f32, tab, wst, B, H, W, bytes_):
    L = _L()
    nb = L.count("vqa_stem_conv_blocks", B, H, W)
    assert nb > 0
    Ho, Wo = _out_hw(H, W)
    y = torch.full((B * Ho * Wo, 64), float("nan"), device=DEV, dtype=torch.bfloat16)
    st = torch.full((nb, 2, 64), float("nan"), device=DEV, dtype=torch.float32)
    if bytes_:
        L.call("vqa_stem_conv_u8", u8.data_ptr(), wst.data_ptr(), y.data_ptr(), st.data_ptr(), B, H, W, tab.data_ptr())
    else:
        L.call("vqa_stem_conv", f32.data_ptr(), wst.data_ptr(), y.data_ptr(), st.data_ptr(), B, H, W)
    return y, st


@pytest.mark.parametrize("shape,norm", [((3, 8, 32), 0), ((2, 16, 31), 1), ((2, 32, 64), 0)])
def test_stem_conv_u8_equals_stem_conv_on_the_normalised_batch(shape, norm):
    B, H, W = shape
    u8, f32, tab, wst = _inputs(B, H, W, norm)
    y0, s0 = _conv(u8, f32, tab, wst, B, H, W, False)
    y1, s1 = _conv(u8, f32, tab, wst, B, H, W, True)
    assert bool(torch.isfinite(y0.float()).all()) and float(y0.float().abs().max()) > 0
    assert torch.equal(y0, y1) and torch.equal(s0, s1)


@pytest.mark.parametrize("shape", [(3, 16, 32), (3, 16, 31)], ids=["vector_fill", "scalar_fill"])
def test_stem_conv_pool_u8_equals_its_sibling(shape):
    L = _L()
    B, H, W = shape
    assert L.count("vqa_stem_conv_pool_ok", B, H, W) == 1
    u8, f32, tab, wst = _inputs(B, H, W, 1 if W % 4 else 0)
    Ho, Wo = _out_hw(H, W)
    Hp, Wp = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
    g = torch.Generator().manual_seed(3)
    coef = torch.cat([torch.randn(64, generator=g), torch.randn(64, generator=g) * 0.5]).to(DEV)      # scale (both signs) | shift
    assert bool((coef[:64] < 0).any()) and bool((coef[:64] > 0).any())
    outs = []
    for bytes_ in (False, True):
        x = torch.full((B * Hp * Wp, 64), float("nan"), device=DEV, dtype=torch.bfloat16)
        if bytes_:
            L.call("vqa_stem_conv_pool_u8", u8.data_ptr(), wst.data_ptr(), coef.data_ptr(), x.data_ptr(), B, H, W, tab.data_ptr())
        else:
            L.call("vqa_stem_conv_pool", f32.data_ptr(), wst.data_ptr(), coef.data_ptr(), x.data_ptr(), B, H, W)
        outs.append(x)
    assert bool(torch.isfinite(outs[0].float()).all()) and float(outs[0].float().max()) > 0
    assert torch.equal(outs[0], outs[1])


def _wgrad_operands(B, H, W, u8, f32, tab, wst):
    """dy for the plain kernels; y, dpool, idx, coef, bcoef for the fused ones (y and idx from the forward kernels, so that the
    argmax codes are the ones the backward expects)."""
    L = _L()
    Ho, Wo = _out_hw(H, W)
    Hp, Wp = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
    g = torch.Generator().manual_seed(5)
    dy = (torch.randn(B * Ho * Wo, 64, generator=g) * 0.5).to(DEV).to(torch.bfloat16)
    y, _ = _conv(u8, f32, tab, wst, B, H, W, False)
    coef = torch.stack([torch.randn(64, generator=g), torch.randn(64, generator=g) * 0.5, torch.randn(64, generator=g) * 0.1,
                        torch.rand(64, generator=g) + 0.5]).to(DEV).contiguous()
    pooled = torch.empty((B * Hp * Wp, 64), device=DEV, dtype=torch.bfloat16)
    idx = torch.empty((B * Hp * Wp, 64), device=DEV, dtype=torch.uint8)
    L.call("vqa_stem_pool_fwd", 1, y.data_ptr(), coef.data_ptr(), pooled.data_ptr(), idx.data_ptr(), B, Ho, Wo, 64)
    dpool = (torch.randn(B * Hp * Wp, 64, generator=g) * 0.5).to(DEV).to(torch.bfloat16)
    bcoef = (torch.randn(3, 64, generator=g) * 0.3).to(DEV).contiguous()
    return dy, y, dpool, idx, coef, bcoef


def _wgrad(fused, bytes_, ops, u8, f32, tab, dw0, B, H, W, with_ws=True):
    L = _L()
    dy, y, dpool, idx, coef, bcoef = ops
    dw = dw0.clone()
    wsf = L.count("vqa_stem_wgrad_blocks", B, H, W) * 64 * 147
    assert wsf > 0
    ws = torch.empty(wsf, device=DEV, dtype=torch.float32) if with_ws else None
    img = u8 if bytes_ else f32
    tail = (tab.data_ptr(),) if bytes_ else ()
    wsa = (None, 0) if ws is None else (ws.data_ptr(), wsf)
    if fused:
        L.call("vqa_stem_wgrad_fused" + ("_u8" if bytes_ else ""), img.data_ptr(), y.data_ptr(), dpool.data_ptr(), idx.data_ptr(),
               coef.data_ptr(), bcoef.data_ptr(), dw.data_ptr(), B, H, W, *wsa, *tail)
    else:
        L.call("vqa_stem_wgrad" + ("_u8" if bytes_ else ""), img.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, H, W, *wsa, *tail)
    return dw


# (2, 8, 32): the smallest; (2, 32, 160): Wo = 80, a row contracted in pieces (nsplit > 1); (129, 64, 32): 1032 row blocks over the
# 1024-workgroup cap, so the grid-stride loop wraps
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("shape", [(2, 8, 32), (2, 32, 160), (129, 64, 32)])
def test_stem_wgrad_u8_equals_its_sibling(shape, fused):
    B, H, W = shape
    u8, f32, tab, wst = _inputs(B, H, W, 0)
    if shape == (129, 64, 32):
        assert B * (_out_hw(H, W)[0] // 4) == 1032 and _L().count("vqa_stem_wgrad_blocks", B, H, W) == 1024
    ops = _wgrad_operands(B, H, W, u8, f32, tab, wst)
    dw0 = torch.randn(64, 7, 7, 3, generator=torch.Generator().manual_seed(9)).to(DEV)      # += into the same nonzero start
    a = _wgrad(fused, False, ops, u8, f32, tab, dw0, B, H, W)
    b = _wgrad(fused, True, ops, u8, f32, tab, dw0, B, H, W)
    assert bool(torch.isfinite(a).all()) and not torch.equal(a, dw0)
    assert torch.equal(a, b)


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_stem_wgrad_u8_without_scratch(fused):
    """ws = NULL: the kernels add their partial sums with float atomics.  At (1, 8, 64) there is one workgroup, so every element gets
    exactly one add and the result does not depend on an order: bit-equal to the sibling's, and to the scratch route's."""
    B, H, W = 1, 8, 64
    assert _L().count("vqa_stem_wgrad_blocks", B, H, W) == 1
    u8, f32, tab, wst = _inputs(B, H, W, 0)
    ops = _wgrad_operands(B, H, W, u8, f32, tab, wst)
    dw0 = torch.randn(64, 7, 7, 3, generator=torch.Generator().manual_seed(9)).to(DEV)
    a = _wgrad(fused, False, ops, u8, f32, tab, dw0, B, H, W, with_ws=False)
    b = _wgrad(fused, True, ops, u8, f32, tab, dw0, B, H, W, with_ws=False)
    c = _wgrad(fused, True, ops, u8, f32, tab, dw0, B, H, W, with_ws=True)
    assert not torch.equal(a, dw0) and torch.equal(a, b) and torch.equal(b, c)


def test_u8_entries_refuse_a_null_table_and_unsupported_shapes():
    L = _L()
    B, H, W = 2, 8, 32
    u8, f32, tab, wst = _inputs(B, H, W, 0)
    ops = _wgrad_operands(B, H, W, u8, f32, tab, wst)
    dy, y, dpool, idx, coef, bcoef = ops
    dw = torch.zeros(64, 7, 7, 3, device=DEV)
    out = torch.empty((B * 4 * 16, 64), device=DEV, dtype=torch.bfloat16)
    c2 = torch.zeros(128, device=DEV)

    def calls(b, h, w, table):
        return [("vqa_stem_conv_u8", (u8.data_ptr(), wst.data_ptr(), out.data_ptr(), None, b, h, w, table)),
                ("vqa_stem_conv_pool_u8", (u8.data_ptr(), wst.data_ptr(), c2.data_ptr(), out.data_ptr(), b, h, w, table)),
                ("vqa_stem_wgrad_u8", (u8.data_ptr(), dy.data_ptr(), dw.data_ptr(), b, h, w, None, 0, table)),
                ("vqa_stem_wgrad_fused_u8", (u8.data_ptr(), y.data_ptr(), dpool.data_ptr(), idx.data_ptr(), coef.data_ptr(), bcoef.data_ptr(),
                                             dw.data_ptr(), b, h, w, None, 0, table))]
    for name, args in calls(B, H, W, None):                                  # a null table
        with pytest.raises(RuntimeError, match="status 1000"):
            L.call(name, *args)
    for name, args in calls(B, 10, 32, tab.data_ptr()):                      # Ho = 5: no multiple of the row block; Hp = 3: no multiple of 4
        with pytest.raises(RuntimeError, match="status 1000"):
            L.call(name, *args)
    for bad in ((float("nan"), 0.0, 0.0, 1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 0.0, 1.0, float("inf"), 1.0)):
        with pytest.raises(RuntimeError, match="status 1000"):
            L.call("vqa_u8_norm_table", *bad, tab.data_ptr())
    with pytest.raises(RuntimeError, match="status 1000"):
        L.call("vqa_u8_norm_table", 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, None)
    torch.cuda.synchronize()
    assert torch.equal(dw, torch.zeros_like(dw))                             # nothing was launched
