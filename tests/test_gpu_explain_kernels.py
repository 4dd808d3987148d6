"""GPU: the four explain kernels (csrc/explain_ops.hip) against the fp64 references of tests/_explainref.py computed on the same
stored operands, fp32 and bf16 inputs.

Bounds.  vqa_gradcam sums P terms (the channel means), then C products, in fp32: |cam - ref| <= (P + C + 3) * 2^-24 * S' with
S'[b][p] = sum_c mean_p |dfeat| * |feat| -- 4e-5 * S' at (P, C) = (144, 512); 1e-4 * S' leaves room for another summation tree.
vqa_attention_map adds at most ncl * H * L = 320 non-negative terms: 2e-5 relative, held to 1e-6 + 1e-4 * ref.  vqa_class_seed
is exact.  vqa_heatmap_render is exact where every intermediate is (map values k / 256, a power-of-two scale, alpha = 0.5) and within
one level otherwise: an index off by one moves the blend by at most alpha."""
import pytest
import torch

import _explainref as R
from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]


def _rand(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV).to(dtype)


def _call(name, *args):
    """Raw status of a C-ABI entry on the current stream (the wrappers raise on a non-zero one)."""
    L = sub("_lib")
    return getattr(L.lib(), name)(*args, L.stream())


# ------------------------------------------------------------------------------------------------ vqa_gradcam
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,P,C", [(3, 49, 512), (2, 144, 512), (1, 1, 8), (2, 4, 64)])
def test_gradcam_matches_fp64(B, P, C, dtype):
    K = sub("kernels")
    feat, dfeat = _rand((B, P, C), 10 + P, dtype), _rand((B, P, C), 20 + P, dtype) * 0.01
    ref, sprime = R.gradcam(feat, dfeat)
    cam = K.gradcam(feat, dfeat, B, P, C, normalize=False)
    torch.cuda.synchronize()
    assert cam.dtype == torch.float32 and tuple(cam.shape) == (B, P)
    err = (cam.double() - ref).abs()
    print(f"gradcam {B}x{P}x{C} {dtype}: max err / S' = {float((err / sprime.clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= 1e-4 * sprime).all())
    if B * P >= 64:
        assert bool((ref > 0).any()) and bool((ref == 0).any())                 # both sides of the ReLU are exercised
    # normalised: exactly the unnormalised values divided by their row maximum, in fp32
    mx = cam.amax(1, keepdim=True)
    want = torch.where(mx > 0, cam / mx, cam)
    assert torch.equal(K.gradcam(feat, dfeat, B, P, C, normalize=True), want)
    # bit-reproducible
    assert torch.equal(K.gradcam(feat, dfeat, B, P, C, normalize=False), cam)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_gradcam_all_negative_image_is_exactly_zero(dtype):
    K = sub("kernels")
    B, P, C = 3, 49, 512
    feat, dfeat = _rand((B, P, C), 31, dtype), _rand((B, P, C), 32, dtype)
    feat[1] = -feat[1].abs() - 0.5                 # with positive channel weights every weighted sum of image 1 is negative
    dfeat[1] = dfeat[1].abs() + 0.5
    for normalize in (False, True):
        cam = K.gradcam(feat, dfeat, B, P, C, normalize=normalize)
        assert torch.equal(cam[1], torch.zeros_like(cam[1]))
        assert bool((cam[0] > 0).any()) and bool((cam[2] > 0).any()) and bool(torch.isfinite(cam).all())
        if normalize:
            assert float(cam[0].max()) == 1.0 and float(cam[2].max()) == 1.0


def test_gradcam_refuses_shapes_it_does_not_take():
    feat, cam = _rand((2, 4, 2048), 33), torch.full((2, 4), 7.0, device=DEV)
    for C in (12, 4, 0, 2048):
        assert _call("vqa_gradcam", 0, feat.data_ptr(), feat.data_ptr(), cam.data_ptr(), 2, 4, C, 0) == 1000
    assert _call("vqa_gradcam", 0, feat.data_ptr(), feat.data_ptr(), cam.data_ptr(), 2, 0, 64, 0) == 1000
    assert _call("vqa_gradcam", 2, feat.data_ptr(), feat.data_ptr(), cam.data_ptr(), 2, 4, 64, 0) == 1000
    assert _call("vqa_gradcam", 0, feat.data_ptr(), None, cam.data_ptr(), 2, 4, 64, 0) == 1000
    torch.cuda.synchronize()
    assert bool((cam == 7.0).all())                # nothing was launched
    with pytest.raises(RuntimeError, match="status 1000"):
        sub("kernels").gradcam(feat[:, :, :12].contiguous(), feat[:, :, :12].contiguous(), 2, 4, 12)


# ------------------------------------------------------------------------------------------------ vqa_class_seed
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_class_seed_is_exact(dtype):
    K = sub("kernels")
    B, N = 9, 1000
    x = _rand((B, N), 41, dtype)
    x[1, 700] = x[1, 30] = x[1].max() + 1          # a tie: the lower index wins
    x[2, 500] = float("nan")                       # a NaN ranks first
    x[3, 10] = x[3, 900] = float("nan")            # ... NaNs among themselves by index
    x[4] = 0.0                                     # every entry ties
    x[4, 5] = -0.0
    x[5, 999] = x[5].max() + 1                     # the last column
    chosen, dl = K.class_seed(x)
    ref_c, ref_d = R.class_seed(x)
    torch.cuda.synchronize()
    assert chosen.dtype == torch.int64 and dl.dtype == dtype and tuple(dl.shape) == (B, N)
    assert chosen.tolist()[:6] == [int(ref_c[0]), 30, 500, 10, 0, 999]
    assert torch.equal(chosen, ref_c) and torch.equal(dl.double(), ref_d)
    assert torch.equal(chosen, K.softmax_topk(x, 1)[0][:, 0])
    # given ids
    ids = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(42)).to(DEV)
    chosen, dl = K.class_seed(x, ids)
    assert torch.equal(chosen, ids) and torch.equal(dl.double(), R.class_seed(x, ids)[1])
    # a row stride greater than N
    wide = _rand((B, N + 24), 43, dtype)
    wide[:, N:] = 1e4                              # beyond the row: must not be seen
    view = wide[:, :N]
    chosen, dl = K.class_seed(view)
    assert torch.equal(chosen, R.class_seed(view)[0]) and torch.equal(dl.double(), R.class_seed(view)[1]) and dl.is_contiguous()
    assert torch.equal(chosen, K.softmax_topk(view, 1)[0][:, 0])
    # small and odd widths, one row
    for n in (1, 7, 64, 65):
        y = _rand((1, n), 44 + n, dtype)
        chosen, dl = K.class_seed(y)
        assert torch.equal(chosen, R.class_seed(y)[0]) and torch.equal(dl.double(), R.class_seed(y)[1])
    assert _call("vqa_class_seed", 0, x.data_ptr(), 10, None, chosen.data_ptr(), dl.data_ptr(), 1, 64) == 1000      # ld < N


# ------------------------------------------------------------------------------------------------ vqa_attention_map
def _attention_case(ncl, B, H, L, P, seed):
    caw = torch.softmax(_rand((ncl, B, H, L, P), seed) * 2, dim=-1).contiguous()
    lens = torch.randint(1, L + 1, (B,), generator=torch.Generator().manual_seed(seed + 1))
    ragged = (torch.arange(L)[None, :] < lens[:, None]).float().to(DEV)
    return caw, ragged


@pytest.mark.parametrize("ncl,B,H,L,P", [(2, 3, 8, 20, 49), (1, 2, 8, 5, 144), (2, 1, 1, 1, 1)])
def test_attention_map_matches_fp64(ncl, B, H, L, P):
    K = sub("kernels")
    caw, ragged = _attention_case(ncl, B, H, L, P, 50 + P)
    allpad = ragged.clone()
    allpad[B - 1] = 0.0                            # one all-padding question
    for name, mask in (("ragged", ragged), ("none", None), ("all-padding row", allpad)):
        ref = R.attention_map(caw, mask)
        out = K.attention_map(caw, mask, normalize=False)
        torch.cuda.synchronize()
        assert out.dtype == torch.float32 and tuple(out.shape) == (B, P)
        rows = slice(0, B - 1) if mask is allpad else slice(0, B)
        err = (out.double() - ref)[rows].abs()
        assert bool((err <= 1e-6 + 1e-4 * ref[rows]).all()), name
        assert bool(((out[rows].double().sum(1) - 1).abs() <= 1e-5).all()), name
        if mask is allpad:
            assert bool(torch.isnan(out[B - 1]).all()) and bool(torch.isnan(ref[B - 1]).all())
        mx = torch.nan_to_num(out, nan=0.0).amax(1, keepdim=True)
        norm = K.attention_map(caw, mask, normalize=True)
        want = torch.where(mx > 0, out / mx, out)
        assert torch.equal(torch.nan_to_num(norm, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), name
        assert torch.equal(torch.nan_to_num(K.attention_map(caw, mask, normalize=False), nan=-1.0), torch.nan_to_num(out, nan=-1.0))


def test_attention_map_ignores_what_padding_tokens_hold():
    K = sub("kernels")
    caw, ragged = _attention_case(2, 3, 8, 20, 49, 60)
    out = K.attention_map(caw, ragged, normalize=False)
    dirty = caw.clone()
    dirty[ragged[None, :, None, :].expand(2, 3, 8, 20) == 0] = float("nan")
    assert torch.equal(K.attention_map(dirty, ragged, normalize=False), out)
    out0 = torch.full((3, 49), 7.0, device=DEV)
    assert _call("vqa_attention_map", caw.data_ptr(), None, out0.data_ptr(), 2, 3, 8, 200, 49, 0) == 1000      # L * P > 8192
    assert _call("vqa_attention_map", caw.data_ptr(), None, out0.data_ptr(), 0, 3, 8, 20, 49, 0) == 1000
    torch.cuda.synchronize()
    assert bool((out0 == 7.0).all())


# ------------------------------------------------------------------------------------------------ vqa_heatmap_render
def _table(seed):
    return torch.randint(0, 256, (256, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(torch.uint8).to(DEV)


def _base(B, H, W, seed):
    return torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(torch.uint8).to(DEV)


@pytest.mark.parametrize("src,dst", [((7, 7), (56, 56)), ((2, 3), (8, 12)), ((12, 12), (96, 96))])
def test_heatmap_render_exact_case(src, dst):
    """Map values k / 256, weights that are multiples of 1/16 (scale 8) or 1/8 (scale 4), alpha = 0.5: every intermediate is exact in
    fp32 (products below 2^24), so the bytes equal the fp64 reference's."""
    K = sub("kernels")
    B = 3
    maps = (torch.randint(0, 257, (B,) + src, generator=torch.Generator().manual_seed(70 + src[0])).float() / 256).to(DEV)
    lut, base = _table(71), _base(B, dst[0], dst[1], 72)
    out = K.heatmap_render(maps, base=base, alpha=0.5, colormap=lut)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B,) + dst + (3,)
    assert torch.equal(out, R.render(maps, dst, lut, base, 0.5))
    # without a base the output is the table lookup
    assert torch.equal(K.heatmap_render(maps, size=dst, colormap=lut), R.render(maps, dst, lut))


@pytest.mark.parametrize("src,dst", [((3, 3), (8, 8)), ((7, 7), (40, 64)), ((7, 7), (30, 41))])
def test_heatmap_render_within_one_level(src, dst):
    """Random maps at a scale that is no power of two (and, 41 wide, the byte-wise route for a width that is no multiple of 4),
    alpha = 0.4, the grey ramp lut[i] = (i, i, i): an index off by one moves the blend by 0.4, so every byte is within one level."""
    K = sub("kernels")
    B = 2
    maps = torch.rand((B,) + src, generator=torch.Generator().manual_seed(80 + dst[1])).to(DEV)
    lut = torch.arange(256, dtype=torch.uint8)[:, None].repeat(1, 3).to(DEV)
    base = _base(B, dst[0], dst[1], 81)
    out = K.heatmap_render(maps, base=base, alpha=0.4, colormap=lut)
    ref = R.render(maps, dst, lut, base, 0.4)
    diff = (out.int() - ref.int()).abs()
    print(f"render {src}->{dst}: {int((diff > 0).sum())} of {diff.numel()} bytes differ by one level")
    assert int(diff.max()) <= 1
    plain = (K.heatmap_render(maps, size=dst, colormap=lut).int() - R.render(maps, dst, lut).int()).abs()
    assert int(plain.max()) <= 1


def test_heatmap_render_special_values_and_refusals():
    K = sub("kernels")
    lut = _table(90)
    maps = torch.tensor([[[float("nan"), -1.0], [2.0, 0.5]]], device=DEV)
    out = K.heatmap_render(maps, size=(2, 2), colormap=lut)
    assert torch.equal(out[0, 0, 0], lut[0]) and torch.equal(out[0, 0, 1], lut[0]) and torch.equal(out[0, 1, 0], lut[255])
    assert torch.equal(out[0, 1, 1], lut[128])                                  # floor(0.5 * 255 + 0.5)
    # the default table, and alpha at both ends
    d = K.default_colormap().to(DEV)
    base = _base(1, 2, 2, 91)
    assert torch.equal(K.heatmap_render(maps, size=(2, 2)), R.render(maps, (2, 2), d))
    assert torch.equal(K.heatmap_render(maps, base=base, alpha=0.0), base)
    assert torch.equal(K.heatmap_render(maps, base=base, alpha=1.0), R.render(maps, (2, 2), d))
    keep = torch.full((1, 2, 2, 3), 9, dtype=torch.uint8, device=DEV)
    for alpha in (-0.5, 1.5, float("nan")):
        assert _call("vqa_heatmap_render", maps.data_ptr(), None, lut.data_ptr(), keep.data_ptr(), 1, 2, 2, 2, 2, alpha) == 1000
    assert _call("vqa_heatmap_render", maps.data_ptr(), None, lut.data_ptr(), keep.data_ptr(), 1, 2, 2, 0, 2, 0.5) == 1000
    torch.cuda.synchronize()
    assert bool((keep == 9).all())
