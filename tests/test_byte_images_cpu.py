"""CPU: the host side of uint8 images end to end -- every refusal of the ByteImages wrapper and its shape, the five new C-ABI entries
in the ctypes table with the header's arity, and the torch restatement of the norm table (tests/_bytesref.py) that the GPU tests
compare the device table against: per channel it is monotone in the byte value and holds the bf16 rounding of the fp32 expression."""
import os
import re

import pytest
import torch

import _bytesref as R
from _pkg import REPO, pkg, sub


def _BI():
    return pkg().load_dropin_byte_images()


def test_wrapper_members_and_shape():
    BI = _BI()
    u8 = torch.zeros(5, 6, 7, 3, dtype=torch.uint8)
    b = BI.ByteImages(u8)
    assert b.data is u8 and b.shape_nchw == (5, 3, 6, 7) and len(b) == 5
    assert b.mean == tuple(BI.IMAGENET_MEAN) and b.std == tuple(BI.IMAGENET_STD)
    b = BI.ByteImages(u8, R.ODD[0], R.ODD[1])
    assert b.mean == R.ODD[0] and b.std == R.ODD[1]
    assert sub("kernels").is_byte_images(b) and not sub("kernels").is_byte_images(u8)
    assert pkg().load_dropin().ByteImages is BI.ByteImages             # exported beside ImageFeatures


@pytest.mark.parametrize("bad", [torch.zeros(2, 4, 4, 3), torch.zeros(2, 4, 4, 3, dtype=torch.int8), torch.zeros(2, 4, 4, 3, dtype=torch.int64),
                                 [[[[0, 0, 0]]]]])
def test_wrapper_refuses_other_dtypes(bad):
    with pytest.raises(TypeError):
        _BI().ByteImages(bad)


def test_wrapper_refuses_bad_shapes_and_statistics():
    BI = _BI()
    u8 = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    nan, inf = float("nan"), float("inf")
    for t in (u8[0], u8.unsqueeze(0), torch.zeros(2, 3, 4, 4, dtype=torch.uint8),          # rank 3, rank 5, channels first
              torch.zeros(2, 4, 3, 4, dtype=torch.uint8).transpose(2, 3),                  # [2, 4, 4, 3] but not contiguous
              torch.zeros(2, 4, 8, 3, dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(ValueError):
            BI.ByteImages(t)
    for mean, std in (((nan, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.0, inf, 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0), (1.0, 1.0, 1.0)),
                      ((0.0, 0.0, 0.0), (1.0, 0.0, 1.0)), ((0.0, 0.0, 0.0), (1.0, 1.0, nan)), ((0.0, 0.0, 0.0), (inf, 1.0, 1.0)),
                      ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), 1.0)):
        with pytest.raises(ValueError):
            BI.ByteImages(u8, mean, std)


def test_wrapper_refuses_gradients_and_host_normalisation():
    b = _BI().ByteImages(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    assert b.requires_grad is False and b.requires_grad_(False) is b
    with pytest.raises(TypeError, match="float images"):
        b.requires_grad_()
    with pytest.raises(RuntimeError, match="GPU only"):
        b.to_float()


def test_signatures_hold_the_new_entries_with_the_headers_arity():
    L = sub("_lib")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vqa_hip.h")).read(), flags=re.S)
    want = {"vqa_u8_norm_table": 8, "vqa_stem_conv_u8": 9, "vqa_stem_conv_pool_u8": 9, "vqa_stem_wgrad_u8": 10, "vqa_stem_wgrad_fused_u8": 14}
    for name, n in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(L.SIGNATURES[name]) == n, name
    # a sibling's arguments, with the table in front of the stream
    for name in ("vqa_stem_conv", "vqa_stem_conv_pool", "vqa_stem_wgrad", "vqa_stem_wgrad_fused"):
        assert L.SIGNATURES[name + "_u8"] == L.SIGNATURES[name][:-1] + [L.P, L.P]


@pytest.mark.parametrize("mean,std", [R.IMAGENET, R.ODD])
def test_reference_table_is_monotone_and_is_the_rounded_fp32_value(mean, std):
    t = R.table(mean, std)
    assert t.shape == (3, 256) and t.dtype == torch.bfloat16
    f = t.float()
    for c in range(3):
        d = f[c, 1:] - f[c, :-1]
        assert bool((d >= 0).all() if std[c] > 0 else (d <= 0).all())                      # monotone per channel (bf16 may tie)
        assert float(f[c, 0]) != float(f[c, 255])
        for v in (0, 1, 127, 128, 254, 255):                                               # f2bf of the fp32 value, element by element
            x = (torch.tensor(float(v), dtype=torch.float32) / 255 - torch.tensor(mean[c], dtype=torch.float32)) / torch.tensor(std[c], dtype=torch.float32)
            assert R.f2bf_bits(float(x)) == int(t[c, v].view(torch.int16)) & 0xFFFF, (c, v)
    # every entry: within half a bf16 ulp of the fp32 value (8 significand bits: half an ulp is at most 2^-8 |x|)
    x32 = R.table_f32(mean, std)
    assert bool(((f - x32).abs() <= x32.abs() * 2.0 ** -8).all())


def test_step_key_separates_byte_images_by_mean_and_std():
    SG, BI = sub("stepgraph"), _BI()
    u8 = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    kw = dict(features=False, token_ids=torch.zeros(2, 4, dtype=torch.long), attention_mask=None, image_index=None,
              targets=torch.zeros(2, dtype=torch.long), plan=None, loss_kind="ce", loss_opts=(0.0, None, None), ema=False, metrics=None,
              flat_ptr=1, wsrc_ptr=2, table_id=None)
    a = SG.step_key(images=BI.ByteImages(u8), **kw)
    assert a == SG.step_key(images=BI.ByteImages(u8.clone()), **kw)
    assert a != SG.step_key(images=BI.ByteImages(u8, R.ODD[0], R.ODD[1]), **kw)
    assert a != SG.step_key(images=BI.ByteImages(u8, std=(0.5, 0.5, 0.5)), **kw)
    assert a != SG.step_key(images=torch.zeros(2, 3, 8, 8), **kw) and a != SG.step_key(images=u8, **kw)
