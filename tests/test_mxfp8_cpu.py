"""CPU: the MXFP8 quantization rule's oracle (tests/_mxfp8.py) against hand-computed codes, the C ABI of the MXFP8 entries, and
VQAModel.set_inference_precision's validation."""
import os
import re

import pytest
import torch

import _mxfp8 as MX
from _pkg import REPO, pkg, sub


def _block(vals, dtype=torch.float32):
    x = torch.zeros(32, dtype=dtype)
    x[: len(vals)] = torch.tensor(vals, dtype=torch.float64).to(dtype)
    return x


def test_zero_block():
    for z in (0.0, -0.0):
        q, s = MX.quant(torch.full((32,), z))
        assert s.tolist() == [127] and q.tolist() == [0] * 32          # +0 even for -0 inputs


def test_rne_ties_and_subnormals_at_unit_scale():
    # amax 256 -> floor(log2) = 8 -> X = 0: x / 2^X = x
    x = _block([256.0, 2.0 ** -8, 3 * 2.0 ** -10, 2.0 ** -10, 1.0625, -1.1875, 2.0 ** -9, 5 * 2.0 ** -11, -(2.0 ** -6)])
    q, s = MX.quant(x)
    assert s.tolist() == [127]
    #   256 = 2^8 -> 0x78; 2^-8 = 2 subnormal steps -> 0x02; 1.5 steps ties to even 2 -> 0x02; 0.5 step ties to 0 -> 0x00;
    #   1.0625 ties between 1.0 (0x38) and 1.125 to even -> 0x38; -1.1875 ties between 1.125 and 1.25 to even -> 1.25 = 0xBA;
    #   2^-9 = 1 step -> 0x01; 1.25 steps -> 0x01; -2^-6 = smallest normal -> 0x88
    assert q[:9].tolist() == [0x78, 0x02, 0x02, 0x00, 0x38, 0xBA, 0x01, 0x01, 0x88]
    assert q[9:].tolist() == [0] * 23


def test_scaled_block_and_subnormal_results():
    # amax 3e-3: floor(log2) = -9 -> X = -17, scale code 110; x * 2^17
    x = _block([3e-3, -1e-3, 2.0 ** -26, 2.0 ** -27])
    q, s = MX.quant(x)
    assert s.tolist() == [110]
    # 3e-3 * 2^17 = 393.216 -> 384 (0x7C, step 32 above 256: 384 < 393.2 < 416); -131.072 -> -128 (0xF0);
    # 2^-26 * 2^17 = 2^-9 -> 0x01 (smallest subnormal); 2^-27 * 2^17 = 2^-10 -> half a step, ties to 0
    assert q[:4].tolist() == [0x7C, 0xF0, 0x01, 0x00]


def test_values_between_448_and_512_saturate():
    x = _block([511.0, 480.0, -500.0, 449.0, 448.0, 447.0])           # amax 511 -> X = 0: x / 2^X reaches (448, 512)
    q, s = MX.quant(x)
    assert s.tolist() == [127]
    assert q[:6].tolist() == [0x7E, 0x7E, 0xFE, 0x7E, 0x7E, 0x7E]       # 447 rounds to 448 as well (step 32 above 256)


def test_extreme_scales():
    q, s = MX.quant(_block([1.5 * 2.0 ** 127, -(2.0 ** 120)]))          # X = 127 - 8 = 119
    assert s.tolist() == [246] and q[:2].tolist() == [0x7C, 0xC0]      # 1.5 * 2^8 = 384 -> 0x7C; -2^120 / 2^119 = -2 -> 0xC0


def test_tiny_block_clamps_the_exponent():
    x = _block([2.0 ** -140, 2.0 ** -130])                             # floor(log2) - 8 = -138 -> clamped to -127
    q, s = MX.quant(x)
    assert s.tolist() == [0]
    # 2^-140 * 2^127 = 2^-13 -> 0; 2^-130 * 2^127 = 2^-3 -> 0x20
    assert q[:2].tolist() == [0x00, 0x20]


def test_nonfinite_blocks():
    for bad in (float("inf"), float("-inf"), float("nan")):
        x = torch.cat([_block([1.0, bad, 3.0]), _block([1.0, 2.0])])
        q, s = MX.quant(x)
        assert s.tolist() == [255, 120]                                 # clean block: amax 2 -> X = -7
        assert q[32:34].tolist() == [0x70, 0x78]
        assert torch.isnan(MX.dequant(q, s)[:32]).all()


def test_bf16_input_and_dequant_round_trip():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(64, 128, generator=g) * torch.exp2(torch.randint(-20, 20, (64, 4), generator=g).float()).repeat_interleave(32, 1))
    for dt in (torch.float32, torch.bfloat16):
        q, s = MX.quant(x.to(dt))
        d = MX.dequant(q, s)
        ref = x.to(dt).double()
        blk_max = ref.abs().reshape(64, 4, 32).amax(-1, keepdim=True).expand(64, 4, 32).reshape(64, 128)
        # e4m3 RNE: relative error <= 2^-4, but x / 2^X in (448, 512) saturates to 448 (<= 1/8); subnormal results: absolute
        # half a step, 2^-10 * 2^X <= 2^-18 of the block's amax
        assert ((d - ref).abs() <= 2.0 ** -3 * ref.abs() + 2.0 ** -18 * blk_max).all()


def _header_symbols():
    txt = open(os.path.join(REPO, "include", "vqa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(?:int|long long)\s+(vqa_\w+)\s*\(", txt))


def test_mxfp8_entries_are_declared_and_bound():
    names = {"vqa_mx_quant", "vqa_fold_bn_mxfp8", "vqa_conv_mxfp8"}
    assert names <= _header_symbols()
    assert names <= set(sub("_lib").SIGNATURES)
    assert "mxfp8.hip" in sub("build").SOURCES


def _cpu_model(dtype):
    M = pkg().load_dropin()
    return M.VQAModel(vocab_size=50, embed_dim=32, num_answers=10, num_transformer_layers=1, num_attention_heads=4,
                      ffn_hidden_dim=64, num_cross_layers=1, compute_dtype=dtype, seed=0)


def test_set_inference_precision_validation():
    m = _cpu_model("bf16")
    assert m.inference_precision == "bf16"
    assert m.set_inference_precision("mxfp8") is m and m.inference_precision == "mxfp8"
    with pytest.raises(ValueError):
        m.set_inference_precision("fp8")
    assert m.inference_precision == "mxfp8"
    sd = m.state_dict()
    assert not any("precision" in k for k in sd)
    m.set_inference_precision("bf16")
    assert m.inference_precision == "bf16"
    f = _cpu_model("fp32")
    with pytest.raises(ValueError):
        f.set_inference_precision("mxfp8")
    assert f.set_inference_precision("bf16").inference_precision == "bf16"
    with pytest.raises(AttributeError):
        m.inference_precision = "mxfp8"
