"""tests/_foldref.py checked without a GPU.

1. The reference is the reference: its folded block equals oracle.vqa_oracle.residual_block(..., training=False) in fp64 to 1e-10
   on the jittered state dict (with the small-variance channel of _foldref.state_dict), for all 8 blocks, and its stem the
   oracle's eval stem.
2. The bound would catch a subtly wrong kernel: on both shapes of tests/test_gpu_inference_insitu.py, with bf16 rounding of every
   store standing in for the kernels, the checks of that test (_foldref.check_block / check_operands through Checker.check at
   T_BF16) pass for the faultless stand-in and flag each of _foldref.FAULTS in every block it applies to, in a per-image or
   per-channel slice:
     bias_dropped              conv2's folded bias of one channel is zero
     relu_before_addend        relu(conv2 + b2) + res in place of relu(conv2 + b2 + res)
     shortcut_stride1_cropped  the 1x1 shortcut taken at stride 1 and cropped to the output size (blocks with a downsample)
     image_zeroed              the last image's block output is zero
     no_eps                    the fold uses running_var without eps
   The faultless stand-in accumulates in fp32 and stores in bf16: it is also the measurement of the one bound that is wider than
   T_BF16, _foldref.T_CONV2_CHANNEL (twice the stand-in's worst channel of a block output; asserted below)."""
import pytest
import torch

import _foldref as R
from _insitu import Checker, T_BF16
from oracle import vqa_oracle as O

CFG = O.full_config()
SD = R.state_dict(CFG, R.SD_SEED)


def test_small_variance_channel_keeps_the_scale_and_needs_eps():
    plain = O.init_state_dict(CFG, R.SD_SEED, jitter=True)
    c = R.SMALL_VAR_CHANNEL
    for wname, bn in R.fold_pairs(SD):
        assert float(SD[bn + ".running_var"][c]) == pytest.approx(2e-5)
        w, b, _ = R.fold_sd(SD, wname, bn)
        w0 = plain[wname][c].double() * plain[bn + ".weight"][c].double()                     # the folded scale is the plain gamma
        assert float((w[c] - w0).abs().max()) <= 1e-6 * float(w0.abs().max())
        wn, _, _ = R.fold_sd(SD, wname, bn, eps=0.0)
        assert float((wn[c] / w[c]).mean()) == pytest.approx(1.5 ** 0.5, rel=1e-6)
    assert len(R.fold_pairs(SD)) == 19                              # 8 x 2 convs and the 3 shortcuts of stages 2 to 4


def test_folded_block_equals_the_oracle_block_in_fp64():
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in SD.items()}
    g = torch.Generator().manual_seed(1)
    for p, s, b, cin, cout, stride in R.blocks():
        x = torch.randn(2, cin, 9, 11, generator=g, dtype=torch.float64)
        ref = O.residual_block(x, sd64, p, stride, False, None)
        a1, res, out = R.folded_block(x, R.folded_operands(SD, p), stride)
        assert out.shape == ref.shape and float((out - ref).abs().max()) <= 1e-10 * max(1.0, float(ref.abs().max())), p
        assert ("downsample" in R.folded_operands(SD, p)) == (b == 0 and s > 1)
    img = torch.randn(2, 3, 40, 64, generator=g, dtype=torch.float64)
    st = "image_encoder.stem."
    got = R.stem(img, SD[st + "0.weight"], SD[st + "1.weight"], SD[st + "1.bias"], SD[st + "1.running_mean"], SD[st + "1.running_var"])
    ref = O.stem(img, sd64, False, None)
    assert float((got - ref).abs().max()) <= 1e-10 * max(1.0, float(ref.abs().max()))
    # a whole stage: two folded blocks and the stage's attention
    x = torch.randn(2, 128, 6, 5, generator=g, dtype=torch.float64)
    y = x
    for p, s, b, cin, cout, stride in R.blocks()[4:6]:
        y = R.folded_block(y, R.folded_operands(SD, p), stride)[2]
    ref = O.residual_stage(x, sd64, 3, False, None)
    assert float((R.stage_attention(y, SD, 3) - ref).abs().max()) <= 1e-10 * max(1.0, float(ref.abs().max()))


def _kernel_operands(ops):
    """what the bf16 kernels read: the folded weight rounded to bf16, the bias in fp32"""
    return {k: (R.rnd_bf16(w), b.float().double()) for k, (w, b) in ops.items()}


def _flagged(ck):
    assert ck.fails, "not flagged"
    assert any(str(f[1]).startswith("dim") for f in ck.fails), ck.fails          # a per-image or per-channel slice failed


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_bound_passes_the_stand_in_and_flags_every_fault(name):
    B, IH, IW = R.CONFIGS[name]
    images = R.images(name)
    st = "image_encoder.stem."
    x = R.rnd_bf16(R.stem(R.rnd_bf16(images), R.rnd_bf16(SD[st + "0.weight"]), SD[st + "1.weight"], SD[st + "1.bias"],
                          SD[st + "1.running_mean"], SD[st + "1.running_var"]))
    good = Checker()
    for p, s, b, cin, cout, stride in R.blocks():
        ref_ops = R.folded_operands(SD, p)
        ops = _kernel_operands(ref_ops)
        a1, _, out = R.folded_block(x, ops, stride, R.rnd_bf16, acc=torch.float32)
        for k in ops:
            R.check_operands(good, f"{p} {k}", *ops[k], *ref_ops[k], T_BF16)
        R.check_block(good, p, x, a1, out, ops, stride, T_BF16)
        for fault in R.FAULTS:
            ck = Checker()
            if fault == "no_eps":                                     # a fault of the fold: caught where the operands are checked
                bad = _kernel_operands(R.folded_operands(SD, p, eps=0.0))
                for k in bad:
                    R.check_operands(ck, f"{p} {k}", *bad[k], *ref_ops[k], T_BF16)
            elif fault == "shortcut_stride1_cropped" and "downsample" not in ops:
                continue
            else:
                fa1, _, fout = R.folded_block(x, ops, stride, R.rnd_bf16, fault=fault)
                R.check_block(ck, p, x, fa1, fout, ops, stride, T_BF16)
            try:
                _flagged(ck)
            except AssertionError as e:
                raise AssertionError(f"{name} {p} {fault}: {e}")
        if b == 1:
            x = R.stage_attention(out, SD, s, R.rnd_bf16, R.rnd_bf16)
            R.check_attention(good, s, out, x, SD, T_BF16)
        else:
            x = out
    good.finish(f"faultless bf16 stand-in, config {name}")
    # the widened bound is at most twice the reference's own noise, measured here
    worst = good.by_class["conv2 channel /slice"]
    print(f"config {name}: worst channel of a block output, stand-in against fp64: {worst:.3e}")
    # (a quarter of slack: another fp32 summation order moves a few roundings of conv2 + b2, and with them the worst channel)
    assert worst <= 1.25 * R.CONV2_CHANNEL_NOISE and (name != "b" or worst >= 0.75 * R.CONV2_CHANNEL_NOISE), worst
