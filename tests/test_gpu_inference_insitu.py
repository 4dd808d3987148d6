"""GPU: a live bf16 Conv+BN-folded eval forward -- the route behind predict(), encode_images() + answer(), predict_topk,
encode_features() and the frozen-CNN fine-tuning step -- checked block by block against fp64.

One eng.forward(..., training=False, want_aux=True, need_tape=False, record=rec) under torch.no_grad() per configuration, with
kernels.PROFILE recording and every C-ABI launch name kept through _lib._HOOK.  Then every step of the image half is restated in fp64
on the CPU (tests/_foldref.py) FROM THE EXACT bf16 TENSOR THE STEP CONSUMED ON THE GPU, so no error is carried from one check into
the next:
  fold       eng._fold_bn()'s 19 operands and biases (8 x 2 convs, the shortcuts of stages 2 to 4) against the fp64 fold of the fp32
             masters, element by element within the counted bound of test_gpu_inference.py (4 fp32 operations + the bf16 store)
  stem       block 0's recorded input against conv7x7/2 (bf16 images, bf16 stem weights) -> eval BatchNorm -> ReLU -> MaxPool
  conv1      rec[p + ".a1"] against relu(conv(x, w1') + b1): x the recorded block input, w1' / b1 the GPU-folded operands
  conv2      the block output against relu(conv(a1 of the KERNEL, w2') + b2 + res), res = the block input or
             bf16(conv1x1_s(x, wd') + bd)
  wiring     block 1's input IS block 0's output; the shapes follow the stride
  attention  the next stage's block input (stage 4: aux["image_features"]) against SE -> spatial attention of the stage's last block
             output; image_features (fp32 NCHW) is bit for bit the bf16 NHWC features of encode_features(), transposed
  logits     finite, and bit for bit those of the same call without record and want_aux
Configurations (_foldref.CONFIGS; weights: init_state_dict(jitter=True) plus a channel with running_var = 2 eps per BatchNorm):
  a  B = 4, 224 x 224: M = 196 at stage 4, one full 128-row tile and a tail, on 7 x 7 maps
  b  B = 3, 96 x 96: maps of 24, 12, 6 and 3; padding touches most outputs, M = 27 at stage 4
  c  B = 2, 40 x 64: vqa_stem_conv_pool_ok refuses it (10 pooled rows are no multiple of 4) while vqa_stem_conv takes it: the
     two-kernel eval stem (vqa_stem_conv + vqa_stem_pool_fwd on running statistics), and non-square maps down to 2 x 2
Launches asserted: vqa_fold_bn_batch once; vqa_stem_conv_pool in a and b (vqa_stem_conv + vqa_stem_pool_fwd in c); no vqa_bn_apply*,
vqa_bn_stats_finalize, vqa_conv8p or vqa_conv3x3_c64p*.

Bounds: _insitu.Checker.check with T_BF16 = 4e-3 on the whole tensor and on every per-image and per-channel slice, except the
per-channel slices of a block output: _foldref.T_CONV2_CHANNEL = 3.08e-2, twice the noise of the reference itself (the fp64
restatement against an fp32-accumulated CPU restatement with bf16 stores: 1.54e-2, tests/test_fold_ref_cpu.py), because the kernel
rounds conv2 + b2 to bf16 before it adds the residual.  tests/test_fold_ref_cpu.py shows that these bounds flag a dropped bias, a
misplaced ReLU, a shortcut at the wrong stride, a zeroed image and a fold without eps.
Where a kernel consumed a bf16 tensor that no record holds (vqa_spatial_fwd the SE output; vqa_stem_pool_fwd the conv output in c),
the restatement rounds its fp64 value there.

Measured on an MI355X, worst relative error per class (whole tensor | worst per-image or per-channel slice), configs a / b / c:
  fold (operands, at T_BF16)             1.67e-3 | 2.14e-3 in all three; against the counted bound: weights 1.000 (the bf16 half-ulp
                                         itself), bias 0.856 of it
  stem                                   1.65e-3 | 1.70e-3    1.65e-3 | 1.84e-3    1.68e-3 | 2.07e-3
  conv1, conv2 + shortcut per image      2.23e-3 | 2.59e-3    2.17e-3 | 2.78e-3    2.19e-3 | 3.19e-3      (bound 4e-3)
  conv2 + shortcut per channel           1.23e-2              1.24e-2              2.15e-2                (bound 3.08e-2; c: stage 4
                                         block 0, 8 values per channel)
  attention                              1.70e-3 | 2.42e-3    1.69e-3 | 2.61e-3    1.70e-3 | 3.01e-3
The three cases take 3.9 s together (the fp64 restatement of config a is the longest part)."""
import pytest
import torch

import _foldref as R
from _insitu import Checker, T_BF16
from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORBIDDEN = ("vqa_bn_apply", "vqa_bn_stats_finalize", "vqa_conv8p", "vqa_conv3x3_c64p")


def _live_forward(name):
    P = pkg()
    L, K = P._lib, P.kernels
    cfg = O.full_config()
    sd = R.state_dict(cfg, R.SD_SEED)
    m = P.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    eng = m._ensure_engine()
    assert eng.fold_eval and eng.fuse_stem_eval and eng.infer_precision == "bf16"
    B = R.CONFIGS[name][0]
    images = R.images(name).to(DEV)
    _, ids, mask, _ = O.synthetic_batch(B, seed=R.IMAGE_SEED + 1)
    ids, maskf = ids.to(DEV), mask.float().to(DEV)
    rec, names = {}, []
    saved = (K.PROFILE, K.PROFILE_VARIANTS, K.PROFILE_STAGED)
    K.PROFILE, K.PROFILE_VARIANTS, K.PROFILE_STAGED = [], [], {}
    prev = L._HOOK[0]

    def hook(entry, args):
        names.append((entry, args))
        return prev(entry, args) if prev is not None else None
    L._HOOK[0] = hook
    try:
        with torch.no_grad():
            logits, aux, tape = eng.forward(images, ids, maskf, False, want_aux=True, need_tape=False, record=rec)
        torch.cuda.synchronize()
        syms = [e[0] for e in K.PROFILE]
    finally:
        L._HOOK[0] = prev
        K.PROFILE, K.PROFILE_VARIANTS, K.PROFILE_STAGED = saved
    assert tape is None
    with torch.no_grad():
        plain, _, _ = eng.forward(images, ids, maskf, False, need_tape=False)
        feat = eng.encode_features(images)
        folded = eng._fold_bn()
    torch.cuda.synchronize()
    return dict(eng=eng, sd=sd, images=images, rec=rec, names=names, syms=syms, logits=logits, aux=aux, plain=plain, feat=feat, folded=folded)


def _check_launches(name, run):
    entries = [n for n, _ in run["names"]]
    assert entries.count("vqa_fold_bn_batch") == 1
    assert not [n for n in entries if n.startswith(FORBIDDEN)], [n for n in entries if n.startswith(FORBIDDEN)]
    B, IH, IW = R.CONFIGS[name]
    L = sub("_lib")
    if name == "c":
        assert not L.count("vqa_stem_conv_pool_ok", B, IH, IW) and L.count("vqa_stem_conv_blocks", B, IH, IW) > 0
        assert entries.count("vqa_stem_conv") == 1 and entries.count("vqa_stem_pool_fwd") == 1 and "vqa_stem_conv_pool" not in entries
        assert "stem_conv_kernel" in run["syms"]
    else:
        assert entries.count("vqa_stem_conv_pool") == 1 and "vqa_stem_conv" not in entries and "vqa_stem_pool_fwd" not in entries
        assert "stem_conv_pool_kernel" in run["syms"]
    assert entries.count("vqa_se_fwd") == 4 and entries.count("vqa_spatial_fwd") == 2 and entries.count("vqa_nhwc_to_nchw") == 1


def _check_fold(ck, run):
    """The 19 operands of the live fold: element by element within the counted bound, and through the checker at T_BF16."""
    sd, folded = run["sd"], run["folded"]
    pairs = R.fold_pairs(sd)
    assert len(pairs) == 19 and set(folded) == {w for w, _ in pairs}
    worst_w = worst_b = 0.0
    for wname, bn in pairs:
        wref, bref, prod = R.fold_sd(sd, wname, bn)
        wref = wref.permute(0, 2, 3, 1).reshape(wref.shape[0], -1)               # the masters and the operands are [N][R][S][Cin]
        w, b = folded[wname][0].cpu(), folded[wname][1].cpu()
        assert w.dtype == torch.bfloat16 and b.dtype == torch.float32 and w.shape == wref.shape
        worst_w = max(worst_w, R.error_in_bounds(w, wref, R.fold_weight_tol(wref, True)))
        worst_b = max(worst_b, R.error_in_bounds(b, bref, R.fold_bias_tol(bref, prod)))
        R.check_operands(ck, wname[len("image_encoder."):], w, b, wref, bref, T_BF16)
    print(f"live fold: worst error / counted bound: weights {worst_w:.3f}, bias {worst_b:.3f}")
    assert worst_w <= 1.0 and worst_b <= 1.0, (worst_w, worst_b)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_live_bf16_folded_eval_forward_block_by_block(name):
    torch.set_num_threads(16)
    run = _live_forward(name)
    sd, rec, folded, eng = run["sd"], run["rec"], run["folded"], run["eng"]
    B, IH, IW = R.CONFIGS[name]
    _check_launches(name, run)
    assert torch.isfinite(run["logits"]).all() and torch.equal(run["logits"], run["plain"])
    assert len(rec) == 16 and set(rec) == {p for p, *_ in R.blocks()} | {p + ".a1" for p, *_ in R.blocks()}
    ck = Checker()
    _check_fold(ck, run)

    # stem: the kernels read the fp32 image and round it to bf16 as they load it; the stem weights are packed in bf16
    H, W = ((IH - 1) // 2 + 1 - 1) // 2 + 1, ((IW - 1) // 2 + 1 - 1) // 2 + 1
    st = "image_encoder.stem."
    x0 = rec["image_encoder.stage1.blocks.0"][0]
    assert x0.dtype == torch.bfloat16 and x0.shape == (B * H * W, 64)
    ref = R.stem(R.rnd_bf16(run["images"].cpu()), R.rnd_bf16(sd[st + "0.weight"]), sd[st + "1.weight"], sd[st + "1.bias"],
                 sd[st + "1.running_mean"], sd[st + "1.running_var"], between=R.rnd_bf16 if name == "c" else None)
    ck.check("stem", R.nchw(x0, B, H, W), ref, T_BF16, cls="stem")

    prev_out = None
    for p, s, b, cin, cout, stride in R.blocks():
        xin, out = rec[p]
        a1 = rec[p + ".a1"]
        Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
        assert xin.shape == (B * H * W, cin) and a1.shape == (B * Ho * Wo, cout) and out.shape == (B * Ho * Wo, cout), p
        assert all(t.dtype == torch.bfloat16 and t.is_contiguous() for t in (xin, a1, out)), p
        if b == 1:
            assert xin is prev_out, p                                  # wiring: block 1 reads block 0's output itself
        ops = {"conv1": (R.oihw(folded[p + ".conv1.weight"][0], cin, 3), folded[p + ".conv1.weight"][1].cpu().double()),
               "conv2": (R.oihw(folded[p + ".conv2.weight"][0], cout, 3), folded[p + ".conv2.weight"][1].cpu().double())}
        if (p + ".downsample.0.weight") in eng.E:
            ops["downsample"] = (R.oihw(folded[p + ".downsample.0.weight"][0], cin, 1), folded[p + ".downsample.0.weight"][1].cpu().double())
        assert ("downsample" in ops) == (b == 0 and s > 1)
        x64, out64 = R.nchw(xin, B, H, W), R.nchw(out, B, Ho, Wo)
        R.check_block(ck, p[len("image_encoder."):], x64, R.nchw(a1, B, Ho, Wo), out64, ops, stride, T_BF16)
        H, W, prev_out = Ho, Wo, out
        if b == 1:                                                     # the stage's attention, into the next stage or the features
            if s < 4:
                nxt = R.nchw(rec[f"image_encoder.stage{s + 1}.blocks.0"][0], B, H, W)
            else:
                feats = run["aux"]["image_features"]
                assert feats.dtype == torch.float32 and feats.shape == (B, 512, H, W) and run["feat"].shape == (B, H, W, 512)
                assert torch.equal(feats, run["feat"].float().permute(0, 3, 1, 2)), "vqa_nhwc_to_nchw: not the bf16 features transposed"
                nxt = feats.cpu().double()
            R.check_attention(ck, s, out64, nxt, sd, T_BF16)
    ck.finish(f"live bf16 folded eval forward, config {name}")
