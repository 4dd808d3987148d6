"""float64 references of the Conv+BN-folded eval route (engine._fold_bn, _stem_fwd, _stages_fwd with fold_eval) in plain torch on the
CPU.  No GPU and nothing of the package: vqa_fold_bn_batch, the three vqa_igemm forms of a folded residual block and the one-launch
stem are judged against these (tests/test_gpu_inference.py, tests/test_gpu_inference_insitu.py); tests/test_fold_ref_cpu.py
shows on the CPU that the folded block below IS oracle.vqa_oracle.residual_block(training=False) and that Checker.check at T_BF16
flags each of the FAULTS.

The folded block as the engine launches it (activations NCHW here, [B*H*W][C] there):
    a1  = relu(conv3x3_s(x, w1') + b1)                                   vqa_igemm, bias, relu = 1
    res = x   or   conv1x1_s(x, wd') + bd                                vqa_igemm, bias (blocks with a downsample)
    out = relu(conv3x3(a1, w2') + b2 + res)                              vqa_igemm, bias, addend, relu = 2
with w' = w * gamma / sqrt(running_var + eps) and b = beta - running_mean * that scale.  A bf16 kernel stores a1, res and out in
bf16 and rounds conv2 + b2 to bf16 before the addend is added (gemm_conv.hip's epilogue): `rnd` stands in for those stores."""
import torch
import torch.nn.functional as F

from oracle import vqa_oracle as O

EPS = 1e-5
U32 = 2.0 ** -24                          # fp32 unit roundoff: half an ulp, relative to the value
STAGE_CHANNELS = (64, 128, 256, 512)
SMALL_VAR_CHANNEL = 5                     # see state_dict()
FAULTS = ("bias_dropped", "relu_before_addend", "shortcut_stride1_cropped", "image_zeroed", "no_eps")
# (name, batch, image height, width) of the live forwards; "c" is a size the one-launch stem refuses (pooled rows no multiple of 4)
# while the two-kernel stem takes it (conv output rows a multiple of 4, columns of 16)
CONFIGS = {"a": (4, 224, 224), "b": (3, 96, 96), "c": (2, 40, 64)}


SD_SEED, IMAGE_SEED = 3, 50               # shared by the CPU self-check and the GPU test: the stand-in's noise is measured on the same data


def images(name):
    """the fp32 NCHW images of configuration `name` (synthetic_batch draws squares: the larger side, cropped)"""
    B, IH, IW = CONFIGS[name]
    img, _, _, _ = O.synthetic_batch(B, seed=IMAGE_SEED, image_size=max(IH, IW))
    return img[:, :, :IH, :IW].contiguous()


def blocks():
    """(prefix, stage, block, Cin, Cout, stride) of the 8 residual blocks in forward order"""
    out, cin = [], 64
    for s, cout in enumerate(STAGE_CHANNELS, start=1):
        for b in range(2):
            out.append((f"image_encoder.stage{s}.blocks.{b}", s, b, cin, cout, 2 if (b == 0 and s > 1) else 1))
            cin = cout
    return out


def fold_pairs(sd):
    """(conv weight name, BatchNorm prefix) of the 20 folded pieces in engine._fold_bn's order"""
    pairs = []
    for p, *_ in blocks():
        pairs += [(p + ".conv1.weight", p + ".bn1"), (p + ".conv2.weight", p + ".bn2")]
        if (p + ".downsample.0.weight") in sd:
            pairs.append((p + ".downsample.0.weight", p + ".downsample.1"))
    return pairs


def state_dict(cfg, seed):
    """O.init_state_dict(cfg, seed, jitter=True) with one edge added: in every residual-block BatchNorm, channel SMALL_VAR_CHANNEL has
    running_var = 2 * eps, and its gamma is scaled by sqrt(3 * eps) so that the folded scale is the jittered gamma itself (about 1,
    like every other channel's).  The jitter alone leaves running_var in [0.9, 1.1], where eps changes the scale by 5e-6: with this
    channel a fold without eps is off by sqrt(3 / 2) in one channel of every conv."""
    sd = O.init_state_dict(cfg, seed, jitter=True)
    for _, bn in fold_pairs(sd):
        sd[bn + ".running_var"][SMALL_VAR_CHANNEL] = 2 * EPS
        sd[bn + ".weight"][SMALL_VAR_CHANNEL] *= (3 * EPS) ** 0.5
    return sd


# ------------------------------------------------------------------------------------------------ the fold and its counted bound
def fold(w, gamma, beta, rm, rv, eps=EPS):
    """fp64 from the fp32 inputs: (w * scale [N][...], beta - rm * scale, |rm * scale|)"""
    scale = gamma.double() / (rv.double() + eps).sqrt()
    prod = rm.double() * scale
    return w.double() * scale.view(-1, *([1] * (w.dim() - 1))), beta.double() - prod, prod.abs()


def fold_sd(sd, wname, bn, eps=EPS):
    return fold(sd[wname], sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"], sd[bn + ".running_var"], eps)


def bf16_half_ulp(v):
    """half the distance between neighbouring bf16 numbers (8 significant bits) at |v|: 2^(floor(log2 |v|) - 8); 0 at 0"""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.exp2(e.double() - 9))


def fold_weight_tol(wref, bf16):
    """fold_bn_batch_kernel performs 4 fp32 operations per weight (rv + eps, sqrtf, gamma / ., w * .): 4 * 2^-24 |ref| (3.5 to first
    order, the sqrt halves the first; the rest covers the second-order terms).  bf16: plus one bf16 RNE half-ulp for the store."""
    tol = 4 * U32 * wref.abs()
    return tol + bf16_half_ulp(wref.abs() + tol) if bf16 else tol


def fold_bias_tol(bref, prod):
    """5 fp32 operations: the three of the scale, rm * scale, beta - .  The first four are relative to the PRODUCT rm * scale, only
    the subtraction to the result: 4 * 2^-24 |rm * scale| + 2^-24 |ref| (five half-ulps of the result alone mis-count the case
    where beta and rm * scale cancel)."""
    return 4 * U32 * prod + U32 * bref.abs()


def error_in_bounds(got, ref, tol):
    """max |got - ref| / tol; where tol == 0 (a zero gamma) got must equal ref exactly"""
    err = (got.double() - ref).abs()
    zero = tol == 0
    assert bool((err[zero] == 0).all()), "an element with a zero bound differs"
    return float((err[~zero] / tol[~zero]).max()) if bool((~zero).any()) else 0.0


# ------------------------------------------------------------------------------------------------ stem and blocks
def stem(images, w, gamma, beta, rm, rv, between=None):
    """conv7x7/2 pad 3 -> eval BatchNorm -> ReLU -> MaxPool3x3/2 pad 1, fp64; images and w as the kernel reads them.  between: the
    rounding of the conv output where it is stored (the two-kernel stem: vqa_stem_pool_fwd consumed a bf16 tensor); the one-launch
    stem keeps it in registers."""
    scale = gamma.double() / (rv.double() + EPS).sqrt()
    shift = beta.double() - rm.double() * scale
    y = F.conv2d(images.double(), w.double(), None, stride=2, padding=3)
    y = y if between is None else between(y)
    return F.max_pool2d(torch.relu(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)), 3, 2, 1)


def _bias(b):
    return b.double().view(1, -1, 1, 1)


def conv1(x, w1, b1, stride):
    return torch.relu(F.conv2d(x.double(), w1.double(), None, stride=stride, padding=1) + _bias(b1))


def shortcut(x, wd, bd, stride):
    return F.conv2d(x.double(), wd.double(), None, stride=stride, padding=0) + _bias(bd)


def conv2(a1, w2, b2, res):
    return torch.relu(F.conv2d(a1.double(), w2.double(), None, stride=1, padding=1) + _bias(b2) + res.double())


def same(t):
    return t


def rnd_bf16(t):
    return t.to(torch.bfloat16).double()


def folded_operands(sd, p, eps=EPS):
    """{"conv1" | "conv2" | "downsample": (w' OIHW fp64, b fp64)} of block p from the state dict"""
    ops = {"conv1": fold_sd(sd, p + ".conv1.weight", p + ".bn1", eps)[:2], "conv2": fold_sd(sd, p + ".conv2.weight", p + ".bn2", eps)[:2]}
    if (p + ".downsample.0.weight") in sd:
        ops["downsample"] = fold_sd(sd, p + ".downsample.0.weight", p + ".downsample.1", eps)[:2]
    return ops


def folded_block(x, ops, stride, rnd=same, fault=None, acc=torch.float64):
    """(a1, res, out) of one folded block from its input x (NCHW) and folded operands `ops`.  rnd: the rounding of every store (`same`:
    the fp64 reference; rnd_bf16: a stand-in for the bf16 kernels, which also round conv2 + b2 before the addend); acc: the dtype
    the convolutions accumulate in (float32 for the stand-in).  ops are rounded by the caller when they stand in for bf16 operands.
    fault: one of FAULTS, a deliberately wrong kernel (no_eps is a fault of the operands: the caller passes
    folded_operands(..., eps=0))."""
    assert fault is None or fault in FAULTS
    (w1, b1), (w2, b2) = ops["conv1"], ops["conv2"]
    if fault == "bias_dropped":
        b2 = b2.clone()
        b2[int(b2.abs().argmax())] = 0.0

    def conv(t, w, b, s, pad):
        return (F.conv2d(t.to(acc), w.to(acc), None, stride=s, padding=pad) + b.to(acc).view(1, -1, 1, 1)).double()
    a1 = rnd(torch.relu(conv(x, w1, b1, stride, 1)))
    if "downsample" in ops:
        wd, bd = ops["downsample"]
        if fault == "shortcut_stride1_cropped":
            res = rnd(conv(x, wd, bd, 1, 0)[:, :, : a1.shape[2], : a1.shape[3]])
        else:
            res = rnd(conv(x, wd, bd, stride, 0))
    else:
        res = x.double()
    y2 = rnd(conv(a1, w2, b2, 1, 1))
    out = rnd(torch.relu(y2) + res) if fault == "relu_before_addend" else rnd(torch.relu(y2 + res))
    if fault == "image_zeroed":
        out = out.clone()
        out[out.shape[0] - 1] = 0.0
    return a1, res, out


def stage_attention(x, sd, s, between=same, last=same):
    """SE then spatial attention of stage s on the NCHW output of its last block, fp64, by the oracle's own functions.
    between: the rounding of the tensor vqa_se_fwd stores and vqa_spatial_fwd reads (stages 3 and 4 have both modules); last: of the
    stage's final store.  (same, same) is the oracle's stage tail; (rnd_bf16, same) the restatement of a bf16 forward, whose spatial
    kernel consumed a bf16 tensor; (rnd_bf16, rnd_bf16) the stand-in for the kernels."""
    ap = f"image_encoder.stage{s}.attention"
    x = x.double()
    has_spatial = (ap + ".spatial.conv.weight") in sd
    if (ap + ".se.fc1.weight") in sd:
        x = O.se_attention(x, sd[ap + ".se.fc1.weight"].double(), sd[ap + ".se.fc2.weight"].double())
        x = between(x) if has_spatial else x
    if has_spatial:
        x = O.spatial_attention(x, sd[ap + ".spatial.conv.weight"].double())
    return last(x)


def nchw(t, B, H, W):
    """engine layout [B*H*W][C] -> NCHW fp64 on the CPU"""
    return t.detach().cpu().double().view(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def oihw(w2d, cin, r):
    """a folded [N][R*S*Cin] operand (KRSC) -> OIHW fp64 on the CPU"""
    return w2d.detach().cpu().double().view(w2d.shape[0], r, r, cin).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ the checks of one block
def check_operands(ck, tag, got_w, got_b, ref_w, ref_b, tol):
    """folded operands against the fp64 fold through Checker.check, per output channel (the exact, counted bound of the GPU tests is
    error_in_bounds; this is the same comparison at the in-situ bound, for the fault self-check)"""
    ck.check(tag + " w'", got_w.reshape(got_w.shape[0], -1), ref_w.reshape(ref_w.shape[0], -1), tol, dims=(0,), cls="fold")
    ck.check(tag + " b", got_b.reshape(-1, 1), ref_b.reshape(-1, 1), tol, dims=(), cls="fold")


# Per-CHANNEL slices of a block output need more than T_BF16: the kernel rounds conv2 + b2 to bf16 BEFORE it adds the residual (the
# order tests/test_gpu_exact_integer.py pins), so a channel in which conv2 + b2 and the residual cancel carries half a bf16 ulp of
# the larger operand.  Measured as the reference's own noise, never from a kernel: the fp64 restatement against the fp32-accumulated
# CPU restatement of the same step with its bf16 stores (tests/test_fold_ref_cpu.py, same weights and images as the GPU test): worst
# channel 1.22e-2 at B = 4, 224 x 224, 1.54e-2 at B = 3, 96 x 96 (27 values per channel at stage 4) and 1.31e-2 at B = 2, 40 x 64.
# The bound is twice the largest.  The whole tensor and the per-image slices stay at T_BF16 (stand-in: 2.2e-3 / 3.5e-3).
CONV2_CHANNEL_NOISE = 1.54e-2
T_CONV2_CHANNEL = 2 * CONV2_CHANNEL_NOISE


def check_block(ck, p, x, a1, out, ops, stride, tol):
    """One folded block of a live forward restated from the tensors it consumed: a1 from the block input x, the output from the
    KERNEL's a1 and from the shortcut stored in bf16 (or the block input).  x, a1, out: NCHW; ops: the operands the kernels read.
    tol (T_BF16) holds for both tensors as a whole and for every slice but the output's channels: T_CONV2_CHANNEL."""
    ck.check(p + " conv1", a1, conv1(x, *ops["conv1"], stride), tol)
    res = rnd_bf16(shortcut(x, *ops["downsample"], stride)) if "downsample" in ops else x.double()
    ref = conv2(a1, *ops["conv2"], res)
    ck.check(p + " conv2+shortcut", out, ref, tol, dims=(0,))
    ck.check(p + " conv2+shortcut channels", out, ref, tol, dims=(1,), cls="conv2 channel", slice_tol=T_CONV2_CHANNEL)


def check_attention(ck, s, x_out, nxt, sd, tol):
    """Stage s's SE + spatial attention: `nxt` (the next stage's block input, or the features) from the last block's output x_out.
    Where the stage has both modules the spatial kernel read the SE kernel's bf16 output: the restatement rounds there too."""
    ck.check(f"stage{s} attention", nxt, stage_attention(x_out, sd, s, between=rnd_bf16), tol, cls="attention")
