"""GPU: every layer of a LIVE bf16 train step, forward and backward, checked locally against fp32 / fp64 math -- at B = 64 (dropout
off), at the benchmarked B = 512, 224x224 with dropout on (bench.py default), at the stress shape B = 256, 384x384, d = 512, 8 text
layers (bench.py --config stress), and grouped (forward with kv_index, many questions per image) at N = 512 questions, 224x224,
dropout on: "g5" over U = 103 images (question i on image i // 5, tools/bench_grouped_train.py's q = 5) and "gmix" over U = 160
images with 0 .. 12 questions each in shuffled order (images 0 and U - 1 have none).

Why this test exists.  The end-to-end bf16 gradient check (tests/_bf16check.py) can only hold a CNN weight tensor to the noise floor
of bf16 itself on this model -- relative error 0.4-0.55 per tensor against the fp32 oracle, the same for PyTorch's own CPU bf16
autocast, and measured to be INDEPENDENT of the batch size (B = 8 and B = 64 give the same figures, tools/diag_bf16_relerr.py: at
random init the batch gradient of a CNN weight is the small residual of per-sample gradients that cancel, and rounding noise
scales with the per-sample magnitude).  So a wiring error of a few ten percent in the bf16 engine path would hide there, and the
full-size tests (test_gpu_fullsize.py) check only invariants of a training step.  Several code paths run only at the benchmarked
sizes (conv8p 196-row tiles at 2 or 1 rounds, the persistent weight-gradient kernels above 256 workgroups, fixed-point BatchNorm
sums over 1.6 M / 2.36 M rows, the SE / stem fusions at full size, the hoisted cross-attention K / V with dropout).

Here the comparison is LOCAL: the tape holds every forward activation and the engine hands out the gradients entering and leaving
each backward section (HipEngine.capture), so each layer's result is compared with plain torch math (never this package's kernels)
applied to the EXACT bf16 tensors that layer consumed in the live step, with the dropout masks regenerated from the recorded seeds
(tests/_dropmask.py).  Every comparison is a global relative norm AND the same bound per image and per output channel
(tests/_insitu.py).  Per-image forward checks and data gradients of convolutions use the first and last 16 images (the last land
in the tail tiles); weight gradients, BatchNorm statistics and their sums always use the full batch.

Bounds (class: bound, global and per slice; measured worst over the five configurations):
  bf16        4e-3   bf16-stored outputs of one op, forward and data gradients: the rounding of the stored value (2.4e-3 / 3.4e-3)
  wgrad       2e-4   fp32 weight and bias gradients from the captured operands, 2.8e-5 / 6.3e-5 (the conv references sum chunks of
                     8 images in fp64: a single fp32 reduction over 1.6 M rows adds ~1e-3 of its own in channels whose sum cancels)
  bnparam     1e-3   BatchNorm and LayerNorm parameter gradients (7e-7 / 1.9e-5)
  fp32        1e-4   fp32-stored forward values (SE, spatial attention, BatchNorm coefficients, running buffers: 6.7e-5);
                     a batch mean and a BatchNorm shift are measured in standard deviations of their channel (a mean near 0 has no
                     relative scale of its own): T_SIGMA 5e-4, measured 2.5e-4 (statistics summed from the fp32 conv output, the
                     reference from the stored bf16 y)
  probs       1e-6   attention probabilities, fp32 from bf16 Q / K (1.5e-7)
  attn        T_ATTN dQ / dK / dV of the attention backward (below)
Token side: every op of every attention / FFN block, the projector, the fusion tail and the answer head is checked on its own,
forward and backward, from the stored inputs of that op and the gradient the engine captured in front of it (HipEngine.capture_io);
no check runs through more than one stored rounding.
Residual-block backward semantics (models/cnn_backbone.py:164-197, nn.BatchNorm2d training mode):
    g    = dout * (out > 0)                                   (or dout itself when the producer already applied the mask)
    dy2  = BatchNorm-backward(g; y2, batch statistics)       d gamma2 / d beta2 in the flat gradient buffer
    dyd  = same for the 1x1 shortcut's BatchNorm             (first block of stages 2-4)
    dW2  = conv-weight-gradient(a1, dy2)     da1 = conv-input-gradient(dy2, W2)
    dy1  = BatchNorm-backward(da1 * (bn1(y1) > 0); y1)       dW1 = conv-weight-gradient(x, dy1)     dWd = (x, dyd)
    dx   = conv-input-gradient(dy1, W1) + [g | conv-input-gradient(dyd, Wd)]   (* (x > 0) when handed to the previous block masked)
CPU time of the references (16 threads, measured): 11 s at B = 64, 41 s at B = 512, 71 s at the stress shape; the live step itself
takes about a second.  The tape is copied block by block and freed as it goes.
Grouped steps: the CNN, SE, spatial attention, stem and projector run (and are checked) at U image rows, the text encoder, pools, gate
and head at N question rows.  The cross-attention references gather K / V by the image index, redraw the dropout mask per question,
and sum the per-question dK / dV into image rows in fp64 (tests/_insitu.py attn_core_bwd); the K / V weight gradients, norm_kv and the
image-token gradient chain then run over U * 49 rows.  Also checked: the CSR of the index against a stable argsort, exact zeros in
every image-token gradient row of an image without questions, the grouped kernels in kernels.PROFILE, and the weight-gradient plans
of the stage-2 entry conv and the stage-3 / 4 convs (U = 103: all on the 4-wave split kernel, which B = 512 never uses; U = 160: the
non-entry stage-3 / 4 convs on the 8-wave DMA kernel).
"""
import math
import time

import pytest
import torch
import torch.nn.functional as F

from _dropmask import keep_mask
from _insitu import (T_ATTN, T_ATTN_SLICE, T_BF16, T_BNPARAM, T_FP32, T_PROBS, T_SIGMA, T_WGRAD, Checker, attn_core_bwd, attn_core_fwd,
                     bn_bwd, channel_moments, check_csr, check_zero_rows, empty_images, nchw, rnd)
from _pkg import pkg
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
NSUB = 16                                  # per-image checks: the first and the last NSUB images

CONFIGS = {
    "b64": dict(B=64, image=224, model={}, dropout=False),
    "b512": dict(B=512, image=224, model={}, dropout=True),
    "stress": dict(B=256, image=384, model=dict(embed_dim=512, num_transformer_layers=8, num_answers=2000, num_image_tokens=144),
                   dropout=True),
    # grouped (forward with kv_index): B questions over U images
    "g5": dict(B=512, U=103, image=224, model={}, dropout=True),       # tools/bench_grouped_train.py's q = 5: question i on image i // 5
    "gmix": dict(B=512, U=160, image=224, model={}, dropout=True),     # 0 .. 12 questions per image, shuffled (_gmix_index)
}
# kernels that must have run in the B = 512 step (the top of profiles/r04_bench_b512_serial_kernel_stats.csv), as kernels.PROFILE
# spells them
B512_SYMBOLS = ("conv8p_kernel<2, 4>", "conv8p_kernel<4, 2>", "wgrad_dma_kernel<256, 256, 2>", "wgrad3x3_c128p_kernel",
                "conv3x3_c64p_kernel<8, 0>", "conv3x3_c64p_kernel<8, 1>", "conv3x3_c64p_kernel<8, 2>", "stem_conv_kernel",
                "stem_wgrad_kernel<true>")

# the grouped step's own launches (as kernels.PROFILE spells them): the CSR of the image index, the indexed attention with dropout
# and its backward that sums dK / dV per image
GROUPED_SYMBOLS = ("hbm:token:index_csr", "hbm:attention:attention_fwd_mfma_idx_train", "hbm:attention:attention_bwd_mfma_idx")


def _keep(seed, shape, p):
    n = 1
    for s in shape:
        n *= s
    return torch.from_numpy(keep_mask(seed, n, p)).view(*shape).double() / (1.0 - p)


def _gmix_index(N=512, U=160, seed=11):
    """N questions over U images, shuffled: images 0 and U - 1 (the tail tiles) and a few others get none, image 1 gets 9 and
    image U // 2 gets 12, the rest 1 .. 6."""
    g = torch.Generator().manual_seed(seed)
    cnt = torch.randint(1, 7, (U,), generator=g)
    fixed = {0: 0, U - 1: 0, 37: 0, 101: 0, 1: 9, U // 2: 12}
    free = [u for u in range(U) if u not in fixed]
    for u, v in fixed.items():
        cnt[u] = v
    k = 0
    while int(cnt.sum()) != N:                 # bring the total to N within 1 .. 6 per free image
        u = free[k % len(free)]
        k += 1
        if int(cnt.sum()) < N and cnt[u] < 6:
            cnt[u] += 1
        elif int(cnt.sum()) > N and cnt[u] > 1:
            cnt[u] -= 1
    idx = torch.repeat_interleave(torch.arange(U), cnt)
    return idx[torch.randperm(N, generator=g)]


def _image_index(name):
    """The image index of a grouped configuration (long [B] on the CPU), or None."""
    c = CONFIGS[name]
    if "U" not in c:
        return None
    idx = torch.arange(c["B"]) // 5 if name == "g5" else _gmix_index(c["B"], c["U"])
    assert int(idx.min()) >= 0 and int(idx.max()) < c["U"]
    return idx


def _live_step(name):
    """One training step through the engine exactly as bench.py configures the model (bf16, two streams), with the tape and the
    capture kept and kernels.PROFILE recording the launches.  Grouped configurations run eng.forward(..., kv_index=) on the first
    U images of the batch (as HipTrainer.step(..., image_index=) does).  run["B"]: image rows (U), run["Bq"]: question rows."""
    P = pkg()
    c = CONFIGS[name]
    kw = dict(c["model"])
    if not c["dropout"]:
        kw.update(dropout=0.0, answer_dropout=0.0)
    cfg = O.full_config(**kw)
    sd = O.init_state_dict(cfg, 7, jitter=True)
    m = P.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    eng = m._ensure_engine()
    B = c["B"]
    images, ids, mask, answers = (t.to(DEV) for t in O.synthetic_batch(B, seed=77, image_size=c["image"], num_answers=cfg["num_answers"]))
    maskf = mask.float()
    index = _image_index(name)
    U = B if index is None else c["U"]
    images = images[:U].contiguous()
    kv_index = None if index is None else index.to(device=DEV, dtype=torch.int32)
    K = P.kernels
    saved = (K.PROFILE, K.PROFILE_VARIANTS, K.PROFILE_STAGED)
    K.PROFILE, K.PROFILE_VARIANTS, K.PROFILE_STAGED = [], [], {}
    try:
        eng.capture, eng.capture_io = {}, {}
        logits, _, tape = eng.forward(images, ids, maskf, True, False, need_tape=True, kv_index=kv_index)
        dl = torch.empty_like(logits)
        loss = torch.zeros(1, device=DEV)
        P._lib.call("vqa_cross_entropy", 0, logits.data_ptr(), answers.data_ptr(), loss.data_ptr(), dl.data_ptr(), None, B, logits.shape[1],
                    1.0, None, None)
        G = torch.zeros_like(m._flat)
        eng.backward(tape, dl, G)
        torch.cuda.synchronize()
        syms = [e[0] for e in K.PROFILE]
    finally:
        cap = {**eng.capture, **eng.capture_io}      # (residual-block prefixes and section prefixes do not collide)
        eng.capture = eng.capture_io = None
        K.PROFILE, K.PROFILE_VARIANTS, K.PROFILE_STAGED = saved
    assert tape["B"] == U and tape["Bq"] == B
    return dict(m=m, eng=eng, cfg=cfg, sd=sd, B=U, Bq=B, index=index, images=images, ids=ids, maskf=maskf, logits=logits, tape=tape,
                cap=cap, G=G, syms=syms)


class _Params:
    """Views of the flat parameter / gradient buffers as the kernels see them."""

    def __init__(self, run):
        self.flat, self.G, self.E = run["m"]._flat.detach(), run["G"], run["eng"].E

    def _krsc(self, buf, name):                 # OIHW view of a [Cout][R][S][Cin] conv weight
        e = self.E[name]
        co, ci, r, s_ = e.shape
        return buf[e.offset: e.offset + e.numel].view(co, r, s_, ci).permute(0, 3, 1, 2).contiguous().cpu()

    def conv_w(self, name):                     # bf16-rounded working copy
        return rnd(self._krsc(self.flat, name))

    def conv_g(self, name):
        return self._krsc(self.G, name)

    def vec(self, name, grad=False):
        e = self.E[name]
        return (self.G if grad else self.flat)[e.offset: e.offset + e.numel].view(e.shape).cpu()

    def lin_w(self, name):                      # bf16 GEMM operand, fp64
        return rnd(self.vec(name)).double()


def _sel(B):
    """Images of the per-image checks: the whole batch up to B = 64, else the first and the last NSUB."""
    return list(range(NSUB)) + list(range(B - NSUB, B)) if B > 64 else list(range(B))


def _wgrad_ref(x, wshape, dy, stride, padding):
    """conv weight gradient over the full batch: fp32 per chunk of 8 images, the chunks summed in fp64 (a single fp32 reduction over
    1.6 M rows carries its own rounding into channels whose sum cancels)."""
    dw = torch.zeros(wshape, dtype=torch.float64)
    for i in range(0, x.shape[0], 8):
        dw += torch.nn.grad.conv2d_weight(x[i: i + 8], wshape, dy[i: i + 8], stride=stride, padding=padding).double()
    return dw


# ------------------------------------------------------------------ CNN
def _check_bn_coef(ck, tag, y_nchw_full, coef, gamma, beta, run, prefix, n):
    """coef rows (scale, shift, batch mean, 1/sqrt(var+eps)) against fp64 statistics of the stored conv output; running buffers
    against the momentum update with the unbiased variance."""
    mean, var = channel_moments(y_nchw_full)
    inv = 1.0 / torch.sqrt(var + O.BN_EPS)
    coef = coef.double().cpu()
    # a batch mean near 0 has no relative scale of its own: its error and the shift's are measured in standard deviations of the
    # channel's input / output (a mean off by 1e-4 sigma moves every normalised value by 1e-4)
    ck.check_abs(tag + " mean", (coef[2] - mean) * inv, T_SIGMA, cls="fp32")
    ck.check(tag + " invstd", coef[3], inv, T_FP32, dims=(0,), cls="fp32")
    ck.check(tag + " scale", coef[0], gamma.double() * inv, T_FP32, dims=(0,), cls="fp32")
    ck.check_abs(tag + " shift", (coef[1] - (beta.double() - mean * gamma.double() * inv)) / gamma.double().abs(), T_SIGMA, cls="fp32")
    eng, rm0, rv0 = run["eng"], run["sd"][prefix + ".running_mean"], run["sd"][prefix + ".running_var"]      # (the step updates in place)
    m_ = O.BN_MOMENTUM
    ck.check(tag + " running_mean", eng.buf[prefix + ".running_mean"].cpu(), (1 - m_) * rm0.double() + m_ * mean, T_FP32, dims=(0,), cls="fp32")
    ck.check(tag + " running_var", eng.buf[prefix + ".running_var"].cpu(), (1 - m_) * rv0.double() + m_ * var * n / (n - 1), T_FP32, dims=(0,),
             cls="fp32")


def _check_stem(ck, run, W):
    eng, tape, cap, B = run["eng"], run["tape"], run["cap"], run["B"]
    st = tape["stem"]
    _, IH, IW, _, H1, W1 = st["geom"][:6]
    Hp, Wp = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
    sel = _sel(B)
    ws = W.conv_w("image_encoder.stem.0.weight")
    coef = st["coef"].cpu()
    sc, sh = coef[0].view(1, -1, 1, 1), coef[1].view(1, -1, 1, 1)
    # ---- forward: conv on the subset, statistics on the full batch
    img_s = rnd(st["images"][sel].cpu())
    y_s = nchw(st["y"], B, H1, W1, sel)
    ck.check("stem y", y_s, F.conv2d(img_s, ws, stride=2, padding=3), T_BF16)
    y_full = nchw(st["y"], B, H1, W1)
    _check_bn_coef(ck, "stem bn", y_full, coef, W.vec("image_encoder.stem.1.weight"), W.vec("image_encoder.stem.1.bias"), run,
                   "image_encoder.stem.1", B * H1 * W1)
    del y_full
    a_s = torch.relu(y_s * sc + sh)
    pooled_ref = F.max_pool2d(a_s, 3, 2, 1)
    x_s = nchw(tape["stages"][0]["blocks"][0]["x"], B, Hp, Wp, sel)
    ck.check("stem pool", x_s, pooled_ref, T_BF16)
    # idx: the window position (r*3 + s) of a maximum (bf16 ties make the index itself ambiguous: its VALUE is checked)
    idx_s = nchw(st["idx"], B, Hp, Wp, sel).long()
    flat_i = _routed_index(idx_s, Hp, Wp, W1)
    at_idx = a_s.flatten(2).gather(2, flat_i.flatten(2)).view_as(pooled_ref)
    ih = 2 * torch.arange(Hp).view(1, 1, -1, 1) - 1 + idx_s // 3          # the indexed position must lie inside the plane (a padded
    iw = 2 * torch.arange(Wp).view(1, 1, 1, -1) - 1 + idx_s % 3           # window slot is never a maximum)
    inside = (ih >= 0) & (ih < H1) & (iw >= 0) & (iw < W1)
    ok = bool(((idx_s < 9) & inside & (at_idx >= pooled_ref - 1e-6 * pooled_ref.abs())).all())
    ck.expect("stem idx", ok, "argmax byte does not point at a window maximum")
    # ---- backward: captured pooled gradient routed through the tape's idx, ReLU, BatchNorm backward (batch statistics), 7x7 wgrad
    dxc = cap["image_encoder.stem"]["dxc"]
    mean, inv = coef[2].view(1, -1, 1, 1), coef[3].view(1, -1, 1, 1)
    n = B * H1 * W1
    chunks = [list(range(i, min(i + 32, B))) for i in range(0, B, 32)]

    def g_of(ch):
        y = nchw(st["y"], B, H1, W1, ch)
        idx = nchw(st["idx"], B, Hp, Wp, ch).long()
        dp = nchw(dxc, B, Hp, Wp, ch)
        dmax = torch.zeros(len(ch), 64, H1 * W1)
        dmax.scatter_add_(2, _routed_index(idx, Hp, Wp, W1).flatten(2), dp.flatten(2))
        g = dmax.view(len(ch), 64, H1, W1) * ((y * sc + sh) > 0)
        return g, (y - mean) * inv

    dbeta_y = torch.zeros(64, dtype=torch.float64)
    dgamma_y = torch.zeros(64, dtype=torch.float64)
    for ch in chunks:
        g, xh = g_of(ch)
        dbeta_y += g.double().sum((0, 2, 3))
        dgamma_y += (g * xh).double().sum((0, 2, 3))
    # The engine reduces the stem's BatchNorm-backward sums over the stored bf16 POOLED output, never touching the 112 x 112 tensors
    # (engine.py _stem_bwd): every window routes its gradient to its argmax, whose post-ReLU value is the pooled output, so
    # sum g = sum dpool * [pooled > 0] and sum g * xhat = sum dpool * [pooled > 0] * (pooled - beta) / gamma.  That is the local
    # reference.  The same sums over the routed y (above): d beta is identical and asserted; d gamma differs by the bf16 rounding of
    # `pooled`, which the heavily cancelling sum of g * xhat amplifies -- measured 3.9e-3 globally and up to 7.4e-2 in one channel
    # (B = 512), reported below.
    pooled = nchw(tape["stages"][0]["blocks"][0]["x"], B, Hp, Wp).double()
    dpool = nchw(dxc, B, Hp, Wp).double() * (pooled > 0)
    gam64 = W.vec("image_encoder.stem.1.weight").double().view(1, -1, 1, 1)
    bet64 = W.vec("image_encoder.stem.1.bias").double().view(1, -1, 1, 1)
    dbeta = dpool.sum((0, 2, 3))
    dgamma = (dpool * (pooled - bet64) / gam64).sum((0, 2, 3))
    del pooled, dpool
    ck.check("stem dgamma", W.vec("image_encoder.stem.1.weight", grad=True), dgamma, T_BNPARAM, dims=(0,), cls="bnparam")
    ck.check("stem dbeta", W.vec("image_encoder.stem.1.bias", grad=True), dbeta, T_BNPARAM, dims=(0,), cls="bnparam")
    ck.check("stem dgamma (routed y)", W.vec("image_encoder.stem.1.weight", grad=True), dgamma_y, T_BNPARAM, dims=(0,), cls="report",
             assert_=False)
    ck.check("stem dbeta (routed y)", W.vec("image_encoder.stem.1.bias", grad=True), dbeta_y, T_BNPARAM, dims=(0,), cls="bnparam")
    gam = W.vec("image_encoder.stem.1.weight").view(1, -1, 1, 1)
    dw = torch.zeros(64, 3, 7, 7, dtype=torch.float64)
    for ch in chunks:
        g, xh = g_of(ch)
        dy = gam * inv * (g - dbeta.float().view(1, -1, 1, 1) / n - xh * dgamma.float().view(1, -1, 1, 1) / n)
        # the fused weight-gradient kernel rebuilds dy row by row and feeds it to bf16 MFMA: its operand is bf16(dy)
        dw += torch.nn.grad.conv2d_weight(rnd(st["images"][ch].cpu()), (64, 3, 7, 7), rnd(dy), stride=2, padding=3).double()
    ck.check("stem dW", W.conv_g("image_encoder.stem.0.weight"), dw, T_WGRAD, cls="wgrad")


def _routed_index(idx, Hp, Wp, W1):
    """Flat position in the H1 x W1 plane of the window element idx = r*3 + s of every pooled output (ih = 2*oh-1+r, iw = 2*ow-1+s)."""
    oh = torch.arange(Hp).view(1, 1, -1, 1)
    ow = torch.arange(Wp).view(1, 1, 1, -1)
    ih = (2 * oh - 1 + idx // 3).clamp(min=0)
    iw = (2 * ow - 1 + idx % 3).clamp(min=0)
    return ih * W1 + iw


def _check_block(ck, run, W, s, rec):
    """Forward (y1, c1, a1, y2, c2, yd / cd, out) and backward of one residual block."""
    eng, cap, B = run["eng"], run["cap"], run["B"]
    sel = _sel(B)
    p, c = rec["p"], cap[rec["p"]]
    H, Wd_, Ho, Wo, stride = rec["g1"][1], rec["g1"][2], rec["g1"][4], rec["g1"][5], rec["g1"][8]
    tg = f"stage{s}.{p[-1]}"
    fused12 = rec["a1"] is None
    a1_t = rec["a1"]
    if fused12:              # stage 1: conv2 and its weight gradient rebuild relu(bn1(y1)) in LDS, the tensor is never stored;
                             # what they consumed is exactly this bf16 value (kernel-level bit-equality: tests/test_gpu_cnn_fused.py)
        # y1 * scale + shift is ONE fma in the kernels: the fp64 value rounded once to fp32 is that (torch's separate mul and add
        # round twice, and where the shift cancels most of the product that moves a1 by one bf16 step -- 0.25% of one channel's
        # elements at U = 103, a 4e-4 error in that input channel of dW2 that is the reference's own)
        a1_t = torch.relu((rec["y1"].double() * rec["c1"][0].double() + rec["c1"][1].double()).float()).to(rec["y1"].dtype)
    x, y1, a1, y2, out = (nchw(t, B, h, w) for t, h, w in ((rec["x"], H, Wd_), (rec["y1"], Ho, Wo), (a1_t, Ho, Wo), (rec["y2"], Ho, Wo),
                                                            (rec["out"], Ho, Wo)))
    del a1_t
    W1, W2 = W.conv_w(p + ".conv1.weight"), W.conv_w(p + ".conv2.weight")
    c1, c2 = rec["c1"].cpu(), rec["c2"].cpu()
    M = B * Ho * Wo
    # ---- forward
    ck.check(f"{tg} y1", y1[sel], F.conv2d(x[sel], W1, stride=stride, padding=1), T_BF16)
    _check_bn_coef(ck, f"{tg} bn1", y1, c1, W.vec(p + ".bn1.weight"), W.vec(p + ".bn1.bias"), run, p + ".bn1", M)
    if not fused12:
        ck.check(f"{tg} a1", a1[sel], torch.relu(y1[sel] * c1[0].view(1, -1, 1, 1) + c1[1].view(1, -1, 1, 1)), T_BF16)
    ck.check(f"{tg} y2", y2[sel], F.conv2d(a1[sel], W2, padding=1), T_BF16)
    _check_bn_coef(ck, f"{tg} bn2", y2, c2, W.vec(p + ".bn2.weight"), W.vec(p + ".bn2.bias"), run, p + ".bn2", M)
    has_ds = "yd" in rec
    if has_ds:
        yd, cd = nchw(rec["yd"], B, Ho, Wo), rec["cd"].cpu()
        Wdn = W.conv_w(p + ".downsample.0.weight")
        ck.check(f"{tg} yd", yd[sel], F.conv2d(x[sel], Wdn, stride=stride), T_BF16)
        _check_bn_coef(ck, f"{tg} bnd", yd, cd, W.vec(p + ".downsample.1.weight"), W.vec(p + ".downsample.1.bias"), run, p + ".downsample.1", M)
        short = yd[sel] * cd[0].view(1, -1, 1, 1) + cd[1].view(1, -1, 1, 1)
    else:
        short = x[sel]
    ck.check(f"{tg} out", out[sel], torch.relu(y2[sel] * c2[0].view(1, -1, 1, 1) + c2[1].view(1, -1, 1, 1) + short), T_BF16)
    # ---- backward
    dout = nchw(c["dout"], B, Ho, Wo)
    g = dout if c["masked"] else dout * (out > 0)
    del dout, out
    dy2_ref, dg2, db2 = bn_bwd(g, y2, c2, W.vec(p + ".bn2.weight"))
    dy2 = nchw(c["dy2"], B, Ho, Wo)
    ck.check(f"{tg} dy2", dy2[sel], dy2_ref[sel], T_BF16)
    del dy2_ref
    ck.check(f"{tg} dgamma2", W.vec(p + ".bn2.weight", grad=True), dg2, T_BNPARAM, dims=(0,), cls="bnparam")
    ck.check(f"{tg} dbeta2", W.vec(p + ".bn2.bias", grad=True), db2, T_BNPARAM, dims=(0,), cls="bnparam")
    if has_ds:
        dyd_ref, dgd, dbd = bn_bwd(g, yd, cd, W.vec(p + ".downsample.1.weight"))
        dyd = nchw(c["dyd"], B, Ho, Wo)
        ck.check(f"{tg} dyd", dyd[sel], dyd_ref[sel], T_BF16)
        del dyd_ref, yd
        ck.check(f"{tg} dgamma_d", W.vec(p + ".downsample.1.weight", grad=True), dgd, T_BNPARAM, dims=(0,), cls="bnparam")
        ck.check(f"{tg} dbeta_d", W.vec(p + ".downsample.1.bias", grad=True), dbd, T_BNPARAM, dims=(0,), cls="bnparam")
    ck.check(f"{tg} dW2", W.conv_g(p + ".conv2.weight"), _wgrad_ref(a1, W2.shape, dy2, 1, 1), T_WGRAD,
             cls="wgrad")
    da1 = nchw(c["da1"], B, Ho, Wo)
    ck.check(f"{tg} da1", da1[sel], torch.nn.grad.conv2d_input(a1[sel].shape, W2, dy2[sel], stride=1, padding=1), T_BF16)
    del a1, dy2
    relu1 = (y1 * c1[0].view(1, -1, 1, 1) + c1[1].view(1, -1, 1, 1)) > 0
    dy1_ref, dg1, db1 = bn_bwd(da1 * relu1, y1, c1, W.vec(p + ".bn1.weight"))
    del relu1, da1, y1
    dy1 = nchw(c["dy1"], B, Ho, Wo)
    ck.check(f"{tg} dy1", dy1[sel], dy1_ref[sel], T_BF16)
    del dy1_ref
    ck.check(f"{tg} dgamma1", W.vec(p + ".bn1.weight", grad=True), dg1, T_BNPARAM, dims=(0,), cls="bnparam")
    ck.check(f"{tg} dbeta1", W.vec(p + ".bn1.bias", grad=True), db1, T_BNPARAM, dims=(0,), cls="bnparam")
    ck.check(f"{tg} dW1", W.conv_g(p + ".conv1.weight"), _wgrad_ref(x, W1.shape, dy1, stride, 1), T_WGRAD,
             cls="wgrad")
    dx_ref = torch.nn.grad.conv2d_input(x[sel].shape, W1, dy1[sel], stride=stride, padding=1)
    if has_ds:
        dyd = nchw(c["dyd"], B, Ho, Wo)
        ck.check(f"{tg} dWd", W.conv_g(p + ".downsample.0.weight"), _wgrad_ref(x, Wdn.shape, dyd, stride, 0),
                 T_WGRAD, cls="wgrad")
        dx_ref = dx_ref + torch.nn.grad.conv2d_input(x[sel].shape, Wdn, dyd[sel], stride=stride, padding=0)
    else:
        dx_ref = dx_ref + g[sel]                                     # identity path: the masked gradient of the block output
    if c["handed"]:
        dx_ref = dx_ref * (x[sel] > 0)                               # handed to the previous block already masked by ITS ReLU
    ck.check(f"{tg} dx", nchw(c["dx"], B, H, Wd_, sel), dx_ref, T_BF16)
    return int(c["masked"]), int(c["handed"]), int(fused12)


def _check_se(ck, run, W, s, r):
    B, cap = run["B"], run["cap"]
    ap = f"image_encoder.stage{s}.attention"
    HW, C = r["HW"], r["C"]
    Hs = int(round(math.sqrt(HW)))
    x = nchw(r["x"], B, Hs, HW // Hs).double()
    w1, w2 = W.vec(ap + ".se.fc1.weight").double(), W.vec(ap + ".se.fc2.weight").double()
    pooled = x.mean((2, 3))
    hidden = torch.relu(pooled @ w1.t())
    scale = torch.sigmoid(hidden @ w2.t())
    ck.check(f"stage{s} se pooled", r["pooled"].cpu(), pooled, T_FP32, cls="fp32")
    ck.check(f"stage{s} se hidden", r["hidden"].cpu(), hidden, T_FP32, cls="fp32")
    ck.check(f"stage{s} se scale", r["scale"].cpu(), scale, T_FP32, cls="fp32")
    out_t = cap[ap + ".se"]
    # the SE output is the next op's input on the tape: spatial attention's x, or the next stage's first block's x, or the features
    sel = _sel(B)
    out_ref = (x[sel] * scale[sel][:, :, None, None])
    nxt = _se_output(run, s)
    ck.check(f"stage{s} se out", nchw(nxt, B, Hs, HW // Hs, sel), out_ref, T_BF16)
    # backward: fp64 autograd of O.se_attention on the tape's x; dxn carries the last block's ReLU mask (x > 0)
    xg = x.clone().requires_grad_(True)
    w1g, w2g = w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
    dout = nchw(out_t["dout"], B, Hs, HW // Hs).double()
    O.se_attention(xg, w1g, w2g).backward(dout)
    ck.check(f"stage{s} se dx", nchw(out_t["dx"], B, Hs, HW // Hs, sel), (xg.grad * (x > 0))[sel], T_BF16)
    ck.check(f"stage{s} se dW1", W.vec(ap + ".se.fc1.weight", grad=True), w1g.grad, T_WGRAD, cls="wgrad")
    ck.check(f"stage{s} se dW2", W.vec(ap + ".se.fc2.weight", grad=True), w2g.grad, T_WGRAD, cls="wgrad")


def _se_output(run, s):
    srec = run["tape"]["stages"][s - 1]
    if "spatial" in srec:
        return srec["spatial"]["x"]
    if s < 4:
        return run["tape"]["stages"][s]["blocks"][0]["x"]
    return run["tape"]["proj"]["feat"]


def _check_spatial(ck, run, W, s, r):
    B, cap = run["B"], run["cap"]
    ap = f"image_encoder.stage{s}.attention"
    H, Wd_, C = r["H"], r["W"], r["C"]
    x = nchw(r["x"], B, H, Wd_).double()
    w = W.vec(ap + ".spatial.conv.weight").double()
    amax = r["amax"].cpu().long().view(B, 1, H, Wd_)
    mx = x.max(1, keepdim=True)[0]
    av = x.mean(1, keepdim=True)
    p2 = r["pooled2"].cpu().view(B, H, Wd_, 2).permute(0, 3, 1, 2)
    ck.check(f"stage{s} spatial pooled2", p2, torch.cat([mx, av], 1), T_FP32, cls="fp32")
    ck.expect(f"stage{s} spatial amax", bool(((amax >= 0) & (amax < C)).all()) and torch.equal(x.gather(1, amax.clamp(0, C - 1)), mx),
              "argmax channel does not hold the channel maximum")
    amap = torch.sigmoid(F.conv2d(torch.cat([mx, av], 1), w, padding=3))
    ck.check(f"stage{s} spatial amap", r["amap"].cpu().view(B, 1, H, Wd_), amap, T_FP32, cls="fp32")
    sel = _sel(B)
    nxt = run["tape"]["stages"][s]["blocks"][0]["x"] if s < 4 else run["tape"]["proj"]["feat"]
    ck.check(f"stage{s} spatial out", nchw(nxt, B, H, Wd_, sel), (x * amap)[sel], T_BF16)
    # backward: fp64 autograd of O.spatial_attention's formula with the max routed to the kernel's argmax channel
    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    m_ = xg.gather(1, amax.clamp(0, C - 1))
    a_ = torch.sigmoid(F.conv2d(torch.cat([m_, xg.mean(1, keepdim=True)], 1), wg, padding=3))
    c = cap[ap + ".spatial"]
    (xg * a_).backward(nchw(c["dout"], B, H, Wd_).double())
    ck.check(f"stage{s} spatial dx", nchw(c["dx"], B, H, Wd_, sel), xg.grad[sel], T_BF16)
    ck.check(f"stage{s} spatial dW", W.vec(ap + ".spatial.conv.weight", grad=True), wg.grad, T_WGRAD, cls="wgrad")


# ------------------------------------------------------------------ token side (fp64)
def _ln(x, W, prefix):
    return F.layer_norm(x, (x.shape[-1],), W.vec(prefix + ".weight").double(), W.vec(prefix + ".bias").double(), O.LN_EPS)


def _cpu(t):
    return t.cpu().double()


def _lnw(W, prefix):
    return W.vec(prefix + ".weight").double(), W.vec(prefix + ".bias").double()


def _rnd64(t):
    return rnd(t.float()).double()


def _ln_bwd_ref(x, dy, W, prefix):
    """fp64 LayerNorm backward at the stored input x with the captured upstream gradient dy: (dx, dgamma, dbeta)."""
    w, b = _lnw(W, prefix)
    xg, wg, bg = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    F.layer_norm(xg, (x.shape[-1],), wg, bg, O.LN_EPS).backward(dy)
    return xg.grad, wg.grad, bg.grad


def _check_lin_grads(ck, W, tag, wname, bname, dz, x, dz_bias=None):
    """Linear weight / bias gradients in G from the captured output gradient dz and the stored input x.  dz_bias: the gradient the
    bias sum is taken of when it is not the stored dz (vqa_bias_act_bwd sums the fp32 product before rounding it)."""
    ck.check(f"{tag} d{wname.rsplit('.', 2)[-2]}", W.vec(wname, grad=True), dz.t() @ x, T_WGRAD, cls="wgrad")
    if bname:
        ck.check(f"{tag} d{bname.rsplit('.', 2)[-2]}.bias", W.vec(bname, grad=True), (dz if dz_bias is None else dz_bias).sum(0), T_WGRAD,
                 dims=(0,), cls="wgrad")


def _check_ln_grads(ck, W, tag, prefix, dg, db):
    short = prefix.rsplit(".", 1)[-1]
    ck.check(f"{tag} d{short}.weight", W.vec(prefix + ".weight", grad=True), dg, T_BNPARAM, dims=(0,), cls="bnparam")
    ck.check(f"{tag} d{short}.bias", W.vec(prefix + ".bias", grad=True), db, T_BNPARAM, dims=(0,), cls="bnparam")


def _attn_fwd_local(rec, loc, W, kmask, index=None):
    """probs from the stored Q / K and ctx from the stored probs / V, fp64.  index: image of every question (indexed attention:
    K / V hold one batch per image; the dropout mask is drawn per question, as the plain kernel draws it per batch)."""
    B, Lq, Lk, H, hd, p = rec["B"], rec["Lq"], rec["Lk"], rec["heads"], rec["hd"], rec["p"]
    Qh = loc["Q"].view(B, Lq, H, hd).transpose(1, 2)
    Kh = loc["K"].view(-1, Lk, H, hd).transpose(1, 2)
    Vh = loc["V"].view(-1, Lk, H, hd).transpose(1, 2)
    P = rec["probs"].cpu().double()
    keep = _keep(rec["sa"], (B, H, Lq, Lk), p)
    probs, ctx = attn_core_fwd(Qh, Kh, Vh, P, keep, kmask=kmask, index=index)
    return probs, ctx.transpose(1, 2).reshape(B * Lq, -1), (Qh, Kh, Vh, P, keep)


def _check_attn_block(ck, run, W, rec, tag, kmask, dkv_next, index=None):
    """Every op of one attention + FFN block, forward and backward, from the stored / captured operands of THAT op.  index: the
    image of every question when K / V are per image (grouped cross-attention): dK / dV, the K / V weight gradients, norm_kv's
    backward and the image-token gradient run over U * Lk rows."""
    c = run["cap"][rec["attn"]]
    B, Lq, H, hd, p = rec["B"], rec["Lq"], rec["heads"], rec["hd"], rec["p"]
    ck.expect(f"{tag} indexed", (rec.get("csr") is not None) == (index is not None), "the tape and the test disagree on the index")
    d = H * hd
    attn, fc1, fc2 = rec["attn"], rec["fc1"], rec["fc2"]
    Wq, Wk, Wv, Wo = (W.lin_w(attn + f".W_{w}.weight") for w in "qkvo")
    W1, W2 = W.lin_w(fc1 + ".weight"), W.lin_w(fc2 + ".weight")
    b1, b2 = W.vec(fc1 + ".bias").double(), W.vec(fc2 + ".bias").double()
    loc = {k: _cpu(rec[k]) for k in ("q_in", "kv_in", "nq", "nkv", "Q", "K", "V", "ctx", "x1", "nf", "h", "out")}
    for k in ("Q", "K", "V"):                  # column views of the fused [M][3d] / [M][2d] projections
        loc[k] = loc[k][:, :d]
    k_o, k_1, k_2 = (_keep(rec[sd], shp, p) for sd, shp in (("so", (B * Lq, d)), ("s1", (B * Lq, W1.shape[0])), ("s2", (B * Lq, d))))
    # ---- forward
    ck.check(f"{tag} nq", loc["nq"], _ln(loc["q_in"], W, rec["norm_q"]), T_BF16)
    if not rec["self_attn"]:
        ck.check(f"{tag} nkv", loc["nkv"], _ln(loc["kv_in"], W, rec["norm_kv"]), T_BF16)
    ck.check(f"{tag} Q", loc["Q"], loc["nq"] @ Wq.t(), T_BF16)
    ck.check(f"{tag} K", loc["K"], loc["nkv"] @ Wk.t(), T_BF16)
    ck.check(f"{tag} V", loc["V"], loc["nkv"] @ Wv.t(), T_BF16)
    probs, ctx, (Qh, Kh, Vh, P, keep_a) = _attn_fwd_local(rec, loc, W, kmask, index)
    ck.check(f"{tag} probs", rec["probs"].cpu(), probs, T_PROBS, cls="probs")
    ck.check(f"{tag} ctx", loc["ctx"], ctx, T_BF16)
    ck.check(f"{tag} x1", loc["x1"], loc["q_in"] + (loc["ctx"] @ Wo.t()) * k_o, T_BF16)
    ck.check(f"{tag} nf", loc["nf"], _ln(loc["x1"], W, rec["norm_f"]), T_BF16)
    ck.check(f"{tag} h", loc["h"], torch.relu(loc["nf"] @ W1.t() + b1) * k_1, T_BF16)
    ck.check(f"{tag} out", loc["out"], loc["x1"] + (loc["h"] @ W2.t() + b2) * k_2, T_BF16)
    # ---- backward, op by op (out = x1 + drop(fc2(drop(relu(fc1(nf))))), nf = LN(x1), x1 = q_in + drop(W_o ctx))
    g = {k: (None if c[k] is None else _cpu(c[k])) for k in ("dout", "dz2", "dz1", "dnf", "dx1", "dzo", "dctx", "dQ", "dK", "dV", "dnq",
                                                               "dnkv", "dq", "dkv")}
    for k in ("dQ", "dK", "dV"):
        g[k] = g[k][:, :d]
    ck.check(f"{tag} dz2", g["dz2"], g["dout"] * k_2, T_BF16)
    _check_lin_grads(ck, W, tag, fc2 + ".weight", fc2 + ".bias", g["dz2"], loc["h"], dz_bias=g["dout"] * k_2)
    # fused data gradient + ReLU / dropout backward: the product is rounded to bf16 before the keep scale (kernels.linear_dgrad_act)
    ck.check(f"{tag} dz1", g["dz1"], _rnd64(g["dz2"] @ W2) * (loc["h"] > 0) / (1.0 - p), T_BF16)
    _check_lin_grads(ck, W, tag, fc1 + ".weight", fc1 + ".bias", g["dz1"], loc["nf"])
    ck.check(f"{tag} dnf", g["dnf"], g["dz1"] @ W1, T_BF16)
    dx1, dgf, dbf = _ln_bwd_ref(loc["x1"], g["dnf"], W, rec["norm_f"])
    ck.check(f"{tag} dx1", g["dx1"], dx1 + g["dout"], T_BF16)
    _check_ln_grads(ck, W, tag, rec["norm_f"], dgf, dbf)
    ck.check(f"{tag} dzo", g["dzo"], g["dx1"] * k_o, T_BF16)
    _check_lin_grads(ck, W, tag, attn + ".W_o.weight", None, g["dzo"], loc["ctx"])
    ck.check(f"{tag} dctx", g["dctx"], g["dzo"] @ Wo, T_BF16)
    # attention core, closed form on the stored probabilities (dK / dV summed per image over its questions when indexed)
    dC = g["dctx"].view(B, Lq, H, hd).transpose(1, 2)
    dQ, dK, dV = attn_core_bwd(Qh, Kh, Vh, P, keep_a, dC, index=index, n_kv=Kh.shape[0])
    flat = lambda t: t.transpose(1, 2).reshape(-1, d)
    ck.check(f"{tag} dQ", g["dQ"], flat(dQ), T_ATTN, cls="attn", slice_tol=T_ATTN_SLICE)
    ck.check(f"{tag} dK", g["dK"], flat(dK), T_ATTN, cls="attn", slice_tol=T_ATTN_SLICE)
    ck.check(f"{tag} dV", g["dV"], flat(dV), T_ATTN, cls="attn", slice_tol=T_ATTN_SLICE)
    if index is not None:                      # the same per image (all Lk rows of an image as one slice)
        ck.check(f"{tag} dK per image", g["dK"].reshape(Kh.shape[0], -1), flat(dK).reshape(Kh.shape[0], -1), T_ATTN, dims=(0,), cls="attn",
                 slice_tol=T_ATTN_SLICE)
        ck.check(f"{tag} dV per image", g["dV"].reshape(Kh.shape[0], -1), flat(dV).reshape(Kh.shape[0], -1), T_ATTN, dims=(0,), cls="attn",
                 slice_tol=T_ATTN_SLICE)
    _check_lin_grads(ck, W, tag, attn + ".W_q.weight", None, g["dQ"], loc["nq"])
    _check_lin_grads(ck, W, tag, attn + ".W_k.weight", None, g["dK"], loc["nkv"])
    _check_lin_grads(ck, W, tag, attn + ".W_v.weight", None, g["dV"], loc["nkv"])
    if rec["self_attn"]:
        ck.check(f"{tag} dnq", g["dnq"], g["dQ"] @ Wq + g["dK"] @ Wk + g["dV"] @ Wv, T_BF16)
    else:
        ck.check(f"{tag} dnq", g["dnq"], g["dQ"] @ Wq, T_BF16)
        ck.check(f"{tag} dnkv", g["dnkv"], g["dK"] @ Wk + g["dV"] @ Wv, T_BF16)
    dq, dgq, dbq = _ln_bwd_ref(loc["q_in"], g["dnq"], W, rec["norm_q"])
    ck.check(f"{tag} dq", g["dq"], dq + g["dx1"], T_BF16)
    _check_ln_grads(ck, W, tag, rec["norm_q"], dgq, dbq)
    if not rec["self_attn"]:                   # the image-token gradient carries the layers after this one (the addend)
        dkv, dgk, dbk = _ln_bwd_ref(loc["kv_in"], g["dnkv"], W, rec["norm_kv"])
        ck.check(f"{tag} dkv", g["dkv"], dkv + (0 if dkv_next is None else _cpu(dkv_next)), T_BF16)
        _check_ln_grads(ck, W, tag, rec["norm_kv"], dgk, dbk)


def _check_token_side(ck, run, W):
    """Question rows (text, pools, gate, head) at B = run["Bq"], image-token rows (projector, norm_kv, K / V) at U = run["B"]."""
    eng, tape, cap, cfg = run["eng"], run["tape"], run["cap"], run["cfg"]
    B, U, d, index = run["Bq"], run["B"], cfg["embed_dim"], run["index"]
    ids, maskf = run["ids"].cpu(), run["maskf"].cpu().double()
    L = ids.shape[1]
    # ---- embedding + positional encoding + dropout
    em = tape["embed"]
    emb = W.vec("text_encoder.token_embedding.weight").double()
    pe = eng.buf["text_encoder.positional_encoding.pe"].cpu().double()[0, :L]
    keep_e = _keep(em["seed"], (B * L, d), em["p"])
    xt_ref = (emb[ids.view(-1)] * math.sqrt(d) + pe.repeat(B, 1)) * keep_e
    ck.check("embed", _cpu(tape["tlayers"][0]["q_in"]), xt_ref, T_BF16)
    # ---- text layers
    for l, rec in enumerate(tape["tlayers"]):
        _check_attn_block(ck, run, W, rec, f"text{l}", maskf, None)
    # embedding gradient from the first layer's input gradient
    dx0 = _cpu(cap[tape["tlayers"][0]["attn"]]["dq"]) * keep_e * math.sqrt(d)
    demb = torch.zeros_like(emb).index_add_(0, ids.view(-1), dx0)
    demb[0] = 0
    ck.check("embed demb", W.vec("text_encoder.token_embedding.weight", grad=True), demb, T_WGRAD, dims=(1,), cls="wgrad")
    # ---- final norm
    fn = tape["final_norm"]
    pl = tape["pool"]
    enc = _cpu(pl["enc"])
    ck.check("final_norm", enc, _ln(_cpu(fn["x"]), W, "text_encoder.final_norm"), T_BF16)
    # ---- projector: Linear, LayerNorm, dropout, + position embedding
    pr = tape["proj"]
    ntok = pr["ntok"]
    feat, pz = _cpu(pr["feat"]), _cpu(pr["pz"])
    pj = "fusion.image_projector.projection"
    Wp, bp = W.lin_w(pj + ".0.weight"), W.vec(pj + ".0.bias").double()
    pos = W.vec("fusion.image_projector.position_embedding").double().view(-1, d)[:ntok]
    keep_p = _keep(pr["seed"], (U * ntok, d), pr["p"])
    ck.check("proj linear", pz, feat @ Wp.t() + bp, T_BF16)
    ck.check("proj ln+dropout+pos", _cpu(tape["clayers"][0]["kv_in"]), _ln(pz, W, pj + ".1") * keep_p + pos.repeat(U, 1), T_BF16)
    # ---- cross-attention layers (the K / V gradient of layer l includes those of the layers after it)
    ncl = len(tape["clayers"])
    for l, rec in enumerate(tape["clayers"]):
        nxt = cap[tape["clayers"][l + 1]["attn"]]["dkv"] if l + 1 < ncl else None
        _check_attn_block(ck, run, W, rec, f"cross{l}", None, nxt, index=index)
    # projector backward: dimg (the first cross layer's image-token gradient) -> LN + dropout -> Linear -> features
    cp = cap["fusion.image_projector"]
    dimg, dpz = _cpu(cp["dimg"]), _cpu(cp["dpz"])
    ck.check("proj dimg", dimg, _cpu(cap[tape["clayers"][0]["attn"]]["dkv"]), T_BF16)
    dpz_ref, dgp, dbp = _ln_bwd_ref(pz, dimg * keep_p, W, pj + ".1")
    ck.check("proj dpz", dpz, dpz_ref, T_BF16)
    _check_ln_grads(ck, W, "proj", pj + ".1", dgp, dbp)
    ck.check("proj dpos", W.vec("fusion.image_projector.position_embedding", grad=True).view(-1, d)[:ntok],
             dimg.view(U, ntok, d).sum(0), T_WGRAD, cls="wgrad")
    _check_lin_grads(ck, W, "proj", pj + ".0.weight", pj + ".0.bias", dpz, feat)
    ck.check("proj dfeat", _cpu(cp["dfeat"]), dpz @ Wp, T_BF16)
    if "image_encoder.stage4.attention.spatial" in cap:
        ck.expect("proj dfeat -> spatial", cap["image_encoder.stage4.attention.spatial"]["dout"] is cp["dfeat"], "not the same tensor")
    if index is not None:
        # an image without questions receives no image-token gradient anywhere: every one of its rows is exactly zero, from each
        # cross layer's dK / dV down to the gradient entering the CNN (its BatchNorm statistics still count it: _check_bn_coef)
        empty = empty_images(index, U)
        for l, rec in enumerate(tape["clayers"]):
            cl = cap[rec["attn"]]
            for k in ("dK", "dV", "dnkv", "dkv"):
                check_zero_rows(ck, f"cross{l} {k}", cl[k].cpu(), U, empty)
        for k in ("dimg", "dpz", "dfeat"):
            check_zero_rows(ck, f"proj {k}", cp[k].cpu(), U, empty)
        if "image_encoder.stage4.attention.spatial" in cap:
            check_zero_rows(ck, "stage4 spatial dout", cap["image_encoder.stage4.attention.spatial"]["dout"].cpu(), U, empty)
    # ---- masked pool pair, gate, output norm
    q_last = _cpu(pl["q"])
    m3 = maskf.view(B, L, 1)
    cnt = m3.sum(1).clamp(min=1)
    Wg, bg = W.lin_w("fusion.gate.gate.0.weight"), W.vec("fusion.gate.gate.0.bias").double()
    cat = _cpu(pl["cat"])
    ck.check("pool cat", cat, torch.cat([(q_last.view(B, L, d) * m3).sum(1) / cnt, (enc.view(B, L, d) * m3).sum(1) / cnt], 1), T_BF16)
    ck.check("gate z", _cpu(pl["z"]), cat @ Wg.t() + bg, T_BF16)
    sg = torch.sigmoid(_cpu(pl["z"]))
    ck.check("gate fused_pre", _cpu(pl["fused_pre"]), sg * cat[:, :d] + (1 - sg) * cat[:, d:], T_BF16)
    ck.check("output_norm", _cpu(tape["head"]["fused"]), _ln(_cpu(pl["fused_pre"]), W, "fusion.output_norm"), T_BF16)
    cf = cap["fusion"]
    dfp_ref, dgo, dbo = _ln_bwd_ref(_cpu(pl["fused_pre"]), _cpu(cf["dfused"]), W, "fusion.output_norm")
    dfp = _cpu(cf["dfp"])
    ck.check("fusion dfp", dfp, dfp_ref, T_BF16)
    _check_ln_grads(ck, W, "fusion", "fusion.output_norm", dgo, dbo)
    dzg = _cpu(cf["dzg"])
    ck.check("gate dz", dzg, dfp * (cat[:, :d] - cat[:, d:]) * sg * (1 - sg), T_BF16)
    _check_lin_grads(ck, W, "fusion", "fusion.gate.gate.0.weight", "fusion.gate.gate.0.bias", dzg, cat)
    dcat = _cpu(cf["dcat"])
    ck.check("gate dcat", dcat, torch.cat([dfp * sg, dfp * (1 - sg)], 1) + dzg @ Wg, T_BF16)
    ck.check("pool dq", _cpu(cf["dq"]), (dcat[:, None, :d] * m3 / cnt[:, None]).reshape(B * L, d), T_BF16)
    ck.expect("pool dq -> cross", cap[tape["clayers"][-1]["attn"]]["dout"] is cf["dq"], "not the same tensor")
    ck.check("pool denc", _cpu(cf["denc_pool"]), (dcat[:, None, d:] * m3 / cnt[:, None]).reshape(B * L, d), T_BF16)
    denc = _cpu(cf["denc"])
    ck.check("fusion denc", denc, _cpu(cf["denc_pool"]) + _cpu(cap[tape["clayers"][0]["attn"]]["dq"]), T_BF16)
    dxf, dgfn, dbfn = _ln_bwd_ref(_cpu(fn["x"]), denc, W, "text_encoder.final_norm")
    ck.check("final_norm dx", _cpu(cap[tape["tlayers"][-1]["attn"]]["dout"]), dxf, T_BF16)
    _check_ln_grads(ck, W, "final_norm", "text_encoder.final_norm", dgfn, dbfn)
    # ---- answer head (dropout after both hidden ReLUs)
    hd_ = tape["head"]
    c = "answer_head.classifier"
    W0, W3, W6 = W.lin_w(c + ".0.weight"), W.lin_w(c + ".3.weight"), W.lin_w(c + ".6.weight")
    b0, b3, b6 = (W.vec(c + f".{i}.bias").double() for i in (0, 3, 6))
    fused, h1, h2 = _cpu(hd_["fused"]), _cpu(hd_["h1"]), _cpu(hd_["h2"])
    k1, k2 = _keep(hd_["s1"], tuple(h1.shape), hd_["p"]), _keep(hd_["s2"], tuple(h2.shape), hd_["p"])
    ck.check("head h1", h1, torch.relu(fused @ W0.t() + b0) * k1, T_BF16)
    ck.check("head h2", h2, torch.relu(h1 @ W3.t() + b3) * k2, T_BF16)
    ck.check("logits", _cpu(run["logits"]), h2 @ W6.t() + b6, T_BF16)
    ch = cap["answer_head"]
    dl, dz0 = _cpu(ch["dlogits"]), _cpu(ch["dz0"])
    ph = hd_["p"]
    _check_lin_grads(ck, W, "head", c + ".6.weight", c + ".6.bias", dl, h2)
    # fused data gradient + ReLU / dropout backward: the product is rounded to bf16 before the keep scale (kernels.linear_dgrad_act)
    dz3 = _cpu(ch["dz3"])
    ck.check("head dz3", dz3, _rnd64(dl @ W6) * (h2 > 0) / (1.0 - ph), T_BF16)
    _check_lin_grads(ck, W, "head", c + ".3.weight", c + ".3.bias", dz3, h1)
    ck.check("head dz0", dz0, _rnd64(dz3 @ W3) * (h1 > 0) / (1.0 - ph), T_BF16)
    _check_lin_grads(ck, W, "head", c + ".0.weight", c + ".0.bias", dz0, fused)
    ck.check("head dfused", _cpu(ch["dfused"]), dz0 @ W0, T_BF16)
    ck.expect("head dfused -> fusion", ch["dfused"] is cf["dfused"] or torch.equal(ch["dfused"], cf["dfused"]), "differs")


def _wgrad_plans(run, at=None):
    """{conv: (kind, tile n, tile k, nsplit)} of vqa_wgrad (kernels.wgrad_plan) for the conv weight gradients of this step that go
    through kernels.wgrad -- the stage-2 entry conv and every 3x3 conv of stages 3 and 4 -- at its image batch, or at `at` images."""
    K = pkg().kernels
    plans = {}
    for s in (2, 3, 4):
        for rec in run["tape"]["stages"][s - 1]["blocks"]:
            for conv, g in (("conv1", rec["g1"]), ("conv2", rec["g2"])):
                if s == 2 and not (conv == "conv1" and "yd" in rec):
                    continue                   # (the 128 -> 128 convs of stage 2 run the c128 patch kernel)
                B, H, W_, C, Ho, Wo, R, S = g[:8]
                if at is not None:
                    B = at
                plans[f"stage{s}.{rec['p'][-1]}.{conv}"] = K.wgrad_plan(torch.bfloat16, K.LOADER_NHWC, B * Ho * Wo, rec["Cout"], R * S * C, B, H,
                                                                         W_, C, R, S)[:4]
    return plans


def _wgrad_symbol(plan):
    """kernels.wgrad's PROFILE symbol of a bf16 plan."""
    kind, tn, tk = plan[:3]
    return f"wgrad_dma_kernel<{tn}, {tk}, 2>" if kind else f"wgrad_kernel<unsigned short, {tn}, {tk}, 0>"


def _check_grouped(ck, run, name, syms):
    """What only a grouped step has: the CSR of the image index, its own kernels, and the weight-gradient kernels its image batch
    selects (the planner gives the 8-wave DMA kernel only to problems of >= 3e10 FLOP)."""
    tape, index, U = run["tape"], run["index"], run["B"]
    _, offsets, order, n_kv = tape["csr"]
    ck.expect("csr images", n_kv == U, f"{n_kv} != {U}")
    check_csr(ck, "csr", index, U, offsets, order)
    missing = [s for s in GROUPED_SYMBOLS if s not in syms]
    assert not missing, (missing, sorted(syms))
    plans, plans512 = _wgrad_plans(run), _wgrad_plans(run, at=512)
    print(f"{name}: wgrad plans (kind, tile n, tile k, nsplit) at U = {U}: {plans}; at 512: {plans512}")
    missing = [(c, _wgrad_symbol(pl)) for c, pl in plans.items() if _wgrad_symbol(pl) not in syms]
    assert not missing, (missing, sorted(syms))
    if name == "g5":                           # U = 103: every one of them drops to the 4-wave split kernel, which B = 512 does not use
        assert all(pl[0] == 0 for pl in plans.values()), plans
        assert all(pl[0] == 1 for pl in plans512.values()), plans512
    else:                                      # U = 160: the non-entry stage-3 / 4 convs (3.7e10 FLOP) keep the DMA kernel
        assert {c for c, pl in plans.items() if pl[0] == 1} == {"stage3.1.conv1", "stage3.1.conv2", "stage3.0.conv2", "stage4.1.conv1",
                                                                "stage4.1.conv2", "stage4.0.conv2"}, plans
        cnt = torch.bincount(index, minlength=U)
        assert int(cnt[0]) == 0 and int(cnt[U - 1]) == 0 and int(cnt.max()) >= 9, cnt
        assert not bool((index[1:] >= index[:-1]).all())          # shuffled


CPU_SECONDS = {}


@pytest.mark.parametrize("name", ["b64", "b512", "stress", "g5", "gmix"])
def test_every_layer_of_a_live_bf16_step_matches_fp32_math_locally(name):
    torch.set_num_threads(16)
    t0 = time.perf_counter()
    run = _live_step(name)
    eng, tape, B = run["eng"], run["tape"], run["B"]
    t_gpu = time.perf_counter() - t0
    # the benchmark's kernels really ran in this step
    syms = set(run["syms"])
    if name == "b512":
        missing = [s for s in B512_SYMBOLS if s not in syms]
        assert not missing, (missing, sorted(syms))
    ck = Checker()
    if run["index"] is not None:
        _check_grouped(ck, run, name, syms)
    W = _Params(run)
    _check_stem(ck, run, W)
    n_handed = n_masked = n_fused12 = nblk = 0
    for s, srec in enumerate(tape["stages"], start=1):
        for rec in srec["blocks"]:
            mk, hd, fu = _check_block(ck, run, W, s, rec)
            n_masked += mk; n_handed += hd; n_fused12 += fu; nblk += 1
        if "se" in srec:
            _check_se(ck, run, W, s, srec["se"])
        if "spatial" in srec:
            _check_spatial(ck, run, W, s, srec["spatial"])
    _check_token_side(ck, run, W)
    CPU_SECONDS[name] = round(time.perf_counter() - t0 - t_gpu, 1)
    print(f"\n{name}: live step {t_gpu:.1f} s, references {CPU_SECONDS[name]} s")
    # the schedule this test is about really ran: second blocks hand their gradient over masked, first blocks of a stage do not
    assert nblk == 8
    assert n_handed == 4 and n_masked >= 4, (n_handed, n_masked)
    assert n_fused12 == 2, n_fused12         # both stage-1 blocks ran conv1 -> bn1 -> relu -> conv2 without a1 (engine.fuse_bn_conv)
    ck.finish(name)
