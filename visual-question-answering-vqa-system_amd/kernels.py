"""Thin tensor-level wrappers over the C ABI (one Python function per exported kernel family).

Layouts: CNN activations are NHWC `[B, H, W, C]`, tokens `[rows, D]`; compute dtype T is float32 (parity
path, fp32 MFMA) or bfloat16 (throughput path, bf16 MFMA with fp32 accumulation).  All statistics,
coefficients, weight gradients and optimizer state are float32.  Functions allocate outputs with torch
(the caching allocator is the only allocator) and launch on the current stream.
"""
from __future__ import annotations

import collections
import os

import torch

from . import _lib as L
from ._lib import call, dt, ptr

LOADER_NHWC, LOADER_STEM = 0, 1

# Optional live profiling (bench.py): when PROFILE is a list, the wrappers bracket their launch with events on the
# launch stream (prof_begin / prof_end) and append (kernel symbol, algorithmic FLOPs, start event, end event, algorithmic bytes).
PROFILE = None
PROFILE_VARIANTS = []        # (symbol, variant label, FLOPs, start event, end event) of launches whose symbol covers several code paths
PROFILE_STAGED = {}      # symbol -> bytes staged through LDS-DMA by its profiled launches (conv8p)


def prof_begin():
    """Start of a profiled launch: a recorded timing event while PROFILE is a list, else None (no event is created)."""
    if PROFILE is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def prof_end(e0, sym, flops, nbytes):
    """End of the launch prof_begin() opened (e0 not None): appends (sym, flops, e0, e1, nbytes) to PROFILE; returns e1."""
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    PROFILE.append((sym, flops, e0, e1, nbytes))
    return e1

# HBM-bound entries (no FLOPs worth counting): algorithmic bytes of one call from its C-ABI argument list -- the tensors the op
# must read and write once; recorded as ("hbm:<class>:<entry>", 0, e0, e1, bytes) while PROFILE is a list.  A formula reads
# its arguments by the parameter names of include/vqa_hip.h (L.ARGNAMES), so an argument inserted into an entry moves none of them.
_P = lambda p: 1 if p else 0           # optional operand present
_ES = lambda d: 2 if d else 4          # element size of the compute dtype argument (0 = f32, 1 = bf16)
# attention, es = element size (the _mfma entries take no dtype: 2): Q, K, V in and ctx out at row stride ldc (+ probs fp32); the backward
# also reads dctx and writes dQ, dK, dV
_attn_fwd = lambda a, es: (a.B * (a.Lq + 2 * a.Lk) * a.ldc + a.B * a.Lq * a.ldc) * es + a.B * a.H * a.Lq * a.Lk * 4
_attn_bwd = lambda a, es: 2 * (a.B * (a.Lq + 2 * a.Lk) * a.ldc) * es + a.B * a.Lq * a.ldc * es + a.B * a.H * a.Lq * a.Lk * 4
# indexed form (answer(), forward_grouped): queries, ctx and probs per question, K / V once per image; the backward reads Q, K, V, dctx and
# probs and writes dQ per question, dK / dV once per image
_attn_fwd_idx = lambda a, es: (2 * a.B * a.Lq * a.H * a.hd + 2 * a.n_kv * a.Lk * a.H * a.hd) * es + a.B * a.H * a.Lq * a.Lk * 4
_attn_bwd_idx = lambda a, es: (3 * a.B * a.Lq + 4 * a.n_kv * a.Lk) * a.ldc * es + a.B * a.H * a.Lq * a.Lk * 4
_bn_bwd_apply = lambda a: a.numel * _ES(a.dtype) * (3 + _P(a.outact) + 2 * _P(a.y2))
_soft_loss = lambda a: a.B * a.N * (_ES(a.dtype) + 4) + a.B * a.K * (8 + 4 * _P(a.counts))
_HBM_FORMULAS = {
    # BatchNorm passes (A3): statistics finalize reads the slab; apply reads y (+ residual) and writes out; backward reduce reads
    # dout, y (+ activation, + shortcut y); backward apply reads dout, y (+ activation) and writes dy (+ shortcut: y2 in, dy2 out)
    "vqa_bn_stats_finalize": ("bn", lambda a: a.tiles * a.C * 2 * 4 + a.C * 4 * 8),
    "vqa_bn_apply": ("bn", lambda a: a.numel * _ES(a.dtype) * (2 + _P(a.res))),
    "vqa_bn_apply_pool": ("bn", lambda a: a.B * a.HW * a.C * _ES(a.dtype) * (2 + _P(a.res))),
    "vqa_bn_bwd_reduce": ("bn", lambda a: a.rows * a.C * _ES(a.dtype) * (2 + _P(a.outact) + _P(a.y2))),
    "vqa_bn_apply_acc": ("bn", lambda a: a.B * a.HW * a.C * _ES(a.dtype) * (2 + _P(a.res))),
    "vqa_bn_bwd_apply_acc": ("bn", _bn_bwd_apply),
    "vqa_bn_bwd_finalize": ("bn", lambda a: a.nblk * a.C * 3 * 4),
    "vqa_bn_bwd_apply": ("bn", _bn_bwd_apply),
    "vqa_stem_pool_fwd": ("stem_pool", lambda a: a.B * a.H * a.W * a.C * _ES(a.dtype)
                          + a.B * ((a.H - 1) // 2 + 1) * ((a.W - 1) // 2 + 1) * a.C * (_ES(a.dtype) + 1)),
    # SE / spatial attention (A4, A5): pool read + scale read + write forward; dout, x in and dx out backward
    "vqa_se_fwd": ("se_spatial", lambda a: (2 if a.pool_part else 3) * a.B * a.HW * a.C * _ES(a.dtype)),      # pool sums handed over: no pool read
    "vqa_se_bwd": ("se_spatial", lambda a: (3 + _P(a.bn_y)) * a.B * a.HW * a.C * _ES(a.dtype)),               # + the BatchNorm operand when fused
    "vqa_spatial_fwd": ("se_spatial", lambda a: 3 * a.B * a.H * a.W * a.C * _ES(a.dtype)),
    "vqa_spatial_bwd": ("se_spatial", lambda a: 3 * a.B * a.H * a.W * a.C * _ES(a.dtype)),
    # token side: LayerNorm, bias / activation backward, pools, gate, adds, embedding, attention (its FLOPs are tiny: latency class)
    "vqa_layernorm_fwd": ("token", lambda a: 2 * a.rows * a.D * _ES(a.dtype)),
    "vqa_layernorm_bwd": ("token", lambda a: (3 + _P(a.addend)) * a.rows * a.D * _ES(a.dtype)),
    "vqa_bias_act_bwd": ("token", lambda a: a.M * a.N * _ES(a.dtype) * (1 + _P(a.outact) + _P(a.dz))),
    "vqa_add": ("token", lambda a: 3 * a.n * _ES(a.dtype)),
    "vqa_embed_fwd": ("token", lambda a: a.rows * a.D * (4 + _ES(a.dtype))),
    "vqa_embed_bwd": ("token", lambda a: a.rows * a.D * _ES(a.dtype) + a.V * a.D * 4),
    "vqa_masked_pool_fwd": ("token", lambda a: a.B * a.L * a.D * _ES(a.dtype)),
    "vqa_masked_pool_bwd": ("token", lambda a: a.B * a.L * a.D * _ES(a.dtype)),
    "vqa_masked_pool_pair_fwd": ("token", lambda a: 2 * a.B * a.L * a.D * _ES(a.dtype)),
    "vqa_masked_pool_pair_bwd": ("token", lambda a: 2 * a.B * a.L * a.D * _ES(a.dtype)),
    "vqa_attention_fwd_mfma": ("attention", lambda a: _attn_fwd(a, 2)),
    "vqa_attention_bwd_mfma": ("attention", lambda a: _attn_bwd(a, 2)),
    "vqa_attention_fwd": ("attention", lambda a: _attn_fwd(a, _ES(a.dtype))),
    "vqa_attention_bwd": ("attention", lambda a: _attn_bwd(a, _ES(a.dtype))),
    "vqa_attention_fwd_mfma_idx": ("attention", lambda a: _attn_fwd_idx(a, 2)),
    "vqa_attention_fwd_idx": ("attention", lambda a: _attn_fwd_idx(a, _ES(a.dtype))),
    # indexed form in training: the same traffic with dropout; the CSR of the image index is N + U + 1 ints written from N read
    "vqa_attention_fwd_mfma_idx_train": ("attention", lambda a: _attn_fwd_idx(a, 2)),
    "vqa_attention_fwd_idx_train": ("attention", lambda a: _attn_fwd_idx(a, _ES(a.dtype))),
    "vqa_attention_bwd_mfma_idx": ("attention", lambda a: _attn_bwd_idx(a, 2)),
    "vqa_attention_bwd_idx": ("attention", lambda a: _attn_bwd_idx(a, _ES(a.dtype))),
    "vqa_index_csr": ("token", lambda a: (2 * a.N + a.U + 1) * 4),
    "vqa_cross_entropy": ("token", lambda a: a.B * a.N * (_ES(a.dtype) + 4)),
    # soft targets: the logits traffic of the hard kernel + ids, weights, counts [B][K]; the annotator ids are 8 bytes in, 12 out
    "vqa_cross_entropy_soft": ("token", _soft_loss),
    # sigmoid BCE on the same targets: the same tensors in and out
    "vqa_bce_soft": ("token", _soft_loss),
    # options: the hard kernel's logits traffic + the targets and the class weights once (every wave re-reads them from cache)
    "vqa_cross_entropy_opts": ("token", lambda a: a.B * a.N * (_ES(a.dtype) + 4) + a.B * 8 + a.N * 4 * _P(a.class_weight)),
    "vqa_challenge_accuracy_update": ("token", lambda a: a.B * a.N * 4 + a.B * a.K * 8),
    "vqa_answer_scores": ("token", lambda a: a.B * a.A * 20),
    # weight staging and the optimizer tail (H, N1): cast of the flat buffer, packed data-gradient operands, sum of squares, AdamW
    "vqa_convert": ("optimizer", lambda a: a.n * (_ES(a.dtype_in) + _ES(a.dtype_out))),
    "vqa_sumsq": ("optimizer", lambda a: a.n * 4),
    "vqa_adamw": ("optimizer", lambda a: a.n * 4 * 7),
    "vqa_sumsq_ranges": ("optimizer", lambda a: a.n * 4),
    "vqa_adamw_ranges": ("optimizer", lambda a: a.n * 4 * 7),
    # + the weight average: read and write `ema` (8 B per element); alone: read p, read and write ema
    "vqa_adamw_ema": ("optimizer", lambda a: a.n * 4 * 9),
    "vqa_adamw_ranges_ema": ("optimizer", lambda a: a.n * 4 * 9),
    "vqa_ema_update": ("optimizer", lambda a: a.n * 4 * 3),
    # parameter groups: the range kernels' traffic (the groups' block is 128 bytes)
    "vqa_adamw_groups": ("optimizer", lambda a: a.n * 4 * 7),
    "vqa_adamw_groups_ema": ("optimizer", lambda a: a.n * 4 * 9),
}


def _by_name(name, fn):
    """fn over the entry's named arguments -> a function of the positional argument list (or a prefix of it: the rest reads None)."""
    names = L.ARGNAMES[name]
    args = collections.namedtuple(name, names, defaults=(None,) * len(names))
    return lambda seq: fn(args(*seq))


HBM_BYTES = {name: (cls, _by_name(name, fn)) for name, (cls, fn) in _HBM_FORMULAS.items()}


def _hbm_hook(name, args):
    ent = HBM_BYTES.get(name) if PROFILE is not None else None
    if ent is None:
        return None
    cls, fn = ent
    e0 = prof_begin()
    return lambda: prof_end(e0, f"hbm:{cls}:{name[4:]}", 0.0, float(fn(args)))


L._HOOK[0] = _hbm_hook


def igemm_variant(dtype, loader, M, N, Kw, geom) -> int:
    """The template instantiation the C dispatch (gemm_conv.hip igemm_variant) picks: BM*10000 + BN*10 + flavour."""
    B, H, W, C, Ho, Wo, R, S, stride, pad = geom
    return L.count("vqa_igemm_variant", dt(dtype), loader, M, N, Kw, B, H, W, C, Ho, Wo, R, S, stride, pad)


def igemm_symbol(dtype, loader, var) -> str:
    """Kernel symbol as rocprofv3 prints it: igemm_kernel<T, BM, BN, LOADER, waves, BK, waves/SIMD, ring slots, window loader>."""
    bm, bn, fl = var // 10000, (var % 10000) // 10, var % 10
    return f"igemm_kernel<{_tname(dtype)}, {bm}, {bn}, {loader}, 4, {_bk(dtype)}, 2, 2, {1 if fl == 1 else 0}>"


def _tname(dtype):
    return "unsigned short" if dtype == torch.bfloat16 else "float"


def _bk(dtype):
    return 64 if dtype == torch.bfloat16 else 32


def pack_rows(w2d: torch.Tensor, dtype, kp=None) -> torch.Tensor:
    """[N][K] fp32 -> [N][Kp] T (zero padded)."""
    n, k = w2d.shape
    kp = k if kp is None else kp
    if dtype == torch.float32 and kp == k:
        return w2d
    out = torch.empty((n, kp), device=w2d.device, dtype=dtype)
    call("vqa_pack_rows", dt(dtype), ptr(w2d), ptr(out), n, k, kp)
    return out


def pack_transpose(w3d: torch.Tensor, dtype, out=None, ldo=None, col0=0, flip=False) -> torch.Tensor:
    """[N][T][C] fp32 -> out[c][col0 + t*N + n] T (the data-gradient operand; row stride ldo; flip reverses the taps)."""
    n, t, c = w3d.shape
    if out is None:
        out = torch.empty((c, t, n), device=w3d.device, dtype=dtype)
        ldo = t * n
    call("vqa_pack_transpose", dt(dtype), ptr(w3d), ptr(out), n, t, c, ldo, col0, int(flip))
    return out


def c64p_blocks(B, H, W) -> int:
    return L.count("vqa_conv3x3_c64p_blocks", B, H, W)


def _c64p_sym(H, W, mode):
    """The symbol rocprofv3 prints for a vqa_conv3x3_c64p* launch: <output rows per block (conv_c64.hip c64p_rows), MODE 0 plain | 1 EPI | 2 BNRED>."""
    rbp = 8 if (H % 8 == 0 and 2 * 10 * (W + 2) * 128 + 3072 <= 160 * 1024) else 4
    return "conv3x3_c64p_kernel<%d, %d>" % (rbp, mode)


def conv3x3_c64p(x, w, B, H, W, *, want_stats=False, stats_acc=None):
    """bf16 3x3/1 conv, 64->64 channels, 8-wave LDS-DMA patch kernel (no epilogue inputs).  Returns (out, stats slab | None, blocks).
    stats_acc: a zeroed int64 [2*64 + 1] fixed-point accumulator that receives the BatchNorm sums instead of a slab."""
    nb = c64p_blocks(B, H, W)
    out = torch.empty((B * H * W, 64), device=x.device, dtype=torch.bfloat16)
    stats = torch.empty((nb, 2, 64), device=x.device, dtype=torch.float32) if (want_stats and stats_acc is None) else stats_acc
    e0 = prof_begin()
    call("vqa_conv3x3_c64p", ptr(x), ptr(w), ptr(out), ptr(stats), B, H, W, int(stats_acc is not None))
    if e0 is not None:
        prof_end(e0, _c64p_sym(H, W, 0), 2.0 * B * H * W * 64 * 576, 2 * B * H * W * 64 * 2)
    return out, stats, nb


def conv3x3_c64p_bnred(x, w, B, H, W, bn_y, bn_coef, bn_facc):
    """conv3x3_c64p (data gradient, w = the flipped pack) whose output is the gradient entering relu(BatchNorm(bn_y)): also adds that
    BatchNorm's backward column sums (sum g | sum g * xhat, g = out * [bn_y * scale + shift > 0]) to the zeroed accumulator bn_facc."""
    out = torch.empty((B * H * W, 64), device=x.device, dtype=torch.bfloat16)
    e0 = prof_begin()
    call("vqa_conv3x3_c64p_bnred", ptr(x), ptr(w), ptr(out), ptr(bn_y), ptr(bn_coef), ptr(bn_facc), B, H, W)
    if e0 is not None:
        prof_end(e0, _c64p_sym(H, W, 2), 2.0 * B * H * W * 64 * 576, 3 * B * H * W * 64 * 2)
    return out


def conv3x3_c64p_epi(x, w, B, H, W, *, addend, addmask=None, outmask=None):
    """Data gradient of a 64 -> 64 channel 3x3/1 conv (w = the flipped pack) with the residual block's identity path in the epilogue:
    (conv + addend * (addmask > 0)) * (outmask > 0) on the bf16 conv value (vqa_igemm's epilogue), 8-wave LDS-DMA patch kernel."""
    out = torch.empty((B * H * W, 64), device=x.device, dtype=torch.bfloat16)
    e0 = prof_begin()
    call("vqa_conv3x3_c64p_epi", ptr(x), ptr(w), ptr(out), ptr(addend), ptr(addmask), ptr(outmask), B, H, W)
    if e0 is not None:
        prof_end(e0, _c64p_sym(H, W, 1), 2.0 * B * H * W * 64 * 576, (3 + (addmask is not None) + (outmask is not None)) * B * H * W * 64 * 2)
    return out


def conv3x3_c64p_bn(y, acc, bn, w, B, H, W, count, *, want_stats=False, stats_acc=None, momentum=0.1, eps=1e-5):
    """conv3x3_c64p(relu(BatchNorm_train(y))) without the normalised tensor: y = the previous conv's raw output, acc = its fixed-point
    statistics, bn = (gamma, beta, running_mean, running_var, num_batches_tracked).  Returns (out, stats | None, blocks, coef [4][64])."""
    nb = c64p_blocks(B, H, W)
    out = torch.empty((B * H * W, 64), device=y.device, dtype=torch.bfloat16)
    coef = torch.empty((4, 64), device=y.device, dtype=torch.float32)
    stats = torch.empty((nb, 2, 64), device=y.device, dtype=torch.float32) if (want_stats and stats_acc is None) else stats_acc
    g, b_, rm, rv, nbt = bn
    e0 = prof_begin()
    call("vqa_conv3x3_c64p_bn", ptr(y), ptr(acc), ptr(g), ptr(b_), ptr(rm), ptr(rv), ptr(nbt), ptr(coef), ptr(w), ptr(out), ptr(stats), B, H, W,
         int(stats_acc is not None), float(count), momentum, eps)
    if e0 is not None:
        prof_end(e0, _c64p_sym(H, W, 0), 2.0 * B * H * W * 64 * 576, 2 * B * H * W * 64 * 2)
    return out, stats, nb, coef


def c64w_bn_ok(B, H, W) -> bool:
    return L.count("vqa_wgrad3x3_c64_bn_ok", B, H, W) > 0


def wgrad3x3_c64_bn(y, coef, dy, dw, B, H, W):
    """dw += dy^T gather(relu(y * coef[0] + coef[1])): weight gradient of the conv that conv3x3_c64p_bn ran (8-wave kernel)."""
    e0 = prof_begin()
    wsf = c64w_blocks(B, H, W) * 64 * 576
    ws = torch.empty(wsf, device=y.device, dtype=torch.float32)
    call("vqa_wgrad3x3_c64_bn", ptr(y), ptr(coef), ptr(dy), ptr(dw), B, H, W, ptr(ws), wsf)
    if e0 is not None:
        prof_end(e0, "wgrad3x3_c64", 2.0 * B * H * W * 64 * 576, 2 * B * H * W * 64 * 2)


def conv8p_ok(B, H, W, C, N) -> bool:
    return L.count("vqa_conv8p_ok", B, H, W, C, N) > 0


def conv8p(x, w, B, H, W, C, N, *, transposed=0, stride=1, stats_acc=None, out=None, addend=None, addmask=None, outmask=None, bnred=None):
    """3x3 / 1 / pad 1 conv (or its stride-1 data gradient) on the 8-phase 224(196) x 256 x 64 tile (csrc/gemm8p.hip).  bf16 NHWC."""
    if out is None:
        out = torch.empty((B * ((H - 1) // stride + 1) * ((W - 1) // stride + 1), N), device=x.device, dtype=torch.bfloat16)
    e0 = prof_begin()
    # fused BatchNorm-backward column sums of the stored tile: (y, coef, facc) with the ReLU mask recomputed from y, or
    # (y, coef, facc, False, y2 | None, coef2 | None) for an already masked tile (+ the shortcut BatchNorm sharing the gradient)
    bn_y, bn_coef, bn_facc, bn_self, bn_y2, bn_coef2 = (tuple(bnred) + (True, None, None))[:6] if bnred is not None else (None, None, None, True, None, None)
    call("vqa_conv8p", ptr(x), ptr(w), ptr(out), ptr(stats_acc), ptr(addend), ptr(addmask), ptr(outmask), ptr(bn_y), ptr(bn_coef), ptr(bn_facc),
         int(bool(bn_self)), ptr(bn_y2), ptr(bn_coef2),
         B, H, W, C, N, int(transposed), int(stride))
    if e0 is not None:
        sym = "conv8p_kernel<2, 4>" if N % 256 == 0 else "conv8p_kernel<4, 2>"      # the symbol rocprofv3 prints (the C dispatch: 256 | N)
        flops = 2.0 * out.shape[0] * N * 9 * C
        e1 = prof_end(e0, sym, flops,
                      (B * H * W * C + out.shape[0] * N * (1 + sum(t is not None for t in (addend, addmask, outmask, bn_y, bn_y2))) + N * 9 * C) * 2)
        # (the same symbol runs with and without epilogue inputs -- identity-path gradient / masks / the fused BatchNorm-backward sums:
        #  PROFILE_VARIANTS lets bench.py show the two groups of launches apart)
        PROFILE_VARIANTS.append((sym, "with epilogue inputs" if (addend is not None or outmask is not None or bnred is not None) else "plain",
                                 flops, e0, e1))
        # bytes the launch stages through LDS-DMA (tiles x K tiles x (tile rows + tile columns) x 128): what prices its K loop
        bmp, bn = (224, 256) if N % 256 == 0 else (448, 128)
        rpt = bmp * 7 // 8 if out.shape[0] % (bmp * 7 // 8) == 0 else bmp
        PROFILE_STAGED[sym] = PROFILE_STAGED.get(sym, 0) + (-(-out.shape[0] // rpt)) * (N // bn) * (9 * C // 64) * (bmp + bn) * 128
    return out


def c64w_blocks(B, H, W) -> int:
    """Slabs vqa_wgrad3x3_c64 wants (8-wave LDS-DMA kernel: 4 or 2 rows per block; else the 4-wave kernel); 0: unsupported shape."""
    return L.count("vqa_wgrad3x3_c64_blocks", B, H, W)


def wgrad3x3_c64(x, dy, dw, B, H, W):
    e0 = prof_begin()
    wsf = c64w_blocks(B, H, W) * 64 * 576                     # one partial dW per persistent workgroup, reduced in a fixed order
    ws = torch.empty(wsf, device=x.device, dtype=torch.float32)
    call("vqa_wgrad3x3_c64", ptr(x), ptr(dy), ptr(dw), B, H, W, ptr(ws), wsf)
    if e0 is not None:
        prof_end(e0, "wgrad3x3_c64", 2.0 * B * H * W * 64 * 576, 2 * B * H * W * 64 * 2)   # prefix of both kernels (4-wave / 8-wave DMA)


def c128_wgrad_blocks(B, H, W):
    return L.count("vqa_wgrad3x3_c128_blocks", B, H, W)


def wgrad3x3_c128(x, dy, dw, B, H, W):
    """Stage-2 shape (128 -> 128 channels, 28 x 28): 8-wave LDS-DMA weight-gradient kernel, per-workgroup slabs + fixed-order reduce."""
    e0 = prof_begin()
    wsf = c128_wgrad_blocks(B, H, W) * 128 * 576
    ws = torch.empty(wsf, device=x.device, dtype=torch.float32)
    call("vqa_wgrad3x3_c128", ptr(x), ptr(dy), ptr(dw), B, H, W, ptr(ws), wsf)
    if e0 is not None:
        prof_end(e0, "wgrad3x3_c128p_kernel", 2.0 * B * H * W * 128 * 1152, 2 * B * H * W * 128 * 2)


def dgrad_s2(dy, dyd, wt, B, H, W, C, Ho, Wo, N, R, pad, *, dtype):
    """Data gradient of a stride-2 conv (+ optional 1x1/2 shortcut) with rows grouped by parity class."""
    out = torch.empty((B * Ho * Wo, N), device=dy.device, dtype=dtype)
    e0 = prof_begin()
    call("vqa_dgrad_s2", dt(dtype), ptr(dy), ptr(dyd), ptr(wt), ptr(out), B, H, W, C, Ho, Wo, N, R, pad)
    if e0 is not None:
        flops = 2.0 * B * H * W * C * N * (R * R + (1 if dyd is not None else 0))
        prof_end(e0, f"igemm_kernel<{_tname(dtype)}, 128, {64 if N <= 64 else 128}, 2, 4, {_bk(dtype)}, 2, 2, 0>", flops,
                 (B * H * W * C * (2 if dyd is not None else 1) + B * Ho * Wo * N) * 2)
    return out


def is_byte_images(x) -> bool:
    """A ByteImages of the drop-in utils.byte_images, recognised by its members (that module can be imported under several names)."""
    return hasattr(x, "shape_nchw") and hasattr(x, "to_float") and hasattr(x, "mean") and hasattr(x, "std")


_U8_TABLES = {}


def u8_norm_table(device, mean, std):
    """The bf16 [3][256] table the *_u8 stem entries look bytes up in, built once per (device, mean, std) by vqa_u8_norm_table and
    kept: table[c][v] = bf16((v / 255 - mean[c]) / std[c])."""
    key = (str(device), tuple(mean), tuple(std))
    t = _U8_TABLES.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():          # (a table made inside a capture would live in that graph's pool)
            raise RuntimeError("u8_norm_table: the table of a new (mean, std) cannot be built while a HIP graph is being captured")
        t = torch.empty((3, 256), device=device, dtype=torch.bfloat16)
        call("vqa_u8_norm_table", *(float(v) for v in mean), *(float(v) for v in std), ptr(t))
        _U8_TABLES[key] = t
    return t


def _img_of(img):
    """(device pointer, norm-table pointer | None, bytes per element, entry / symbol suffix) of a stem kernel's image operand: the NCHW
    fp32 tensor, or a ByteImages (uint8 HWC and its table)."""
    if is_byte_images(img):
        return ptr(img.data), ptr(u8_norm_table(img.data.device, img.mean, img.std)), 1, "_u8"
    return ptr(img), None, 4, ""


def _img_device(img):
    return img.data.device if is_byte_images(img) else img.device


def stem_wgrad(img, dy, dw, B, H, W):
    """bf16 stem weight gradient: dw [64][7][7][3] fp32 += dy^T im2col(img).  img: NCHW fp32, or a ByteImages."""
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    ip, tab, esz, sfx = _img_of(img)
    e0 = prof_begin()
    ws, wsf = stem_wgrad_scratch(_img_device(img), B, H, W)
    call("vqa_stem_wgrad" + sfx, ip, ptr(dy), ptr(dw), B, H, W, ptr(ws), wsf, *(() if tab is None else (tab,)))
    if e0 is not None:
        prof_end(e0, f"stem_wgrad{sfx}_kernel<false>", 2.0 * B * Ho * Wo * 64 * 147, B * 3 * H * W * esz + B * Ho * Wo * 64 * 2)


def stem_wgrad_fused(img, y, dpool, idx, coef, bc, dw, B, H, W):
    """Fused stem BatchNorm/ReLU/MaxPool backward + weight gradient (vqa_stem_wgrad_fused): dy is rebuilt per row from y, dpool, idx,
    coef and bc and never written.  img: NCHW fp32, or a ByteImages."""
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    ip, tab, esz, sfx = _img_of(img)
    e0 = prof_begin()
    ws, wsf = stem_wgrad_scratch(dpool.device, B, H, W)
    call("vqa_stem_wgrad_fused" + sfx, ip, ptr(y), ptr(dpool), ptr(idx), ptr(coef), ptr(bc), ptr(dw), B, H, W, ptr(ws), wsf,
         *(() if tab is None else (tab,)))
    if e0 is not None:
        prof_end(e0, f"stem_wgrad{sfx}_kernel<true>", 2.0 * B * Ho * Wo * 64 * 147, B * 3 * H * W * esz + B * Ho * Wo * 64 * 2 + dpool.numel() * 3)


def stem_wgrad_scratch(device, B, H, W):
    """Scratch for the deterministic accumulation of the stem weight-gradient kernels: one [64][147] slab per workgroup."""
    wsf = L.count("vqa_stem_wgrad_blocks", B, H, W) * 64 * 147
    return torch.empty(wsf, device=device, dtype=torch.float32), wsf


def stem_dgrad_pack(w_krsc, dtype):
    """Packed [16][1024] operand of the stem data gradient (compute dtype) from the fp32 KRSC master [64][7][7][3]."""
    wpk = torch.empty(16 * 1024, device=w_krsc.device, dtype=dtype)
    call("vqa_stem_dgrad_pack", dt(dtype), ptr(w_krsc), ptr(wpk))
    return wpk


def stem_dgrad_fused_ok(B, H, W) -> bool:
    return L.count("vqa_stem_dgrad_fused_ok", B, H, W) > 0


def _stem_dgrad_cost(B, H, W):
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    return Ho, Wo, 2.0 * B * Ho * Wo * 64 * 147


def stem_dgrad(dy, wpk, B, H, W):
    """Image gradient NCHW fp32 [B][3][H][W] from a materialised dy [B*Ho*Wo, 64] (fp32 or bf16, vqa_stem_bwd_apply)."""
    dimg = torch.empty((B, 3, H, W), device=dy.device, dtype=torch.float32)
    Ho, Wo, flops = _stem_dgrad_cost(B, H, W)
    e0 = prof_begin()
    call("vqa_stem_dgrad", dt(dy), ptr(dy), ptr(wpk), ptr(dimg), B, H, W)
    if e0 is not None:
        prof_end(e0, f"stem_dgrad_kernel<{'bf16' if dy.dtype == torch.bfloat16 else 'f32'},false>", flops,
                 dy.numel() * dy.element_size() + dimg.numel() * 4)
    return dimg


def stem_dgrad_fused(y, dpool, idx, coef, bc, wpk, B, H, W):
    """Image gradient NCHW fp32 [B][3][H][W] with the stem BN/ReLU/MaxPool backward folded in: dy is rebuilt from y (bf16 raw conv
    output), dpool + idx (pooled gradient, argmax), coef and bc (BatchNorm backward coefficients) and never written."""
    dimg = torch.empty((B, 3, H, W), device=y.device, dtype=torch.float32)
    Ho, Wo, flops = _stem_dgrad_cost(B, H, W)
    e0 = prof_begin()
    call("vqa_stem_dgrad_fused", ptr(y), ptr(dpool), ptr(idx), ptr(coef), ptr(bc), ptr(wpk), ptr(dimg), B, H, W)
    if e0 is not None:
        prof_end(e0, "stem_dgrad_kernel<bf16,true>", flops, B * Ho * Wo * 64 * 2 + dpool.numel() * 3 + dimg.numel() * 4)
    return dimg


def stem_conv_blocks(B, H, W) -> int:
    return L.count("vqa_stem_conv_blocks", B, H, W)


def stem_conv(img, wstem, B, H, W, want_stats):
    """bf16 stem conv 7x7/2 from the NCHW fp32 image, or from a ByteImages.  Returns (y [B*Ho*Wo, 64] bf16, stats slab | None, blocks)."""
    nb = stem_conv_blocks(B, H, W)
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    ip, tab, esz, sfx = _img_of(img)
    dev = _img_device(img)
    y = torch.empty((B * Ho * Wo, 64), device=dev, dtype=torch.bfloat16)
    stats = torch.empty((nb, 2, 64), device=dev, dtype=torch.float32) if want_stats else None
    e0 = prof_begin()
    call("vqa_stem_conv" + sfx, ip, ptr(wstem), ptr(y), ptr(stats), B, H, W, *(() if tab is None else (tab,)))
    if e0 is not None:
        prof_end(e0, f"stem_conv{sfx}_kernel", 2.0 * B * Ho * Wo * 64 * 147, B * 3 * H * W * esz + B * Ho * Wo * 64 * 2)
    return y, stats, nb


def stem_conv_pool(img, wstem, coef, B, H, W):
    """Inference stem in one launch: conv7x7/2 + BatchNorm (running statistics) + ReLU + MaxPool3x3/2 from the NCHW fp32 image or a ByteImages.
    Returns the pooled activation [B*Hp*Wp, 64] bf16, or None when the shape is not supported (the caller takes the two-kernel path)."""
    if not L.count("vqa_stem_conv_pool_ok", B, H, W):
        return None
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    Hp, Wp = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
    ip, tab, esz, sfx = _img_of(img)
    x = torch.empty((B * Hp * Wp, 64), device=_img_device(img), dtype=torch.bfloat16)
    e0 = prof_begin()
    call("vqa_stem_conv_pool" + sfx, ip, ptr(wstem), ptr(coef), ptr(x), B, H, W, *(() if tab is None else (tab,)))
    if e0 is not None:
        prof_end(e0, f"stem_conv_pool{sfx}_kernel", 2.0 * B * Ho * Wo * 64 * 147, B * 3 * H * W * esz + B * Hp * Wp * 64 * 2)
    return x


def igemm(a, w, M, N, Kw, geom, *, dtype, loader=LOADER_NHWC, bias=None, addend=None, addmask=None, outmask=None, want_stats=False,
          transposed=0, relu=0, drop_p=0.0, drop_seed=0, out=None, stats_acc=None):
    """out[M][N] = gather(a) @ w[N][Kw]^T with the fused epilogue.  geom = (B, H, W, C, Ho, Wo, R, S, stride, pad).
    Returns (out, stats_slab | None, mtiles).  stats_acc: a zeroed int64 [2*N + 1] fixed-point accumulator that receives the
    BatchNorm sums instead of a slab (returned in the slab's place, mtiles = 0)."""
    B, H, W, C, Ho, Wo, R, S, stride, pad = geom
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=dtype)
    stats, mt = stats_acc, 0
    if want_stats and stats_acc is None:
        mt = L.count("vqa_igemm_mtiles", M, N, loader)
        stats = torch.empty((mt, 2, N), device=a.device, dtype=torch.float32)
    e0 = prof_begin()
    call("vqa_igemm", dt(dtype), loader, ptr(a), ptr(w), ptr(out), ptr(bias), ptr(addend), ptr(addmask), ptr(outmask), ptr(stats),
         M, N, Kw, B, H, W, C, Ho, Wo, R, S, stride, pad, transposed, relu, float(drop_p), int(drop_seed), int(stats_acc is not None))
    if e0 is not None:
        var = igemm_variant(dtype, loader, M, N, Kw, geom)
        kreal = 147 if loader == LOADER_STEM else Kw
        flops = 2.0 * B * H * W * C * R * S * N if transposed else 2.0 * M * N * kreal
        es = 2 if dtype == torch.bfloat16 else 4
        nbytes = (B * H * W * C * (4 if loader == LOADER_STEM else es)) + (M * N + N * Kw) * es
        prof_end(e0, igemm_symbol(dtype, loader, var), flops, nbytes)
    return out, stats, mt


def mx_quant(x: torch.Tensor, out=None):
    """MXFP8 copy of a bf16 / fp32 [M][C] tensor (C % 32 == 0): (e4m3 codes uint8 [M][C], E8M0 scale codes uint8 [M][C/32]).
    The quantization rule is csrc/mxfp8.hip's (one scale per 32 consecutive elements of a row)."""
    M, C = x.shape
    q, s = out if out is not None else (torch.empty((M, C), device=x.device, dtype=torch.uint8),
                                        torch.empty((M, C // 32), device=x.device, dtype=torch.uint8))
    call("vqa_mx_quant", dt(x), ptr(x), ptr(q), ptr(s), M, C)
    return q, s


def fold_bn_mxfp8(flat, wq, ws, bias, table, nd, blocks, eps=1e-5):
    """Eval Conv+BN fold of the pieces in `table` (vqa_fold_bn_batch's descriptor table) quantized to MXFP8: codes into wq, scales
    into ws (at dst_off / 32), fp32 bias into bias.  Every piece needs dst_off % 32 == 0 and K % 32 == 0 (checked here when `table`
    is still on the host; a device table is the caller's word -- the kernel leaves a piece that breaks it unwritten)."""
    if not table.is_cuda:
        t = table.view(-1, 10)
        if bool(((t[:, 7] % 32) != 0).any()) or bool(((t[:, 6] % 32) != 0).any()):
            raise ValueError("fold_bn_mxfp8: every piece needs dst_off % 32 == 0 and K % 32 == 0")
        table = t.to(wq.device)
    call("vqa_fold_bn_mxfp8", ptr(flat), ptr(wq), ptr(ws), ptr(bias), ptr(table), nd, blocks, float(eps))


def conv_mxfp8(xq, w, M, N, geom, *, bias=None, addend=None, relu=0, want_bf16=True, want_mx=False):
    """NHWC conv of the MXFP8 activation xq = (codes [B*H*W][C], scales [B*H*W][C/32]) with the MXFP8 weight w = (codes [N][R*S*C],
    scales [N][R*S*C/32]); vqa_igemm's epilogue (bias, relu 1 before / 2 after the bf16 addend).  geom = (B, H, W, C, Ho, Wo, R, S,
    stride, pad).  Returns (bf16 out [M][N] | None, its MXFP8 copy (codes, scales) | None)."""
    B, H, W, C, Ho, Wo, R, S, stride, pad = geom
    dev = xq[0].device
    out = torch.empty((M, N), device=dev, dtype=torch.bfloat16) if want_bf16 else None
    oq = (torch.empty((M, N), device=dev, dtype=torch.uint8), torch.empty((M, N // 32), device=dev, dtype=torch.uint8)) if want_mx else (None, None)
    e0 = prof_begin()
    call("vqa_conv_mxfp8", ptr(xq[0]), ptr(xq[1]), ptr(w[0]), ptr(w[1]), ptr(bias), ptr(addend), ptr(out), ptr(oq[0]), ptr(oq[1]),
         M, N, B, H, W, C, Ho, Wo, R, S, stride, pad, relu)
    if e0 is not None:
        nbytes = B * H * W * C * 33 // 32 + N * R * S * C * 33 // 32 + M * N * (2 * int(want_bf16) + 2 * int(addend is not None))
        prof_end(e0, f"conv_mxfp8_kernel<{128 if N % 128 == 0 else 64}>", 2.0 * M * N * R * S * C, nbytes)
    return out, (oq if want_mx else None)


def linear_dgrad_act(dz, wt, M, Kin, N, *, dtype, outact, drop_p, addend=None):
    """dx[M][Kin] = (dz[M][N] @ wt[Kin][N]^T + addend) * (outact > 0) / (1 - drop_p): a Linear's data gradient that leaves with the ReLU(+dropout)
    mask of the layer in front applied (vqa_linear_dgrad_act; bit-equal to igemm followed by vqa_bias_act_bwd)."""
    dx = torch.empty((M, Kin), device=dz.device, dtype=dtype)
    e0 = prof_begin()
    call("vqa_linear_dgrad_act", dt(dtype), ptr(dz), ptr(wt), ptr(dx), ptr(addend), ptr(outact), float(drop_p), M, Kin, N)
    if e0 is not None:
        var = igemm_variant(dtype, LOADER_NHWC, M, Kin, N, linear_geom(M, N))
        es = 2 if dtype == torch.bfloat16 else 4
        prof_end(e0, igemm_symbol(dtype, LOADER_NHWC, var), 2.0 * M * N * Kin, (M * N + 2 * M * Kin + N * Kin) * es)
    return dx


_PLAN_CACHE = {}


def wgrad_plan(dtype, loader, M, N, Kw, B, H, W, C, R, S):
    """(kind, tile_n, tile_k, nsplit, workspace floats) of vqa_wgrad for this problem; kind 1: the 8-wave LDS-DMA kernel."""
    key = (dtype, loader, M, N, Kw, B, H, W, C, R, S)
    pl = _PLAN_CACHE.get(key)
    if pl is None:
        import ctypes as C_
        wsf, kind, tn, tk, ns = C_.c_longlong(0), C_.c_int(0), C_.c_int(0), C_.c_int(0), C_.c_int(0)
        L.lib().vqa_wgrad_plan(dt(dtype), loader, M, N, Kw, B, H, W, C, R, S, C_.byref(wsf), C_.byref(kind), C_.byref(tn), C_.byref(tk),
                               C_.byref(ns))
        pl = _PLAN_CACHE[key] = (kind.value, tn.value, tk.value, ns.value, wsf.value)
    return pl


def wgrad(dy, x, dw, M, N, Kw, geom, *, dtype, loader=LOADER_NHWC):
    """dw[N][Kw] (fp32) += dy[M][N]^T @ gather(x)[M][Kw]: deterministic two-pass split (workspace slabs + fixed-order reduce)."""
    B, H, W, C, Ho, Wo, R, S, stride, pad = geom
    kind, tn, tk, nsplit, wsf = wgrad_plan(dtype, loader, M, N, Kw, B, H, W, C, R, S)
    ws = torch.empty(wsf, device=dy.device, dtype=torch.float32) if wsf else None       # torch's caching allocator, stream-ordered
    e0 = prof_begin()
    call("vqa_wgrad", dt(dtype), loader, ptr(dy), ptr(x), ptr(dw), M, N, Kw, B, H, W, C, Ho, Wo, R, S, stride, pad, ptr(ws), wsf)
    if e0 is not None:
        es = 2 if dtype == torch.bfloat16 else 4
        name = f"wgrad_dma_kernel<{tn}, {tk}, 2>" if kind else f"wgrad_kernel<{_tname(dtype)}, {tn}, {tk}, {loader}>"     # (timing includes the reduce launch)
        prof_end(e0, name, 2.0 * M * N * Kw, (M * N + B * H * W * C) * es + N * Kw * 4)


_GROUP_OK = {}


def wgrad_group_ok(dtype, M, N, Kw):
    """True when vqa_wgrad_group takes this Linear weight gradient (the planner's 4-wave 128x128 split kernel)."""
    key = (dtype, M, N, Kw)
    v = _GROUP_OK.get(key)
    if v is None:
        import ctypes as C_
        one = lambda a: (C_.c_int * 1)(a)
        v = _GROUP_OK[key] = L.count("vqa_wgrad_group_ws", dt(dtype), 1, one(M), one(N), one(Kw)) >= 0
    return v


def wgrad_group(jobs, *, dtype):
    """jobs: up to 8 tuples (dy [M][N], x [M][Kw], dw fp32 [N][Kw] (+=), M, N, Kw) -> one launch + one fixed-order reduce launch;
    every dw is bit-identical to its own wgrad() call."""
    import ctypes as C_
    n = len(jobs)
    VP, IA = C_.c_void_p * n, C_.c_int * n
    dy, x, dw = VP(*[j[0].data_ptr() for j in jobs]), VP(*[j[1].data_ptr() for j in jobs]), VP(*[j[2].data_ptr() for j in jobs])
    Ms, Ns, Ks = IA(*[j[3] for j in jobs]), IA(*[j[4] for j in jobs]), IA(*[j[5] for j in jobs])
    wsf = L.count("vqa_wgrad_group_ws", dt(dtype), n, Ms, Ns, Ks)
    if wsf < 0:
        raise RuntimeError("wgrad_group: a job does not qualify (check wgrad_group_ok first)")
    ws = torch.empty(wsf, device=jobs[0][0].device, dtype=torch.float32) if wsf else None
    e0 = prof_begin()
    call("vqa_wgrad_group", dt(dtype), n, dy, x, dw, Ms, Ns, Ks, ptr(ws), wsf)
    if e0 is not None:
        es = 2 if dtype == torch.bfloat16 else 4
        prof_end(e0, f"wgrad_group_kernel<{_tname(dtype)}, 128, 128, 0>", sum(2.0 * j[3] * j[4] * j[5] for j in jobs),
                 sum((j[3] * j[4] + j[3] * j[5]) * es + j[4] * j[5] * 4 for j in jobs))


def linear_geom(M, K):
    return (M, 1, 1, K, 1, 1, 1, 1, 1, 0)


# ----------------------------------------------------------------------------------------------
# BatchNorm
# ----------------------------------------------------------------------------------------------
def bn_train_coef(stats, mtiles, C, count, gamma, beta, rm, rv, nbt, momentum=0.1, eps=1e-5):
    scratch = torch.empty((64 * 2 * C,), device=stats.device, dtype=torch.float64)
    coef = torch.empty((4, C), device=stats.device, dtype=torch.float32)
    call("vqa_bn_stats_finalize", ptr(stats), mtiles, C, float(count), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt),
         momentum, eps, ptr(scratch), ptr(coef))
    return coef


def bn_eval_coef(C, gamma, beta, rm, rv, eps=1e-5):
    coef = torch.empty((4, C), device=gamma.device, dtype=torch.float32)
    call("vqa_bn_eval_coef", C, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), eps, ptr(coef))
    return coef


def bn_apply(y, coef, C, relu, res=None, rcoef=None):
    out = torch.empty_like(y)
    call("vqa_bn_apply", dt(y), ptr(y), ptr(coef), ptr(res), ptr(rcoef), ptr(out), y.numel(), C, int(relu))
    return out


def bn_apply_acc(y, acc, bn, C, relu, B, HW, count, *, res=None, racc=None, rbn=None, pool=False, momentum=0.1, eps=1e-5):
    """Train-mode BatchNorm apply with the statistics finalize folded in (vqa_bn_apply_acc).  bn / rbn = (gamma, beta, running_mean,
    running_var, num_batches_tracked).  Returns (out, coef [4][C], rcoef | None, pool part | None, chunks)."""
    out = torch.empty_like(y)
    coef = torch.empty((4, C), device=y.device, dtype=torch.float32)
    rcoef = torch.empty((4, C), device=y.device, dtype=torch.float32) if racc is not None else None
    part, chunks = None, 0
    if pool:
        chunks = L.count("vqa_bn_apply_pool_chunks", dt(y), HW, C)
        part = torch.empty((B, chunks, C), device=y.device, dtype=torch.float32)
    g, b_, rm, rv, nbt = bn
    rg, rb, rrm, rrv, rnbt = rbn if rbn is not None else (None,) * 5
    call("vqa_bn_apply_acc", dt(y), ptr(y), ptr(acc), ptr(g), ptr(b_), ptr(rm), ptr(rv), ptr(nbt), ptr(coef), ptr(res), ptr(racc), ptr(rg), ptr(rb),
         ptr(rrm), ptr(rrv), ptr(rnbt), ptr(rcoef), ptr(out), B, HW, C, int(relu), float(count), momentum, eps, ptr(part))
    return out, coef, rcoef, part, chunks


def bn_apply_pool(y, coef, C, relu, B, HW, res=None, rcoef=None):
    """bn_apply of a stage's last block that also leaves the SE pooling sums: returns (out, part [B][chunks][C], chunks)."""
    out = torch.empty_like(y)
    chunks = L.count("vqa_bn_apply_pool_chunks", dt(y), HW, C)
    part = torch.empty((B, chunks, C), device=y.device, dtype=torch.float32)
    call("vqa_bn_apply_pool", dt(y), ptr(y), ptr(coef), ptr(res), ptr(rcoef), ptr(out), B, HW, C, int(relu), ptr(part))
    return out, part, chunks


def bn_bwd(dout, outact, y, coef, gamma, C, training, dgamma, dbeta, y2=None, coef2=None, gamma2=None, dgamma2=None, dbeta2=None,
           self_mask=False, slab=None, nb=0, facc=None, facc_filled=False):
    """BatchNorm backward for g = dout*(outact>0); optional second BN (1x1 shortcut) sharing g.
    self_mask: the ReLU directly follows this BN (no residual), so the mask relu(bn(y)) > 0 is recomputed from y and the
    activation tensor is not read at all (pass outact=None).  Returns dy (and dy2)."""
    rows = y.numel() // C
    if facc is not None:       # fixed-point accumulators + finalize folded into the apply pass (training mode, bf16 schedule)
        if not facc_filled:
            call("vqa_bn_bwd_reduce", dt(y), ptr(dout), ptr(outact), ptr(y), ptr(coef), ptr(y2), ptr(coef2), ptr(facc), rows, C, int(self_mask), 1)
        dy = torch.empty_like(y)
        dy2 = torch.empty_like(y2) if y2 is not None else None
        call("vqa_bn_bwd_apply_acc", dt(y), ptr(dout), ptr(outact), ptr(y), ptr(facc), ptr(gamma), ptr(coef), ptr(dgamma), ptr(dbeta), ptr(dy),
             ptr(y2), ptr(gamma2), ptr(coef2), ptr(dgamma2), ptr(dbeta2), ptr(dy2), y.numel(), C, float(rows), int(self_mask))
        return dy, dy2
    if slab is None:           # (else: the caller already reduced the column sums)
        nb = L.count("vqa_bn_bwd_blocks", rows)
        slab = torch.empty((nb, 3, C), device=y.device, dtype=torch.float32)
        call("vqa_bn_bwd_reduce", dt(y), ptr(dout), ptr(outact), ptr(y), ptr(coef), ptr(y2), ptr(coef2), ptr(slab), rows, C, int(self_mask), 0)
    bc = torch.empty((3, C), device=y.device, dtype=torch.float32)
    call("vqa_bn_bwd_finalize", ptr(slab), nb, C, 1, float(rows), ptr(gamma), ptr(coef), int(training), ptr(dgamma), ptr(dbeta), ptr(bc))
    dy = torch.empty_like(y)
    dy2 = bc2 = None
    if y2 is not None:
        bc2 = torch.empty((3, C), device=y.device, dtype=torch.float32)
        call("vqa_bn_bwd_finalize", ptr(slab), nb, C, 2, float(rows), ptr(gamma2), ptr(coef2), int(training), ptr(dgamma2), ptr(dbeta2), ptr(bc2))
        dy2 = torch.empty_like(y2)
    call("vqa_bn_bwd_apply", dt(y), ptr(dout), ptr(outact), ptr(y), ptr(bc), ptr(dy), ptr(y2), ptr(bc2), ptr(dy2), y.numel(), C,
         ptr(coef) if self_mask else None)
    return dy, dy2


# ----------------------------------------------------------------------------------------------
# token side helpers
# ----------------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, *, eps=1e-5, drop_p=0.0, seed=0, addrow=None, period=1):
    rows, D = x.shape
    out = torch.empty_like(x)
    stats = torch.empty((rows, 2), device=x.device, dtype=torch.float32)
    call("vqa_layernorm_fwd", dt(x), ptr(x), ptr(gamma), ptr(beta), ptr(out), ptr(stats), rows, D, eps, float(drop_p), int(seed),
         ptr(addrow), period)
    return out, stats


_WS_CACHE = {}


def reduce_ws(name, *args):
    """Scratch floats of a fixed-order reduction entry (vqa_layernorm_bwd_ws / vqa_bias_act_bwd_ws), cached by shape."""
    key = (name,) + args
    v = _WS_CACHE.get(key)
    if v is None:
        v = _WS_CACHE[key] = int(L.count(name, *args))
    return v


_FOLD_DESC = {}


def ln_bwd_folds(dtype, rows, D, period):
    """[(ws offset, rows, stride, columns, n0), ...] of a deferred vqa_layernorm_bwd (cached by shape)."""
    key = (dtype, rows, D, period)
    v = _FOLD_DESC.get(key)
    if v is None:
        import ctypes as C_
        out = (C_.c_longlong * 10)()
        n = L.count("vqa_layernorm_bwd_folds", dt(dtype), rows, D, period, out)
        v = _FOLD_DESC[key] = [tuple(int(out[5 * i + k]) for k in range(5)) for i in range(n)]
    return v


def fold_group(jobs):
    """jobs: (part tensor, element offset, rows, stride, columns, dst0, n0, dst1 | None): the deferred folds of LayerNorm / bias backward
    calls, one launch per 48 jobs; each job keeps its scratch tensor alive until here."""
    import ctypes as C_
    n = len(jobs)
    if not n:
        return
    VP, IA, LA = C_.c_void_p * n, C_.c_int * n, C_.c_longlong * n
    call("vqa_fold_group", n, VP(*[j[0].data_ptr() + 4 * j[1] for j in jobs]), IA(*[j[2] for j in jobs]), LA(*[j[3] for j in jobs]),
         IA(*[j[4] for j in jobs]), VP(*[j[5].data_ptr() for j in jobs]), IA(*[j[6] for j in jobs]),
         VP(*[(j[7].data_ptr() if j[7] is not None else None) for j in jobs]))


def layernorm_bwd(dout, x, gamma, stats, dgamma, dbeta, *, addend=None, drop_p=0.0, seed=0, dadd=None, period=1, fixed_order=True, foldq=None):
    """fixed_order: dgamma / dbeta / dadd are summed through per-workgroup partial rows + an index-order fold (bit-reproducible);
    False -> float atomics.  foldq (a list): the folds are not launched here but appended as fold_group() jobs."""
    rows, D = x.shape
    dx = torch.empty_like(x)
    ws = None
    per = period if dadd is not None else 0
    if fixed_order:
        ws = torch.empty((reduce_ws("vqa_layernorm_bwd_ws", dt(x), rows, D, per),), device=x.device, dtype=torch.float32)
    defer = int(foldq is not None and ws is not None)
    call("vqa_layernorm_bwd", dt(x), ptr(dout), ptr(x), ptr(gamma), ptr(stats), ptr(addend), ptr(dx), ptr(dgamma), ptr(dbeta),
         rows, D, float(drop_p), int(seed), ptr(dadd), period, ptr(ws), defer)
    if defer:
        folds = ln_bwd_folds(x.dtype, rows, D, per)
        off, nr, st, nc, n0 = folds[0]
        foldq.append((ws, off, nr, st, nc, dgamma, n0, dbeta))
        if len(folds) > 1:
            off, nr, st, nc, n0 = folds[1]
            foldq.append((ws, off, nr, st, nc, dadd, n0, None))
    return dx


STATS_CHUNK = 8192           # VQA_STATS_CHUNK of include/vqa_hip.h: elements one workgroup of vqa_tensor_stats reduces
STATS_MAX_ROWS = 4096
_STATS_SCRATCH = {}          # device -> fp32 scratch of vqa_tensor_stats (four words per chunk), grown on demand


class StatsTable(tuple):
    """(device table int64 [P][3] of {lo, hi, first_chunk}, P, chunks) as stats_table() returns it; `extent` is the largest hi, so
    that tensor_stats() can refuse a buffer the table reaches beyond."""
    extent = 0


def stats_rows(ranges):
    """Host half of stats_table: ([[lo, hi, first_chunk], ...] in the given order, chunks).  ValueError for an empty range, a lo that
    is negative or no multiple of 4, ranges that overlap, no range at all or more than 4096."""
    ranges = [(int(lo), int(hi)) for lo, hi in ranges]
    if not 1 <= len(ranges) <= STATS_MAX_ROWS:
        raise ValueError(f"stats_table: between 1 and {STATS_MAX_ROWS} ranges, got {len(ranges)}")
    for lo, hi in ranges:
        if hi <= lo:
            raise ValueError(f"stats_table: empty range [{lo}, {hi})")
        if lo < 0 or lo % 4:
            raise ValueError(f"stats_table: range [{lo}, {hi}) must start at a non-negative multiple of 4 elements")
    ordered = sorted(ranges)
    for (_, hi0), (lo1, hi1) in zip(ordered, ordered[1:]):
        if lo1 < hi0:
            raise ValueError(f"stats_table: range [{lo1}, {hi1}) overlaps the range that ends at {hi0}")
    rows, chunks = [], 0
    for lo, hi in ranges:
        rows.append([lo, hi, chunks])
        chunks += (hi - lo + STATS_CHUNK - 1) // STATS_CHUNK
    return rows, chunks


def stats_table(ranges, device="cuda"):
    """The table vqa_tensor_stats reads, from (lo, hi) pairs on the host: a StatsTable (device table, P, chunks).  One row per range,
    in the given order; ValueError as stats_rows.  The copy goes out from pinned memory without a sync when `device` is a GPU."""
    rows, chunks = stats_rows(ranges)
    t = torch.tensor(rows, dtype=torch.int64)
    if torch.device(device).type == "cuda":
        t = t.pin_memory().to(device, non_blocking=True)
    out = StatsTable((t, len(rows), chunks))
    out.extent = max(r[1] for r in rows)
    return out


def tensor_stats(x, table, y=None, out=None):
    """Per-range {sumsq f32, absmax f32, nonfinite u32, zeros u32} of the flat fp32 buffer x -- of x - y when y is given -- as an
    int32 [P][4] device tensor (vqa_tensor_stats: two launches on the current stream, no host sync; view columns 0 and 1 as float32).
    table: a StatsTable of stats_table() on x's device.  out: an int32 [P][4] contiguous tensor to write into (a slot of a ring)."""
    tab, P, chunks = table
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous()):
        raise ValueError("tensor_stats: x must be a contiguous flat fp32 buffer on the GPU (there is no CPU path)")
    if tab.device != x.device:
        raise ValueError(f"tensor_stats: the table lives on {tab.device}, x on {x.device}")
    if x.numel() < table.extent:
        raise ValueError(f"tensor_stats: the table reaches element {table.extent}, x has {x.numel()}")
    if y is not None and not (y.dtype == torch.float32 and y.shape == x.shape and y.device == x.device and y.is_contiguous()):
        raise ValueError("tensor_stats: y must be a contiguous fp32 buffer of x's size on x's device")
    if out is None:
        out = torch.empty((P, 4), device=x.device, dtype=torch.int32)
    elif tuple(out.shape) != (P, 4) or out.dtype != torch.int32 or out.device != x.device or not out.is_contiguous():
        raise ValueError(f"tensor_stats: out must be a contiguous int32 tensor of shape ({P}, 4) on {x.device}")
    scratch = _STATS_SCRATCH.get(x.device)
    if scratch is None or scratch.numel() < 4 * chunks:
        scratch = _STATS_SCRATCH[x.device] = torch.empty((4 * chunks,), device=x.device, dtype=torch.float32)
    call("vqa_tensor_stats", ptr(x), ptr(y), ptr(tab), P, chunks, ptr(out), ptr(scratch))
    return out


def gather_rows(src, index, out=None):
    """out[i] = src[index[i]] along the first dimension, one launch (vqa_gather_rows).  src: contiguous [n_src, ...] of any dtype whose
    rows are a multiple of 16 bytes; index: contiguous int32 [n] on src's device with every entry in [0, n_src) -- the CALLER checks the
    range (ImageFeatures.select does), the kernel only refuses to read outside src.  Returns [n, ...] in src's dtype."""
    if src.dim() < 1 or not src.is_contiguous():
        raise ValueError("gather_rows: src must be contiguous with at least one dimension")
    if index.dtype != torch.int32 or index.dim() != 1 or index.device != src.device or not index.is_contiguous():
        raise ValueError(f"gather_rows: index must be a contiguous int32 vector on {src.device}")
    n, n_src = index.shape[0], src.shape[0]
    row_bytes = (src.numel() // n_src if n_src else 0) * src.element_size()
    if n and (row_bytes <= 0 or row_bytes % 16):
        raise ValueError(f"gather_rows: rows of {row_bytes} bytes; a positive multiple of 16 is needed")
    shape = (n,) + tuple(src.shape[1:])
    if out is None:
        out = torch.empty(shape, device=src.device, dtype=src.dtype)
    elif tuple(out.shape) != shape or out.dtype != src.dtype or out.device != src.device or not out.is_contiguous():
        raise ValueError(f"gather_rows: out must be a contiguous {src.dtype} tensor of shape {shape} on {src.device}")
    if n:
        call("vqa_gather_rows", ptr(src), ptr(index), ptr(out), n, row_bytes, n_src)
    return out


def softmax_topk(logits, k, allowed=None, scale=1.0, want_logits=False):
    """The k best columns of every row of logits [B][N] (fp32 or bf16, unit column stride, any row stride >= N) with their softmax
    probabilities, one launch (vqa_softmax_topk).  allowed: bool / uint8 [N] (shared) or [B][N], non-zero = the column may be picked
    (the others count as -inf); scale = 1 / temperature.  Order: value descending, ties and NaNs (which rank first) by index -- a
    stable descending sort.  Returns (indices int64 [B][k], probs fp32 [B][k], fp32 copy of the raw logits [B][N] | None)."""
    B, N = logits.shape
    if logits.stride(1) != 1 and N > 1:
        raise ValueError("softmax_topk: logits need a unit column stride")
    ld = logits.stride(0) if B > 1 else max(logits.stride(0), N)
    ald = 0
    if allowed is not None:
        if allowed.dtype not in (torch.bool, torch.uint8) or tuple(allowed.shape) not in ((N,), (B, N)) or allowed.device != logits.device:
            raise ValueError(f"softmax_topk: allowed must be bool / uint8 [{N}] or [{B}, {N}] on {logits.device}")
        allowed = allowed.contiguous()
        if allowed.dtype == torch.bool:
            allowed = allowed.view(torch.uint8)
        ald = N if allowed.dim() == 2 else 0
    idx = torch.empty((B, k), device=logits.device, dtype=torch.int64)
    probs = torch.empty((B, k), device=logits.device, dtype=torch.float32)
    lf = torch.empty((B, N), device=logits.device, dtype=torch.float32) if want_logits else None
    call("vqa_softmax_topk", dt(logits), ptr(logits), ld, ptr(allowed), ald, float(scale), ptr(idx), ptr(probs), ptr(lf), B, N, int(k))
    return idx, probs, lf


def cross_entropy_opts(logits, targets, *, class_weight=None, ignore_index=None, label_smoothing=0.0, loss=None, need_grad=True,
                       logits_f32=None, gscale=1.0, err=None, fixed_order=True, acc=None, empty=None):
    """F.cross_entropy(logits, targets, weight=class_weight, ignore_index=, label_smoothing=, reduction="mean") and its gradient in one
    launch (vqa_cross_entropy_opts; include/vqa_hip.h has the formulas and the W == 0 rule).  logits [B][N] fp32 or bf16, contiguous;
    targets int64 [B]; class_weight fp32 [N] on the device or None; ignore_index None: no target is ignored.
    loss (fp32, one element) is accumulated into and created zeroed when None; err / empty: int32 device counters (+=) or None;
    acc: VQAAccuracy's three int64 counters or None; logits_f32: an fp32 [B][N] tensor to fill or None.
    fixed_order: the row terms are folded in row order (bit-reproducible); False -> float atomics on the loss.
    Returns (loss, dlogits in the dtype of logits | None)."""
    B, N = logits.shape
    if not logits.is_contiguous() or targets.dtype != torch.int64 or tuple(targets.shape) != (B,) or not targets.is_contiguous():
        raise ValueError("cross_entropy_opts: contiguous logits [B, N] and contiguous int64 targets [B] expected")
    if class_weight is not None and (class_weight.dtype != torch.float32 or tuple(class_weight.shape) != (N,)
                                     or class_weight.device != logits.device or not class_weight.is_contiguous()):
        raise ValueError(f"cross_entropy_opts: class_weight must be a contiguous fp32 [{N}] tensor on {logits.device}")
    if loss is None:
        loss = torch.zeros((), device=logits.device, dtype=torch.float32)
    dlogits = torch.empty_like(logits) if need_grad else None
    ws = torch.empty((B,), device=logits.device, dtype=torch.float32) if fixed_order else None
    call("vqa_cross_entropy_opts", dt(logits), ptr(logits), ptr(targets), ptr(loss), ptr(dlogits), ptr(logits_f32), B, N, float(gscale),
         ptr(err), ptr(ws), ptr(class_weight), 0 if ignore_index is None else int(ignore_index), int(ignore_index is not None),
         float(label_smoothing), ptr(acc), ptr(empty))
    return loss, dlogits


# ----------------------------------------------------------------------------------------------
# explaining an answer (csrc/explain_ops.hip; include/vqa_hip.h has the formulas)
# ----------------------------------------------------------------------------------------------
def class_seed(logits, ids=None):
    """The class to explain per row of logits [B][N] (fp32 or bf16, unit column stride, any row stride >= N) and the one-hot seed of its
    backward, one launch (vqa_class_seed).  ids: int64 [B] on the device (the caller checks the range), or None for the row's arg-max in
    softmax_topk's order (ties to the lower index, a NaN first).  Returns (chosen int64 [B], dlogits [B][N] in the dtype of logits)."""
    B, N = logits.shape
    if logits.stride(1) != 1 and N > 1:
        raise ValueError("class_seed: logits need a unit column stride")
    ld = logits.stride(0) if B > 1 else max(logits.stride(0), N)
    if ids is not None and (ids.dtype != torch.int64 or tuple(ids.shape) != (B,) or ids.device != logits.device or not ids.is_contiguous()):
        raise ValueError(f"class_seed: ids must be a contiguous int64 [{B}] tensor on {logits.device}")
    chosen = torch.empty((B,), device=logits.device, dtype=torch.int64)
    dlogits = torch.empty((B, N), device=logits.device, dtype=logits.dtype)
    call("vqa_class_seed", dt(logits), ptr(logits), ld, ptr(ids), ptr(chosen), ptr(dlogits), B, N)
    return chosen, dlogits


def gradcam(feat, dfeat, B, P, C, normalize=True):
    """Grad-CAM of the NHWC features: feat, dfeat [B][P][C] (any shape with B * P * C elements, contiguous, one dtype: fp32 or bf16)
    -> fp32 [B][P] = max(0, sum_c mean_p(dfeat)[c] * feat[p][c]), divided by its row maximum when normalize (vqa_gradcam)."""
    if feat.dtype != dfeat.dtype or feat.numel() != B * P * C or dfeat.numel() != B * P * C or not (feat.is_contiguous() and dfeat.is_contiguous()):
        raise ValueError(f"gradcam: feat and dfeat must be contiguous tensors of {B} x {P} x {C} elements in one dtype")
    cam = torch.empty((B, P), device=feat.device, dtype=torch.float32)
    call("vqa_gradcam", dt(feat), ptr(feat), ptr(dfeat), ptr(cam), B, P, C, int(bool(normalize)))
    return cam


def attention_map(caw, maskf=None, normalize=True):
    """Mean of the cross-attention probabilities caw fp32 [ncl][B][H][L][P] over layers, heads and the real tokens of each question
    (maskf: fp32 [B][L], non-zero = real token; None: all) -> fp32 [B][P] (vqa_attention_map)."""
    if caw.dim() != 5 or caw.dtype != torch.float32 or not caw.is_contiguous():
        raise ValueError("attention_map: caw must be a contiguous fp32 [ncl, B, H, L, P] tensor")
    ncl, B, H, L, P = caw.shape
    if maskf is not None and (maskf.dtype != torch.float32 or tuple(maskf.shape) != (B, L) or maskf.device != caw.device or not maskf.is_contiguous()):
        raise ValueError(f"attention_map: the mask must be a contiguous fp32 [{B}, {L}] tensor on {caw.device}")
    out = torch.empty((B, P), device=caw.device, dtype=torch.float32)
    call("vqa_attention_map", ptr(caw), ptr(maskf), ptr(out), ncl, B, H, L, P, int(bool(normalize)))
    return out


def check_alpha(alpha) -> float:
    """The blend weight of heatmap_render: a number in [0, 1] (ValueError otherwise)."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be a number in [0, 1], got {alpha!r}")
    return float(alpha)


def default_colormap() -> torch.Tensor:
    """The default colour table, uint8 [256][3] on the CPU: piecewise linear through a few anchor colours (dark blue, blue, cyan,
    yellow, red, dark red at equal distances), rounded to the nearest level.  Built in integer arithmetic: the same bytes everywhere."""
    anchors = ((0, 0, 128), (0, 0, 255), (0, 255, 255), (255, 255, 0), (255, 0, 0), (128, 0, 0))
    seg = len(anchors) - 1
    rows = []
    for i in range(256):
        k = min(i * seg // 255, seg - 1)
        num = i * seg - k * 255                       # position inside segment k, in 1/255ths
        rows.append([(a * (255 - num) + b * num + 127) // 255 for a, b in zip(anchors[k], anchors[k + 1])])
    return torch.tensor(rows, dtype=torch.uint8)


_COLORMAPS = {}


def heatmap_render(maps, size=None, base=None, alpha=0.5, colormap=None):
    """A batch of maps as pictures, one launch (vqa_heatmap_render): maps fp32 [B][Hm][Wm] on the device are upsampled bilinearly
    (F.interpolate, align_corners=False) to size = (H, W), looked up in the colour table (uint8 [256][3]; None: default_colormap())
    and, with a base (uint8 [B][H][W][3] on the device), blended over it as alpha * colour + (1 - alpha) * base.  size defaults to
    the base's.  Returns uint8 [B][H][W][3].  Usable on any fp32 map (Grad-CAM, attention, an input-gradient saliency)."""
    alpha = check_alpha(alpha)
    if not isinstance(maps, torch.Tensor) or maps.dim() != 3 or maps.dtype != torch.float32:
        raise ValueError("heatmap_render: maps must be an fp32 [B, Hm, Wm] tensor")
    B, Hm, Wm = maps.shape
    if base is not None:
        if (not isinstance(base, torch.Tensor) or base.dtype != torch.uint8 or base.dim() != 4 or base.shape[0] != B or base.shape[3] != 3
                or base.device != maps.device):
            raise ValueError(f"heatmap_render: the base must be a uint8 [{B}, H, W, 3] tensor on {maps.device}, got "
                             + (f"{base.dtype} {tuple(base.shape)} on {base.device}" if isinstance(base, torch.Tensor) else type(base).__name__))
        if size is None:
            size = (base.shape[1], base.shape[2])
        elif tuple(size) != (base.shape[1], base.shape[2]):
            raise ValueError(f"heatmap_render: size {tuple(size)} differs from the base's {tuple(base.shape[1:3])}")
        base = base.contiguous()
    if size is None:
        raise ValueError("heatmap_render: without a base the output size (H, W) is required")
    H, W = (int(v) for v in size)
    if H < 1 or W < 1:
        raise ValueError(f"heatmap_render: size must be positive, got {tuple(size)}")
    if colormap is None:
        key = str(maps.device)
        colormap = _COLORMAPS.get(key)
        if colormap is None:
            colormap = _COLORMAPS[key] = default_colormap().to(maps.device)
    elif (not isinstance(colormap, torch.Tensor) or colormap.dtype != torch.uint8 or tuple(colormap.shape) != (256, 3)):
        raise ValueError("heatmap_render: the colour table must be a uint8 [256, 3] tensor")
    else:
        colormap = colormap.to(maps.device).contiguous()
    if not maps.is_cuda:
        raise RuntimeError("heatmap_render: the maps are on the CPU; this implementation only runs on an MI355X (no CPU path)")
    maps = maps.contiguous()
    out = torch.empty((B, H, W, 3), device=maps.device, dtype=torch.uint8)
    call("vqa_heatmap_render", ptr(maps), ptr(base), ptr(colormap), ptr(out), B, Hm, Wm, H, W, alpha)
    return out
