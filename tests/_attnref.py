"""float64 reference of the attention entries (csrc/attention.hip: the VALU and the bf16 MFMA form, each plain, with an upstream
gradient on the saved softmax (_dp) and indexed (_idx, _idx_train)), per-element bounds derived from the rounding sites of each form,
the operand generators and the case table.  Plain torch on the CPU, nothing of the package.  test_attn_ref_cpu.py validates all of it
without a GPU (autograd, mask semantics, stand-ins inside the bounds, mutants outside); test_gpu_attention_fp64.py judges the kernels.

Reference (evaluate(), prec = float64), from the operands as stored in the compute dtype:
  S = Q K^T / sqrt(hd); keys with kmask == 0 (so -0.0 too; 0.25, -1 and 2 keep) get -inf; P = softmax(S);
  Pd = P keep / (1 - p), keep = _dropmask.keep_mask(seed, B H Lq Lk, p) at ((b H + h) Lq + i) Lk + j, p the fp32 value; ctx = Pd V.
  Backward, closed form, from the probs buffer the kernel reads taken as an exact input (so its bound carries no forward error):
  dV = Pd^T dctx; dP = keep / (1 - p) (dctx V^T) + dprobs; dS = P (dP - rowsum(P dP)) / sqrt(hd); dQ = dS K; dK = dS^T Q.
  Indexed: K, V, kmask of question b are those of image kv_index[b]; dK, dV are summed per image; no question: exact zeros.

Bounds.  u = U32 = 2^-24 (one fp32 rounding of r costs at most u |r|), w = U16 = 2^-8 (one bf16 rounding; the project's figure).
All per element, in fp64, from absolute-value products; read off attention.hip, site by site:
  logits   ds_ij = (hd + 2) u sum_d |q_id| |k_jd| / sqrt(hd): an fp32 dot of hd terms, the division, and sqrtf(hd) itself (inexact at
           hd 32).  MFMA: hd + 3, it multiplies by 1 / sqrtf(hd): root, reciprocal, product.
  probs    |dP_ij| <= P_ij expm1(ds_ij + log sum_l P_il exp(ds_il) + u |s_ij - m_i| + (Lk + c) u) + 2^-126.
           The first two terms are the exact image of logit errors of at most ds (to first order ds_ij + sum_l P_il ds_il);
           u |s - m| is the rounding of expf's argument; Lk u the row sum; 2^-126 (smallest normal) covers flushed subnormals.
           c covers expf and the division (MFMA: reciprocal and product); it is measured, not derived: see C_EXP.
  stores   every output bound ends with + 2^-126: a result below the smallest normal is stored as a subnormal or as zero.
  ctx      dPd = dP ks + 2 u Pd (p > 0: 1.f - p and the division); through |V|; plus (Lk + 1) u sum_j Pd_ij |v_jd| (accumulation);
           MFMA adds w sum_j Pd_ij |v_jd| (the dropped probabilities become a bf16 MFMA operand).  bf16 store: store_bound().
  backward ks = 1.f / (1.f - p): 2 u.  dP: (hd + 3) u ks sum_d |dctx_id| |v_jd| (dot, ks, product), + u |dP| where dprobs is added.
           t_i: sum_j P_ij ddP_ij + (Lk + 1) u sum_j |dP_ij P_ij|.
           |ddS| <= [P (ddP + dt) + n u |P (dP - t)|] / sqrt(hd), n = 4 (subtraction, product, division, sqrtf(hd)), MFMA 5
           (subtraction, two products, root and reciprocal of 1 / sqrtf(hd)).  The last term is relative to the CANCELLED value: in
           the peaked cases the first one, absolute, is what matters.
           MFMA rounds dS and Pd to bf16 before the second MFMA: w |dS|, w |Pd|; Pd = P ks costs 3 u before that.
           dQ: ddS through |K| + Lk u sum |dS| |k|; dK: ddS through |Q| + n u sum |dS| |q|, dV: dPd through |dctx| + n u sum Pd |dctx|,
           n = Lq x the questions of the image (indexed: one accumulation over all of them, one output rounding).
The GPU file adds the fp64 evaluation's own rounding in worst(): bound (1 + 2^-30) + 2^-45 |ref|."""
import dataclasses
import math
import types

import numpy as np
import torch

from _attnbits import REPEATS
from _dropmask import keep_mask

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DT = {"fp32": F32, "bf16": BF16}
U32 = 2.0 ** -24
U16 = 2.0 ** -8
FLT_MIN = 2.0 ** -126
SENT = -8192.0                                    # sentinel of every output buffer (a bf16 number no case produces)
SEED = 0x5EED0000025                              # a plain seed word (bit 63 clear)
FAMILIES = (("valu", "fp32"), ("valu", "bf16"), ("mfma", "bf16"))
B0, H0 = 3, 3                                     # 9 (batch, head) problems: odd against 4, 2 and 1 waves per workgroup
SHAPES = ((1, 1), (5, 20), (20, 20), (20, 31), (20, 32), (20, 33), (20, 49), (32, 64), (20, 65), (5, 144), (32, 160))
MODEL_SHAPES = ((20, 20, 32), (20, 49, 64), (20, 144, 32), (32, 160, 64))     # the model's shapes and the top of the MFMA form
LDS_BYTES = 160 * 1024

C_EXP = 4.0
"""c of the probs bound.  The need is measured at the randn / no mask / p = 0 cases as the worst, over the probabilities above
2^-100, of (log(1 + |P_kernel - P_ref| / P_ref) - a0) / u, a0 the exponent of the bound without c (c_need()): what is left for c to
carry once the derived terms have carried theirs.
  Measured on MI355X, valu/fp32: -141.6     CPU fp32 stand-in: -153.7
Both are negative: the worst-case logit terms ((hd + 2) u sum |q| |k|) already carry expf, the division and the tree sum at these
cases, so twice the larger need is below zero and c is held at its floor instead, the count of the sites it stands for: expf to 1 ulp
= 2 u (the device library's stated accuracy), the division u (MFMA: reciprocal and product, 2 u): c = 4."""


# ------------------------------------------------------------------------------------------------- launch limits (host mirrors)
def valu_lds_floats(bwd, Lq, Lk, hd):
    """AttnValuLds<BWD>::floats()"""
    ldh, ldp = hd + 1, Lk + 1
    qo, kv, pd = Lq * ldh, Lk * ldh, Lq * ldp
    return (2 if bwd else 1) * (qo + pd) + 2 * kv


def valu_fits(bwd, Lq, Lk, hd):
    return valu_lds_floats(bwd, Lq, Lk, hd) * 4 <= LDS_BYTES


def valu_max_lk(bwd, Lq, hd):
    Lk = 1
    while valu_fits(bwd, Lq, Lk + 1, hd):
        Lk += 1
    return Lk


def mfma_fits(Lq, Lk, hd):
    return Lq <= 32 and Lk <= 160 and hd in (32, 64)


def mfma_nkt(Lk):
    return 2 if Lk <= 64 else 5


LK_FWD_MAX, LK_BWD_MAX = valu_max_lk(False, 20, 64), valu_max_lk(True, 20, 64)
IDX_BWD_NKD = 256 * 40                            # vqa_attention_bwd_idx: Lk * hd accumulators at most


# ------------------------------------------------------------------------------------------------------------------ the cases
@dataclasses.dataclass(frozen=True)
class Case:
    fam: str
    dname: str
    Lq: int
    Lk: int
    hd: int
    kind: str = "randn"                           # randn | peaked | offset
    mask: str = "none"                            # none | prefix | sparse | odd | row
    p: float = 0.0
    entry: str = "plain"                          # plain | dp | idx_infer | idx_train
    wide: bool = False
    backward: bool = True

    @property
    def indexed(self):
        return self.entry.startswith("idx")

    @property
    def B(self):
        return len(REPEATS) if self.indexed else B0

    @property
    def images(self):
        return 4 if self.indexed else B0

    @property
    def packed(self):
        return self.Lq == self.Lk and not self.indexed and not self.wide

    @property
    def has_bwd(self):
        return self.backward and self.entry != "idx_infer"

    @property
    def id(self):
        return (f"{self.fam}-{self.dname}-{self.entry}-{self.Lq}x{self.Lk}x{self.hd}-{self.kind}-{self.mask}-p{self.p}"
                + ("-wide" if self.wide else "") + ("" if self.backward else "-fwd"))


def cases():
    out = []
    for fam, dn in FAMILIES:
        C = lambda *a, **k: out.append(Case(fam, dn, *a, **k))
        for hd in (32, 64):                       # every (Lq, Lk, hd) once
            for Lq, Lk in SHAPES:
                C(Lq, Lk, hd)
        if fam == "valu":                         # beyond the MFMA limits, up to the LDS limits
            C(33, 161, 48)
            C(20, 196, 64)
            C(20, LK_BWD_MAX, 64)
            C(20, LK_FWD_MAX, 64, backward=False)
        for i, (Lq, Lk, hd) in enumerate(MODEL_SHAPES):
            C(Lq, Lk, hd, kind="peaked")
            C(Lq, Lk, hd, kind="offset")
            C(Lq, Lk, hd, mask="prefix")
            C(Lq, Lk, hd, mask="sparse", p=0.1)
            C(Lq, Lk, hd, mask="odd")
            C(Lq, Lk, hd, mask="row", p=0.5)
            C(Lq, Lk, hd, kind="peaked", mask="sparse", p=0.1)
            C(Lq, Lk, hd, p=0.1, wide=(i == 1))
            C(Lq, Lk, hd, p=0.5)
            C(Lq, Lk, hd, entry="dp", p=0.1, wide=(i == 2))
            C(Lq, Lk, hd, entry="dp", kind="peaked")
            C(Lq, Lk, hd, entry="dp", kind="offset", mask="row", p=0.1)
            C(Lq, Lk, hd, entry="idx_infer", mask="sparse")
            C(Lq, Lk, hd, entry="idx_infer", kind="offset", mask="odd")
            C(Lq, Lk, hd, entry="idx_train", p=0.1, wide=(i == 1))
            C(Lq, Lk, hd, entry="idx_train", mask="row")
            C(Lq, Lk, hd, entry="idx_train", kind="peaked", mask="sparse", p=0.5)
    return out


CASES = cases()


def find(**kw):
    """the one case of the table with these fields (the others at their defaults)"""
    want = dataclasses.replace(Case("valu", "fp32", 20, 20, 32), **kw)
    assert want in CASES, want
    return want


# ----------------------------------------------------------------------------------------------------------------- the operands
def _seed_of(case):
    """the same operands for every family: the forms are judged against ONE reference (bf16 rounds what fp32 keeps)"""
    s = 17
    for ch in dataclasses.replace(case, fam="", dname="").id:
        s = (s * 1000003 + ord(ch)) % (2 ** 31 - 1)
    return s


def _kmask(case, g):
    U, Lk = case.images, case.Lk
    if case.mask == "none":
        return None
    if case.mask == "prefix":
        m = torch.zeros(U, Lk)
        for u in range(U):
            m[u, :max(1, Lk - (u * Lk) // (U + 1) - 1)] = 1.0
        return m
    assert Lk >= 20, "the sparse masks need room for a kept key"
    keep = torch.rand(U, Lk, generator=g) >= 0.25                # about a quarter of the keys masked
    keep[:, 0] = False
    keep[:, Lk - 1] = False
    if Lk >= 64:
        keep[:, 32:64] = False                                  # a whole MFMA key tile
    keep[:, 1] = True
    if case.mask == "row":
        keep[U - 1, :] = False                                  # every key of the last batch / image
    if case.mask == "odd":
        vals = torch.tensor([0.25, -1.0, 2.0, 1.0]).repeat(Lk // 4 + 1)[:Lk].expand(U, Lk)
        return torch.where(keep, vals, torch.tensor(-0.0))
    return keep.float()


def make_inputs(case):
    """every operand of the case as CPU tensors in the layout the entries take; deterministic"""
    g = torch.Generator().manual_seed(_seed_of(case))
    B, U, H, Lq, Lk, hd = case.B, case.images, H0, case.Lq, case.Lk, case.hd
    d, dt = H * hd, DT[case.dname]
    rn = lambda *s: torch.randn(*s, generator=g)
    if case.kind == "randn":
        q, k = rn(B * Lq, d), rn(U * Lk, d)
    elif case.kind == "peaked":
        q, k = 5 * rn(B * Lq, d), 5 * rn(U * Lk, d)
    else:
        q, k = 3 + 0.25 * rn(B * Lq, d), 30 / math.sqrt(hd) + 0.25 * rn(U * Lk, d)
    v = rn(U * Lk, d)
    I = types.SimpleNamespace(case=case, B=B, U=U, H=H, Lq=Lq, Lk=Lk, hd=hd, d=d, dtype=dt)
    if case.packed:
        I.qkv = torch.cat([q, k, v], 1).to(dt).contiguous()
        I.q = I.k = I.v = I.qkv
        I.ldq = I.ldk = I.ldv = 3 * d
        I.qc, I.kc, I.vc = 0, d, 2 * d
    else:
        I.q, I.k = q.to(dt).contiguous(), torch.cat([k, v], 1).to(dt).contiguous()
        I.v = I.k
        I.ldq, I.ldk, I.ldv = d, 2 * d, 2 * d
        I.qc, I.kc, I.vc = 0, 0, d
    I.ldc = d + 8 if case.wide else d
    I.dctx = rn(B * Lq, I.ldc).to(dt).contiguous()
    I.dprobs = rn(B, H, Lq, Lk) if case.entry == "dp" else None
    I.kmask = _kmask(case, g)
    I.kv_index = torch.tensor(REPEATS if case.indexed else range(B), dtype=torch.int64)
    I.p = float(np.float32(case.p))
    I.seed = SEED
    n = B * H * Lq * Lk
    I.keep = torch.from_numpy(keep_mask(SEED, n, case.p)).view(B, H, Lq, Lk) if case.p > 0 else torch.ones(B, H, Lq, Lk, dtype=torch.bool)
    return I


def heads(buf, ld, col0, n, L, H, hd):
    """[n][H][L][hd] view of the rows of a [rows][ld] buffer, head h in columns [col0 + h hd, col0 + (h + 1) hd)"""
    return buf.reshape(-1).as_strided((n, H, L, hd), (L * ld, hd, ld, 1), col0)


def unheads(x):
    n, H, L, hd = x.shape
    return x.transpose(1, 2).reshape(n * L, H * hd)


# --------------------------------------------------------------------------------------------------- the formula, in any precision
MUTANTS = ("no_max", "scale", "rowsum_tail", "pv_tail", "mask_gt", "mask_batch", "drop_swap", "dv_scale", "t_nodp", "v_head", "ld_as_d",
           "dk_pad", "dk_image")


def evaluate(I, probs=None, prec=F64, mfma_sites=False, round_out=False, mutant=None):
    """Forward and (where the case has one) backward in precision prec.  probs: the [B][H][Lq][Lk] buffer the backward reads (None:
    this evaluation's own).  mfma_sites: round to bf16 where the MFMA form does (Pd before P V; dS and Pd before the second MFMA).
    round_out: round ctx, dq, dk, dv once to the compute dtype.  mutant: one of MUTANTS, a defect the bounds must catch.
    Returns a namespace of [.][H][L][.] tensors (S, P, Pd, ks, ...) and the outputs in buffer layout (probs, ctx, dq, dk, dv)."""
    assert mutant is None or mutant in MUTANTS
    T, B, U, H, Lq, Lk, hd, idx = prec, I.B, I.U, I.H, I.Lq, I.Lk, I.hd, I.kv_index
    r16 = (lambda x: x.to(BF16).to(T)) if mfma_sites else (lambda x: x)
    rout = (lambda x: x.to(I.dtype).to(T)) if round_out else (lambda x: x)
    R = types.SimpleNamespace()
    q = heads(I.q, I.d if mutant == "ld_as_d" else I.ldq, I.qc, B, Lq, H, hd).to(T)
    k = heads(I.k, I.ldk, I.kc, U, Lk, H, hd).to(T)[idx]
    v = heads(I.v, I.ldv, I.vc, U, Lk, H, hd).to(T)[idx]
    vf = v[:, [(h ^ 1) % H for h in range(H)]] if mutant == "v_head" else v
    rscale = torch.tensor(math.sqrt(hd + 1 if mutant == "scale" else hd), dtype=T)
    S = (q @ k.transpose(-1, -2)) / rscale
    if I.kmask is not None:
        km = I.kmask[torch.arange(B) % U if mutant == "mask_batch" else idx]
        masked = (km <= 0.5) if mutant == "mask_gt" else (km == 0)
        S = S.masked_fill(masked.view(B, 1, 1, Lk), -math.inf)
    m = S.max(-1, keepdim=True).values
    e = torch.exp(S if mutant == "no_max" else S - m)
    P = e / (e.sum(-1, keepdim=True) - (e[..., -1:] if mutant == "rowsum_tail" else 0))
    keep = I.keep
    if mutant == "drop_swap" and I.case.p > 0:
        flat = torch.from_numpy(keep_mask(I.seed, B * H * Lq * Lk, I.case.p))
        bh, i, j = torch.meshgrid(torch.arange(B * H), torch.arange(Lq), torch.arange(Lk), indexing="ij")
        keep = flat[(bh * Lk + j) * Lq + i].view(B, H, Lq, Lk)
    one = torch.tensor(1.0, dtype=T)
    ks = keep.to(T) * (one / (one - torch.tensor(I.p, dtype=T)))
    Pd = P * ks
    Pv = Pd.clone()
    if mutant == "pv_tail":
        Pv[..., -1] = 0
    ctx = rout(r16(Pv) @ vf)
    R.q, R.k, R.v, R.S, R.m, R.P, R.ks, R.Pd = q, k, v, S, m, P, ks, Pd
    R.probs, R.ctx = P, unheads(ctx)
    if not I.case.has_bwd:
        return R
    Pg = P if probs is None else probs.to(T)
    o = heads(I.dctx, I.ldc, 0, B, Lq, H, hd).to(T)
    dP = (o @ vf.transpose(-1, -2)) * ks
    t_src = dP
    if I.dprobs is not None:
        dP = dP + I.dprobs.to(T)
        t_src = t_src if mutant == "t_nodp" else dP
    t = (t_src * Pg).sum(-1, keepdim=True)
    dS = Pg * (dP - t) / rscale
    Pdg = Pg * (keep.to(T) if mutant == "dv_scale" else ks)
    dq = r16(dS) @ k
    dkb = r16(dS).transpose(-1, -2) @ q
    dvb = r16(Pdg).transpose(-1, -2) @ o
    if mutant == "dk_pad":                        # rows Lq .. 31 of the query tile taken from the next batch's rows
        n = min(32 - Lq, Lq)
        dkb[:-1] += dS[1:, :, :n].transpose(-1, -2) @ q[1:, :, :n]
    tgt = (idx + 1) % U if mutant == "dk_image" else idx
    dk = torch.zeros(U, H, Lk, hd, dtype=T).index_add_(0, tgt, dkb)
    dv = torch.zeros(U, H, Lk, hd, dtype=T).index_add_(0, idx, dvb)
    R.o, R.Pg, R.dP, R.t, R.dS, R.Pdg = o, Pg, dP, t, dS, Pdg
    R.dq, R.dk, R.dv = unheads(rout(dq)), unheads(rout(dk)), unheads(rout(dv))
    return R


def reference(I, probs=None):
    return evaluate(I, probs=probs)


def standin(I, fam):
    """the formula in fp32 on the CPU, for the MFMA form with its bf16 roundings; the backward reads this forward's probs"""
    f = evaluate(I, prec=F32, mfma_sites=(fam == "mfma"), round_out=True)
    if I.case.has_bwd:
        b = evaluate(I, probs=f.probs, prec=F32, mfma_sites=(fam == "mfma"), round_out=True)
        f.dq, f.dk, f.dv = b.dq, b.dk, b.dv
    return f


# ------------------------------------------------------------------------------------------------------------------- the bounds
def store_bound(e, ref, dtype):
    """e: the fp32 result's error.  2^-126, the smallest normal of fp32 and of bf16: a result below it is stored as a subnormal or as 0"""
    return (e * (1 + U16) + U16 * ref.abs() if dtype == BF16 else e) + FLT_MIN


def logit_bound(I, R, fam):
    return (I.hd + (3 if fam == "mfma" else 2)) * U32 * (R.q.abs() @ R.k.abs().transpose(-1, -2)) / math.sqrt(I.hd)


def probs_exponent(I, R, fam):
    """a0: the relative error of a probability is at most expm1(a0 + c u)"""
    ds = logit_bound(I, R, fam)
    x = torch.where(R.P > 0, (R.S - R.m).abs(), torch.zeros_like(R.S))
    lse = torch.log((R.P * torch.exp(ds)).sum(-1, keepdim=True))
    return ds + lse + U32 * x + I.Lk * U32


def forward_bounds(I, R, fam, c=None):
    """R: reference(I).  -> {"probs": [B][H][Lq][Lk], "ctx": [B Lq][d]}; NaN where the reference is NaN"""
    c = C_EXP if c is None else c
    mf, Lk = fam == "mfma", I.Lk
    bP = R.P * torch.expm1(probs_exponent(I, R, fam) + c * U32) + FLT_MIN
    bPd = bP * R.ks + (2 * U32 * R.Pd if I.case.p > 0 else 0)
    av = R.v.abs()
    acc = R.Pd @ av
    bctx = bPd @ av + (Lk + 1) * U32 * acc + (U16 * acc if mf else 0)
    return {"probs": bP, "ctx": store_bound(unheads(bctx), R.ctx, I.dtype)}


def backward_bounds(I, R, fam):
    """R: reference(I, probs) with the probs buffer the kernel read.  -> {"dq", "dk", "dv"} in buffer layout"""
    mf, Lq, Lk, hd, U, H, idx = fam == "mfma", I.Lq, I.Lk, I.hd, I.U, I.H, I.kv_index
    P, rs = R.Pg, math.sqrt(hd)
    bdP = (hd + 3) * U32 * R.ks * (R.o.abs() @ R.v.abs().transpose(-1, -2))
    if I.dprobs is not None:
        bdP = bdP + U32 * R.dP.abs()
    bt = (P * bdP).sum(-1, keepdim=True) + (Lk + 1) * U32 * (R.dP * P).abs().sum(-1, keepdim=True)
    bdS = (P * (bdP + bt) + (5 if mf else 4) * U32 * (P * (R.dP - R.t)).abs()) / rs
    bdS = bdS + FLT_MIN                           # P (dP - t) of a probability near 2^-126 is a subnormal (or flushed)
    bPd = 3 * U32 * R.Pdg + FLT_MIN
    if mf:
        bdS = bdS * (1 + U16) + U16 * R.dS.abs()
        bPd = bPd * (1 + U16) + U16 * R.Pdg
    count = torch.bincount(idx, minlength=U).double().view(U, 1, 1, 1)
    img = lambda x: torch.zeros(U, H, Lk, hd, dtype=F64).index_add_(0, idx, x)
    bdq = bdS @ R.k.abs() + Lk * U32 * (R.dS.abs() @ R.k.abs())
    bdk = img(bdS.transpose(-1, -2) @ R.q.abs()) + Lq * count * U32 * img(R.dS.abs().transpose(-1, -2) @ R.q.abs())
    bdv = img(bPd.transpose(-1, -2) @ R.o.abs()) + Lq * count * U32 * img(R.Pdg.transpose(-1, -2) @ R.o.abs())
    return {n: store_bound(unheads(b), getattr(R, n), I.dtype) for n, b in (("dq", bdq), ("dk", bdk), ("dv", bdv))}


def worst(got, ref, bound):
    """worst err / bound over the elements; inf where the reference is NaN and got is not, where got is not finite and the reference
    is, or where a zero bound is missed.  The fp64 evaluation's own rounding is added to the bound."""
    got, b = got.double(), bound * (1 + 2.0 ** -30) + 2.0 ** -45 * ref.abs()
    nan = ref.isnan()
    if not bool(got[nan].isnan().all()):
        return math.inf
    err = (got - ref).abs()
    ratio = torch.where(nan | (err == 0), torch.zeros_like(err), err / b)
    ratio = torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)
    return float(ratio.max()) if ratio.numel() else 0.0


def c_need(I, R, fam, got_probs):
    """what is left for c to carry, in units of u (see C_EXP)"""
    big = R.P > 2.0 ** -100
    rel = (got_probs.double() - R.P).abs()[big] / R.P[big]
    return float(((torch.log1p(rel) - probs_exponent(I, R, fam)[big]) / U32).max())
