"""GPU: many questions per image in training at the kernel level -- vqa_index_csr against a stable argsort, the indexed attention
backward (vqa_attention_bwd_idx, vqa_attention_bwd_mfma_idx: dQ per question, dK / dV summed per image) against fp64 autograd on
the gathered K / V, and the bit-exact routes: identity index (dropout included) equal to vqa_attention_bwd(_mfma) and the _train
forwards equal to vqa_attention_fwd(_mfma), an unused image's exact zeros, and two launches giving the same bits."""
import math

import pytest
import torch

from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, LQ = 4, 20
# U = 4 images: repeats, image 1 never asked about, out of order
INDEX = [3, 3, 0, 2, 0, 3, 2]
ENTRIES = [("mfma", torch.bfloat16), ("valu", torch.float32), ("valu", torch.bfloat16)]
TOL = {torch.float32: 1e-5, torch.bfloat16: 2e-2}          # norm-relative error of dQ / dK / dV against fp64


def _csr(idx, U):
    L = sub("_lib")
    offsets = torch.full((U + 1,), -5, device=DEV, dtype=torch.int32)
    order = torch.full((idx.numel(),), -5, device=DEV, dtype=torch.int32)
    L.call("vqa_index_csr", idx.data_ptr(), idx.numel(), U, offsets.data_ptr(), order.data_ptr())
    return offsets, order


def _inputs(U, B, Lk, hd, dtype, seed):
    d = H * hd
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B * LQ, d, generator=g).to(DEV, dtype)
    kv = torch.randn(U * Lk, 2 * d, generator=g).to(DEV, dtype)           # K | V per image token (row stride 2d), like the engine
    dctx = torch.randn(B * LQ, d, generator=g).to(DEV, dtype)
    return q, kv, dctx


def _fwd(kind, dtype, q, kv, idx, U, B, Lk, hd, p, seed, plain=False):
    L = sub("_lib")
    d = H * hd
    probs = torch.full((B, H, LQ, Lk), -7.0, device=DEV)
    ctx = torch.full((B * LQ, d), -7.0, device=DEV, dtype=dtype)
    if plain:
        args = (q.data_ptr(), kv.data_ptr(), kv[:, d:].data_ptr(), d, 2 * d, 2 * d, None, probs.data_ptr(), ctx.data_ptr(), d, B, H, LQ, Lk,
                hd, p, seed)
        name = "vqa_attention_fwd_mfma" if kind == "mfma" else "vqa_attention_fwd"
    else:
        args = (q.data_ptr(), kv.data_ptr(), kv[:, d:].data_ptr(), d, 2 * d, 2 * d, idx.data_ptr(), U, None, probs.data_ptr(),
                ctx.data_ptr(), d, B, H, LQ, Lk, hd, p, seed)
        name = "vqa_attention_fwd_mfma_idx_train" if kind == "mfma" else "vqa_attention_fwd_idx_train"
    if kind == "valu":
        args = (L.dt(dtype),) + args
    L.call(name, *args)
    return probs, ctx


def _bwd(kind, dtype, dctx, q, kv, probs, csr, U, B, Lk, hd, p, seed):
    """csr = (offsets, order) -> the indexed backward; None -> the plain one (U == B)."""
    L = sub("_lib")
    d = H * hd
    dq = torch.full((B * LQ, d), -7.0, device=DEV, dtype=dtype)
    dkv = torch.full((U * Lk, 2 * d), -7.0, device=DEV, dtype=dtype)
    head = (dctx.data_ptr(), d, q.data_ptr(), kv.data_ptr(), kv[:, d:].data_ptr(), d, 2 * d, 2 * d, probs.data_ptr())
    tail = (dq.data_ptr(), dkv.data_ptr(), dkv[:, d:].data_ptr(), d, 2 * d, 2 * d, B, H, LQ, Lk, hd, p, seed)
    if csr is None:
        args, name = head + tail, "vqa_attention_bwd"
    else:
        args, name = head + (csr[0].data_ptr(), csr[1].data_ptr(), U) + tail, "vqa_attention_bwd_idx"
    if kind == "mfma":
        name = name.replace("vqa_attention_bwd", "vqa_attention_bwd_mfma")
    else:
        args = (L.dt(dtype),) + args
    L.call(name, *args)
    return dq, dkv


def _reference(q, kv, dctx, index, U, B, Lk, hd):
    d = H * hd
    q64 = q.double().requires_grad_(True)
    kv64 = kv.double().requires_grad_(True)
    ii = torch.as_tensor(index, device=DEV, dtype=torch.long)
    kvg = kv64.view(U, Lk, 2 * d)[ii]
    qf = q64.view(B, LQ, H, hd).transpose(1, 2)
    kf = kvg[..., :d].reshape(B, Lk, H, hd).transpose(1, 2)
    vf = kvg[..., d:].reshape(B, Lk, H, hd).transpose(1, 2)
    pr = torch.softmax(qf @ kf.transpose(-1, -2) / math.sqrt(hd), -1)
    ctx = (pr @ vf).transpose(1, 2).reshape(B * LQ, d)
    ctx.backward(dctx.double())
    return q64.grad, kv64.grad


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp_min(1e-30))


def test_index_csr_matches_a_stable_argsort():
    g = torch.Generator().manual_seed(3)
    for U, N in ((4, 7), (1, 5), (9, 1), (300, 2500), (3000, 700), (5, 0)):
        idx = torch.randint(0, U, (N,), generator=g, dtype=torch.int32)
        if N >= 3:
            idx[-1] = idx[0]                                           # (a repeat across the chunk boundary for N > 1024)
        offsets, order = _csr(idx.to(DEV), U)
        torch.cuda.synchronize()
        cnt = torch.bincount(idx.long(), minlength=U)
        exp_off = torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)])
        assert torch.equal(offsets.cpu().long(), exp_off), (U, N)
        assert torch.equal(order.cpu().long(), torch.argsort(idx.long(), stable=True)), (U, N)


def test_index_csr_flags_an_index_out_of_range():
    for bad in ([0, 4, 1], [0, -1, 2]):
        offsets, order = _csr(torch.tensor(bad, device=DEV, dtype=torch.int32), 4)
        torch.cuda.synchronize()
        assert (offsets == -1).all() and (order == -1).all()


@pytest.mark.parametrize("entry", ENTRIES, ids=["mfma_bf16", "valu_fp32", "valu_bf16"])
@pytest.mark.parametrize("Lk", [49, 144])
@pytest.mark.parametrize("hd", [32, 64])
def test_indexed_backward_matches_fp64_on_gathered_kv(entry, Lk, hd):
    kind, dtype = entry
    U, B = 4, len(INDEX)
    q, kv, dctx = _inputs(U, B, Lk, hd, dtype, seed=Lk * 100 + hd)
    idx = torch.tensor(INDEX, device=DEV, dtype=torch.int32)
    csr = _csr(idx, U)
    probs, _ = _fwd(kind, dtype, q, kv, idx, U, B, Lk, hd, 0.0, 0)
    dq, dkv = _bwd(kind, dtype, dctx, q, kv, probs, csr, U, B, Lk, hd, 0.0, 0)
    rq, rkv = _reference(q, kv, dctx, INDEX, U, B, Lk, hd)
    torch.cuda.synchronize()
    d = H * hd
    assert torch.isfinite(dq.float()).all() and torch.isfinite(dkv.float()).all()
    tol = TOL[dtype]
    assert _rel(dq, rq) < tol
    used = [u for u in range(U) if u in INDEX]
    rows = torch.cat([torch.arange(u * Lk, (u + 1) * Lk) for u in used]).to(DEV)
    assert _rel(dkv[rows, :d], rkv[rows, :d]) < tol                    # dK
    assert _rel(dkv[rows, d:], rkv[rows, d:]) < tol                    # dV
    assert (dkv[Lk:2 * Lk] == 0).all()                                 # image 1 has no question: exact zeros
    # two launches: the same bits (fixed-order sums, no atomics)
    dq2, dkv2 = _bwd(kind, dtype, dctx, q, kv, probs, csr, U, B, Lk, hd, 0.0, 0)
    torch.cuda.synchronize()
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)


@pytest.mark.parametrize("entry", ENTRIES, ids=["mfma_bf16", "valu_fp32", "valu_bf16"])
@pytest.mark.parametrize("Lk", [49, 144])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_identity_index_is_bit_equal_to_the_plain_entries(entry, Lk, hd, p):
    kind, dtype = entry
    B = 5
    q, kv, dctx = _inputs(B, B, Lk, hd, dtype, seed=11 + Lk + hd)
    idx = torch.arange(B, device=DEV, dtype=torch.int32)
    seed = (3 << 12) | 7
    p1, c1 = _fwd(kind, dtype, q, kv, idx, B, B, Lk, hd, p, seed)
    p2, c2 = _fwd(kind, dtype, q, kv, idx, B, B, Lk, hd, p, seed, plain=True)
    dq1, dkv1 = _bwd(kind, dtype, dctx, q, kv, p1, _csr(idx, B), B, B, Lk, hd, p, seed)
    dq2, dkv2 = _bwd(kind, dtype, dctx, q, kv, p2, None, B, B, Lk, hd, p, seed)
    torch.cuda.synchronize()
    assert torch.equal(p1, p2) and torch.equal(c1, c2)
    assert torch.equal(dq1, dq2) and torch.equal(dkv1, dkv2)
