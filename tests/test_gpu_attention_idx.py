"""GPU: indexed cross-attention forward (vqa_attention_fwd_mfma_idx, vqa_attention_fwd_idx) -- query batch b reads the K / V /
kmask rows of image kv_index[b] -- against an fp64 torch formula on the gathered K / V, and bit-equal to the plain entries for
the identity index."""
import math

import pytest
import torch

from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (n_kv, index): repeats + an unused image (1) out of order; every image once in reverse order
INDICES = {"repeats_unused": (4, [3, 3, 0, 2, 0, 3]), "reversed": (4, [3, 2, 1, 0])}
ENTRIES = [("vqa_attention_fwd_mfma_idx", torch.bfloat16), ("vqa_attention_fwd_idx", torch.float32), ("vqa_attention_fwd_idx", torch.bfloat16)]
TOL = {torch.float32: (1e-5, 1e-4), torch.bfloat16: (2e-5, 3e-2)}      # (probs, ctx): bf16 ctx is rounded (and P before PV on MFMA)


def _inputs(n_kv, B, H, Lq, Lk, hd, dtype, masked, seed):
    d = H * hd
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B * Lq, d, generator=g).to(DEV, dtype)
    kv = torch.randn(n_kv * Lk, 2 * d, generator=g).to(DEV, dtype)     # K | V of one image token per row (row stride 2d), like the engine
    kmask = None
    if masked:
        lens = torch.randint(1, Lk + 1, (n_kv,), generator=g)
        lens[0] = Lk
        kmask = (torch.arange(Lk)[None, :] < lens[:, None]).float().to(DEV)
    return q, kv, kmask


def _run(name, dtype, q, kv, kmask, idx, n_kv, B, H, Lq, Lk, hd):
    L = sub("_lib")
    d = H * hd
    probs = torch.full((B, H, Lq, Lk), -7.0, device=DEV)
    ctx = torch.full((B * Lq, d), -7.0, device=DEV, dtype=dtype)
    args = (q.data_ptr(), kv.data_ptr(), kv[:, d:].data_ptr(), d, 2 * d, 2 * d, idx.data_ptr(), n_kv,
            None if kmask is None else kmask.data_ptr(), probs.data_ptr(), ctx.data_ptr(), d, B, H, Lq, Lk, hd)
    if name == "vqa_attention_fwd_idx":
        args = (sub("_lib").dt(dtype),) + args
    L.call(name, *args)
    return probs, ctx


def _plain(name, dtype, q, kv, kmask, B, H, Lq, Lk, hd):
    L = sub("_lib")
    d = H * hd
    probs = torch.full((B, H, Lq, Lk), -7.0, device=DEV)
    ctx = torch.full((B * Lq, d), -7.0, device=DEV, dtype=dtype)
    args = (q.data_ptr(), kv.data_ptr(), kv[:, d:].data_ptr(), d, 2 * d, 2 * d, None if kmask is None else kmask.data_ptr(),
            probs.data_ptr(), ctx.data_ptr(), d, B, H, Lq, Lk, hd, 0.0, 0)
    if name == "vqa_attention_fwd":
        args = (sub("_lib").dt(dtype),) + args
    L.call(name, *args)
    return probs, ctx


def _reference(q, kv, kmask, idx, B, H, Lq, Lk, hd):
    d = H * hd
    ii = torch.as_tensor(idx, device=DEV, dtype=torch.long)
    kvg = kv.double().view(-1, Lk, 2 * d)[ii]                          # gathered K / V [B][Lk][2d]
    qf = q.double().view(B, Lq, H, hd).transpose(1, 2)
    kf = kvg[..., :d].reshape(B, Lk, H, hd).transpose(1, 2)
    vf = kvg[..., d:].reshape(B, Lk, H, hd).transpose(1, 2)
    s = qf @ kf.transpose(-1, -2) / math.sqrt(hd)
    if kmask is not None:
        s = s.masked_fill(kmask[ii][:, None, None, :] == 0, float("-inf"))
    pr = torch.softmax(s, -1)
    return pr, (pr @ vf).transpose(1, 2).reshape(B * Lq, d)


@pytest.mark.parametrize("entry", ENTRIES, ids=["mfma_bf16", "valu_fp32", "valu_bf16"])
@pytest.mark.parametrize("Lk", [49, 144])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("Lq", [1, 7, 20, 32])
@pytest.mark.parametrize("which", list(INDICES))
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "kmask"])
def test_indexed_attention_matches_fp64_on_gathered_kv(entry, Lk, hd, Lq, which, masked):
    name, dtype = entry
    n_kv, index = INDICES[which]
    B, H = len(index), 4
    q, kv, kmask = _inputs(n_kv, B, H, Lq, Lk, hd, dtype, masked, seed=Lk * 1000 + hd * 10 + Lq)
    idx = torch.tensor(index, device=DEV, dtype=torch.int32)
    probs, ctx = _run(name, dtype, q, kv, kmask, idx, n_kv, B, H, Lq, Lk, hd)
    pr, ref = _reference(q, kv, kmask, index, B, H, Lq, Lk, hd)
    torch.cuda.synchronize()
    tp, tc = TOL[dtype]
    assert torch.isfinite(probs).all() and torch.isfinite(ctx.float()).all()
    assert (probs.double() - pr).abs().max().item() < tp
    assert (ctx.double() - ref).abs().max().item() < tc
    if masked:                                                         # masked key rows follow the index: exactly zero probability
        km = kmask[torch.as_tensor(index, device=DEV, dtype=torch.long)]
        assert (probs * (km[:, None, None, :] == 0)).abs().max().item() == 0.0


@pytest.mark.parametrize("pair", [("vqa_attention_fwd_mfma_idx", "vqa_attention_fwd_mfma", torch.bfloat16),
                                  ("vqa_attention_fwd_idx", "vqa_attention_fwd", torch.float32),
                                  ("vqa_attention_fwd_idx", "vqa_attention_fwd", torch.bfloat16)], ids=["mfma_bf16", "valu_fp32", "valu_bf16"])
@pytest.mark.parametrize("Lk", [49, 144])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "kmask"])
def test_identity_index_is_bit_equal_to_the_plain_entry(pair, Lk, hd, masked):
    name, plain, dtype = pair
    B, H, Lq = 5, 4, 20
    q, kv, kmask = _inputs(B, B, H, Lq, Lk, hd, dtype, masked, seed=7 + Lk + hd)
    idx = torch.arange(B, device=DEV, dtype=torch.int32)
    p1, c1 = _run(name, dtype, q, kv, kmask, idx, B, B, H, Lq, Lk, hd)
    p2, c2 = _plain(plain, dtype, q, kv, kmask, B, H, Lq, Lk, hd)
    torch.cuda.synchronize()
    assert torch.equal(p1, p2) and torch.equal(c1, c2)

