"""GPU: attention backward with an upstream gradient on the saved softmax (vqa_attention_bwd_dp / vqa_attention_bwd_mfma_dp, the
kernels behind gradients on aux['cross_attention_weights']) and the gradient-tap accumulate (vqa_grad_tap_add)."""
import math

import pytest
import torch

from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (form, compute dtype): the VALU kernel in both dtypes, the MFMA kernel in bf16
FORMS = [("valu", torch.float32), ("valu", torch.bfloat16), ("mfma", torch.bfloat16)]
# every attention shape the model reaches: 49 image tokens (d=256 -> hd 32), 144 image tokens (d=512 -> hd 64), 20 text tokens
SHAPES = [(3, 8, 20, 49, 32), (2, 8, 20, 144, 64), (2, 8, 20, 49, 64), (2, 8, 20, 144, 32), (3, 8, 20, 20, 32)]


def _inputs(B, H, Lq, Lk, hd, T, seed):
    d = H * hd
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B * Lq, d, generator=g).to(DEV, T)
    k = torch.randn(B * Lk, d, generator=g).to(DEV, T)
    v = torch.randn(B * Lk, d, generator=g).to(DEV, T)
    dctx = torch.randn(B * Lq, d, generator=g).to(DEV, T)
    probs = torch.softmax(torch.randn(B, H, Lq, Lk, generator=g) * 2, -1).to(DEV)
    dprobs = torch.randn(B, H, Lq, Lk, generator=g).to(DEV)
    return q, k, v, dctx, probs, dprobs


def _bwd(form, T, B, H, Lq, Lk, hd, q, k, v, dctx, probs, dprobs, p, seed=4321):
    """One launch of the chosen entry; dprobs None -> the existing entry (no upstream probability gradient)."""
    L = sub("_lib")
    d = H * hd
    dq = torch.full((B * Lq, d), 7.0, device=DEV, dtype=T)
    dk = torch.full((B * Lk, d), 7.0, device=DEV, dtype=T)
    dv = torch.full((B * Lk, d), 7.0, device=DEV, dtype=T)
    name = "vqa_attention_bwd_mfma" if form == "mfma" else "vqa_attention_bwd"
    pr = (probs.data_ptr(),) if dprobs is None else (probs.data_ptr(), dprobs.data_ptr())
    args = (dctx.data_ptr(), d, q.data_ptr(), k.data_ptr(), v.data_ptr(), d, d, d, *pr, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
            d, d, d, B, H, Lq, Lk, hd, p, seed)
    if form == "valu":
        args = (L.dt(T),) + args
    L.call(name + ("" if dprobs is None else "_dp"), *args)
    return dq, dk, dv


@pytest.mark.parametrize("form,T", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dp_with_zero_dprobs_is_bit_equal(form, T, shape, p):
    B, H, Lq, Lk, hd = shape
    q, k, v, dctx, probs, _ = _inputs(B, H, Lq, Lk, hd, T, seed=Lk * 10 + hd)
    ref = _bwd(form, T, B, H, Lq, Lk, hd, q, k, v, dctx, probs, None, p)
    got = _bwd(form, T, B, H, Lq, Lk, hd, q, k, v, dctx, probs, torch.zeros_like(probs), p)
    torch.cuda.synchronize()
    for a, b, nm in zip(got, ref, ("dq", "dk", "dv")):
        assert torch.equal(a, b), nm


@pytest.mark.parametrize("form,T", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dp_alone_matches_fp64(form, T, shape, p):
    """dctx = 0: dP = dprobs whatever the dropout mask, so dS = P (G - rowsum(P G)) / sqrt(hd), dQ = dS K, dK = dS^T Q, dV = 0."""
    B, H, Lq, Lk, hd = shape
    q, k, v, dctx, probs, dprobs = _inputs(B, H, Lq, Lk, hd, T, seed=Lk * 10 + hd + 1)
    dq, dk, dv = _bwd(form, T, B, H, Lq, Lk, hd, q, k, v, torch.zeros_like(dctx), probs, dprobs, p)
    torch.cuda.synchronize()
    P, Gp = probs.double(), dprobs.double()
    dS = P * (Gp - (P * Gp).sum(-1, keepdim=True)) / math.sqrt(hd)
    qh = q.double().view(B, Lq, H, hd).transpose(1, 2)
    kh = k.double().view(B, Lk, H, hd).transpose(1, 2)
    rq = (dS @ kh).transpose(1, 2).reshape(B * Lq, H * hd)
    rk = (dS.transpose(-1, -2) @ qh).transpose(1, 2).reshape(B * Lk, H * hd)
    tol = 1e-5 if T == torch.float32 else 1.5e-2
    for a, r, nm in ((dq, rq, "dq"), (dk, rk, "dk")):
        err = float((a.double() - r).norm() / r.norm())
        assert err < tol, (nm, err)
    assert float(dv.float().abs().max()) == 0.0


@pytest.mark.parametrize("form,T", FORMS)
@pytest.mark.parametrize("shape", SHAPES[:2])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dp_is_linear_in_its_two_gradients(form, T, shape, p):
    B, H, Lq, Lk, hd = shape
    q, k, v, dctx, probs, dprobs = _inputs(B, H, Lq, Lk, hd, T, seed=Lk * 10 + hd + 2)
    both = _bwd(form, T, B, H, Lq, Lk, hd, q, k, v, dctx, probs, dprobs, p)
    ctx_only = _bwd(form, T, B, H, Lq, Lk, hd, q, k, v, dctx, probs, torch.zeros_like(probs), p)
    dp_only = _bwd(form, T, B, H, Lq, Lk, hd, q, k, v, torch.zeros_like(dctx), probs, dprobs, p)
    torch.cuda.synchronize()
    tol = 1e-5 if T == torch.float32 else 2e-2
    for a, b, c, nm in zip(both, ctx_only, dp_only, ("dq", "dk", "dv")):
        r = b.double() + c.double()
        err = float((a.double() - r).norm() / r.norm())
        assert err < tol, (nm, err)


def test_dp_rejects_a_null_dprobs():
    L = sub("_lib")
    B, H, Lq, Lk, hd = 1, 8, 20, 49, 32
    q, k, v, dctx, probs, _ = _inputs(B, H, Lq, Lk, hd, torch.bfloat16, seed=5)
    d = H * hd
    out = torch.empty(B * Lk, d, device=DEV, dtype=torch.bfloat16)
    common = (dctx.data_ptr(), d, q.data_ptr(), k.data_ptr(), v.data_ptr(), d, d, d, probs.data_ptr(), None, out.data_ptr(),
              out.data_ptr(), out.data_ptr(), d, d, d, B, H, Lq, Lk, hd, 0.0, 1)
    for name, args in (("vqa_attention_bwd_mfma_dp", common), ("vqa_attention_bwd_dp", (1,) + common)):
        with pytest.raises(RuntimeError, match="argument"):
            L.call(name, *args)


@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
def test_grad_tap_rows_with_stride(T):
    """layout 0: one half of a [B][2d] gradient (row stride 2d); the other half is untouched."""
    L = sub("_lib")
    B, d = 37, 256
    g = torch.Generator().manual_seed(9)
    acc = torch.randn(B, 2 * d, generator=g).to(DEV, T)
    tap = torch.randn(B, d, generator=g).to(DEV)
    want = acc.float().clone()
    want[:, d:] = (want[:, d:] + tap).to(T).float()
    got = acc.clone()
    L.call("vqa_grad_tap_add", L.dt(T), tap.data_ptr(), got[:, d:].data_ptr(), B, d, 2 * d, 0)
    torch.cuda.synchronize()
    assert torch.equal(got.float(), want)


@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C,H,W", [(3, 512, 7, 7), (2, 512, 12, 12), (1, 70, 5, 3)])
def test_grad_tap_nchw_into_nhwc(T, B, C, H, W):
    """layout 1: an NCHW fp32 gradient (aux['image_features']) added into the NHWC [B*H*W][C] stage-4 gradient."""
    L = sub("_lib")
    g = torch.Generator().manual_seed(B * C + H)
    acc = torch.randn(B * H * W, C, generator=g).to(DEV, T)
    tap = torch.randn(B, C, H, W, generator=g).to(DEV)
    want = (acc.float() + tap.permute(0, 2, 3, 1).reshape(B * H * W, C)).to(T)
    got = acc.clone()
    L.call("vqa_grad_tap_add", L.dt(T), tap.data_ptr(), got.data_ptr(), B * H * W, C, H * W, 1)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
