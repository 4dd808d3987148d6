"""Torch (CPU) oracle of the MXFP8 quantization rule of csrc/mxfp8.hip, and its dequantization.

Blocks are 32 consecutive elements of the last axis.  amax = max |x| on the value as stored; amax == 0 -> scale code 127 and +0
elements; amax finite -> X = clamp(floor(log2 amax) - 8, -127, 127), scale code X + 127, element = e4m3fn RNE of
clamp(x / 2^X, -448, 448) (torch's cast is RNE and does not saturate, hence the clamp); a block holding Inf / NaN -> scale code 255
and element codes 0x7F (the kernels' choice; the rule leaves them unspecified)."""
import torch


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as float32, exactly, for integer e in [-126, 127]."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def quant(x: torch.Tensor):
    """x [..., C] (C % 32 == 0), bf16 or fp32 -> (codes uint8 [..., C], scale codes uint8 [..., C / 32])."""
    shp = x.shape
    xf = x.detach().cpu().float().reshape(-1, 32)
    finite = torch.isfinite(xf).all(1)
    amax = torch.where(finite, xf.abs().amax(1), torch.zeros(()))
    _, e = torch.frexp(amax)                        # amax = m 2^e, m in [0.5, 1): floor(log2 amax) = e - 1
    X = (e.to(torch.int64) - 1 - 8).clamp(-127, 127)
    X = torch.where(amax == 0, torch.zeros_like(X), X)
    y = (xf * _pow2(-X)[:, None]).clamp(-448.0, 448.0)
    q = y.to(torch.float8_e4m3fn).view(torch.uint8)
    q = torch.where((amax == 0)[:, None], torch.zeros_like(q), q)
    q = torch.where(finite[:, None], q, torch.full_like(q, 0x7F))
    s = torch.where(finite, X + 127, torch.full_like(X, 255)).to(torch.uint8)
    return q.reshape(shp), s.reshape(*shp[:-1], shp[-1] // 32)


def dequant(q: torch.Tensor, s: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """codes [..., C] + scale codes [..., C / 32] -> values (scale code 255 -> NaN)."""
    v = q.cpu().view(torch.float8_e4m3fn).to(dtype)
    sc = torch.exp2(s.cpu().to(dtype) - 127)
    sc = torch.where(s.cpu() == 255, torch.full_like(sc, float("nan")), sc)
    return (v.reshape(*v.shape[:-1], -1, 32) * sc[..., None]).reshape(v.shape)
