"""fp64 torch references of the explain kernels (csrc/explain_ops.hip; include/vqa_hip.h has the formulas), on whatever device
their operands live.  Shared by tests/test_explain_cpu.py, tests/test_gpu_explain_kernels.py and tests/test_gpu_explain_model.py."""
import torch


def class_seed(logits, ids=None):
    """(chosen int64 [B], one-hot fp64 [B][N]).  Arg-max in vqa_softmax_topk's order: a NaN first, then the value descending, ties to
    the lower index."""
    x = logits.double()
    B, N = x.shape
    if ids is None:
        key = torch.where(torch.isnan(x), torch.full_like(x, float("inf")), x)
        first_nan = torch.isnan(x).int().argmax(1)
        has_nan = torch.isnan(x).any(1)
        best = (key == key.max(1, keepdim=True).values).int().argmax(1)          # the first index that holds the maximum
        ids = torch.where(has_nan, first_nan, best)
    onehot = torch.zeros((B, N), dtype=torch.float64, device=x.device)
    onehot[torch.arange(B, device=x.device), ids.long()] = 1.0
    return ids.long(), onehot


def gradcam(feat, dfeat, normalize=False):
    """feat, dfeat [B][P][C] -> (cam fp64 [B][P], S' fp64 [B][P]) with S' = sum_c mean_p |dfeat| * |feat|, the scale of the kernel's
    rounding error: |cam_fp32 - cam| <= (P + C + 3) * 2^-24 * S'."""
    f, g = feat.double(), dfeat.double()
    cam = torch.relu((g.mean(1, keepdim=True) * f).sum(2))
    sprime = (g.abs().mean(1, keepdim=True) * f.abs()).sum(2)
    if normalize:
        mx = cam.amax(1, keepdim=True)
        cam = torch.where(mx > 0, cam / mx, cam)
    return cam, sprime


def gradcam_nchw(feat, grad):
    """The same from NCHW tensors [B][C][H][W] (aux["image_features"] and its gradient): (cam [B][H][W], S' [B][H][W])."""
    B, C, H, W = feat.shape
    to = lambda t: t.reshape(B, C, H * W).transpose(1, 2)
    cam, sp = gradcam(to(feat), to(grad))
    return cam.view(B, H, W), sp.view(B, H, W)


def attention_map(caw, mask=None, normalize=False):
    """caw [ncl][B][H][L][P], mask [B][L] (non-zero = real token) or None -> fp64 [B][P]; 0 / 0 = NaN without a real token."""
    w = caw.double()
    ncl, B, H, L, P = w.shape
    m = torch.ones((B, L), dtype=torch.float64, device=w.device) if mask is None else (mask != 0).double()
    s = (w * m[None, :, None, :, None]).sum((0, 2, 3))
    out = s / (ncl * H * m.sum(1))[:, None]
    if normalize:
        mx = torch.nan_to_num(out, nan=0.0).amax(1, keepdim=True)
        out = torch.where(mx > 0, out / mx, out)
    return out


def _source(n_out, n_in, device):
    s = ((torch.arange(n_out, dtype=torch.float64, device=device) + 0.5) * n_in / n_out - 0.5).clamp_min(0.0)
    i0 = s.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, s - i0.double()


def upsample(maps, size):
    """Bilinear sample of maps [B][Hm][Wm] at F.interpolate's align_corners=False source positions, fp64 [B][H][W]."""
    m = maps.double()
    H, W = size
    y0, y1, wy = _source(H, m.shape[1], m.device)
    x0, x1, wx = _source(W, m.shape[2], m.device)
    top = m[:, y0][:, :, x0] * (1 - wx) + m[:, y0][:, :, x1] * wx
    bot = m[:, y1][:, :, x0] * (1 - wx) + m[:, y1][:, :, x1] * wx
    return top * (1 - wy)[None, :, None] + bot * wy[None, :, None]


def render(maps, size, lut, base=None, alpha=0.5):
    """vqa_heatmap_render in fp64: uint8 [B][H][W][3]."""
    t = upsample(maps, size)
    idx = torch.nan_to_num((t * 255 + 0.5).floor(), nan=0.0).clamp(0, 255).long()
    col = lut.to(maps.device).double()[idx]                                   # [B][H][W][3]
    if base is None:
        return col.to(torch.uint8)
    return (alpha * col + (1 - alpha) * base.double() + 0.5).floor().clamp(0, 255).to(torch.uint8)
