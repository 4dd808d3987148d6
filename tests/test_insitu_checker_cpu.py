"""CPU: negative controls of the in-situ checker (tests/_insitu.py).  A bf16-stored conv output of a batch large enough that the
global relative norm alone is blind to a one-channel error must pass as stored, and fail with the last image's rows zeroed or
with one channel scaled by 1 + 2^-5."""
import torch
import torch.nn.functional as F

from _insitu import Checker, nchw, rnd, slice_errors


def _stored_conv(B=96, C=128, H=12, W=12, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(B, C, H, W, generator=g))
    w = rnd(torch.randn(C, C, 3, 3, generator=g) / 24)
    ref = F.conv2d(x, w, padding=1)
    # what a correct bf16 kernel hands out: the fp32 result rounded once, in the engine's [B*H*W, C] layout
    stored = rnd(ref).permute(0, 2, 3, 1).reshape(B * H * W, C).to(torch.bfloat16)
    return stored, ref, (B, H, W)


def test_checker_accepts_a_correctly_rounded_tensor():
    stored, ref, (B, H, W) = _stored_conv()
    ck = Checker()
    ck.check("y", nchw(stored, B, H, W), ref, 4e-3)
    ck.finish("control")


def test_checker_rejects_the_last_image_zeroed():
    stored, ref, (B, H, W) = _stored_conv()
    bad = stored.clone()
    bad[(B - 1) * H * W:] = 0                                        # the last image's rows (a skipped tail round)
    ck = Checker()
    ck.check("y", nchw(bad, B, H, W), ref, 4e-3)
    assert f"dim0[{B - 1}]" in [f[1] for f in ck.fails], ck.fails       # the last image itself is named
    assert float(slice_errors(nchw(bad, B, H, W), ref, 0)[B - 1]) > 0.99


def test_checker_rejects_one_channel_scaled_where_the_global_norm_cannot():
    stored, ref, (B, H, W) = _stored_conv()
    c = 77
    bad = stored.float()
    bad[:, c] *= 1 + 2 ** -5
    bad = bad.to(torch.bfloat16)
    got = nchw(bad, B, H, W)
    glob = float((got - ref).norm() / ref.norm())
    assert glob < 4e-3, glob                                         # the global relative norm alone passes it ...
    ck = Checker()
    ck.check("y", got, ref, 4e-3)
    assert len(ck.fails) == 1 and ck.fails[0][1] == f"dim1[{c}]", ck.fails      # ... the per-channel check does not
    assert ck.fails[0][2] > 2 ** -5 * 0.9


def test_checker_rejects_nan():
    stored, ref, (B, H, W) = _stored_conv()
    bad = stored.clone()
    bad[5, 3] = float("nan")
    ck = Checker()
    ck.check("y", nchw(bad, B, H, W), ref, 4e-3)
    assert ck.fails


def test_near_zero_slices_are_measured_against_the_floor():
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(8, 16, 4, 4, generator=g)
    ref[:, 3] *= 1e-6                                                # a dead channel: relative rounding noise there stays small
    got = ref + 1e-3 * ref.abs().mean() * torch.randn(ref.shape, generator=g) / 1e2
    ck = Checker()
    ck.check("y", got, ref, 4e-3)
    ck.finish("floor")
