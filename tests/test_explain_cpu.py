"""CPU: the host side of VQAModel.explain / Explanation.render -- the default colour table, the fp64 render reference against
F.interpolate, the plan of the backward that stops at the image features, and every refusal that needs no GPU."""
import pytest
import torch
import torch.nn.functional as F

import _explainref as R
from _pkg import pkg, sub
from oracle import vqa_oracle as O


def _small_model():
    cfg = O.full_config(vocab_size=50, num_answers=12, embed_dim=64, num_transformer_layers=1, num_cross_layers=1, ffn_hidden_dim=64)
    return pkg().load_dropin().VQAModel(**cfg, compute_dtype="fp32", seed=3).eval(), cfg


def _inputs(B=2, L=6):
    g = torch.Generator().manual_seed(1)
    return torch.randn(B, 3, 64, 64, generator=g), torch.randint(0, 50, (B, L), generator=g), torch.ones(B, L, dtype=torch.long)


def test_default_colormap_is_a_uint8_table_through_its_anchors():
    K = sub("kernels")
    lut = K.default_colormap()
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3) and lut.device.type == "cpu"
    assert lut[0].tolist() == [0, 0, 128] and lut[51].tolist() == [0, 0, 255] and lut[102].tolist() == [0, 255, 255]
    assert lut[153].tolist() == [255, 255, 0] and lut[204].tolist() == [255, 0, 0] and lut[255].tolist() == [128, 0, 0]
    assert torch.equal(lut, K.default_colormap())
    assert len({tuple(r) for r in lut.tolist()}) == 256                      # every level has a colour of its own


@pytest.mark.parametrize("src,dst", [((7, 7), (56, 56)), ((3, 3), (8, 8)), ((7, 7), (40, 64)), ((12, 12), (96, 96)), ((2, 3), (8, 12)),
                                     ((9, 5), (4, 3))])
def test_render_reference_upsamples_like_interpolate(src, dst):
    m = torch.rand((2,) + src, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    ref = F.interpolate(m[:, None], size=dst, mode="bilinear", align_corners=False)[:, 0]
    assert torch.allclose(R.upsample(m, dst), ref, rtol=0, atol=1e-12)


def test_render_reference_table_lookup_and_blend():
    lut = torch.stack([torch.arange(256), 255 - torch.arange(256), torch.full((256,), 7)], 1).to(torch.uint8)
    m = torch.tensor([[[0.0, 1.0], [float("nan"), 2.0]]])
    out = R.render(m, (2, 2), lut)
    assert out[0, 0, 0].tolist() == [0, 255, 7] and out[0, 0, 1].tolist() == [255, 0, 7]
    assert out[0, 1, 0].tolist() == [0, 255, 7] and out[0, 1, 1].tolist() == [255, 0, 7]          # NaN -> entry 0, 2 -> entry 255
    base = torch.full((1, 2, 2, 3), 100, dtype=torch.uint8)
    assert R.render(m, (2, 2), lut, base, 0.5)[0, 0, 1].tolist() == [178, 50, 54]                # floor(0.5 c + 50 + 0.5)


def test_explain_plan_stops_at_the_image_features_and_resolve_is_unchanged():
    FT, LY = sub("finetune"), sub("layout")
    pe = [e for e in LY.build_entries(O.full_config()) if e.is_param]
    pl = FT.explain_plan(pe)
    assert pl.modes == (False,) * 4 and not any(pl.trainable) and not pl.images_grad
    assert pl.no_param_grads and pl.features_grad and pl.need_dfeat and pl.need_dfused and pl.fusion_bwd
    assert not pl.text and not pl.need_denc and not pl.cnn_tape and not pl.cnn_trains and pl.cnn_low is None and pl.cnn_levels() == []
    assert all(pl.frozen(e.offset, e.numel) for e in pe)                     # no weight-gradient launch survives _frozen_g
    # what existing callers get is what they got: the new case is opt-in
    frozen = FT.Plan(pe, (False,) * len(pe), (False,) * 4, False)
    assert not frozen.need_dfeat and not frozen.fusion_bwd and not frozen.no_param_grads and not frozen.features_grad
    assert frozen.key() == ((False,) * 4, (False,) * len(pe), False) and pl.key() != frozen.key()

    class P:
        def __init__(self, rg):
            self.requires_grad = rg
    assert FT.resolve(pe, [P(True)] * len(pe), (True,) * 4, False) is None
    got = FT.resolve(pe, [P(False)] * len(pe), (False,) * 4, True)
    assert got.cnn_low == 0 and got.need_dfeat and not got.no_param_grads


def test_explain_refuses_cpu_inputs():
    m, _ = _small_model()
    images, ids, mask = _inputs()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.explain(images, ids, mask)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.explain(images, ids, mask, answers=torch.tensor([1, 2]), methods=("gradcam",))


def test_explain_checks_its_arguments_before_anything_is_launched():
    m, cfg = _small_model()
    images, ids, mask = _inputs()
    for bad in ((), ("saliency",), ("gradcam", "gradcam"), "guided"):
        with pytest.raises(ValueError, match="methods"):
            m.explain(images, ids, mask, methods=bad)
    for bad in (torch.tensor([1]), torch.tensor([[1, 2]]), torch.tensor([1, 2, 3])):
        with pytest.raises(ValueError, match="answers"):
            m.explain(images, ids, mask, answers=bad)
    with pytest.raises(ValueError, match="integers"):
        m.explain(images, ids, mask, answers=torch.tensor([1.0, 2.0]))
    with pytest.raises(IndexError):
        m.explain(images, ids, mask, answers=torch.tensor([0, cfg["num_answers"]]))
    with pytest.raises(IndexError):
        m.explain(images, ids, mask, answers=torch.tensor([-1, 0]))
    with pytest.raises(TypeError):
        m.explain(images, ids, mask, image_index=torch.tensor([0, 0]))
    with pytest.raises(RuntimeError, match="inference only"):
        m.train().explain(images, ids, mask)
    m.eval()
    cfg0 = dict(cfg, num_cross_layers=0)
    m0 = pkg().load_dropin().VQAModel(**cfg0, compute_dtype="fp32", seed=3).eval()
    with pytest.raises(ValueError, match="cross-attention"):
        m0.explain(images, ids, mask)
    with pytest.raises(RuntimeError, match="no CPU path"):                   # gradcam alone passes the checks and reaches the device test
        m0.explain(images, ids, mask, methods=("gradcam",))


def test_render_checks_its_arguments_before_anything_is_launched():
    M = pkg().load_dropin()
    ex = M.Explanation(torch.zeros(2, 12), torch.zeros(2, dtype=torch.long), torch.rand(2, 7, 7), None)
    for bad in (-0.1, 1.5, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="alpha"):
            ex.render(alpha=bad, size=(8, 8))
    with pytest.raises(ValueError, match="which"):
        ex.render("saliency", size=(8, 8))
    with pytest.raises(ValueError, match="no 'attention' map"):
        ex.render("attention", size=(8, 8))
    with pytest.raises(ValueError, match="size"):
        ex.render()                                                          # no base, no size
    for bad in (torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(3, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 8, 8, 3)):
        with pytest.raises(ValueError, match="base"):
            ex.render(base=bad)
    with pytest.raises(ValueError, match="size"):
        ex.render(base=torch.zeros(2, 8, 8, 3, dtype=torch.uint8), size=(4, 4))
    with pytest.raises(ValueError, match="colour table"):
        ex.render(size=(8, 8), colormap=torch.zeros(256, 3))
