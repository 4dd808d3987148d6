"""GPU: VQAModel.explain / Explanation.render end to end.

fp32 against the route that existed before (forward(return_aux=True) + autograd.grad on aux["image_features"], CAM in fp64) within
the kernel bound of tests/test_gpu_explain_kernels.py, and against the CPU oracle within 2e-3 * |S'|_2 per image (the project's 1e-3
bars for that gradient and for fp32 forward parity, added); bf16 held to tests/_bf16check.py's form against the oracle under torch's
bf16 autocast; ByteImages bit for bit; and nothing else moves: gradients, buffers, parameters, tapes, the captured inference graph,
a HipTrainer run with an explain() between two of its steps.
Two shapes, each built once: B = 3 at 224 x 224 (the 7 x 7 grid) and B = 2 at 384 x 384 with 144 image tokens and d = 512."""
import pytest
import torch

import _explainref as R
from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = {
    "224": dict(cfg=dict(), B=3, size=224, seed=71),
    "384": dict(cfg=dict(vocab_size=500, num_answers=2000, embed_dim=512, num_transformer_layers=2, num_image_tokens=144), B=2,
                size=384, seed=73),
}
_CACHE = {}


def _model(cfg, sd, dtype):
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _case(name):
    """Configuration, weights, batch and the fp32 model of a shape: made once, never written."""
    if name not in _CACHE:
        c = CASES[name]
        cfg = O.full_config(**c["cfg"])
        sd = O.init_state_dict(cfg, c["seed"], jitter=True)
        images, ids, mask, answers = O.synthetic_batch(c["B"], seed=10 * c["seed"], image_size=c["size"], vocab=cfg["vocab_size"],
                                                       num_answers=cfg["num_answers"])
        _CACHE[name] = dict(cfg=cfg, sd=sd, cpu=(images, ids, mask, answers), dev=tuple(t.to(DEV) for t in (images, ids, mask, answers)),
                            fp32=_model(cfg, sd, "fp32"))
    return _CACHE[name]


def _oracle_cam(name, autocast=False):
    """(cam, S') of the CPU oracle for the batch's answers, through test_gpu_aux_grad.py's _oracle_with_leaf construction: the image
    features made a leaf that the rest of the forward consumes."""
    key = (name, "oracle", autocast)
    if key not in _CACHE:
        c = _case(name)
        cfg, sd = c["cfg"], {k: v.clone() for k, v in c["sd"].items()}
        images, ids, mask, answers = c["cpu"]
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            feat = O.image_encoder(images, sd, False, {}).detach().requires_grad_(True)
            text, _ = O.text_encoder(ids, mask, sd, cfg, False)
            fused, _ = O.fusion(feat, text, mask, sd, cfg, False)
            logits = O.answer_head(fused, sd, cfg, False)
            (g,) = torch.autograd.grad(logits.float()[torch.arange(len(answers)), answers].sum(), feat)
        _CACHE[key] = R.gradcam_nchw(feat.detach(), g)
    return _CACHE[key]


def _per_image(t):
    return t.reshape(t.shape[0], -1).double().norm(dim=1)


# ------------------------------------------------------------------------------------------------ fp32
@pytest.mark.parametrize("name", list(CASES))
def test_fp32_gradcam_and_logits_match_the_autograd_route(name):
    c = _case(name)
    m = c["fp32"]
    images, ids, mask, answers = c["dev"]
    logits, aux = m(images, ids, mask, return_aux=True)                       # eval mode under autograd: the taped forward
    (g,) = torch.autograd.grad(logits[torch.arange(len(answers)), answers].sum(), aux["image_features"])
    ref, sprime = R.gradcam_nchw(aux["image_features"].detach(), g)
    ex = m.explain(images, ids, mask, answers=answers, normalize=False)
    torch.cuda.synchronize()
    n = int(round(c["cfg"].get("num_image_tokens", 49) ** 0.5))
    assert tuple(ex.gradcam.shape) == (len(answers), n, n) and ex.gradcam.dtype == torch.float32 and ex.gradcam.is_cuda
    assert tuple(ex.attention.shape) == (len(answers), n, n) and ex.attention.dtype == torch.float32
    assert ex.logits.dtype == torch.float32 and torch.equal(ex.logits, logits.detach())
    assert ex.answers.dtype == torch.int64 and torch.equal(ex.answers, answers)
    err = (ex.gradcam.double() - ref).abs()
    print(f"{name}: max |cam - cam_autograd| / S' = {float((err / sprime.clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= 1e-4 * sprime).all())
    assert bool((ref > 0).any()) and float(_per_image(ref).min()) > 0            # every image has a map to compare
    # the same under no_grad, and normalised: each map divided by its maximum
    with torch.no_grad():
        ex2 = m.explain(images, ids, mask, answers=answers, normalize=True)
    mx = ex.gradcam.flatten(1).amax(1)[:, None, None]
    assert torch.equal(ex2.gradcam, torch.where(mx > 0, ex.gradcam / mx, ex.gradcam)) and torch.equal(ex2.logits, ex.logits)


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_matches_the_cpu_oracle(name):
    c = _case(name)
    m = c["fp32"]
    images, ids, mask, answers = c["dev"]
    ref, sprime = _oracle_cam(name)
    ex = m.explain(images, ids, mask, answers=answers, normalize=False)
    ratio = _per_image(ex.gradcam.cpu() - ref) / _per_image(sprime)
    print(f"{name}: |cam - cam_oracle|_2 / |S'_oracle|_2 per image = {[f'{v:.2e}' for v in ratio.tolist()]}")
    assert bool((ratio <= 2e-3).all())
    assert float(_per_image(ref).min()) > 0
    # answers=None explains the arg-max of this call's own logits
    auto = m.explain(images, ids, mask, methods=("gradcam",), normalize=False)
    assert auto.attention is None and torch.equal(auto.answers, auto.logits.argmax(1)) and torch.equal(auto.logits, ex.logits)
    same = m.explain(images, ids, mask, answers=auto.answers.cpu().int(), methods="gradcam", normalize=False)      # CPU ids, another dtype
    assert torch.equal(same.gradcam, auto.gradcam) and torch.equal(same.answers, auto.answers)
    # attention: the masked token mean of get_attention_maps()["cross_attention_spatial"]
    with torch.no_grad():
        vis = m.get_attention_maps(images, ids, mask)["cross_attention_spatial"].double()          # [B, L, n, n]
    w = mask.double()
    want = (vis * w[:, :, None, None]).sum(1) / w.sum(1)[:, None, None]
    err = float((ex.attention.double() - want).abs().max())
    print(f"{name}: max |attention - token mean of get_attention_maps| = {err:.2e}")
    assert err <= 1e-5
    assert bool(((ex.attention.flatten(1).sum(1) - 1).abs() <= 1e-5).all())
    only = m.explain(images, ids, mask, methods=("attention",), normalize=False)
    assert only.gradcam is None and torch.equal(only.attention, ex.attention)


# ------------------------------------------------------------------------------------------------ bf16
def _bf16_model():
    if "bf16" not in _CACHE:
        c = _case("224")
        _CACHE["bf16"] = _model(c["cfg"], c["sd"], "bf16")
    return _CACHE["bf16"]


def test_bf16_gradcam_within_the_noise_of_torch_autocast():
    """e = |cam - cam_fp32| / |cam_fp32| per image against the fp32 oracle's CAM, for the HIP bf16 model and for the oracle under
    torch's bf16 autocast: e_hip <= 1.25 * e_autocast + 0.10 (tests/_bf16check.py's form)."""
    c = _case("224")
    images, ids, mask, answers = c["dev"]
    ref, _ = _oracle_cam("224")
    acb, _ = _oracle_cam("224", autocast=True)
    ex = _bf16_model().explain(images, ids, mask, answers=answers, normalize=False)
    e_hip = _per_image(ex.gradcam.cpu() - ref) / _per_image(ref)
    e_acb = _per_image(acb - ref) / _per_image(ref)
    print(f"bf16 Grad-CAM per image: e_hip = {[f'{v:.3f}' for v in e_hip.tolist()]}, e_autocast = {[f'{v:.3f}' for v in e_acb.tolist()]}")
    assert bool((e_hip <= 1.25 * e_acb + 0.10).all())
    assert torch.equal(ex.answers, answers) and bool(torch.isfinite(ex.logits).all())


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_byte_images_give_the_same_bits(dtype):
    BI = pkg().load_dropin_byte_images().ByteImages
    c = _case("224")
    m = _bf16_model() if dtype == "bf16" else c["fp32"]
    _, ids, mask, answers = c["dev"]
    u8 = torch.randint(0, 256, (len(answers), 224, 224, 3), generator=torch.Generator().manual_seed(5), dtype=torch.int64).to(torch.uint8).to(DEV)
    a = m.explain(BI(u8), ids, mask)
    b = m.explain(BI(u8).to_float(), ids, mask)
    for got, want in zip(a, b):
        assert torch.equal(got, want)
    assert bool((a.gradcam.flatten(1).amax(1) == 1).all()) and bool((a.attention.flatten(1).amax(1) == 1).all())


# ------------------------------------------------------------------------------------------------ nothing is disturbed
def _bn(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}


def test_explain_leaves_the_model_as_it_was():
    c = _case("224")
    m = _model(c["cfg"], c["sd"], "bf16")
    images, ids, mask, answers = c["dev"]
    with torch.no_grad():
        before = m(images, ids, mask)[0].clone()                              # B <= 64: the captured graph of this shape
        top_before = m.predict(images, ids, mask, top_k=3)
    flat, bn, tapes = m._flat.detach().clone(), _bn(m), len(m._tapes)
    assert all(p.grad is None for p in m.parameters())
    m.explain(images, ids, mask)
    m.explain(images, ids, mask, answers=answers)
    assert all(p.grad is None for p in m.parameters())                        # None stays None
    m(images, ids, mask)[0].sum().backward()                                  # now every parameter holds a gradient
    grads = [p.grad.detach().clone() for p in m.parameters()]
    ex = m.explain(images, ids, mask)
    torch.cuda.synchronize()
    assert not ex.logits.requires_grad and not ex.gradcam.requires_grad
    assert all(torch.equal(p.grad, g) for p, g in zip(m.parameters(), grads))
    assert torch.equal(m._flat, flat) and not m.training and len(m._tapes) == tapes
    now = _bn(m)
    assert all(torch.equal(now[k], bn[k]) for k in bn)
    with torch.no_grad():
        assert torch.equal(m(images, ids, mask)[0], before)
        top_after = m.predict(images, ids, mask, top_k=3)
    assert torch.equal(top_after[0], top_before[0]) and torch.equal(top_after[1], top_before[1])


def test_explain_between_two_training_steps_changes_nothing():
    """Four HipTrainer steps, dropout on, bf16, with an explain() between steps 2 and 3: loss, logits, parameters and both moments
    equal those of the run without it, bit for bit."""
    c = _case("224")
    T = sub("trainer").HipTrainer
    batches = []
    for k in range(4):
        images, ids, mask, answers = O.synthetic_batch(4, seed=900 + k)
        mask[:, 0] = 1
        batches.append(tuple(t.to(DEV) for t in (images, ids, mask, answers)))

    def run(with_explain):
        m = _model(c["cfg"], c["sd"], "bf16").train()
        tr = T(m)
        rec = []
        for k, (images, ids, mask, answers) in enumerate(batches):
            if with_explain and k == 2:
                m.eval()
                ex = m.explain(*batches[0][:3])
                assert bool(torch.isfinite(ex.gradcam).all())
                m.train()
            loss, logits = tr.step(images, ids, mask, answers)
            rec.append((loss.clone(), logits.clone()))
        torch.cuda.synchronize()
        return rec, m._flat.detach().clone(), tr.m.clone(), tr.v.clone(), _bn(m)

    ra, fa, ma, va, ba = run(False)
    rb, fb, mb, vb, bb = run(True)
    for k, ((la, ga), (lb, gb)) in enumerate(zip(ra, rb)):
        assert torch.equal(la, lb) and torch.equal(ga, gb), k
    assert torch.equal(fa, fb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert all(torch.equal(ba[k], bb[k]) for k in ba)
    assert c["cfg"]["dropout"] > 0 and not torch.equal(ra[0][1], ra[1][1])


# ------------------------------------------------------------------------------------------------ errors, render
def test_explain_errors_on_the_device():
    c = _case("224")
    m = c["fp32"]
    images, ids, mask, answers = c["dev"]
    try:
        with pytest.raises(RuntimeError, match="inference only"):
            m.train().explain(images, ids, mask)
    finally:
        m.eval()
    bad = answers.clone()
    bad[1] = m.num_answers
    with pytest.raises(IndexError):
        m.explain(images, ids, mask, answers=bad)                             # a device tensor: one read for the range check
    with pytest.raises(TypeError):
        m.explain(images, ids, mask, image_index=torch.zeros(len(answers), dtype=torch.long, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.explain(images.cpu(), ids, mask)
    cfg0 = O.full_config(num_cross_layers=0)
    m0 = _model(cfg0, O.init_state_dict(cfg0, 75, jitter=True), "fp32")
    with pytest.raises(ValueError, match="cross-attention"):
        m0.explain(images, ids, mask)
    ex0 = m0.explain(images, ids, mask, methods=("gradcam",))                  # without cross-attention the image does not reach the logits
    assert torch.equal(ex0.gradcam, torch.zeros_like(ex0.gradcam))


def test_render_is_the_kernel_call_it_stands_for():
    K = sub("kernels")
    BI = pkg().load_dropin_byte_images().ByteImages
    c = _case("224")
    images, ids, mask, answers = c["dev"]
    B = len(answers)
    u8 = torch.randint(0, 256, (B, 224, 224, 3), generator=torch.Generator().manual_seed(6), dtype=torch.int64).to(torch.uint8).to(DEV)
    ex = c["fp32"].explain(BI(u8), ids, mask)
    out = ex.render(base=BI(u8))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, 224, 224, 3) and out.is_cuda
    assert torch.equal(out, K.heatmap_render(ex.gradcam, base=u8, alpha=0.5))
    assert torch.equal(out, ex.render("gradcam", base=u8, size=(224, 224)))
    # against fp64: neighbouring entries of the default table differ by at most 5 levels, so an index off by one moves the blend by 2.5
    assert int((out.int() - R.render(ex.gradcam, (224, 224), K.default_colormap(), u8, 0.5).int()).abs().max()) <= 3
    grey = torch.arange(256, dtype=torch.uint8)[:, None].repeat(1, 3)
    att = ex.render("attention", alpha=0.3, colormap=grey, base=u8)
    assert torch.equal(att, K.heatmap_render(ex.attention, base=u8, alpha=0.3, colormap=grey.to(DEV)))
    assert int((att.int() - R.render(ex.attention, (224, 224), grey, u8, 0.3).int()).abs().max()) <= 1
    small = ex.render("attention", size=(28, 28))
    assert tuple(small.shape) == (B, 28, 28, 3) and torch.equal(small, K.heatmap_render(ex.attention, size=(28, 28)))
    for bad in (u8[:, :, :, :2], u8[:1], u8.permute(0, 3, 1, 2).contiguous(), u8.float()):
        with pytest.raises(ValueError, match="base"):
            ex.render(base=bad)
    with pytest.raises(ValueError, match="size"):
        ex.render()
