"""Fine-tuning with frozen parts on the GPU: requires_grad and per-part eval() honoured by HipTrainer and by loss.backward(), checked
against the functional oracle composed per part with torch autograd, torch.optim.AdamW and clip_grad_norm_ over the trainable
tensors; the launches the backward skips are counted through the _lib.call hook."""
import pytest
import torch
import torch.nn.functional as F

from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = O.full_config(dropout=0.0, answer_dropout=0.0, vocab_size=100, num_answers=10, embed_dim=32)
CNN_KERNELS = ("vqa_conv", "vqa_wgrad3x3", "vqa_bn_", "vqa_se_bwd", "vqa_spatial_bwd", "vqa_stem_", "vqa_dgrad_s2")
WGRAD_KERNELS = ("vqa_wgrad", "vqa_wgrad_group", "vqa_wgrad3x3_c64", "vqa_wgrad3x3_c64_bn", "vqa_wgrad3x3_c128", "vqa_stem_wgrad",
                 "vqa_stem_wgrad_fused", "vqa_embed_bwd")


def _model(sd, dtype="fp32"):
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _batch(seed, B=4):
    return O.synthetic_batch(B, seed=seed, image_size=64, seq_len=10, vocab=100, num_answers=10)


class _Oracle:
    """OracleTrainer's step with per-part modes: frozen tensors have requires_grad False, so AdamW and clip_grad_norm_ skip them."""

    def __init__(self, sd, lr, frozen=lambda n: False):
        self.names = O.parameter_names(CFG)
        self.sd = {k: v.clone() for k, v in sd.items()}
        self.params = [self.sd[k] for k in self.names]
        self.set_frozen(frozen)
        self.opt = torch.optim.AdamW(self.params, lr=lr, weight_decay=0.01)

    def set_frozen(self, frozen):
        for n in self.names:
            self.sd[n].requires_grad_(not frozen(n))

    def logits(self, images, ids, mask, modes, nb):
        cnn, txt, fus, head = modes
        feat = O.image_encoder(images, self.sd, cnn, nb)
        text, _ = O.text_encoder(ids, mask, self.sd, CFG, txt)
        fused, _ = O.fusion(feat, text, mask, self.sd, CFG, fus)
        return O.answer_head(fused, self.sd, CFG, head)

    def step(self, images, ids, mask, answers, modes):
        self.opt.zero_grad(set_to_none=True)
        nb = {}
        loss = F.cross_entropy(self.logits(images, ids, mask, modes, nb), answers)
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p for p in self.params if p.grad is not None], 1.0)
        self.opt.step()
        self.sd.update(nb)
        return float(loss.detach())


def _track(m, ot, start, trainable, rel):
    P = dict(m.named_parameters())
    for n in ot.names:
        if not trainable(n):
            continue
        moved = (ot.sd[n].detach() - start[n]).norm().item()
        err = (P[n].detach().cpu() - ot.sd[n].detach()).norm().item()
        assert err <= rel * moved + 1e-7, (n, err, moved)


@pytest.mark.parametrize("dtype,loss_tol,rel", [("fp32", 2e-4, 0.15), ("bf16", 3e-2, 0.6)])
def test_frozen_backbone_hiptrainer_tracks_the_oracle(dtype, loss_tol, rel):
    sd = O.init_state_dict(CFG, 13, jitter=True)
    m = _model(sd, dtype)
    m.image_encoder.requires_grad_(False)
    m.image_encoder.eval()
    cnn_before = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("image_encoder.")}
    tr = pkg().trainer.HipTrainer(m, lr=1e-3)
    frozen = lambda n: n.startswith("image_encoder.")
    ot = _Oracle(sd, 1e-3, frozen)
    start = {n: sd[n].clone() for n in ot.names}
    for step in range(3):
        images, ids, mask, answers = _batch(500 + step)
        lo = ot.step(images, ids, mask, answers, (False, True, True, True))
        loss, _ = tr.step(images.to(DEV), ids.to(DEV), mask.to(DEV), answers.to(DEV))
        torch.cuda.synchronize()
        assert abs(float(loss.item()) - lo) < loss_tol * (step + 1), (step, float(loss.item()), lo)
    st = m.state_dict()
    for k, v in cnn_before.items():                 # CNN parameters and BatchNorm buffers bit-unchanged
        assert torch.equal(st[k], v), k
    _track(m, ot, start, lambda n: not frozen(n), rel)
    if dtype == "bf16":                             # the operand copy the range kernel wrote equals a fresh cast
        assert torch.equal(tr.engine.wsrc, m._flat.to(torch.bfloat16))


def _grads(m):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}


def _loss_backward(m, batch, images_grad=False):
    images, ids, mask, answers = [t.to(DEV) for t in batch]
    if images_grad:
        images = images.clone().requires_grad_(True)
    logits, _ = m(images, ids, mask)
    F.cross_entropy(logits, answers).backward()
    torch.cuda.synchronize()
    return images


def test_frozen_backbone_through_loss_backward():
    sd = O.init_state_dict(CFG, 17, jitter=True)
    batch = _batch(700)
    trainable = lambda n: not n.startswith("image_encoder.")
    # train-mode CNN (fp32): the untaped CNN forward is the taped one's arithmetic, so the trainable gradients are bit-equal
    a, b = _model(sd), _model(sd)
    a.image_encoder.requires_grad_(False)
    _loss_backward(a, batch); _loss_backward(b, batch)
    ga, gb = _grads(a), _grads(b)
    for n in ga:
        if trainable(n):
            assert torch.equal(ga[n], gb[n]), n
        else:
            assert ga[n] is None, n
    # eval-mode CNN: Conv+BN-folded route against the taped eval route of an all-trainable model
    a, b = _model(sd), _model(sd)
    for mm in (a, b):
        mm.image_encoder.eval()
    a.image_encoder.requires_grad_(False)
    _loss_backward(a, batch); _loss_backward(b, batch)
    ga, gb = _grads(a), _grads(b)
    for n in ga:
        if trainable(n):
            scale = max(float(gb[n].abs().max()), 1e-6)
            assert float((ga[n] - gb[n]).abs().max()) <= 2e-3 * scale + 1e-6, n
        else:
            assert ga[n] is None, n


class _Calls:
    def __init__(self):
        self.names = []

    def __enter__(self):
        L = sub("_lib")
        self._old = L._HOOK[0]
        L._HOOK[0] = lambda name, args: self.names.append(name)
        return self

    def __exit__(self, *a):
        sub("_lib")._HOOK[0] = self._old


def _backward_calls(m, batch, images_grad=False):
    images, ids, mask, answers = [t.to(DEV) for t in batch]
    if images_grad:
        images = images.clone().requires_grad_(True)
    logits, _ = m(images, ids, mask)
    loss = F.cross_entropy(logits, answers)
    torch.cuda.synchronize()
    with _Calls() as c:
        loss.backward()
        torch.cuda.synchronize()
    return c.names, images


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_backward_skips_frozen_launches(dtype):
    sd = O.init_state_dict(CFG, 19, jitter=True)
    batch = _batch(710)
    # CNN frozen, no image gradient: no CNN kernel in the backward
    m = _model(sd, dtype)
    m.image_encoder.requires_grad_(False)
    names, _ = _backward_calls(m, batch)
    assert not [n for n in names if n.startswith(CNN_KERNELS)], sorted(set(names))
    assert "vqa_embed_bwd" in names
    # stages 1-2 and the stem frozen: no stage-1/2 block and no stem launch
    m = _model(sd, dtype)
    for part in (m.image_encoder.stem, m.image_encoder.stage1, m.image_encoder.stage2):
        part.requires_grad_(False)
    m._ensure_engine().capture = {}
    names, _ = _backward_calls(m, batch)
    ran = set(m._engine.capture)
    m._engine.capture = None
    assert ran and all(k.startswith(("image_encoder.stage3.", "image_encoder.stage4.")) for k in ran), ran
    assert not [n for n in names if n.startswith("vqa_stem_")]
    # the embedding frozen: no vqa_embed_bwd
    m = _model(sd, dtype)
    m.text_encoder.token_embedding.requires_grad_(False)
    names, _ = _backward_calls(m, batch)
    assert "vqa_embed_bwd" not in names and "vqa_attention_bwd" in "".join(names)
    # a frozen model under saliency: no weight-gradient launch, the image gradient bit-equal to the full backward's
    m = _model(sd, dtype)
    m.requires_grad_(False)
    names, x = _backward_calls(m, batch, images_grad=True)
    assert not [n for n in names if n in WGRAD_KERNELS], sorted(set(names))
    ref = _model(sd, dtype)
    _, xr = _backward_calls(ref, batch, images_grad=True)
    assert torch.equal(x.grad, xr.grad)


def test_mixed_modes_cnn_eval_rest_train():
    sd = O.init_state_dict(CFG, 23, jitter=True)
    m = _model(sd)
    m.train(); m.image_encoder.eval()
    images, ids, mask, answers = _batch(720)
    run_before = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    logits, _ = m(images.to(DEV), ids.to(DEV), mask.to(DEV))
    F.cross_entropy(logits, answers.to(DEV)).backward()
    torch.cuda.synchronize()
    st = m.state_dict()
    for k, v in run_before.items():
        assert torch.equal(st[k], v), k
    ot = _Oracle(sd, 1e-3)
    with torch.no_grad():
        ref = ot.logits(images, ids, mask, (False, True, True, True), None)
    assert float((logits.detach().cpu() - ref).abs().max()) < 1e-3 * max(1.0, float(ref.abs().max()))
    # and the same without autograd
    with torch.no_grad():
        l2, _ = m(images.to(DEV), ids.to(DEV), mask.to(DEV))
    assert float((l2.cpu() - ref).abs().max()) < 1e-3 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_trainable_set_changing_mid_run(dtype):
    sd = O.init_state_dict(CFG, 29, jitter=True)
    m = _model(sd, dtype)
    tr = pkg().trainer.HipTrainer(m, lr=1e-3)
    frozen = lambda n: n.startswith("text_encoder.")
    ot = _Oracle(sd, 1e-3, frozen)
    start = {n: sd[n].clone() for n in ot.names}
    m.text_encoder.requires_grad_(False)
    for step in range(4):
        if step == 2:
            m.text_encoder.requires_grad_(True)
            ot.set_frozen(lambda n: False)
        images, ids, mask, answers = _batch(800 + step)
        ot.step(images, ids, mask, answers, (True,) * 4)
        tr.step(images.to(DEV), ids.to(DEV), mask.to(DEV), answers.to(DEV))
    torch.cuda.synchronize()
    if dtype == "fp32":
        _track(m, ot, start, lambda n: True, 0.15)
        # moments and per-parameter step counts: text-encoder tensors took 2 AdamW steps, the rest 4
        LY = sub("layout")
        ents = {e.name: e for e in m._param_entries}
        for n, p in zip(ot.names, ot.params):
            s = ot.opt.state[p]
            assert int(s["step"]) == (2 if frozen(n) else 4), n
            mv = LY.view_of(tr.m, ents[n]).cpu()
            ref = s["exp_avg"]
            assert float((mv - ref).norm()) <= 0.15 * float(ref.norm()) + 1e-9, n
        assert tr._lag.cpu().tolist() == [2 if frozen(e.name) else 0 for e in m._param_entries]
    else:
        assert torch.equal(tr.engine.wsrc, m._flat.to(torch.bfloat16))


def test_grouped_step_with_frozen_cnn_matches_the_expanded_step():
    sd = O.init_state_dict(CFG, 31, jitter=True)
    idx = [0, 0, 1, 2, 2, 2]
    images, ids, mask, answers = _batch(900, B=len(idx))
    imgs_u = images[:3]
    a, b = _model(sd), _model(sd)
    for mm in (a, b):
        mm.image_encoder.requires_grad_(False)
        mm.image_encoder.eval()
    ta, tb = pkg().trainer.HipTrainer(a, lr=1e-3), pkg().trainer.HipTrainer(b, lr=1e-3)
    la, _ = ta.step(imgs_u.to(DEV), ids.to(DEV), mask.to(DEV), answers.to(DEV), image_index=torch.tensor(idx))
    lb, _ = tb.step(imgs_u[idx].to(DEV), ids.to(DEV), mask.to(DEV), answers.to(DEV))
    torch.cuda.synchronize()
    assert abs(float(la) - float(lb)) < 1e-4
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    for n in pa:
        assert float((pa[n] - pb[n]).abs().max()) < 1e-5, n
