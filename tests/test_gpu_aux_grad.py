"""GPU: graph-connected aux outputs.  forward(..., return_aux=True) under autograd returns aux tensors on the graph (as in the
reference, models/vqa_model.py:301-311): losses on them train the model, Grad-CAM style autograd.grad / retain_grad / hooks on
image_features, text_features and fused see the full gradient.  Reference for every gradient: autograd of the CPU oracle."""
import pytest
import torch

from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("image_features", "text_features", "text_pooled", "fused", "image_projected", "attended_pooled")
HEAD = "answer_head."


def _model(cfg, sd, dtype, **kw):
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype, **kw)
    m.load_state_dict(sd)
    return m.to(DEV)


def _weights(aux, seed, scale=0.05):
    """Fixed random R_k for every aux tensor (both cross layers included), on the CPU."""
    g = torch.Generator().manual_seed(seed)
    R = {k: torch.randn(tuple(aux[k].shape), generator=g) * scale for k in KEYS}
    R["cross_attention_weights"] = [torch.randn(tuple(w.shape), generator=g) * scale * 20 for w in aux["cross_attention_weights"]]
    return R


def _aux_term(aux, R):
    dev = aux["fused"].device
    t = sum((aux[k].float() * R[k].to(dev)).sum() for k in KEYS)
    return t + sum((w.float() * r.to(dev)).sum() for w, r in zip(aux["cross_attention_weights"], R["cross_attention_weights"]))


def _oracle(sd, cfg, images, ids, mask, answers, training, R, with_ce=True, autocast=False):
    names = O.parameter_names(cfg)
    sdr = {k: (v.clone().requires_grad_(True) if k in set(names) else v.clone()) for k, v in sd.items()}
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        logits, aux = O.vqa_forward(images, ids, mask, sdr, cfg, training, {})
        loss = _aux_term(aux, R)
        if with_ce:
            loss = loss + torch.nn.functional.cross_entropy(logits.float(), answers)
    loss.backward()
    return {n: (sdr[n].grad.detach().float().reshape(-1) if sdr[n].grad is not None else torch.zeros(sdr[n].numel())) for n in names}


def _check_fp32(m, cfg, ref):
    P = dict(m.named_parameters())
    worst = (0.0, None)
    for n in O.parameter_names(cfg):
        gh, gr = P[n].grad.detach().cpu().double().flatten(), ref[n].double()
        if float(gr.norm()) < 1e-12:
            assert float(gh.norm()) < 1e-9, n
            continue
        rel = float((gh - gr).norm() / gr.norm())
        worst = max(worst, (rel, n))
    assert worst[0] < 5e-2, worst


def _run(cfg, sd, B, seed, training, with_ce, image_size=224, dtype="fp32", **kw):
    images, ids, mask, answers = O.synthetic_batch(B, seed=seed, image_size=image_size, vocab=cfg["vocab_size"],
                                                   num_answers=cfg["num_answers"])
    m = _model(cfg, sd, dtype, **kw)
    m.train(training)
    logits, aux = m(images.to(DEV), ids.to(DEV), mask.to(DEV), return_aux=True)
    for k in KEYS:
        assert aux[k].grad_fn is not None, k
    assert all(w.grad_fn is not None for w in aux["cross_attention_weights"])
    R = _weights(aux, seed + 1)
    loss = _aux_term(aux, R)
    if with_ce:
        loss = loss + torch.nn.functional.cross_entropy(logits.float(), answers.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return m, (images, ids, mask, answers), R


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("with_ce", [True, False])
def test_aux_loss_gradients_match_oracle_fp32(training, with_ce):
    """CE(logits) + sum_k <R_k, aux_k> over all seven keys (and the aux-only loss): every parameter gradient within the bar of
    test_train_step_fp32_ragged_shapes_match_oracle; with the aux-only loss the head's gradients are exactly zero."""
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0) if training else O.full_config()
    sd = O.init_state_dict(cfg, 61, jitter=True)
    m, (images, ids, mask, answers), R = _run(cfg, sd, 3, 620, training, with_ce)
    ref = _oracle(sd, cfg, images, ids, mask, answers, training, R, with_ce)
    _check_fp32(m, cfg, ref)
    if not with_ce:
        for n, p in m.named_parameters():
            if n.startswith(HEAD):
                assert torch.equal(p.grad, torch.zeros_like(p.grad)), n
    # the aux term moves the gradients well beyond the bar (so the check above sees it)
    ce_only = _oracle(sd, cfg, images, ids, mask, answers, training, {k: (torch.zeros_like(v) if k != "cross_attention_weights" else
                                                                           [torch.zeros_like(w) for w in v]) for k, v in R.items()}, True)
    names = [n for n in O.parameter_names(cfg) if not n.startswith(HEAD)]
    moved = torch.cat([ref[n] - ce_only[n] for n in names]).norm() / torch.cat([ref[n] for n in names]).norm()
    assert float(moved) > 0.2


def test_aux_loss_stress_shape_144_tokens_fp32():
    """384x384 -> 144 image tokens, d = 512 (head dim 64: the 5-key-tile attention kernels), small batch, train mode."""
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0, vocab_size=500, num_answers=2000, embed_dim=512, num_transformer_layers=8,
                        num_image_tokens=144)
    sd = O.init_state_dict(cfg, 63, jitter=True)
    m, (images, ids, mask, answers), R = _run(cfg, sd, 2, 640, True, True, image_size=384)
    ref = _oracle(sd, cfg, images, ids, mask, answers, True, R, True)
    _check_fp32(m, cfg, ref)


@pytest.mark.parametrize("key", ["image_features", "text_features", "fused"])
def test_grad_wrt_aux_tensor_matches_oracle(key):
    """Grad-CAM: autograd.grad(logits[:, c].sum(), aux[key]) (the whole path from the aux tensor to the logits)."""
    cfg = O.full_config()
    sd = O.init_state_dict(cfg, 65, jitter=True)
    images, ids, mask, _ = O.synthetic_batch(3, seed=660)
    m = _model(cfg, sd, "fp32").eval()
    logits, aux = m(images.to(DEV), ids.to(DEV), mask.to(DEV), return_aux=True)
    c = int(logits[0].argmax())
    (g,) = torch.autograd.grad(logits[:, c].sum(), aux[key])
    torch.cuda.synchronize()
    lr, leaf = _oracle_with_leaf(images, ids, mask, {k: v.clone() for k, v in sd.items()}, cfg, key)
    (gr,) = torch.autograd.grad(lr[:, c].sum(), leaf)
    assert g.shape == gr.shape
    err = float((g.cpu().double() - gr.double()).norm() / gr.double().norm())
    assert err < 1e-3, err


def _oracle_with_leaf(images, ids, mask, sd, cfg, key):
    """Oracle forward with aux[key] made a leaf that the rest of the forward consumes (the oracle's parameters need no grad)."""
    feat = O.image_encoder(images, sd, False, {})
    text, _ = O.text_encoder(ids, mask, sd, cfg, False)
    if key == "image_features":
        feat = feat.detach().requires_grad_(True)
        leaf = feat
    if key == "text_features":
        text = text.detach().requires_grad_(True)
        leaf = text
    fused, _ = O.fusion(feat, text, mask, sd, cfg, False)
    if key == "fused":
        fused = fused.detach().requires_grad_(True)
        leaf = fused
    return O.answer_head(fused, sd, cfg, False), leaf


def test_retain_grad_and_hooks_see_the_total_gradient():
    """aux['image_features'].retain_grad() + a hook on aux['fused']: the total gradient of CE + aux loss, as the oracle's."""
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0)
    sd = O.init_state_dict(cfg, 67, jitter=True)
    images, ids, mask, answers = O.synthetic_batch(3, seed=680)
    m = _model(cfg, sd, "fp32").train()
    logits, aux = m(images.to(DEV), ids.to(DEV), mask.to(DEV), return_aux=True)
    R = _weights(aux, 681)
    aux["image_features"].retain_grad()
    seen = {}
    aux["fused"].register_hook(lambda g: seen.__setitem__("fused", g.detach().clone()))
    loss = torch.nn.functional.cross_entropy(logits, answers.to(DEV)) + _aux_term(aux, R)
    loss.backward()
    torch.cuda.synchronize()
    names = set(O.parameter_names(cfg))
    sdr = {k: (v.clone().requires_grad_(True) if k in names else v.clone()) for k, v in sd.items()}
    lr, auxr = O.vqa_forward(images, ids, mask, sdr, cfg, True, {})
    for k in ("image_features", "fused"):
        auxr[k].retain_grad()
    (torch.nn.functional.cross_entropy(lr, answers) + _aux_term(auxr, R)).backward()
    for got, k in ((aux["image_features"].grad, "image_features"), (seen.get("fused"), "fused")):
        assert got is not None, k
        ref = auxr[k].grad.double()
        err = float((got.cpu().double() - ref).norm() / ref.norm())
        assert err < 1e-3, (k, err)


def test_backward_twice_through_a_node_raises():
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0)
    sd = O.init_state_dict(cfg, 69, jitter=True)
    images, ids, mask, _ = O.synthetic_batch(2, seed=690)
    m = _model(cfg, sd, "fp32").train()
    logits, aux = m(images.to(DEV), ids.to(DEV), mask.to(DEV), return_aux=True)
    torch.autograd.grad(logits.sum(), aux["fused"], retain_graph=True)
    with pytest.raises(RuntimeError, match="are gone"):
        torch.autograd.grad(logits.sum(), aux["fused"])


def _bf16_bounds(got, ref, acb, names, noisy=()):
    """check_bf16_grads' bounds (tests/_bf16check.py) for gradients of an arbitrary loss."""
    rows = []
    for n, dim in names:
        rn = float(ref[n].norm())
        if rn < 1e-10:
            assert float(got[n].norm()) < 1e-6, n
            continue
        rows.append((n, float((got[n] - ref[n]).norm()) / rn, float((acb[n] - ref[n]).norm()) / rn, float(got[n].norm()) / rn, dim))
    for n, e_hip, e_acb, ratio, dim in rows:
        if n in noisy:
            assert 0.25 < ratio < 4.0, (n, ratio)
            continue
        assert e_hip <= 1.25 * e_acb + 0.10, (n, e_hip, e_acb)
        if dim >= 2 and e_acb <= 0.6:
            assert e_hip <= 0.75, (n, e_hip, e_acb)
    keys = [n for n, _ in names]
    G, Rf, A = (torch.cat([d[n] for n in keys]) for d in (got, ref, acb))
    assert float((G - Rf).norm() / Rf.norm()) <= 1.15 * float((A - Rf).norm() / Rf.norm()) + 0.02


def test_aux_loss_bf16_mfma_within_bf16_bounds():
    """The same mixed loss through the bf16 (MFMA attention) path against the fp32 oracle, held to the bounds of
    tests/_bf16check.py (the oracle under torch's own bf16 autocast sets the noise floor)."""
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0)
    sd = O.init_state_dict(cfg, 71, jitter=True)
    m, (images, ids, mask, answers), R = _run(cfg, sd, 8, 710, True, True, dtype="bf16")
    ref = _oracle(sd, cfg, images, ids, mask, answers, True, R, True)
    acb = _oracle(sd, cfg, images, ids, mask, answers, True, R, True, autocast=True)
    P = dict(m.named_parameters())
    names = [(n, P[n].dim()) for n in O.parameter_names(cfg)]
    got = {n: P[n].grad.detach().float().cpu().reshape(-1) for n, _ in names}
    noisy = tuple(f"image_encoder.stage{s}.attention.se.fc1.weight" for s in (1, 2, 3))
    _bf16_bounds(got, ref, acb, names, noisy=noisy)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_logit_loss_is_bit_equal_with_and_without_aux(dtype):
    """Dropout on, same seed: logits and the parameter gradients of a loss on the logits alone are identical between
    return_aux=False and return_aux=True; the aux path adds only the documented conversion launches."""
    cfg = O.full_config()
    sd = O.init_state_dict(cfg, 73, jitter=True)
    images, ids, mask, answers = O.synthetic_batch(4, seed=730)
    L = sub("_lib")
    results = []
    prev = L._HOOK[0]                     # (kernels.py keeps its own launch hook there: chain to it, restore it)
    for want_aux in (False, True):
        m = _model(cfg, sd, dtype, seed=5).train()
        names = []

        def hook(name, args):
            names.append(name)
            return prev(name, args) if prev is not None else None
        L._HOOK[0] = hook
        try:
            logits, aux = m(images.to(DEV), ids.to(DEV), mask.to(DEV), return_aux=want_aux)
            torch.nn.functional.cross_entropy(logits.float(), answers.to(DEV)).backward()
            torch.cuda.synchronize()
        finally:
            L._HOOK[0] = prev
        results.append((logits.detach().clone(), torch.cat([p.grad.flatten() for p in m.parameters()]), names))
    (l0, g0, n0), (l1, g1, n1) = results
    assert torch.equal(l0, l1)
    assert torch.equal(g0, g1)
    extra = list(n1)
    for n in n0:
        assert n in extra, n
        extra.remove(n)
    assert set(extra) <= {"vqa_convert", "vqa_nhwc_to_nchw", "vqa_nchw_to_nhwc", "vqa_grad_tap_add"}, sorted(set(extra))


def _oracle_fn(sd, cfg, images, ids, mask, training, loss_fn):
    names = O.parameter_names(cfg)
    sdr = {k: (v.clone().requires_grad_(True) if k in set(names) else v.clone()) for k, v in sd.items()}
    logits, aux = O.vqa_forward(images, ids, mask, sdr, cfg, training, {})
    loss_fn(logits, aux).backward()
    return {n: (sdr[n].grad.detach().float().reshape(-1) if sdr[n].grad is not None else torch.zeros(sdr[n].numel())) for n in names}


def _hip_fn(m, images, ids, mask, loss_fn):
    logits, aux = m(images.to(DEV), ids.to(DEV), mask.to(DEV), return_aux=True)
    loss_fn(logits, aux).backward()
    torch.cuda.synchronize()


_RT = torch.Generator().manual_seed(750)
_FUSED_T = torch.randn(256, 3, generator=_RT)
LOSSES = {
    # autograd hands the fusion node an expanded (stride-0) gradient for `fused`; the head is not on the path
    "fused_sum": lambda lo, aux: aux["fused"].sum(),
    # ... a transposed (non-contiguous, full-storage) one
    "fused_transposed": lambda lo, aux: (aux["fused"].t() * _FUSED_T.to(aux["fused"].device)).sum(),
    # expanded gradients on every aux tensor
    "every_key_sum": lambda lo, aux: sum(aux[k].sum() for k in KEYS) + sum(w.sum() for w in aux["cross_attention_weights"]) * 0.1,
}


@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_aux_gradients_in_any_layout_match_oracle_fp32(loss):
    """Gradients that autograd hands over expanded or transposed are read in their own layout, not as row-major memory."""
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0)
    sd = O.init_state_dict(cfg, 75, jitter=True)
    images, ids, mask, _ = O.synthetic_batch(3, seed=750)
    m = _model(cfg, sd, "fp32").train()
    _hip_fn(m, images, ids, mask, LOSSES[loss])
    _check_fp32(m, cfg, _oracle_fn(sd, cfg, images, ids, mask, True, LOSSES[loss]))
    for n, p in m.named_parameters():
        if n.startswith(HEAD):
            assert torch.equal(p.grad, torch.zeros_like(p.grad)), n


def test_a_backward_that_stops_at_an_aux_tensor_leaves_nothing_behind():
    """autograd.grad w.r.t. image_features runs the head and fusion nodes but not the encoders node: their parameter gradients
    must not surface in a later backward that reaches the parameters through image_features alone."""
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0)
    sd = O.init_state_dict(cfg, 77, jitter=True)
    images, ids, mask, _ = O.synthetic_batch(3, seed=770)
    m = _model(cfg, sd, "fp32").train()
    logits, aux = m(images.to(DEV), ids.to(DEV), mask.to(DEV), return_aux=True)
    torch.autograd.grad(logits[:, 0].sum(), aux["image_features"], retain_graph=True)
    R = torch.randn(tuple(aux["image_features"].shape), generator=torch.Generator().manual_seed(771))
    loss_fn = lambda lo, a: (a["image_features"] * R.to(a["image_features"].device)).sum()
    loss_fn(logits, aux).backward()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        if n.startswith(HEAD) or n.startswith("fusion."):
            assert torch.equal(p.grad, torch.zeros_like(p.grad)), n
    _check_fp32(m, cfg, _oracle_fn(sd, cfg, images, ids, mask, True, loss_fn))


@pytest.mark.parametrize("loss", ["logits", "aux_only", "image_features_only"])
def test_segments_are_reported_in_order_on_every_path(loss):
    """on_segment sees the same segment names in the same order as the plain backward, also when the aux loss skips parts."""
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0)
    sd = O.init_state_dict(cfg, 79, jitter=True)
    images, ids, mask, answers = O.synthetic_batch(2, seed=790)
    seen = {}
    for path in ("plain", "aux"):
        m = _model(cfg, sd, "bf16").train()
        names = []
        m._on_segment = lambda name, evs: names.append(name)
        if path == "plain":
            logits, _ = m(images.to(DEV), ids.to(DEV), mask.to(DEV))
            torch.nn.functional.cross_entropy(logits.float(), answers.to(DEV)).backward()
        else:
            logits, aux = m(images.to(DEV), ids.to(DEV), mask.to(DEV), return_aux=True)
            if loss == "logits":
                torch.nn.functional.cross_entropy(logits.float(), answers.to(DEV)).backward()
            elif loss == "aux_only":
                _aux_term(aux, _weights(aux, 791)).backward()
            else:
                aux["image_features"].float().pow(2).mean().backward()
        torch.cuda.synchronize()
        seen[path] = names
    assert seen["aux"] == seen["plain"], seen
    assert seen["plain"][:2] == ["answer_head", "fusion"]


def test_aux_loss_without_cross_attention_layers_fp32():
    """num_cross_layers = 0: cross_attention_weights is an empty stack, the image tokens feed only their aux output."""
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0, num_cross_layers=0)
    sd = O.init_state_dict(cfg, 81, jitter=True)
    m, (images, ids, mask, answers), R = _run(cfg, sd, 3, 810, True, True)
    ref = _oracle(sd, cfg, images, ids, mask, answers, True, R, True)
    _check_fp32(m, cfg, ref)
