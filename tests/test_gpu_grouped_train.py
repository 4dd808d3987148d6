"""GPU: many questions per image in TRAINING -- VQAModel.forward_grouped and HipTrainer.step(image_index=) -- against the oracle
composition fusion(image_encoder(images)[image_index], text, ...) with autograd, bit-equal to forward() for the identity index
(dropout on), the eval-mode gradients against the expanded forward, bf16 reproducibility, the trainer against a torch AdamW step
and the errors of the API."""
import pytest
import torch
import torch.nn.functional as F

from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDX = [2, 0, 0, 2, 2, 0, 2]              # U = 3 images, N = 7 questions: repeats, out of order, image 1 never asked about


def _model(dtype, cfg, seed=11):
    sd = O.init_state_dict(cfg, seed, jitter=True)
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.to(DEV), sd


def _batch(U, N, image_size=224, seed=5):
    images, _, _, _ = O.synthetic_batch(U, seed=seed, image_size=image_size)
    _, ids, mask, answers = O.synthetic_batch(N, seed=seed + 1)
    mask[:, 0] = 1
    return images, ids, mask, answers


def _oracle_step(sd, cfg, images, ids, mask, answers, index):
    names = set(O.parameter_names(cfg))
    sdr = {k: (v.clone().requires_grad_(True) if k in names else v.clone()) for k, v in sd.items()}
    nb = {}
    feat = O.image_encoder(images, sdr, True, nb)
    text, _ = O.text_encoder(ids, mask, sdr, cfg, True)
    fused, _ = O.fusion(feat[torch.as_tensor(index)], text, mask, sdr, cfg, True)
    logits = O.answer_head(fused, sdr, cfg, True)
    loss = F.cross_entropy(logits, answers)
    loss.backward()
    return sdr, nb, logits.detach(), float(loss.detach())


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _bn(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_identity_index_is_bit_equal_to_forward(dtype):
    cfg = O.full_config()                                              # dropout on (0.1 / 0.3)
    images, ids, mask, answers = _batch(4, 4)
    x, ids, mask, t = images.to(DEV), ids.to(DEV), mask.to(DEV), answers.to(DEV)
    out = []
    for grouped in (False, True):
        m, _ = _model(dtype, cfg)
        m.train()
        if grouped:
            logits, _ = m.forward_grouped(x, ids, mask, image_index=torch.arange(4))
        else:
            logits, _ = m(x, ids, mask)
        loss = F.cross_entropy(logits.float(), t)
        loss.backward()
        torch.cuda.synchronize()
        out.append((logits.detach(), loss.detach(), _grads(m), _bn(m)))
    (l0, s0, g0, b0), (l1, s1, g1, b1) = out
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    for k in b0:
        assert torch.equal(b0[k], b1[k]), k


@pytest.mark.parametrize("image_size", [224, 384])
def test_fp32_matches_the_oracle_composition(image_size):
    ntok = (image_size // 32) ** 2
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0, num_image_tokens=ntok)
    m, sd = _model("fp32", cfg, seed=21)
    m.train()
    images, ids, mask, answers = _batch(3, len(IDX), image_size=image_size, seed=31)
    logits, _ = m.forward_grouped(images.to(DEV), ids.to(DEV), mask.to(DEV), image_index=torch.tensor(IDX))
    loss = F.cross_entropy(logits, answers.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    sdr, nb, lref, sref = _oracle_step(sd, cfg, images, ids, mask, answers, IDX)
    assert logits.shape == (len(IDX), cfg["num_answers"])
    assert (logits.detach().cpu() - lref).abs().max().item() < 1e-3
    assert abs(loss.item() - sref) < 1e-4
    P = dict(m.named_parameters())
    worst = (0.0, None)
    for n in O.parameter_names(cfg):
        gh, gr = P[n].grad.detach().cpu().double().flatten(), sdr[n].grad.double().flatten()
        if float(gr.norm()) < 1e-12:
            assert float(gh.norm()) < 1e-9, n
            continue
        rel = float((gh - gr).norm() / gr.norm())
        if rel > worst[0]:
            worst = (rel, n)
    assert worst[0] < 5e-2, worst
    st = m.state_dict()
    for k, v in nb.items():
        if "running_" in k:
            assert (st[k].cpu() - v).abs().max().item() < 1e-4, k


def test_eval_mode_gradients_match_the_expanded_forward():
    cfg = O.full_config()
    m, _ = _model("fp32", cfg, seed=23)
    m.eval()
    images, ids, mask, answers = _batch(3, len(IDX), seed=41)
    x, ids, mask, t = images.to(DEV), ids.to(DEV), mask.to(DEV), answers.to(DEV)
    idx = torch.tensor(IDX, device=DEV)
    xg = x.clone().requires_grad_(True)
    logits, _ = m.forward_grouped(xg, ids, mask, image_index=idx)
    F.cross_entropy(logits, t).backward()
    g1, dx1 = _grads(m), xg.grad.detach().clone()
    m.zero_grad()
    xe = x[idx].clone().requires_grad_(True)
    logits_e, _ = m(xe, ids, mask)
    F.cross_entropy(logits_e, t).backward()
    torch.cuda.synchronize()
    g2 = _grads(m)
    assert (logits.detach() - logits_e.detach()).abs().max().item() < 1e-4
    for n in g1:
        den = float(g2[n].norm())
        if den < 1e-12:
            assert float(g1[n].norm()) < 1e-9, n
            continue
        assert float((g1[n] - g2[n]).norm()) / den < 1e-4, n
    dx2 = torch.zeros_like(x).index_add_(0, idx, xe.grad)
    assert float((dx1 - dx2).norm() / dx2.norm()) < 1e-4
    assert (dx1[1] == 0).all()                                         # image 1 has no question


def test_bf16_close_to_the_oracle_and_reproducible():
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0)
    index = [3, 0, 0, 2, 3, 3, 0, 2]
    images, ids, mask, answers = _batch(4, len(index), seed=51)
    _, sd = _model("fp32", cfg, seed=7)
    _, _, _, sref = _oracle_step(sd, cfg, images, ids, mask, answers, index)
    runs = []
    for _ in range(2):
        m, _ = _model("bf16", cfg, seed=7)
        m.train()
        logits, _ = m.forward_grouped(images.to(DEV), ids.to(DEV), mask.to(DEV), image_index=torch.tensor(index))
        loss = F.cross_entropy(logits.float(), answers.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        assert abs(loss.item() - sref) < 2e-2
        g = torch.cat([p.grad.flatten() for p in m.parameters()])
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0
        runs.append((logits.detach(), g))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_trainer_step_with_an_image_index():
    HipTrainer = sub("trainer").HipTrainer
    cfg = O.full_config()
    images, ids, mask, answers = _batch(4, 4, seed=61)
    x, ids4, mask4, t4 = images.to(DEV), ids.to(DEV), mask.to(DEV), answers.to(DEV)
    # identity index: two steps bit-equal to the plain step (dropout on)
    res = []
    for grouped in (False, True):
        m, _ = _model("bf16", cfg, seed=13)
        m.train()
        tr = HipTrainer(m)
        losses = []
        for _ in range(2):
            loss, _ = tr.step(x, ids4, mask4, t4, image_index=torch.arange(4) if grouped else None)
            losses.append(loss.clone())
        torch.cuda.synchronize()
        res.append((torch.cat(losses), m._flat.detach().clone(), _bn(m)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k
    # a real index: one step against an autograd step through forward_grouped (fp32 CE, clip, torch AdamW)
    cfg0 = O.full_config(dropout=0.0, answer_dropout=0.0)
    images, ids, mask, answers = _batch(3, len(IDX), seed=71)
    x, ids, mask, t = images.to(DEV), ids.to(DEV), mask.to(DEV), answers.to(DEV)
    m1, _ = _model("fp32", cfg0, seed=17)
    m1.train()
    loss1, _ = HipTrainer(m1).step(x, ids, mask, t, image_index=torch.tensor(IDX))
    m2, _ = _model("fp32", cfg0, seed=17)
    m2.train()
    opt = torch.optim.AdamW(m2.parameters(), lr=1e-4, weight_decay=0.01)
    logits, _ = m2.forward_grouped(x, ids, mask, image_index=torch.tensor(IDX))
    loss2 = F.cross_entropy(logits.float(), t)
    loss2.backward()
    torch.nn.utils.clip_grad_norm_(list(m2.parameters()), 1.0)
    opt.step()
    torch.cuda.synchronize()
    assert abs(loss1.item() - loss2.item()) < 1e-5 * max(1.0, abs(loss2.item()))
    # AdamW's first step moves an element by ~lr whatever its gradient's size: one whose gradient sits at the fp32 noise floor may
    # move the other way (2 lr); everything else agrees to fp32 rounding
    diff = (m1._flat.detach() - m2._flat.detach()).abs()
    assert diff.max().item() <= 2.5e-4
    assert (diff > 1e-6).float().mean().item() < 1e-3
    for k, v in _bn(m1).items():
        assert torch.equal(v, _bn(m2)[k]), k


def test_errors():
    cfg = O.full_config()
    m, _ = _model("fp32", cfg, seed=3)
    m.train()
    images, ids, mask, answers = _batch(3, len(IDX), seed=81)
    x, ids, mask = images.to(DEV), ids.to(DEV), mask.to(DEV)
    with pytest.raises(IndexError):
        m.forward_grouped(x, ids, mask, image_index=torch.tensor([0, 1, 2, 3, 0, 0, 0]))
    with pytest.raises(IndexError):
        m.forward_grouped(x, ids, mask, image_index=torch.tensor([0, 1, 2, -1, 0, 0, 0], device=DEV))
    with pytest.raises(ValueError):
        m.forward_grouped(x, ids, mask, image_index=torch.tensor([0, 1, 2]))               # wrong length
    with pytest.raises(ValueError):
        m.forward_grouped(x, ids, mask, image_index=torch.zeros(len(IDX)))                 # floating point
    with pytest.raises(ValueError):
        m.forward_grouped(x, ids, mask)                                                    # None: 7 questions, 3 images
    with pytest.raises(NotImplementedError):
        m.forward_grouped(x, ids, mask, image_index=torch.tensor(IDX), return_aux=True)
    tr = sub("trainer").HipTrainer(m)
    with pytest.raises(IndexError):
        tr.step(x, ids, mask, answers.to(DEV), image_index=torch.tensor([0, 1, 2, 5, 0, 0, 0]))
    # without autograd, aux comes back with U image rows and N question rows
    with torch.no_grad():
        logits, aux = m.forward_grouped(x, ids, mask, image_index=torch.tensor(IDX), return_aux=True)
    assert logits.shape[0] == len(IDX)
    assert aux["image_features"].shape[0] == 3 and aux["image_projected"].shape[0] == 3
    assert aux["fused"].shape[0] == len(IDX) and aux["cross_attention_weights"][0].shape[0] == len(IDX)
    # eval mode without autograd delegates to forward(image_index=...)
    m.eval()
    with torch.no_grad():
        a, _ = m.forward_grouped(x, ids, mask, image_index=torch.tensor(IDX))
        b, _ = m(x, ids, mask, image_index=torch.tensor(IDX))
    assert torch.equal(a, b)
