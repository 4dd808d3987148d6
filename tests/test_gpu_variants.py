"""GPU: ablation / shape variants of the drop-in against the CPU oracle (fp32 path, train step with dropout 0):
no SE, no spatial attention, no gating, fewer layers, attention_mask=None, odd batch, non-224 images, short questions,
and eval-mode backward (BatchNorm on running statistics)."""
import numpy as np
import pytest
import torch

from _pkg import pkg
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

VARIANTS = [
    ("no_attention", dict(use_se_attention=False, use_spatial_attention=False), 3, 64, 12, True, True),
    ("se_only", dict(use_spatial_attention=False), 2, 96, 20, True, True),
    ("no_gating_1cross_2text", dict(use_gating=False, num_cross_layers=1, num_transformer_layers=2), 3, 64, 9, True, True),
    ("mask_none", dict(), 2, 64, 20, False, True),
    ("eval_mode_backward", dict(), 2, 64, 14, True, False),
    ("wide_head_dim64", dict(embed_dim=512, num_attention_heads=8, num_answers=24), 2, 64, 20, True, True),
    ("se_reduction_1", dict(se_reduction=1), 2, 64, 12, True, True),
]


@pytest.mark.parametrize("tag,kw,B,isz,L,use_mask,training", VARIANTS)
def test_variant_train_step_matches_oracle(tag, kw, B, isz, L, use_mask, training):
    base = dict(dropout=0.0, answer_dropout=0.0, vocab_size=300, num_answers=40, embed_dim=64)
    base.update(kw)
    cfg = O.full_config(**base)
    sd = O.init_state_dict(cfg, 31, jitter=True)
    images, ids, mask, answers = O.synthetic_batch(B, seed=41, image_size=isz, seq_len=L, vocab=300, num_answers=cfg["num_answers"])
    if not use_mask:
        mask = None
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype="fp32")
    m.load_state_dict(sd)
    m = m.to(DEV)
    m.train(training)
    logits, _ = m(images.to(DEV), ids.to(DEV), None if mask is None else mask.to(DEV))
    loss = torch.nn.functional.cross_entropy(logits, answers.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    tr = O.OracleTrainer(sd, cfg)
    lref, _ = O.vqa_forward(images, ids, mask, tr.sd, cfg, training, {})
    loss_ref = torch.nn.functional.cross_entropy(lref, answers)
    loss_ref.backward()
    assert (logits.detach().cpu() - lref.detach()).abs().max().item() < 1e-3, tag
    assert abs(loss.item() - loss_ref.item()) < 1e-4
    P = dict(m.named_parameters())
    names = O.parameter_names(cfg)
    got = np.array([float(P[n].grad.double().norm()) for n in names])
    ref = np.array([float(tr.sd[n].grad.double().norm()) for n in names])
    rel = np.abs(got - ref) / np.maximum(ref, 1e-6 * ref.max())
    assert rel.max() < 3e-2, (tag, names[int(rel.argmax())], rel.max())


def test_se_reduction_1_bf16_train_step_matches_oracle():
    """The se_reduction_1 variant in the throughput dtype: a bottleneck as wide as the channels (Cr = 512 at stage 4, a 2 x 2 map
    at 64 px, where the SE backward runs 256 threads per sample: Cr > threads), every gradient held to the bf16 noise floor of the
    same model (tests/_bf16check.py)."""
    from _bf16check import check_bf16_grads
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0, vocab_size=300, num_answers=40, embed_dim=64, se_reduction=1)
    sd = O.init_state_dict(cfg, 31, jitter=True)
    images, ids, mask, answers = O.synthetic_batch(2, seed=41, image_size=64, seq_len=12, vocab=300, num_answers=cfg["num_answers"])
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    logits, _ = m(images.to(DEV), ids.to(DEV), mask.to(DEV))
    loss = torch.nn.functional.cross_entropy(logits, answers.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    noisy = {f"image_encoder.stage{s}.attention.se.fc1.weight" for s in (1, 2, 3)}
    worst, lref = check_bf16_grads(m, sd, cfg, images, ids, mask, answers, noisy)
    assert abs(loss.item() - lref) < 3e-2


def test_stress_shape_384px_144_tokens_matches_oracle():
    """BASELINE configs[4] shape at a small batch: 384x384 images -> 12x12 = 144 image tokens, embed_dim 512, 8 text layers,
    2000 answers.  The reference cannot run it (49 hard-coded positions, models/fusion.py:66), so this is ORACLE parity only
    ("parity unpinned" against the reference): fp32 train step with dropout 0, logits / loss / per-tensor gradient norms; the
    keys exceed the MFMA attention tile (144 > 64), so the LDS/VALU attention kernels run."""
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0, vocab_size=500, num_answers=2000, embed_dim=512, num_transformer_layers=8,
                        num_image_tokens=144)
    sd = O.init_state_dict(cfg, 77, jitter=True)
    B = 2
    images, ids, mask, answers = O.synthetic_batch(B, seed=78, image_size=384, seq_len=20, vocab=500, num_answers=2000)
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype="fp32")
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    logits, aux = m(images.to(DEV), ids.to(DEV), mask.to(DEV), return_aux=True)
    assert aux["cross_attention_weights"][0].shape == (B, 8, 20, 144)
    loss = torch.nn.functional.cross_entropy(logits, answers.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    tr = O.OracleTrainer(sd, cfg)
    lref, _ = O.vqa_forward(images, ids, mask, tr.sd, cfg, True, {})
    loss_ref = torch.nn.functional.cross_entropy(lref, answers)
    loss_ref.backward()
    assert (logits.detach().cpu() - lref.detach()).abs().max().item() < 1e-3
    assert abs(loss.item() - loss_ref.item()) < 1e-4
    P = dict(m.named_parameters())
    names = O.parameter_names(cfg)
    got = np.array([float(P[n].grad.double().norm()) for n in names])
    ref = np.array([float(tr.sd[n].grad.double().norm()) for n in names])
    rel = np.abs(got - ref) / np.maximum(ref, 1e-6 * ref.max())
    assert rel.max() < 3e-2, (names[int(rel.argmax())], rel.max())
    # bf16 throughput path at the same shape: finite and close
    mb = pkg().load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    mb.load_state_dict(sd)
    mb = mb.to(DEV).eval()
    with torch.no_grad():
        lb, _ = mb(images.to(DEV), ids.to(DEV), mask.to(DEV))
        le, _ = O.vqa_forward(images, ids, mask, sd, cfg, False, {})       # oracle eval forward on the ORIGINAL buffers
    err = (lb.cpu() - le).abs().max().item() / max(1.0, le.abs().max().item())
    assert torch.isfinite(lb).all() and err < 5e-2, err
    # 49-position model fed a 384x384 image fails like the reference (shape error), not silently
    m49 = pkg().load_dropin().VQAModel(**{k: v for k, v in cfg.items() if k != "num_image_tokens"}, compute_dtype="fp32").to(DEV).eval()
    with pytest.raises(RuntimeError):
        with torch.no_grad():
            m49(images.to(DEV), ids.to(DEV), mask.to(DEV))


def test_stress_shape_bf16_train_step_matches_oracle():
    """BASELINE configs[4] at B=2 in the THROUGHPUT dtype: 384x384 -> 144 image tokens, d=512 (head dim 64), 8 text layers,
    2000 answers, bf16 train step with dropout 0 against the fp32 CPU oracle -- loss, and every tensor's gradient held to the
    bf16 noise floor of the same model (tests/_bf16check.py).  Oracle parity only ("parity unpinned" vs the reference, which
    cannot run this shape).  Cross-attention has 144 keys."""
    from _bf16check import check_bf16_grads
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0, vocab_size=500, num_answers=2000, embed_dim=512, num_transformer_layers=8,
                        num_image_tokens=144)
    sd = O.init_state_dict(cfg, 79, jitter=True)
    B = 2
    images, ids, mask, answers = O.synthetic_batch(B, seed=80, image_size=384, seq_len=20, vocab=500, num_answers=2000)
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    logits, _ = m(images.to(DEV), ids.to(DEV), mask.to(DEV))
    loss = torch.nn.functional.cross_entropy(logits, answers.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    noisy = {f"image_encoder.stage{s}.attention.se.fc1.weight" for s in (1, 2, 3)}
    worst, lref = check_bf16_grads(m, sd, cfg, images, ids, mask, answers, noisy)
    assert abs(loss.item() - lref) < 3e-2
