"""GPU: many questions per image -- forward(..., image_index=), encode_images() / answer() -- against the expanded forward
forward(images[image_index], ...) and the CPU oracle; the bit-exact routes (identity index, answer vs indexed forward, HIP graph vs
eager, one context answered many times), aux outputs, MXFP8, the 144-token shape and every error of the API."""
import pytest
import torch

from _pkg import pkg
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDX = [2, 0, 0, 2, 2, 0, 2]              # U = 3 images, N = 7 questions: repeats, out of order, image 1 never asked about


def _model(dtype, cfg=None, seed=11):
    cfg = cfg or O.full_config()
    sd = O.init_state_dict(cfg, seed, jitter=True)
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd, cfg


def _batch(U=3, N=7, image_size=224, seed=5):
    images, _, _, _ = O.synthetic_batch(U, seed=seed, image_size=image_size)
    _, ids, mask, _ = O.synthetic_batch(N, seed=seed + 1)
    mask[:, 0] = 1
    return images.to(DEV), ids.to(DEV), mask.to(DEV)


@pytest.fixture(scope="module")
def fp32():
    return _model("fp32")


@pytest.fixture(scope="module")
def bf16():
    return _model("bf16")


def _bf16_close(a, b):
    return (a - b).abs().max().item() <= 2e-2 * max(1.0, b.abs().max().item())


def test_fp32_matches_expanded_forward_and_oracle(fp32):
    m, sd, cfg = fp32
    x, ids, mask = _batch()
    idx = torch.tensor(IDX)
    with torch.no_grad():
        got, _ = m(x, ids, mask, image_index=idx)
        exp, _ = m(x[idx.to(DEV)], ids, mask)
    ref, _ = O.vqa_forward(x[idx.to(DEV)].cpu(), ids.cpu(), mask.cpu(), sd, cfg, training=False)
    assert got.shape == (7, cfg["num_answers"])
    assert (got - exp).abs().max().item() < 1e-4
    assert (got.cpu() - ref).abs().max().item() < 1e-3
    assert (got.argmax(-1).cpu() == ref.argmax(-1)).all() and (got.argmax(-1) == exp.argmax(-1)).all()


def test_bf16_matches_expanded_forward(bf16):
    m, _, _ = bf16
    x, ids, mask = _batch()
    idx = torch.tensor(IDX, device=DEV)                  # a device index (one device-to-host read for the range check)
    with torch.no_grad():
        for msk in (mask, None):
            got, _ = m(x, ids, msk, image_index=idx)
            exp, _ = m(x[idx], ids, msk)
            assert torch.isfinite(got).all()
            assert _bf16_close(got, exp)
            assert (got.argmax(-1) == exp.argmax(-1)).all()


def test_bit_exact_routes(bf16):
    m, _, _ = bf16
    x, ids, mask = _batch()
    idx = torch.tensor(IDX)
    _, ids2, mask2 = _batch(seed=9)
    with torch.no_grad():
        m.graph_inference = False
        try:
            # identity index with U == N: the indexed route IS the plain eval forward, bit for bit
            xs = torch.cat([x, x[:1], x[2:], x[1:2], x[:1], x[1:2]])          # 7 images, 7 questions
            assert torch.equal(m(xs, ids, mask, image_index=torch.arange(7))[0], m(xs, ids, mask)[0])
            fe = m(x, ids, mask, image_index=idx)[0]
            ctx = m.encode_images(x)
            ae = m.answer(ctx, ids, mask, image_index=idx)[0]
        finally:
            m.graph_inference = True
        fg = m(x, ids, mask, image_index=idx)[0]          # captured graph of the whole indexed forward
        ag = m.answer(ctx, ids, mask, image_index=idx)[0]  # captured graph of the question path
        assert torch.equal(fe, ae) and torch.equal(fe, fg) and torch.equal(ae, ag)
        # one context, many answers (graph and static buffers refilled in between), each equal to a fresh context's
        a2 = m.answer(ctx, ids2, mask2, image_index=idx.flip(0))[0]
        a1 = m.answer(ctx, ids, mask, image_index=idx)[0]
        b2 = m.answer(m.encode_images(x), ids2, mask2, image_index=idx.flip(0))[0]
        assert torch.equal(a1, ag) and torch.equal(a2, b2)
        # a second context of the same shape replays the same graph with its own K / V
        y, _, _ = _batch(seed=21)
        c2 = m.answer(m.encode_images(y), ids, mask, image_index=idx)[0]
        m.graph_inference = False
        try:
            c2e = m.answer(m.encode_images(y), ids, mask, image_index=idx)[0]
        finally:
            m.graph_inference = True
        assert torch.equal(c2, c2e) and not torch.equal(c2, a1)


def test_broadcast_one_image(bf16):
    m, _, _ = bf16
    x, ids, mask = _batch(U=1)
    with torch.no_grad():
        a, _ = m.answer(m.encode_images(x), ids, mask)                         # image_index=None, U == 1: every question on image 0
        b, _ = m(x, ids, mask, image_index=torch.zeros(7, dtype=torch.long))
        e, _ = m(x.expand(7, -1, -1, -1), ids, mask)
    assert torch.equal(a, b)
    assert _bf16_close(a, e) and (a.argmax(-1) == e.argmax(-1)).all()


def test_aux_outputs_attention_maps_and_predict(fp32):
    m, _, cfg = fp32
    x, ids, mask = _batch()
    idx = torch.tensor(IDX)
    d = cfg["embed_dim"]
    with torch.no_grad():
        lg, aux = m(x, ids, mask, return_aux=True, image_index=idx)
        le, ex = m(x[idx.to(DEV)], ids, mask, return_aux=True)
        la, aa = m.answer(m.encode_images(x), ids, mask, image_index=idx, return_aux=True)
        maps = m.get_attention_maps(x, ids, mask, image_index=idx)
    assert aux["image_features"].shape == (3, 512, 7, 7) and aux["image_projected"].shape == (3, 49, d)
    for k in ("text_features", "text_pooled", "attended_pooled", "fused"):
        assert aux[k].shape == ex[k].shape, k
        assert (aux[k] - ex[k]).abs().max().item() < 1e-4, k
    assert len(aux["cross_attention_weights"]) == cfg["num_cross_layers"]
    for w, we in zip(aux["cross_attention_weights"], ex["cross_attention_weights"]):
        assert w.shape == (7, cfg["num_attention_heads"], 20, 49) and (w - we).abs().max().item() < 1e-5
    # one row per unique image: the expanded run's rows of image u (question 1 asks about image 0, question 0 about image 2)
    for u, i in ((0, 1), (2, 0)):
        assert (aux["image_features"][u] - ex["image_features"][i]).abs().max().item() < 1e-5
        assert (aux["image_projected"][u] - ex["image_projected"][i]).abs().max().item() < 1e-5
    assert (lg - le).abs().max().item() < 1e-4
    assert torch.equal(la, lg) and all(torch.equal(aa[k], aux[k]) for k in ("image_features", "image_projected", "fused"))
    assert maps["cross_attention_spatial"].shape == (7, 20, 7, 7)
    ti, tp = m.predict(x, ids, mask, top_k=3, image_index=idx)
    te, _ = m.predict(x[idx.to(DEV)], ids, mask, top_k=3)
    assert ti.shape == (7, 3) and tp.shape == (7, 3) and torch.equal(ti[:, 0], te[:, 0])


def test_mxfp8_composes():
    m, _, _ = _model("bf16", seed=13)
    m.set_inference_precision("mxfp8")
    x, ids, mask = _batch()
    idx = torch.tensor(IDX)
    with torch.no_grad():
        got, _ = m(x, ids, mask, image_index=idx)
        ctx = m.encode_images(x)
        ans, _ = m.answer(ctx, ids, mask, image_index=idx)
        exp, _ = m(x[idx.to(DEV)], ids, mask)
        m.set_inference_precision("bf16")
        plain, _ = m(x, ids, mask, image_index=idx)
    assert torch.equal(got, ans)
    assert _bf16_close(got, exp) and (got.argmax(-1) == exp.argmax(-1)).all()
    assert not torch.equal(got, plain)                    # the MXFP8 convolutions really ran


def test_144_image_tokens_five_key_tiles():
    cfg = O.full_config(embed_dim=512, num_image_tokens=144, vocab_size=1000)
    m, _, _ = _model("bf16", cfg=cfg, seed=17)
    x, ids, mask = _batch(U=2, N=3, image_size=384)
    idx = torch.tensor([1, 1, 0])
    with torch.no_grad():
        got, aux = m(x, ids, mask, image_index=idx, return_aux=True)
        exp, _ = m(x[idx.to(DEV)], ids, mask)
        ans, _ = m.answer(m.encode_images(x), ids, mask, image_index=idx)
    assert aux["cross_attention_weights"][0].shape == (3, 8, 20, 144)
    assert _bf16_close(got, exp) and (got.argmax(-1) == exp.argmax(-1)).all()
    assert _bf16_close(ans, exp)


def test_errors():
    m, sd, _ = _model("bf16", seed=19)
    x, ids, mask = _batch()
    idx = torch.tensor(IDX)
    with torch.no_grad():
        ctx = m.encode_images(x)
        for bad in (torch.tensor([0, 1, 2, 3, 0, 0, 0]), torch.tensor([0, -1, 0, 0, 0, 0, 0])):
            for dev in ("cpu", DEV):
                with pytest.raises(IndexError):
                    m(x, ids, mask, image_index=bad.to(dev))
                with pytest.raises(IndexError):
                    m.answer(ctx, ids, mask, image_index=bad.to(dev))
        for bad in (torch.zeros(6, dtype=torch.long), torch.zeros(7, 1, dtype=torch.long)):
            with pytest.raises(ValueError):
                m(x, ids, mask, image_index=bad)
            with pytest.raises(ValueError):
                m.answer(ctx, ids, mask, image_index=bad)
        with pytest.raises(ValueError):
            m.answer(ctx, ids, mask)                      # N = 7 questions, U = 3 images: no implied index
    # autograd with parameters that require grad: inference only
    with pytest.raises(RuntimeError, match="inference only"):
        m(x, ids, mask, image_index=idx)
    with pytest.raises(RuntimeError, match="inference only"):
        m.encode_images(x)
    with pytest.raises(RuntimeError, match="inference only"):
        m.answer(ctx, ids, mask, image_index=idx)
    m.train()
    with torch.no_grad():
        for call in (lambda: m(x, ids, mask, image_index=idx), lambda: m.encode_images(x),
                     lambda: m.answer(ctx, ids, mask, image_index=idx)):
            with pytest.raises(RuntimeError, match="inference only"):
                call()
    m.eval()

    def stale_after(change):
        with torch.no_grad():
            c = m.encode_images(x)
            m.answer(c, ids, mask, image_index=idx)       # fresh: fine
        change()
        m.eval()
        with torch.no_grad(), pytest.raises(RuntimeError, match="stale"):
            m.answer(c, ids, mask, image_index=idx)

    stale_after(lambda: m.load_state_dict(sd))

    def adamw_step():
        opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
        for p in m.parameters():
            p.grad = torch.zeros_like(p)
        opt.step()
    stale_after(adamw_step)

    def train_forward():
        m.train()
        with torch.no_grad():
            m(x[:2], ids[:2], mask[:2])
    stale_after(train_forward)
    stale_after(lambda: m.set_inference_precision("bf16"))
    with torch.no_grad():                                 # a fresh context works again
        assert torch.isfinite(m.answer(m.encode_images(x), ids, mask, image_index=idx)[0]).all()
