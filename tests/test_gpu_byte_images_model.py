"""GPU: ByteImages through every public entry that takes images.  The yardstick is the same entry on ByteImages.to_float() -- the
float32 batch the existing pipeline would have produced -- and every comparison is torch.equal: in bf16 the dedicated stem kernels
form the same bf16 operand from the bytes, in fp32 the engine normalises once and takes the float route.  Small model of
tests/test_gpu_step_graph.py (embed_dim 32, 10 answers, 64-px images, L = 10); dropout 0 where one model runs both sides, dropout
0.1 with twin models and one seed for the trainer."""
import pytest
import torch

import _bytesref as R
from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(vocab_size=100, num_answers=10, embed_dim=32)
CFG0 = O.full_config(dropout=0.0, answer_dropout=0.0, **SMALL)
CFG1 = O.full_config(dropout=0.1, answer_dropout=0.1, **SMALL)
DTYPES = ["bf16", "fp32"]
GROUP_INDEX = [0, 1, 1, 0, 2, 0, 2]          # U = 3 images, N = 7 questions
_CACHE = {}


def _BI():
    return pkg().load_dropin_byte_images()


def _sd(cfg_id):
    if ("sd", cfg_id) not in _CACHE:
        _CACHE[("sd", cfg_id)] = O.init_state_dict(CFG0 if cfg_id == 0 else CFG1, 41, jitter=True)
    return _CACHE[("sd", cfg_id)]


def _model(dtype, cfg_id=0, train=False):
    m = pkg().load_dropin().VQAModel(**(CFG0 if cfg_id == 0 else CFG1), compute_dtype=dtype)
    m.load_state_dict(_sd(cfg_id))
    m = m.to(DEV)
    return m.train() if train else m.eval()


def _batch(seed, B=4, U=None, norm=R.IMAGENET):
    """(ByteImages of U (default B) images, its float form, token ids, mask, answers) on the device, made once per key."""
    key = ("batch", seed, B, U, norm)
    if key not in _CACHE:
        _, ids, mask, answers = O.synthetic_batch(B, seed=seed, image_size=64, seq_len=10, vocab=100, num_answers=10)
        bi = _BI().ByteImages(R.images(U or B, 64, 64, seed=seed).to(DEV), *norm)
        _CACHE[key] = (bi, bi.to_float(), ids.to(DEV), mask.to(DEV), answers.to(DEV))
    return _CACHE[key]


def _same_aux(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], (list, tuple)) else ([a[k]], [b[k]])
        assert len(xs) == len(ys)
        for x, y in zip(xs, ys):
            assert torch.equal(x, y), k


# ---------------------------------------------------------------------------------------------------------------- inference
@pytest.mark.parametrize("dtype", DTYPES)
def test_eval_forward_graphed_and_eager(dtype):
    m = _model(dtype)
    bi, f32, ids, mask, _ = _batch(1)
    with torch.no_grad():
        for graphed in (True, False):
            m.graph_inference = graphed
            a, _ = m(bi, ids, mask)
            b, _ = m(f32, ids, mask)
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), graphed
            a2, _ = m(bi, ids, mask)                                    # (the replay of the graph just captured)
            assert torch.equal(a2, b)
        la, aux_a = m(bi, ids, mask, return_aux=True)
        lb, aux_b = m(f32, ids, mask, return_aux=True)
    assert torch.equal(la, lb)
    _same_aux(aux_a, aux_b)
    if dtype == "bf16":                                                 # the graph of a ByteImages holds a uint8 static image buffer
        st = [g[1] for k, g in m._graphs.items() if k[-1] == (bi.mean, bi.std)]
        assert st and all(t.dtype == torch.uint8 and t.shape == bi.data.shape for t in st)


@pytest.mark.parametrize("dtype", DTYPES)
def test_image_index_features_context_and_predict(dtype):
    m = _model(dtype)
    bi, f32, ids, mask, _ = _batch(2, B=7, U=3)
    idx = torch.tensor(GROUP_INDEX)
    with torch.no_grad():
        for graphed in (True, False):
            m.graph_inference = graphed
            a, _ = m(bi, ids, mask, image_index=idx)
            b, _ = m(f32, ids, mask, image_index=idx)
            assert torch.equal(a, b)
            ga, _ = m.forward_grouped(bi, ids, mask, idx)
            assert torch.equal(ga, b)
            ta = m.predict_topk(bi, ids, mask, top_k=3, image_index=idx, return_logits=True)
            tb = m.predict_topk(f32, ids, mask, top_k=3, image_index=idx, return_logits=True)
            assert all(torch.equal(x, y) for x, y in zip(ta, tb))
            pa, pb = m.predict(bi, ids, mask, top_k=3, image_index=idx), m.predict(f32, ids, mask, top_k=3, image_index=idx)
            assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])
            ta = m.predict_topk(bi, ids[:3], mask[:3], top_k=2)
            tb = m.predict_topk(f32, ids[:3], mask[:3], top_k=2)
            assert torch.equal(ta.indices, tb.indices) and torch.equal(ta.probs, tb.probs)
            pa, pb = m.predict(bi, ids[:3], mask[:3], top_k=2), m.predict(f32, ids[:3], mask[:3], top_k=2)
            assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])
        fa, fb = m.encode_features(bi), m.encode_features(f32)
        assert torch.equal(fa.tensor(), fb.tensor())
        ca, cb = m.encode_images(bi), m.encode_images(f32)
        assert ca.num_images == cb.num_images == 3
        xa, _ = m.answer(ca, ids, mask, image_index=idx)
        xb, _ = m.answer(cb, ids, mask, image_index=idx)
        assert torch.equal(xa, xb) and torch.equal(xa, b)


# ---------------------------------------------------------------------------------------------------------------- autograd
def _grads(m, images, ids, mask, answers, grouped_idx=None, return_aux=False):
    m.zero_grad(set_to_none=True)
    if grouped_idx is not None:
        logits, aux = m.forward_grouped(images, ids, mask, grouped_idx)
    else:
        logits, aux = m(images, ids, mask, return_aux=return_aux)
    loss = torch.nn.functional.cross_entropy(logits, answers)
    if return_aux:
        loss = loss + aux["fused"].square().mean() + aux["image_features"].mean()
    loss.backward()
    return logits.detach().clone(), aux, {n: p.grad.clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["plain", "return_aux", "grouped"])
def test_train_mode_autograd_logits_and_every_gradient(dtype, route):
    m = _model(dtype, train=True)
    if route == "grouped":
        bi, f32, ids, mask, answers = _batch(3, B=7, U=3)
        kw = dict(grouped_idx=torch.tensor(GROUP_INDEX))
    else:
        bi, f32, ids, mask, answers = _batch(3)
        kw = dict(return_aux=route == "return_aux")
    la, aux_a, ga = _grads(m, bi, ids, mask, answers, **kw)
    lb, aux_b, gb = _grads(m, f32, ids, mask, answers, **kw)
    assert bool(torch.isfinite(la).all()) and torch.equal(la, lb)
    assert sorted(ga) == sorted(gb) and len(ga) > 100
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    assert float(ga["image_encoder.stem.0.weight"].abs().max()) > 0
    if route == "return_aux":
        _same_aux({k: v for k, v in aux_a.items()}, {k: v for k, v in aux_b.items()})


# ---------------------------------------------------------------------------------------------------------------- trainer
def _state(m, tr, loss, logits):
    return ([loss.clone(), logits.clone(), m._flat.detach().clone(), tr.m.clone(), tr.v.clone()]
            + [b.detach().clone() for _, b in sorted(m.named_buffers())])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graphed", [False, True], ids=["step", "step_graphed"])
def test_trainer_steps_on_bytes_equal_steps_on_floats(dtype, graphed):
    T = pkg().trainer.HipTrainer
    a, b = _model(dtype, 1, train=True), _model(dtype, 1, train=True)
    ta, tb = T(a, lr=1e-3), T(b, lr=1e-3)
    for s in range(5 if graphed else 3):
        bi, f32, ids, mask, answers = _batch(10 + s % 3)
        la, lga = ta.step(f32, ids, mask, answers)
        lb, lgb = (tb.step_graphed if graphed else tb.step)(bi, ids, mask, answers)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(la).all())
        for i, (x, y) in enumerate(zip(_state(a, ta, la, lga), _state(b, tb, lb, lgb))):
            assert torch.equal(x, y), (s, i)
    if graphed:
        assert tb.graph_captures == 1 and len(tb._graphs) == 1
        (static,) = [g[1] for g in tb._graphs.values()]
        assert static["images"][0].dtype == torch.uint8 and static["images"][0].shape == (4, 64, 64, 3)
        # another mean / std: its own graph key and its own table, and still the float route's bits
        bi2, f2, ids, mask, answers = _batch(10, norm=R.ODD)
        tables = sub("kernels")._U8_TABLES
        for s in range(3):
            la, lga = ta.step(f2, ids, mask, answers)
            lb, lgb = tb.step_graphed(bi2, ids, mask, answers)
            assert torch.equal(la, lb) and torch.equal(lga, lgb) and torch.equal(a._flat, b._flat), s
        assert tb.graph_captures == 2 and len(tb._graphs) == 2
        if dtype == "bf16":
            keys = [k for k in tables if k[1:] in ((bi.mean, bi.std), (bi2.mean, bi2.std))]
            assert len(keys) == 2 and tables[keys[0]].data_ptr() != tables[keys[1]].data_ptr()
            for k in keys:
                assert torch.equal(tables[k].cpu().view(torch.int16), R.table(k[1], k[2]).view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_and_the_plain_uint8_tensor():
    T = pkg().trainer.HipTrainer
    m = _model("bf16", train=True)
    tr = T(m, lr=1e-3)
    bi, f32, ids, mask, answers = _batch(1)
    cpu = _BI().ByteImages(bi.data.cpu())
    flat0 = m._flat.detach().clone()
    with pytest.raises(RuntimeError, match="CPU"):
        m(cpu, ids, mask)
    with pytest.raises(RuntimeError, match="must be a tensor on"):
        tr.step(cpu, ids, mask, answers)
    with pytest.raises(RuntimeError, match="expected images"):
        tr.step(bi, ids[:3], mask[:3], answers[:3])                      # a wrong batch against token_ids
    with pytest.raises(RuntimeError, match="expected images"):
        tr.step_graphed(bi, ids[:3], mask[:3], answers[:3])
    assert tr.calls == 0 and torch.equal(m._flat, flat0)                 # refused before anything was counted or launched
    # an image gradient asked of ByteImages
    with pytest.raises(TypeError, match="float images"):
        bi.requires_grad_()
    eng = m._ensure_engine()
    logits, _, tape = eng.forward(bi, ids, mask.float(), True, False, need_tape=True)
    with pytest.raises(TypeError, match="ByteImages"):
        eng.backward(tape, torch.zeros_like(logits), torch.zeros_like(m._flat), want_input_grad=True)
    # a plain uint8 tensor keeps its meaning: the values 0 ... 255 as floats, not normalised
    m.eval()
    t = bi.data.permute(0, 3, 1, 2).contiguous()                         # uint8 [B, 3, H, W]
    with torch.no_grad():
        for graphed in (True, False):
            m.graph_inference = graphed
            a, _ = m(t, ids, mask)
            b, _ = m(t.float(), ids, mask)
            assert torch.equal(a, b)
            c, _ = m(bi, ids, mask)
            assert not torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------------------- input pipeline
@pytest.mark.parametrize("case", ["resize", "resize_crop_flip", "jitter", "normalizer_flip"])
def test_gpu_collate_bytes_equals_float(case):
    P = pkg().load_dropin_preprocess()
    g = torch.Generator().manual_seed(5)
    ragged = case != "normalizer_flip"
    sizes = [(50, 70), (64, 64), (33, 41), (80, 48), (64, 40)] if ragged else [(32, 48)] * 5
    items = [(torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8), torch.arange(6), torch.ones(6, dtype=torch.long), i)
             for i, (h, w) in enumerate(sizes)]
    if case == "resize":
        kw = dict(resizer=P.DeviceImageResizer(size=32))
    elif case == "resize_crop_flip":
        kw = dict(resizer=P.DeviceImageResizer(size=40, crop=32), flip_p=0.5)
    elif case == "jitter":
        jit = P.DeviceColorJitter(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1)
        kw = dict(resizer=P.DeviceImageResizer(size=40, crop=32, jitter=jit), flip_p=0.5)
    else:
        kw = dict(normalizer=P.DeviceImageNormalizer(R.ODD[0], R.ODD[1]), flip_p=0.5)
    fl = P.gpu_collate_fn(items, generator=torch.Generator().manual_seed(9), **kw)
    by = P.gpu_collate_fn(items, generator=torch.Generator().manual_seed(9), output="bytes", **kw)
    assert sub("kernels").is_byte_images(by["images"]) and by["images"].data.dtype == torch.uint8
    assert fl["images"].dtype == torch.float32 and by["images"].shape_nchw == tuple(fl["images"].shape)
    assert torch.equal(by["images"].to_float(), fl["images"])
    if case == "normalizer_flip":
        assert by["images"].mean == R.ODD[0] and by["images"].std == R.ODD[1]
        flips = torch.rand(5, generator=torch.Generator().manual_seed(9)) < 0.5
        assert bool(flips.any()) and not bool(flips.all())              # both kinds of sample were exercised
    for k in ("token_ids", "attention_mask", "answers"):
        assert torch.equal(fl[k], by[k])
    with pytest.raises(ValueError, match="output"):
        P.gpu_collate_fn(items, output="uint8", **kw)
