"""Training and inference from cached image features (VQAModel.encode_features / ImageFeatures, HipEngine.forward_features,
vqa_gather_rows).  The yardstick everywhere is the existing images route with image_encoder.requires_grad_(False).eval(), which is
checked against the oracle elsewhere: the features route issues that route's launches without the CNN forward on the same bits, so
every comparison is torch.equal."""
import pytest
import torch
import torch.nn.functional as F

from _pkg import pkg, sub
from oracle import vqa_oracle as O
from test_gpu_finetune import CNN_KERNELS

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(vocab_size=100, num_answers=10, embed_dim=32)
CFG = O.full_config(dropout=0.1, answer_dropout=0.1, **SMALL)
DTYPES = ["fp32", "bf16"]
GROUP_INDEX = [0, 1, 1, 0, 1, 0, 0]          # U = 3 images, N = 7 questions: images 0 and 1 repeated, image 2 without a question
_CACHE = {}


def _sd(cfg=CFG, seed=41):
    key = ("sd", tuple(sorted(cfg.items())), seed)
    if key not in _CACHE:
        _CACHE[key] = O.init_state_dict(cfg, seed, jitter=True)
    return _CACHE[key]


def _batch(seed, B=4):
    key = ("batch", seed, B)
    if key not in _CACHE:
        _CACHE[key] = [t.to(DEV) for t in O.synthetic_batch(B, seed=seed, image_size=64, seq_len=10, vocab=100, num_answers=10)]
    return _CACHE[key]


def _model(dtype, cfg=CFG, sd=None):
    """A model in train mode whose image encoder is frozen and in eval mode: the set-up both routes are compared in."""
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(_sd(cfg) if sd is None else sd)
    m = m.to(DEV).train()
    m.image_encoder.requires_grad_(False)
    m.image_encoder.eval()
    return m


def _encode(m, images, **kw):
    """encode_features is inference only (eval mode, no autograd): switch over and restore the fine-tuning modes."""
    m.eval()
    with torch.no_grad():
        f = m.encode_features(images, **kw)
    m.train()
    m.image_encoder.eval()
    return f


class _Calls:
    """Names of the launches that go through _lib.call, in order (the hook test_gpu_finetune.py uses), each with a flag."""

    def __init__(self, flag=lambda name: False):
        self.names, self.flags, self._flag = [], [], flag

    def __enter__(self):
        L = sub("_lib")
        self._old = L._HOOK[0]

        def hook(name, args):
            self.names.append(name)
            self.flags.append(self._flag(name))
        L._HOOK[0] = hook
        return self

    def __exit__(self, *a):
        sub("_lib")._HOOK[0] = self._old


def _grouped(seed):
    images, ids, mask, answers = _batch(seed, B=7)
    return images[:3].contiguous(), ids, mask, answers, torch.tensor(GROUP_INDEX)


# ---------------------------------------------------------------------------------------------------------------- 1: eval equality
@pytest.mark.parametrize("dtype", DTYPES)
def test_eval_forward_from_features_equals_the_images_forward(dtype):
    m = _model(dtype).eval()
    m.graph_inference = False                     # the eager eval forward is the yardstick
    images, ids, mask, _ = _batch(100)
    with torch.no_grad():
        feats = m.encode_features(images)
        assert feats.num_images == 4 and feats.tensor().dtype == m.compute_dtype and tuple(feats.tensor().shape) == (4, 2, 2, 512)
        lf, none = m(feats, ids, mask)
        li, _ = m(images, ids, mask)
        assert none is None and torch.equal(lf, li)
        lf, af = m(feats, ids, mask, return_aux=True)
        li, ai = m(images, ids, mask, return_aux=True)
        assert torch.equal(lf, li) and sorted(af) == sorted(ai)
        for k in ai:
            if isinstance(ai[k], (list, tuple)):
                assert len(af[k]) == len(ai[k]) and all(torch.equal(x, y) for x, y in zip(af[k], ai[k])), k
            else:
                assert torch.equal(af[k], ai[k]), k
        # many questions per image
        imu, ids7, mask7, _, idx = _grouped(101)
        fu = m.encode_features(imu)
        for kw in (dict(), dict(return_aux=True)):
            lf, af = m.forward_grouped(fu, ids7, mask7, image_index=idx, **kw)
            li, ai = m.forward_grouped(imu, ids7, mask7, image_index=idx, **kw)
            assert torch.equal(lf, li)
            if kw:
                assert torch.equal(af["image_features"], ai["image_features"]) and torch.equal(af["fused"], ai["fused"])
        l2, _ = m(fu, ids7, mask7, image_index=idx)
        assert torch.equal(l2, li)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- 2, 9: trainer bit-equality
def _state(m, tr, loss, logits):
    return [loss.clone(), logits.clone(), m._flat.detach().clone(), tr.m.clone(), tr.v.clone(), tr.ema.clone()]


def _soft(answers):
    ST = pkg().load_dropin_soft_targets()
    ids = torch.stack([answers, (answers + 1) % 10], dim=1).int().contiguous()
    w = torch.tensor([0.7, 0.3], device=DEV).repeat(answers.shape[0], 1).contiguous()
    return ST.SoftTargets(ids, w)


def _run_pair(dtype, case, steps=3, trainer_kw=None):
    """Two models from one state dict; `a` steps on features, `b` on the images.  The features of every step's images are encoded
    once, before step 0, into one bank (chunk by chunk, each chunk at the batch size the images route runs its CNN at) and selected
    from it per step.  After every step the loss, the logits, every parameter, both Adam moments and the EMA buffer must be equal."""
    a, b = _model(dtype), _model(dtype)
    kw = dict(lr=1e-3, ema_decay=0.99)
    kw.update(trainer_kw or {})
    ta, tb = pkg().trainer.HipTrainer(a, **kw), pkg().trainer.HipTrainer(b, **kw)
    data = [_grouped(300 + s) if case == "grouped" else _batch(200 + s) + [None] for s in range(steps)]
    U = data[0][0].shape[0]
    bank = a.features_from_tensor(torch.empty((steps * U, 2, 2, 512), device=DEV, dtype=a.compute_dtype))
    for s in range(steps):
        _encode(a, data[s][0], out=bank, at=s * U)
    for s, (images, ids, mask, answers, idx) in enumerate(data):
        tgt = answers
        if case == "soft":
            tgt = _soft(answers)
        elif case == "loss_opts":
            tgt = answers.clone()
            tgt[1] = -100                                      # an ignored row
        feats = bank.select(torch.arange(s * U, (s + 1) * U))
        la, lga = ta.step(feats, ids, mask, tgt, image_index=idx)
        lb, lgb = tb.step(images, ids, mask, tgt, image_index=idx)
        torch.cuda.synchronize()
        for x, y in zip(_state(a, ta, la, lga), _state(b, tb, lb, lgb)):
            assert torch.equal(x, y), (case, s)
        assert bool(torch.isfinite(la).all())
    ta.check(); tb.check()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["plain", "grouped", "soft", "loss_opts"])
def test_trainer_steps_from_features_are_bit_equal_to_the_images_steps(dtype, case):
    kw = dict(label_smoothing=0.1, ignore_index=-100) if case == "loss_opts" else None
    _run_pair(dtype, case, trainer_kw=kw)


def test_full_size_step_from_features_is_bit_equal():
    """Default configuration at 224 px (49 image tokens: the MFMA attention path and the full-size GEMM tiles), bf16, B = 8."""
    cfg = O.full_config()
    sd = _sd(cfg, 43)
    data = [t.to(DEV) for t in O.synthetic_batch(8, seed=77)]
    a, b = _model("bf16", cfg, sd), _model("bf16", cfg, sd)
    ta, tb = pkg().trainer.HipTrainer(a, lr=1e-3, ema_decay=0.99), pkg().trainer.HipTrainer(b, lr=1e-3, ema_decay=0.99)
    images, ids, mask, answers = data
    feats = _encode(a, images)
    assert tuple(feats.tensor().shape) == (8, 7, 7, 512)
    la, lga = ta.step(feats, ids, mask, answers)
    lb, lgb = tb.step(images, ids, mask, answers)
    torch.cuda.synchronize()
    for x, y in zip(_state(a, ta, la, lga), _state(b, tb, lb, lgb)):
        assert torch.equal(x, y)
    assert bool(torch.isfinite(la).all())


# ----------------------------------------------------------------------------------------------------------------- 3: launch lists
def _recorded_step(m, tr, first, rest):
    """The launch list of one warmed-up step, each launch flagged when it belongs to the CNN forward: issued inside _stem_fwd /
    _stages_fwd (but not by the text encoder, which forward() issues from inside the stage loop), or begin_step's packing of the
    stem conv operands."""
    eng = m._engine
    state = {"cnn": 0, "begin": 0}

    def wrap(name, key, delta):
        orig = getattr(eng, name)

        def f(*a, **k):
            old = state[key]
            state[key] = old + delta if delta else 0
            try:
                return orig(*a, **k)
            finally:
                state[key] = old
        setattr(eng, name, f)

    wrap("_stem_fwd", "cnn", 1)
    wrap("_stages_fwd", "cnn", 1)
    wrap("_text_fwd", "cnn", 0)
    wrap("begin_step", "begin", 1)
    flag = lambda n: state["cnn"] > 0 or (state["begin"] > 0 and n in ("vqa_stem_pack", "vqa_pack_rows"))
    tr.step(first, *rest)                          # warm-up: the first backward packs its operands on demand
    torch.cuda.synchronize()
    with _Calls(flag) as c:
        tr.step(first, *rest)
        torch.cuda.synchronize()
    for name in ("_stem_fwd", "_stages_fwd", "_text_fwd", "begin_step"):
        delattr(eng, name)
    return c


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grouped", [False, True])
def test_features_step_issues_the_images_steps_launches_without_the_cnn_forward(dtype, grouped):
    a, b = _model(dtype), _model(dtype)
    ta, tb = pkg().trainer.HipTrainer(a, lr=1e-3), pkg().trainer.HipTrainer(b, lr=1e-3)
    if grouped:
        images, ids, mask, answers, idx = _grouped(400)
    else:
        (images, ids, mask, answers), idx = _batch(401), None
    feats = _encode(a, images)
    cf = _recorded_step(a, ta, feats, (ids, mask, answers, None, idx))
    ci = _recorded_step(b, tb, images, (ids, mask, answers, None, idx))
    assert not [n for n in cf.names if n.startswith(CNN_KERNELS)], sorted(set(cf.names))
    assert not any(cf.flags)
    assert any(ci.flags) and [n for n in ci.names if n.startswith(CNN_KERNELS)]
    assert cf.names == [n for n, cnn in zip(ci.names, ci.flags) if not cnn]


# --------------------------------------------------------------------------------------------------------------------- 4: autograd
@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_from_features_gives_the_images_routes_gradients(dtype):
    a, b = _model(dtype), _model(dtype)
    imu, ids, mask, y, idx = _grouped(500)
    feats = _encode(a, imu)
    la = a.forward_grouped(feats, ids, mask, image_index=idx)[0]
    lb = b.forward_grouped(imu, ids, mask, image_index=idx)[0]
    assert torch.equal(la, lb)
    F.cross_entropy(la, y).backward()
    F.cross_entropy(lb, y).backward()
    torch.cuda.synchronize()
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    seen = 0
    for n in gb:
        if n.startswith("image_encoder."):
            assert ga[n].grad is None and gb[n].grad is None, n
        else:
            assert ga[n].grad is not None and torch.equal(ga[n].grad, gb[n].grad), n
            seen += 1
    assert seen > 50
    # and the plain form, one question per image
    a.zero_grad(set_to_none=True); b.zero_grad(set_to_none=True)
    images, ids, mask, y = _batch(501)
    la = a(_encode(a, images), ids, mask)[0]
    lb = b(images, ids, mask)[0]
    assert torch.equal(la, lb)
    F.cross_entropy(la, y).backward()
    F.cross_entropy(lb, y).backward()
    torch.cuda.synchronize()
    for n in gb:
        if not n.startswith("image_encoder."):
            assert torch.equal(ga[n].grad, gb[n].grad), n
    with pytest.raises(NotImplementedError):
        a(_encode(a, images), ids, mask, return_aux=True)


# ------------------------------------------------------------------------------------------------------------ 5: gather / select
ROWS = [("bf16", (2, 2, 512)),        # the smallest row: 4096 B, one partial chunk
        ("fp32", (3, 3, 512)),        # 18 432 B = 1152 16-byte vectors: one full 1024-vector chunk and a partial one
        ("bf16", (7, 7, 512))]        # the default shape: 50 176 B, three full chunks and a partial one


@pytest.mark.parametrize("dtype,row", ROWS)
def test_select_equals_torch_indexing(dtype, row):
    m = _model(dtype)
    g = torch.Generator().manual_seed(5)
    bank_t = torch.randn((6,) + row, generator=g).to(DEV, m.compute_dtype)
    bank = m.features_from_tensor(bank_t)
    assert bank.num_images == 6 and bank.tensor() is not None
    for index in ([3], [5, 0, 5, 2, 0]):
        for idt in (torch.int32, torch.int64):
            for dev in ("cpu", DEV):
                ix = torch.tensor(index, dtype=idt, device=dev)
                with _Calls() as c:
                    out = bank.select(ix)
                torch.cuda.synchronize()
                assert c.names == ["vqa_gather_rows"]
                assert out.num_images == len(index) and torch.equal(out.tensor(), bank_t[ix.long().to(DEV)])
    assert bank.select(torch.zeros(0, dtype=torch.long)).num_images == 0
    # the kernel wrapper on rows that are not feature blocks (int64 rows of 16 bytes, more rows than lanes)
    src = torch.arange(2 * 3000, device=DEV).view(3000, 2)
    ix = torch.randint(0, 3000, (4097,), generator=g).to(DEV, torch.int32)
    assert torch.equal(sub("kernels").gather_rows(src, ix), src[ix.long()])
    torch.cuda.synchronize()


def test_select_refuses_bad_indices_before_any_launch():
    m = _model("bf16")
    bank = m.features_from_tensor(torch.zeros((3, 2, 2, 512), device=DEV, dtype=torch.bfloat16))
    with _Calls() as c:
        for bad in (torch.tensor([0, 3]), torch.tensor([-1]), torch.tensor([0, 3], device=DEV), torch.tensor([2, -1], device=DEV, dtype=torch.int32)):
            with pytest.raises(IndexError):
                bank.select(bad)
        for bad in (torch.tensor([0.0, 1.0]), torch.tensor([True, False]), torch.tensor([[0, 1]]), torch.tensor([1.0], device=DEV)):
            with pytest.raises(ValueError):
                bank.select(bad)
        with pytest.raises(ValueError):
            sub("kernels").gather_rows(torch.zeros((4, 3), device=DEV), torch.zeros(1, device=DEV, dtype=torch.int32))    # 12-byte rows
        with pytest.raises(ValueError):
            sub("kernels").gather_rows(torch.zeros((4, 4), device=DEV), torch.zeros(1, device=DEV, dtype=torch.int64))    # index dtype
    assert c.names == []
    # 2^24 chunks (gridDim.x * 256 threads would reach 2^32): status 1000 from the entry, not a launch error
    with pytest.raises(RuntimeError, match="argument/shape error"):
        sub("kernels").gather_rows(torch.zeros((1, 4), device=DEV), torch.zeros(1 << 24, device=DEV, dtype=torch.int32))
    for bad in (torch.zeros((3, 2, 2, 512), device=DEV), torch.zeros((3, 2, 2, 64), device=DEV, dtype=torch.bfloat16),
                torch.zeros((3, 2, 2, 512), dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            m.features_from_tensor(bad)


# --------------------------------------------------------------------------------------------------------------------- 6: validity
def _accepts(m, feats, ids, mask):
    m.eval()
    with torch.no_grad():
        m(feats, ids, mask)
    m.train(); m.image_encoder.eval()


def _refuses(m, feats, ids, mask):
    m.eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="stale"):
        m(feats, ids, mask)
    m.train(); m.image_encoder.eval()


@pytest.mark.parametrize("dtype", DTYPES)
def test_features_survive_steps_that_leave_the_image_encoder_alone(dtype):
    m = _model(dtype)
    tr = pkg().trainer.HipTrainer(m, lr=1e-3, ema_decay=0.99)
    images, ids, mask, answers = _batch(600)
    feats = _encode(m, images)
    before = m._flat.detach().clone()
    for _ in range(3):                              # text encoder, fusion and answer head train
        tr.step(feats, ids, mask, answers)
    torch.cuda.synchronize()
    assert not torch.equal(before, m._flat)
    _accepts(m, feats, ids, mask)
    assert torch.equal(_encode(m, images).tensor(), feats.tensor())       # and they are still what the image encoder gives
    with tr.ema_weights():                          # the average of a frozen image encoder is the image encoder
        _accepts(m, feats, ids, mask)
        m.train(); m.image_encoder.eval()
    tr.step(feats, ids, mask, answers)
    # a torch.optim loop over the trainable parameters keeps them valid too
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    logits, _ = m(feats, ids, mask)
    F.cross_entropy(logits, answers).backward()
    opt.step()
    _accepts(m, feats, ids, mask)
    torch.cuda.synchronize()


def test_features_are_refused_once_the_image_encoder_changed():
    images, ids, mask, answers = _batch(601)

    def fresh():
        m = _model("fp32")
        return m, _encode(m, images)

    # load_state_dict
    m, feats = fresh()
    m.load_state_dict(_sd())
    m.image_encoder.requires_grad_(False)
    _refuses(m, feats, ids, mask)
    # an in-place torch write to an image-encoder parameter (through the Parameter: writes through `.data` bypass torch's version
    # counter altogether, as HipTrainer.params_changed documents; invalidate_features() is the call for those)
    m, feats = fresh()
    with torch.no_grad():
        next(m.image_encoder.parameters()).add_(0)
    _refuses(m, feats, ids, mask)
    m, feats = fresh()
    m.invalidate_features()
    _refuses(m, feats, ids, mask)
    # a train-mode CNN forward: the running statistics move
    m, feats = fresh()
    m.image_encoder.train()
    with torch.no_grad():
        m(images, ids, mask)
    m.image_encoder.eval()
    _refuses(m, feats, ids, mask)
    # a trainer step with an image-encoder parameter trainable
    m, feats = fresh()
    tr = pkg().trainer.HipTrainer(m, lr=1e-3)
    m.image_encoder.stage4.requires_grad_(True)
    tr.step(images, ids, mask, answers)
    m.image_encoder.requires_grad_(False)
    _refuses(m, feats, ids, mask)
    # a torch.optim step that wrote one
    m, feats = fresh()
    m.image_encoder.stage4.requires_grad_(True)
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    F.cross_entropy(m(images, ids, mask)[0], answers).backward()
    opt.step()
    m.image_encoder.requires_grad_(False)
    _refuses(m, feats, ids, mask)
    # .to() and set_inference_precision
    m, feats = fresh()
    m.to(DEV)
    _refuses(m, feats, ids, mask)
    mb = _model("bf16")
    fb = _encode(mb, images)
    mb.set_inference_precision("mxfp8")
    _refuses(mb, fb, ids, mask)
    # another model's features
    m, feats = fresh()
    other = _model("fp32")
    other.eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="another model"):
        other(feats, ids, mask)
    with pytest.raises(RuntimeError, match="another model"):
        pkg().trainer.HipTrainer(other).step(feats, ids, mask, answers)
    torch.cuda.synchronize()


def test_step_on_features_raises_before_any_launch():
    images, ids, mask, answers = _batch(602)
    m = _model("fp32")
    feats = _encode(m, images)
    tr = pkg().trainer.HipTrainer(m, lr=1e-3)
    before = m._flat.detach().clone()

    def raises(match):
        with _Calls() as c:
            with pytest.raises(RuntimeError, match=match):
                tr.step(feats, ids, mask, answers)
            # with an image index the refusal also comes ahead of the index's copy to the device (a CPU index that is out of range
            # would raise IndexError from that check: the features are refused first)
            with pytest.raises(RuntimeError, match=match):
                tr.step(feats, ids, mask, answers, image_index=torch.tensor([0, 1, 2, 99]))
        assert c.names == [] and tr.calls == 0

    m.image_encoder.stage1.requires_grad_(True)                # a trainable CNN parameter
    raises("frozen")
    with pytest.raises(RuntimeError, match="frozen"):
        m(feats, ids, mask)
    m.image_encoder.requires_grad_(False)
    m.image_encoder.train()                                    # a train-mode CNN
    raises("eval")
    m.image_encoder.eval()
    m.invalidate_features()                                    # stale features
    raises("stale")
    torch.cuda.synchronize()
    assert torch.equal(before, m._flat)


def test_ema_weights_keeps_features_only_while_the_average_has_the_models_image_encoder():
    images, ids, mask, answers = _batch(603)
    m = _model("fp32")
    tr = pkg().trainer.HipTrainer(m, lr=1e-3, ema_decay=0.99)          # the average is cloned from these weights
    sd = {k: (v + 0.01 if k.startswith("image_encoder.") and v.is_floating_point() else v) for k, v in _sd().items()}
    m.load_state_dict(sd)                                              # the model's image encoder moves away from the average's
    feats = _encode(m, images)
    tr.step(feats, ids, mask, answers)
    _accepts(m, feats, ids, mask)
    with tr.ema_weights():                                             # inside, the flat buffer holds ANOTHER image encoder
        _refuses(m, feats, ids, mask)
    _refuses(m, feats, ids, mask)                                      # (and conservatively afterwards: encode again)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 7: the context from features
@pytest.mark.parametrize("dtype", DTYPES)
def test_context_from_features_answers_like_the_context_from_images(dtype):
    m = _model(dtype).eval()
    imu, ids, mask, _, idx = _grouped(700)
    with torch.no_grad():
        feats = m.encode_features(imu)
        with _Calls() as c:
            cf = m.encode_images(feats)
        # (vqa_convert is begin_step's bf16 cast of the weights: the "vqa_conv" prefix of CNN_KERNELS matches its name by accident)
        assert not [n for n in c.names if n.startswith(CNN_KERNELS) and n != "vqa_convert"] and "vqa_fold_bn_batch" not in c.names
        ci = m.encode_images(imu)
        assert cf.num_images == ci.num_images == 3
        for graphed in (False, True):
            m.graph_inference = graphed
            assert torch.equal(m.answer(cf, ids, mask, image_index=idx)[0], m.answer(ci, ids, mask, image_index=idx)[0])
            # N = 1: the graphed serving route
            one = (ids[:1], mask[:1])
            assert torch.equal(m.answer(cf, *one, image_index=torch.tensor([2]))[0], m.answer(ci, *one, image_index=torch.tensor([2]))[0])
            tf = m.answer_topk(cf, ids, mask, top_k=3, image_index=idx)
            ti = m.answer_topk(ci, ids, mask, top_k=3, image_index=idx)
            assert torch.equal(tf.indices, ti.indices) and torch.equal(tf.probs, ti.probs)
        m.graph_inference = False
        lf, af = m.answer(cf, ids, mask, image_index=idx, return_aux=True)
        li, ai = m.answer(ci, ids, mask, image_index=idx, return_aux=True)
        assert torch.equal(lf, li) and torch.equal(af["image_features"], ai["image_features"])
        assert torch.equal(af["image_projected"], ai["image_projected"])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 8: chunked bank
@pytest.mark.parametrize("dtype", DTYPES)
def test_bank_filled_in_chunks_equals_one_call(dtype):
    m = _model(dtype).eval()
    m.graph_inference = False
    imu = _grouped(800)[0]
    with torch.no_grad():
        whole = m.encode_features(imu)
        bank = m.features_from_tensor(torch.empty((3, 2, 2, 512), device=DEV, dtype=m.compute_dtype))
        assert m.encode_features(imu[:2], out=bank, at=0) is bank
        m.encode_features(imu[2:], out=bank, at=2)
        back = bank.select(torch.tensor([0, 1, 2]))
        assert torch.equal(back.tensor(), whole.tensor())
        cat = pkg().load_dropin().ImageFeatures.cat([m.encode_features(imu[:2]), m.encode_features(imu[2:])])
        assert torch.equal(cat.tensor(), whole.tensor())
        with pytest.raises(IndexError):
            m.encode_features(imu, out=bank, at=1)
        # a selected block feeds the step like a fresh encoding
        ids, mask = _grouped(800)[1:3]
        assert torch.equal(m(bank.select(torch.tensor(GROUP_INDEX)), ids, mask)[0], m(imu[GROUP_INDEX], ids, mask)[0])
    m.train()
    with pytest.raises(RuntimeError):                      # inference only, like encode_images
        m.encode_features(imu)
    torch.cuda.synchronize()
