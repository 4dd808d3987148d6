"""GPU: top-k answers with probabilities in one launch -- vqa_softmax_topk against the fp64 reference of tests/_topkref.py (exact
indices in every case; probabilities within relative 2e-5 + absolute 1e-30), and VQAModel.predict_topk / answer_topk / TopK against
the kernel run on the model's own logits, bit for bit on the graphed and the eager route.

Probability bound: the test logits keep |x * scale| <= 20, so the fp32 argument scale * y - m has magnitude <= 40 and is rounded
to within 40 * 2^-24 = 2.4e-6; that enters the numerator and every term of the denominator, on top of a few ulp (6e-8 each) from
expf, the fp32 sum and the division: relative 2e-5 against the fp64 softmax of the same (dtype-rounded) logits.  Every assertion
message carries the measured maximum."""
import os

import numpy as np
import pytest
import torch

import _topkref as R
from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
BOUND = 2e-5
INF, NAN = float("inf"), float("nan")


def K():
    return sub("kernels")


def _logits(B, N, dtype, seed, amp=20.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, N, generator=g) * 2 - 1) * amp).to(dtype)          # |x| <= amp survives the rounding to bf16


def _check(x, k, allowed=None, scale=1.0):
    """Run the kernel on x (a CPU tensor is moved; a device tensor, possibly a strided view, is used as it is) and assert the
    reference's indices exactly and its probabilities within the bound.  Returns (indices, probs, measured error)."""
    xd = x if x.is_cuda else x.to(DEV)
    ad = None if allowed is None else allowed.to(DEV)
    idx, probs, _ = K().softmax_topk(xd, k, ad, scale)
    ri, rp = R.topk_ref(xd, k, allowed, scale)
    assert idx.dtype == torch.int64 and probs.dtype == torch.float32 and idx.shape == probs.shape == (x.shape[0], k)
    assert torch.equal(idx.cpu(), ri), "indices differ from the stable descending sort"
    e, nan_ok = R.prob_error(probs, rp)
    assert nan_ok, "a NaN of the reference is a number here"
    assert e <= BOUND, f"max relative probability error {e:.3e} > {BOUND}"
    return idx, probs, e


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))        # NaN-safe bit equality


# ------------------------------------------------------------------------------------------------------------- kernel
# lane / row boundaries of the issue, plus rows of 16 and 32 values per lane exactly and one more (1024 | 1025, 2048 | 2049)
SHAPES = [(1, 1, 1), (5, 63, 5), (5, 64, 5), (5, 65, 5), (3, 130, 64), (2, 37, 37), (5, 1000, 5), (3, 2000, 10),
          (2, 1024, 5), (2, 1025, 5), (2, 2048, 5), (2, 2049, 5)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,N,k", SHAPES)
def test_kernel_matches_reference(B, N, k, dtype):
    x = _logits(B, N, dtype, seed=B * 7919 + N + k)
    idx, probs, e = _check(x, k)
    if k == N:
        s = probs.double().sum(-1)
        assert (s - 1).abs().max().item() <= BOUND, f"sum of all probabilities off by {(s - 1).abs().max().item():.3e}"
    print(f"softmax_topk {IDS[DTYPES.index(dtype)]} B={B} N={N} k={k}: max rel err {e:.3e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_stride_on_a_slice_of_a_larger_buffer(dtype):
    B, N, k = 5, 65, 5
    buf = torch.full((B, N + 3), 1.0e4, dtype=dtype, device=DEV)              # padding columns that would win every pick
    buf[:, :N] = _logits(B, N, dtype, seed=3).to(DEV)
    x = buf[:, :N]
    assert x.stride(0) == N + 3 and not x.is_contiguous()
    idx, _, _ = _check(x, k)
    assert int(idx.max()) < N
    lf = K().softmax_topk(x, k, want_logits=True)[2]
    assert _same(lf, x.float().contiguous())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,N,k", [(5, 65, 5), (3, 130, 64), (5, 1000, 5), (2, 2049, 7)])
def test_ties_resolve_to_the_lowest_index(B, N, k, dtype):
    g = torch.Generator().manual_seed(N)
    x = torch.randint(-3, 4, (B, N), generator=g).to(dtype)                    # seven values: every row is full of ties
    idx, _, _ = _check(x, k)
    v = x.float().gather(1, idx.cpu())
    assert ((v[:, 1:] < v[:, :-1]) | ((v[:, 1:] == v[:, :-1]) & (idx.cpu()[:, 1:] > idx.cpu()[:, :-1]))).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,k", [(65, 64), (1000, 5), (2049, 6)])
def test_special_values(N, k, dtype):
    x = _logits(5, N, dtype, seed=N + 1)
    x[0, ::3] = -INF                                      # some -inf entries: probability exactly 0, ordered last by index
    x[1, 0] = 0.0; x[1, 1] = -0.0                         # signed zeros tie
    x[2, 7] = NAN; x[2, N - 2] = NAN                      # two NaNs among normal rows
    x[3] = NAN                                            # all NaN
    x[4, 5] = -INF
    idx, probs, _ = _check(x, k)
    idx, probs = idx.cpu(), probs.cpu()
    assert idx[2, :2].tolist() == [7, N - 2] and torch.isnan(probs[2]).all()
    assert idx[3].tolist() == list(range(k)) and torch.isnan(probs[3]).all()
    assert not torch.isnan(probs[[0, 1, 4]]).any()        # the neighbours of the NaN rows are unaffected
    n_fin = N - len(range(0, N, 3))
    if k > n_fin:                                         # the picks reach the -inf entries: index order, probability exactly 0
        assert idx[0, n_fin:].tolist() == list(range(0, N, 3))[:k - n_fin] and (probs[0, n_fin:] == 0).all()
    # the same rows one at a time (a workgroup with one live row) give the same bits
    xd = x.to(DEV)
    for r in range(5):
        i1, p1, _ = K().softmax_topk(xd[r:r + 1], k)
        assert torch.equal(i1.cpu()[0], idx[r]) and _same(p1.cpu()[0], probs[r])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mdtype", [torch.bool, torch.uint8], ids=["bool", "uint8"])
@pytest.mark.parametrize("N,k", [(65, 5), (1000, 5), (2049, 5)])
def test_mask(N, k, mdtype, dtype):
    B = 5
    x = _logits(B, N, dtype, seed=N + 17)
    g = torch.Generator().manual_seed(N)
    shared = (torch.rand(N, generator=g) < 0.5)
    shared[:k] = True
    _check(x, k, shared.to(mdtype))
    per = (torch.rand(B, N, generator=g) < 0.3)
    per[:, N - 1] = True
    per[1] = False; per[1, torch.randperm(N, generator=g)[:k]] = True               # exactly k allowed
    per[2] = False; per[2, [3, N - 1]] = True                                       # fewer than k allowed
    per[3] = False                                                                  # nothing allowed
    idx, probs, _ = _check(x, k, per.to(mdtype))
    idx, probs = idx.cpu(), probs.cpu()
    assert sorted(idx[1].tolist()) == sorted(per[1].nonzero().flatten().tolist()) and (probs[1] > 0).all()
    assert sorted(idx[2, :2].tolist()) == [3, N - 1] and idx[2, 2:].tolist() == [j for j in range(N) if j not in (3, N - 1)][:k - 2]
    assert (probs[2, 2:] == 0).all() and abs(float(probs[2, :2].double().sum()) - 1) <= BOUND
    assert idx[3].tolist() == list(range(k)) and torch.isnan(probs[3]).all()
    assert per[0][idx[0]].all() and per[4][idx[4]].all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_raw_logits_copy_is_unmasked_and_bit_equal(dtype):
    B, N, k = 5, 1000, 5
    x = _logits(B, N, dtype, seed=23)
    x[1, 4] = NAN; x[2, 9] = -INF; x[3, 0] = -0.0
    xd = x.to(DEV)
    allowed = (torch.rand(B, N, generator=torch.Generator().manual_seed(2)) < 0.5).to(DEV)
    for a in (None, allowed, allowed[0].contiguous()):
        _, _, lf = K().softmax_topk(xd, k, a, want_logits=True)
        assert lf.dtype == torch.float32 and _same(lf, xd.float())
    assert K().softmax_topk(xd, k)[2] is None


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,N,k", [(5, 65, 5), (5, 1000, 5), (2, 2049, 5)])
def test_temperature(B, N, k, dtype):
    x10 = _logits(B, N, dtype, seed=N + 5, amp=10.0)                # |x * 2| <= 20
    x20 = _logits(B, N, dtype, seed=N + 6, amp=20.0)
    i2, p2, e2 = _check(x10, k, scale=2.0)
    ih, ph, eh = _check(x20, k, scale=0.5)
    i1, p1, e1 = _check(x10, k, scale=1.0)
    assert torch.equal(i1, i2)                                       # the order never sees the scale
    assert not torch.equal(p1, p2)
    i1b, p1b, _ = K().softmax_topk(x10.to(DEV), k, None, 1.0)
    assert torch.equal(i1, i1b) and _same(p1, p1b)                   # run twice: the same bits
    # scale = 1 multiplies by 1.0f, which is exact: the probabilities are those of x itself (what _check(scale=1) compared) and
    # equal, bit for bit, the probabilities of 2 * x at scale 0.5 (both products exact, the same arguments)
    ix, px, _ = K().softmax_topk((x10.float() * 2).to(dtype).to(DEV), k, None, 0.5)
    assert torch.equal(ix, i1) and _same(px, p1)
    print(f"softmax_topk temperature N={N}: max rel err scale 2 {e2:.3e}, 0.5 {eh:.3e}, 1 {e1:.3e}")


def test_argument_errors_return_1000_and_write_nothing():
    L = sub("_lib")
    B, N, k = 3, 70, 5
    x = _logits(B, N, torch.float32, seed=1).to(DEV)
    al = torch.ones(B, N, dtype=torch.uint8, device=DEV)
    idx = torch.full((B, 80), -7, dtype=torch.int64, device=DEV)
    probs = torch.full((B, 80), -7.0, device=DEV)
    fn = L.lib().vqa_softmax_topk
    st = L.stream()
    good = dict(dtype=0, logits=x.data_ptr(), ld=N, allowed=al.data_ptr(), ald=N, scale=1.0, idx=idx.data_ptr(), probs=probs.data_ptr(),
                lf=None, B=B, N=N, K=k)
    order = ["dtype", "logits", "ld", "allowed", "ald", "scale", "idx", "probs", "lf", "B", "N", "K"]
    bad = [dict(logits=None), dict(idx=None), dict(probs=None), dict(B=0), dict(N=0), dict(K=0), dict(B=-1), dict(K=65), dict(K=N + 1),
           dict(N=3, ld=3, ald=3, K=5), dict(N=4, K=5),                # K > N on its own (K <= 64)
           dict(ld=N - 1), dict(ald=N - 1), dict(ald=1), dict(ald=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=INF), dict(scale=NAN),
           dict(dtype=2), dict(dtype=-1)]
    for b in bad:
        a = dict(good, **b)
        assert fn(*[a[n] for n in order], st) == 1000, b
    torch.cuda.synchronize()
    assert (idx == -7).all() and (probs == -7.0).all()
    assert fn(*[good[n] for n in order], st) == 0                     # the same arguments without the error do launch
    torch.cuda.synchronize()
    ri, _ = R.topk_ref(x, k)
    assert torch.equal(idx.view(-1)[:B * k].view(B, k).cpu(), ri)
    with pytest.raises(RuntimeError):
        K().softmax_topk(x, N + 1)
    with pytest.raises(RuntimeError):
        K().softmax_topk(x[:, :3], 5)                                 # K > N with K <= 64
    with pytest.raises(ValueError):
        K().softmax_topk(x, k, torch.ones(N + 1, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        K().softmax_topk(x, k, torch.ones(N, device=DEV))


# -------------------------------------------------------------------------------------------------------------- model
IDX = [2, 0, 0, 2, 2, 0, 2]              # U = 3 images, N = 7 questions (tests/test_gpu_multi_question.py)


def _model(dtype, seed=11):
    cfg = O.full_config()
    sd = O.init_state_dict(cfg, seed, jitter=True)
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), cfg


def _batch(U=3, N=7, seed=5):
    images, _, _, _ = O.synthetic_batch(U, seed=seed)
    _, ids, mask, _ = O.synthetic_batch(N, seed=seed + 1)
    mask[:, 0] = 1
    return images.to(DEV), ids.to(DEV), mask.to(DEV)


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def model(request):
    m, cfg = _model(request.param)
    return m, cfg, request.param


def _expect(m, x, ids, mask, k, amask=None, temperature=1.0, image_index=None):
    """kernels.softmax_topk on the model's own logits: what predict_topk must equal bit for bit."""
    with torch.no_grad():
        lg = m(x, ids, mask, image_index=image_index)[0]
    i, p, _ = K().softmax_topk(lg, k, amask, 1.0 / temperature)
    return i, p, lg


def _assert_topk(t, exp, what=""):
    i, p, lg = exp
    assert _same(t.indices, i), what + ": indices"
    assert _same(t.probs, p), what + ": probabilities"
    if t.logits is not None:
        assert t.logits.dtype == torch.float32 and _same(t.logits, lg), what + ": logits"


def test_predict_topk_equals_the_kernel_on_the_models_logits(model):
    """Graphed at B = 1 and B = 3, eager at the same B = 3 (graph_max_batch = 2 on the instance).  predict()'s indices agree on every
    row whose k + 1 best logits are distinct (a tie at the k-th place leaves torch.topk's choice open as much as one inside)."""
    m, cfg, _ = model
    x, ids, mask = _batch(3, 3)
    with torch.no_grad():
        for B in (1, 3):
            t = m.predict_topk(x[:B], ids[:B], mask[:B], top_k=5, return_logits=True)
            assert t.indices.shape == (B, 5) and t.logits.shape == (B, cfg["num_answers"])
            _assert_topk(t, _expect(m, x[:B], ids[:B], mask[:B], 5), f"graphed B={B}")
            assert m.predict_topk(x[:B], ids[:B], mask[:B]).logits is None
        graphs = len(m._graphs)
        m.graph_max_batch = 2
        try:
            t = m.predict_topk(x, ids, mask, top_k=5, return_logits=True)
            _assert_topk(t, _expect(m, x, ids, mask, 5), "eager B=3")
            assert len(m._graphs) == graphs                           # nothing was captured for it
        finally:
            del m.graph_max_batch
        pi, pp = m.predict(x, ids, mask, top_k=5)
        t = m.predict_topk(x, ids, mask, top_k=5, return_logits=True)
        top = t.logits.topk(6, dim=-1).values
        distinct = (top[:, 1:] != top[:, :-1]).all(-1)
        assert distinct.any()
        assert torch.equal(pi[distinct], t.indices[distinct])
        assert (pp[distinct] - t.probs[distinct]).abs().max().item() <= 1e-5


def test_replay_returns_copies_and_follows_the_input(model):
    m, _, _ = model
    x, ids, mask = _batch(3, 3)
    x2, ids2, mask2 = _batch(3, 3, seed=9)
    with torch.no_grad():
        t1 = m.predict_topk(x, ids, mask, top_k=5, return_logits=True)
        keep = [v.clone() for v in t1]
        t2 = m.predict_topk(x2, ids2, mask2, top_k=5, return_logits=True)
        _assert_topk(t2, _expect(m, x2, ids2, mask2, 5), "second input")
        assert not _same(t2.logits, t1.logits)
        for a, b in zip(t1, keep):
            assert _same(a, b)                                        # the first result is no view of a static buffer
        assert len({v.data_ptr() for v in t1} | {v.data_ptr() for v in t2}) == 6


def test_graphs_are_keyed_on_k_mask_and_temperature(model):
    m, cfg, _ = model
    x, ids, mask = _batch(3, 3)
    A = cfg["num_answers"]
    amask = (torch.rand(A, generator=torch.Generator().manual_seed(1)) < 0.2).to(DEV)
    amask2 = (torch.rand(3, A, generator=torch.Generator().manual_seed(2)) < 0.2).to(DEV)
    steps = [dict(top_k=3), dict(top_k=5), dict(top_k=5, answer_mask=amask), dict(top_k=5, answer_mask=amask2),
             dict(top_k=5, answer_mask=amask.to(torch.uint8)), dict(top_k=5, temperature=2.5), dict(top_k=3, return_logits=True), dict(top_k=3)]
    with torch.no_grad():
        for s in steps:
            t = m.predict_topk(x, ids, mask, **s)
            assert t.indices.shape == (3, s["top_k"]) and (t.logits is not None) == bool(s.get("return_logits"))
            _assert_topk(t, _expect(m, x, ids, mask, s["top_k"], s.get("answer_mask"), s.get("temperature", 1.0)), str(sorted(s)))
            if "answer_mask" in s:
                am = s["answer_mask"].bool()
                assert (am.expand(3, A).gather(1, t.indices)).all()  # (far more than 5 answers are allowed in every row)


def test_image_index_and_contexts(model):
    m, cfg, dtype = model
    x, ids, mask = _batch()
    idx = torch.tensor(IDX)
    amask = (torch.rand(7, cfg["num_answers"], generator=torch.Generator().manual_seed(4)) < 0.5).to(DEV)
    with torch.no_grad():
        ctx = m.encode_images(x)
        for kw in (dict(), dict(answer_mask=amask, temperature=0.7)):
            a = m.predict_topk(x, ids, mask, top_k=5, image_index=idx, return_logits=True, **kw)
            b = m.answer_topk(ctx, ids, mask, top_k=5, image_index=idx, return_logits=True, **kw)
            for u, v in zip(a, b):
                assert _same(u, v)
            _assert_topk(a, _expect(m, x, ids, mask, 5, kw.get("answer_mask"), kw.get("temperature", 1.0), image_index=idx), "indexed")
        # answer_topk against the kernel on answer()'s logits, graphed and eager, implied index included
        lg = m.answer(ctx, ids, mask, image_index=idx)[0]
        i, p, _ = K().softmax_topk(lg, 5)
        _assert_topk(m.answer_topk(ctx, ids, mask, image_index=idx, return_logits=True), (i, p, lg), "answer graphed")
        ctx1 = m.encode_images(x[:1])
        lg1 = m.answer(ctx1, ids, mask)[0]
        i1, p1, _ = K().softmax_topk(lg1, 5)
        _assert_topk(m.answer_topk(ctx1, ids, mask, return_logits=True), (i1, p1, lg1), "answer, one image, implied index")
        m.graph_max_batch = 2
        try:
            lg = m.answer(ctx, ids, mask, image_index=idx)[0]
            i, p, _ = K().softmax_topk(lg, 5)
            _assert_topk(m.answer_topk(ctx, ids, mask, image_index=idx, return_logits=True), (i, p, lg), "answer eager")
            _assert_topk(m.answer_topk(ctx1, ids, mask, return_logits=True), (i1, p1, lg1), "answer eager, implied index")
        finally:
            del m.graph_max_batch
        # the expanded batch: the same answers within the logit noise of the route (tests/test_gpu_multi_question.py's bounds)
        e = m.predict_topk(x[idx.to(DEV)], ids, mask, top_k=5, return_logits=True)
        a = m.predict_topk(x, ids, mask, top_k=5, image_index=idx, return_logits=True)
        d = a.logits - e.logits
        bound = 1e-4 if dtype == "fp32" else 2e-2 * max(1.0, e.logits.abs().max().item())
        assert d.abs().max().item() <= bound, d.abs().max().item()
        assert torch.equal(a.indices[:, 0], e.indices[:, 0])


def _lenmask(lens, L=20):
    return (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).long()


def test_all_padding_question(model, golden_dir):
    """The case behind tests/golden/full_eval_allpad.npz: row 2 has no token.  Its logits are NaN, so its probabilities are NaN and
    its indices 0 ... k-1.  The other rows' logits equal those of the batch without that row within 1e-3 in fp32 (the bound of
    test_gpu_model.py::test_eval_allpad_row_nan_like_reference) and within bf16 route noise in bf16; per row, wherever the gaps
    between the k + 1 best logits exceed twice that bound, the indices are equal; the r-th probability of every such row is within
    exp(2 bound) - 1 relative."""
    m, cfg, dtype = model
    g = np.load(os.path.join(golden_dir, "full_eval_allpad.npz"))
    images, ids, _, _ = O.synthetic_batch(4, seed=11)
    mask = _lenmask([20, 15, 7, 5]); mask[2] = 0
    x, ids, mask = images.to(DEV), ids.to(DEV), mask.to(DEV)
    k = 5
    with torch.no_grad():
        t = m.predict_topk(x, ids, mask, top_k=k, return_logits=True)
        _assert_topk(t, _expect(m, x, ids, mask, k), "all-pad batch")
        assert (torch.isnan(t.logits).cpu().numpy() == np.isnan(g["logits"])).all()
        assert torch.isnan(t.probs[2]).all() and t.indices[2].tolist() == list(range(k))
        keep = [0, 1, 3]
        assert not torch.isnan(t.probs[keep]).any()
        w = m.predict_topk(x[keep], ids[keep], mask[keep], top_k=k, return_logits=True)
        # fp32: the bound of the existing all-pad test; bf16: the logit noise between two routes of one question, as in
        # test_image_index_and_contexts (a batch of 3 and a batch of 4 may round differently in bf16)
        bound = 1e-3 if dtype == "fp32" else 2e-2 * max(1.0, w.logits.abs().max().item())
        dl = (t.logits[keep] - w.logits).abs().max().item()
        rel = ((t.probs[keep] - w.probs).abs() / w.probs).max(-1).values
        top = w.logits.topk(k + 1, dim=-1).values
        clear = ((top[:, :-1] - top[:, 1:]) > 2 * bound).all(-1)            # rows whose k + 1 best logits cannot change places
        print(f"all-pad {dtype}: max |dlogit| {dl:.3e} (bound {bound:.3e}), rel prob err per row {rel.tolist()}, "
              f"clear rows {int(clear.sum())}/3")
        assert dl < bound, dl
        assert torch.equal(t.indices[keep][clear], w.indices[clear])
        # every row, clear or not: the r-th largest of a row moves by at most the bound whichever index holds it (order statistics are
        # 1-Lipschitz in the sup norm), so numerator and denominator are each within exp(+-bound) and the quotient within exp(2 bound)
        assert (rel <= float(np.expm1(2 * bound)) + 1e-6).all(), rel.tolist()


def test_errors(model):
    m, cfg, _ = model
    x, ids, mask = _batch(3, 3)
    A = cfg["num_answers"]
    with torch.no_grad():
        ctx = m.encode_images(x)
        for k in (0, 65, A + 1, -1, 2.0, True):
            with pytest.raises(ValueError):
                m.predict_topk(x, ids, mask, top_k=k)
            with pytest.raises(ValueError):
                m.answer_topk(ctx, ids, mask, top_k=k)
        for t in (0, -1, INF, NAN, 0.0, "warm"):
            with pytest.raises(ValueError):
                m.predict_topk(x, ids, mask, temperature=t)
            with pytest.raises(ValueError):
                m.answer_topk(ctx, ids, mask, temperature=t)
        for am in (torch.ones(A + 1, dtype=torch.bool, device=DEV), torch.ones(2, A, dtype=torch.bool, device=DEV),
                   torch.ones(3, A, 1, dtype=torch.bool, device=DEV), torch.ones(A, device=DEV), torch.ones(A, dtype=torch.int64, device=DEV),
                   torch.ones(A, dtype=torch.bool), [True] * A):
            with pytest.raises(ValueError):
                m.predict_topk(x, ids, mask, answer_mask=am)
            with pytest.raises(ValueError):
                m.answer_topk(ctx, ids, mask, answer_mask=am)
        with pytest.raises(RuntimeError):
            m.predict_topk(x.cpu(), ids.cpu(), mask.cpu())
        with pytest.raises(RuntimeError):
            m.answer_topk(ctx, ids.cpu(), mask.cpu())
        with pytest.raises(IndexError):
            m.predict_topk(x, ids, mask, image_index=torch.tensor([0, 1, 3]))
        with pytest.raises(ValueError):
            m.predict_topk(x, ids, mask, image_index=torch.tensor([0, 1]))
        with pytest.raises(ValueError):
            m.answer_topk(object(), ids, mask)
        m.train()
        try:
            with pytest.raises(RuntimeError):
                m.predict_topk(x, ids, mask)
            with pytest.raises(RuntimeError):
                m.answer_topk(ctx, ids, mask)
            assert m.training                                         # (and it did not switch the mode for the caller)
        finally:
            m.eval()
        m.predict_topk(x, ids, mask)                                  # still fine after the refusals
        m.answer_topk(ctx, ids, mask)
        m.load_state_dict(m.state_dict())                             # bumps the context epoch: the context is stale now
        with pytest.raises(RuntimeError):
            m.answer_topk(ctx, ids, mask)


def test_to_records(model):
    m, _, _ = model
    x, ids, mask = _batch(3, 3)
    with torch.no_grad():
        t = m.predict_topk(x, ids, mask, top_k=4)
    calls = []

    def decode(i):
        assert type(i) is int
        calls.append(i)
        return f"answer-{i}"

    recs = t.to_records(decode)
    il, pl = t.indices.tolist(), t.probs.tolist()
    assert calls == [i for row in il for i in row]                    # once per emitted index, in order
    assert len(recs) == 3
    for r, irow, prow in zip(recs, il, pl):
        assert set(r) == {"answers", "top_answer", "confidence"}
        assert r["answers"] == [{"answer": f"answer-{i}", "probability": p, "index": i} for i, p in zip(irow, prow)]
        assert r["top_answer"] == f"answer-{irow[0]}" and r["confidence"] == prow[0]
        assert all(type(a["probability"]) is float for a in r["answers"])
