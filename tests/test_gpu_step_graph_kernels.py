"""The kernels under HipTrainer.step_graphed, entry by entry (include/vqa_hip.h, "step state on the device"):
  * vqa_step_state_set writes the block the header declares;
  * each vqa_adamw*_dev entry gives the bits of its by-value twin on p, m, v, the bf16 copy, ema, skipped (and lag);
  * every exported entry that takes a dropout seed gives the same outputs for the plain seed W | site and for the flagged seed word
    that points at a device word holding W, and other outputs once that word is rewritten.
All comparisons are torch.equal.  Shapes are the smallest with a partial tile / a tail (M = 70, N = 40; n = 1027)."""
import math

import pytest
import torch

from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _L():
    return sub("_lib")


def _SG():
    return sub("stepgraph")


def _state(calls, seed_step=0, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, max_norm=1.0, gscale=1.0, ema_decay=0.0, ema_warmup=0):
    st = torch.zeros(_SG().STATE_BYTES // 4, device=DEV, dtype=torch.int32)
    _L().call("vqa_step_state_set", st.data_ptr(), calls, seed_step, lr, b1, b2, eps, wd, max_norm, gscale, ema_decay, ema_warmup)
    return st


def test_step_state_set_writes_the_declared_block():
    SG = _SG()
    w = SG.seed_step(3, 0x5EED, 12345)
    st = _state(1000, w, lr=3e-4, b1=0.8, b2=0.99, eps=1e-6, wd=0.05, max_norm=0.5, gscale=0.25, ema_decay=0.999, ema_warmup=1)
    torch.cuda.synchronize()
    s = SG.StepState.from_buffer_copy(st.cpu().numpy().tobytes())
    f32 = lambda x: torch.tensor(x, dtype=torch.float32).item()
    assert (s.calls, s.seed_step, s.ema_warmup) == (1000, w, 1)
    assert [s.lr, s.b1, s.b2, s.eps, s.wd, s.max_norm, s.gscale, s.ema_decay] == [f32(x) for x in (3e-4, 0.8, 0.99, 1e-6, 0.05, 0.5, 0.25, 0.999)]
    assert list(s._pad) == [0, 0, 0]
    L = _L()
    for bad in (dict(calls=0), dict(seed_step=w | 5), dict(seed_step=w | (1 << 63))):        # refused without a launch
        kw = dict(dict(calls=1, seed_step=w), **bad)
        with pytest.raises(RuntimeError):
            L.call("vqa_step_state_set", st.data_ptr(), kw["calls"], kw["seed_step"], 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0, 0.0, 0)
    with pytest.raises(RuntimeError):
        L.call("vqa_step_state_set", st.data_ptr() + 8, 1, w, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0, 0.0, 0)      # not 16-byte aligned
    torch.cuda.synchronize()
    assert SG.StepState.from_buffer_copy(st.cpu().numpy().tobytes()).calls == 1000


# ---------------------------------------------------------------------------------------------------------------- AdamW twins
HYPER = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)


def _adam_inputs(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    p = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g) * 0.1
    m = torch.randn(n, generator=g) * 0.01
    v = torch.rand(n, generator=g) * 0.01
    e = torch.randn(n, generator=g)
    return [t.to(DEV) for t in (p, gr, m, v, e)]


def _run_adamw(dev, ranges, ema, n, calls, skipped2, skip, max_norm, warmup, decay=0.99):
    """One launch of vqa_adamw[_ranges][_ema][_dev]; returns every buffer the entry may write."""
    L = _L()
    p, g, m, v, e = _adam_inputs(n, 7)
    pb = torch.full((n,), 3.0, device=DEV, dtype=torch.bfloat16)
    sumsq = torch.zeros(1 + 2048, device=DEV)
    sumsq[0] = (g.double() ** 2).sum().float()                 # |g| ~ 0.1 sqrt(n): clipped at max_norm 0.05, untouched at 1e9
    skipf = torch.tensor([skip], device=DEV, dtype=torch.int32)
    skipped = torch.tensor([0, 0, skipped2], device=DEV, dtype=torch.int32)
    # steps each range's parameter spent frozen; a range's Adam step number calls - skipped[2] - lag must stay >= 1
    lag = torch.tensor([0, 2, 5] if calls - skipped2 > 5 or skip else [0, 0, 0], device=DEV, dtype=torch.int32)
    frozen = torch.tensor([1], device=DEV, dtype=torch.int32)
    # three ranges of a 64-element buffer, rows {lo, hi, pos, lag index}; the elements outside them must stay as they are
    table = torch.tensor([[0, 8, 0, 0], [16, 40, 8, 1], [48, 64, 32, 2]], dtype=torch.int64).to(DEV)
    gscale = 0.5
    if dev:
        st = _state(calls, 0, max_norm=max_norm, gscale=gscale, ema_decay=decay if ema else 0.0, ema_warmup=warmup if ema else 0, **HYPER)
        hyper, tail = (st.data_ptr(),), ()
        ema_args = (e.data_ptr(),) if ema else ()
    else:
        hyper, tail = (HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], HYPER["wd"], calls), (max_norm, gscale)
        ema_args = (e.data_ptr(), decay, warmup) if ema else ()
    name = "vqa_adamw" + ("_ranges" if ranges else "") + ("_ema" if ema else "") + ("_dev" if dev else "")
    if ranges:
        L.call(name, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), table.data_ptr(), 3, 48, *hyper, sumsq.data_ptr(), *tail,
               skipf.data_ptr(), skipped.data_ptr(), lag.data_ptr(), frozen.data_ptr(), 1, pb.data_ptr(), *ema_args)
    else:
        L.call(name, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, *hyper, sumsq.data_ptr(), *tail,
               skipf.data_ptr(), skipped.data_ptr(), pb.data_ptr(), *ema_args)
    torch.cuda.synchronize()
    return dict(p=p, m=m, v=v, bf16=pb, ema=e, skipped=skipped, lag=lag)


CALLS = [(1, 0), (7, 1), (1000, 13)]          # (calls, skipped[2]): Adam's step number is their difference (1, 6, 987)


@pytest.mark.parametrize("ranges", [False, True], ids=["plain", "ranges"])
@pytest.mark.parametrize("ema,warmup", [(False, 0), (True, 0), (True, 1)], ids=["adamw", "ema", "ema_warmup"])
@pytest.mark.parametrize("max_norm", [0.05, 1e9], ids=["clip", "noclip"])
@pytest.mark.parametrize("calls,skipped2", CALLS)
def test_dev_adamw_is_bit_equal_to_its_by_value_twin(ranges, ema, warmup, max_norm, calls, skipped2):
    n = 64 if ranges else 1027
    a = _run_adamw(False, ranges, ema, n, calls, skipped2, 0, max_norm, warmup)
    b = _run_adamw(True, ranges, ema, n, calls, skipped2, 0, max_norm, warmup)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    p0 = _adam_inputs(n, 7)[0]
    assert not torch.equal(a["p"], p0) and bool(torch.isfinite(a["p"]).all())          # the update was applied
    if ranges:
        assert torch.equal(a["p"][8:16], p0[8:16]) and torch.equal(a["p"][40:48], p0[40:48]) and a["lag"].tolist() == ([0, 3, 5] if calls > 1 else [0, 1, 0])
        assert a["bf16"][8:16].float().eq(3.0).all()
    assert a["skipped"].tolist() == [0, 0, skipped2]
    if ema:
        assert not torch.equal(a["ema"], _adam_inputs(n, 7)[4])


@pytest.mark.parametrize("ranges", [False, True], ids=["plain", "ranges"])
@pytest.mark.parametrize("ema", [False, True], ids=["adamw", "ema"])
def test_dev_adamw_with_the_skip_flag_writes_nothing_and_bumps_the_counters(ranges, ema):
    n = 64 if ranges else 1027
    a = _run_adamw(False, ranges, ema, n, 7, 2, 3, 0.05, 1)
    b = _run_adamw(True, ranges, ema, n, 7, 2, 3, 0.05, 1)
    p, _, m, v, e = _adam_inputs(n, 7)
    for r in (a, b):
        assert torch.equal(r["p"], p) and torch.equal(r["m"], m) and torch.equal(r["v"], v) and torch.equal(r["ema"], e)
        assert r["bf16"].float().eq(3.0).all() and r["skipped"].tolist() == [3, 1, 3] and r["lag"].tolist() == [0, 2, 5]


# ------------------------------------------------------------------------------------------------------------------- the seeds
def _randn(*shape, seed, dtype=torch.float32, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype).contiguous()


def _entry_igemm(dtype):
    K = sub("kernels")
    M, N, Kin = 70, 40, 64
    x, w, b = _randn(M, Kin, seed=1, dtype=dtype), _randn(N, Kin, seed=2, dtype=dtype, scale=0.2), _randn(N, seed=3)
    return lambda seed: [K.igemm(x, w, M, N, Kin, K.linear_geom(M, Kin), dtype=dtype, bias=b, relu=1, drop_p=0.3, drop_seed=seed)[0]]


def _entry_embed(dtype, bwd):
    L = _L()
    B, Lq, D, V = 3, 5, 40, 11
    rows = B * Lq
    ids = torch.randint(1, V, (B, Lq), generator=torch.Generator().manual_seed(4)).to(DEV)
    emb, pe, dout = _randn(V, D, seed=5), _randn(1, Lq, D, seed=6), _randn(rows, D, seed=7, dtype=dtype)

    def fwd(seed):
        out = torch.empty((rows, D), device=DEV, dtype=dtype)
        L.call("vqa_embed_fwd", L.dt(dtype), ids.data_ptr(), emb.data_ptr(), pe.data_ptr(), out.data_ptr(), rows, Lq, D, V, math.sqrt(D), 0.3, seed)
        return [out]

    def back(seed):
        demb = torch.zeros((V, D), device=DEV)
        L.call("vqa_embed_bwd", L.dt(dtype), ids.data_ptr(), dout.data_ptr(), demb.data_ptr(), rows, D, V, math.sqrt(D), 0.3, seed)
        return [demb]
    return back if bwd else fwd


def _entry_layernorm(dtype, D, bwd):
    L = _L()
    rows = 70
    x, dout = _randn(rows, D, seed=8, dtype=dtype), _randn(rows, D, seed=9, dtype=dtype)
    gamma, beta = _randn(D, seed=10) + 1.0, _randn(D, seed=11)
    out0, st = torch.empty_like(x), torch.empty((rows, 2), device=DEV)
    L.call("vqa_layernorm_fwd", L.dt(dtype), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out0.data_ptr(), st.data_ptr(), rows, D, 1e-5, 0.0, 0,
           None, 1)

    def fwd(seed):
        out, s2 = torch.empty_like(x), torch.empty((rows, 2), device=DEV)
        L.call("vqa_layernorm_fwd", L.dt(dtype), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), s2.data_ptr(), rows, D, 1e-5,
               0.3, seed, None, 1)
        return [out, s2]

    def back(seed):
        dx, dg, db = torch.empty_like(x), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        ws = torch.empty((L.count("vqa_layernorm_bwd_ws", L.dt(dtype), rows, D, 0),), device=DEV)
        L.call("vqa_layernorm_bwd", L.dt(dtype), dout.data_ptr(), x.data_ptr(), gamma.data_ptr(), st.data_ptr(), None, dx.data_ptr(), dg.data_ptr(),
               db.data_ptr(), rows, D, 0.3, seed, None, 1, ws.data_ptr(), 0)
        return [dx, dg, db]
    return back if bwd else fwd


def _entry_bias_act(dtype, N):
    L = _L()
    M = 70
    dout = _randn(M, N, seed=12, dtype=dtype)

    def run(seed):
        dz, db = torch.empty_like(dout), torch.zeros(N, device=DEV)
        ws = torch.empty((L.count("vqa_bias_act_bwd_ws", L.dt(dtype), M, N),), device=DEV)
        L.call("vqa_bias_act_bwd", L.dt(dtype), dout.data_ptr(), None, dz.data_ptr(), db.data_ptr(), M, N, 0.3, seed, ws.data_ptr(), 0)
        return [dz, db]
    return run


def _entry_attention(name):
    """The attention family: B = 3 questions, H = 2 heads, Lq = 5, Lk = 7 (partial tiles everywhere); the _idx entries read the
    K / V of U = 2 images through an index.  MFMA forms: bf16, head dimension 32; the others: fp32, head dimension 8."""
    L = _L()
    mfma, idx = "_mfma" in name, "_idx" in name
    dtype = torch.bfloat16 if mfma else torch.float32
    B, H, Lq, Lk, hd, U = 3, 2, 5, 7, (32 if mfma else 8), 2
    d = H * hd
    nk = U if idx else B
    q, k, v = _randn(B * Lq, d, seed=13, dtype=dtype), _randn(nk * Lk, d, seed=14, dtype=dtype), _randn(nk * Lk, d, seed=15, dtype=dtype)
    dctx, dprobs = _randn(B * Lq, d, seed=16, dtype=dtype), _randn(B, H, Lq, Lk, seed=17, scale=0.1)
    kvi = torch.tensor([1, 0, 1], device=DEV, dtype=torch.int32)
    offsets, order = torch.empty(U + 1, device=DEV, dtype=torch.int32), torch.empty(B, device=DEV, dtype=torch.int32)
    L.call("vqa_index_csr", kvi.data_ptr(), B, U, offsets.data_ptr(), order.data_ptr())
    head = () if mfma else (L.dt(dtype),)
    qkv = (q.data_ptr(), k.data_ptr(), v.data_ptr(), d, d, d)
    alive = (q, k, v, dctx, dprobs, kvi, offsets, order)       # the closures below pass raw pointers: they must own the tensors
    dims = (B, H, Lq, Lk, hd)
    # the softmax before dropout (what the backward reads) does not depend on the seed: taken once from a forward without dropout
    probs0, ctx0 = torch.empty((B, H, Lq, Lk), device=DEV), torch.empty((B * Lq, d), device=DEV, dtype=dtype)
    if idx:
        L.call("vqa_attention_fwd" + ("_mfma" if mfma else "") + "_idx_train", *head, *qkv, kvi.data_ptr(), U, None, probs0.data_ptr(),
               ctx0.data_ptr(), d, *dims, 0.0, 0)
    else:
        L.call("vqa_attention_fwd" + ("_mfma" if mfma else ""), *head, *qkv, None, probs0.data_ptr(), ctx0.data_ptr(), d, *dims, 0.0, 0)

    def fwd(seed, alive=alive):
        probs, ctx = torch.empty_like(probs0), torch.empty_like(ctx0)
        mid = (kvi.data_ptr(), U) if idx else ()
        L.call(name, *head, *qkv, *mid, None, probs.data_ptr(), ctx.data_ptr(), d, *dims, 0.3, seed)
        return [probs, ctx]

    def back(seed, alive=alive):
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        mid = (offsets.data_ptr(), order.data_ptr(), U) if idx else ((dprobs.data_ptr(),) if name.endswith("_dp") else ())
        L.call(name, *head, dctx.data_ptr(), d, *qkv, probs0.data_ptr(), *mid, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), d, d, d, *dims, 0.3, seed)
        return [dq, dk, dv]
    return fwd if "_fwd" in name else back


F32, BF16 = torch.float32, torch.bfloat16
SEEDED = {
    "vqa_igemm-fp32": lambda: _entry_igemm(F32), "vqa_igemm-bf16": lambda: _entry_igemm(BF16),
    "vqa_embed_fwd-fp32": lambda: _entry_embed(F32, False), "vqa_embed_fwd-bf16": lambda: _entry_embed(BF16, False),
    "vqa_embed_bwd-fp32": lambda: _entry_embed(F32, True), "vqa_embed_bwd-bf16": lambda: _entry_embed(BF16, True),
    "vqa_layernorm_fwd-fp32-40": lambda: _entry_layernorm(F32, 40, False), "vqa_layernorm_fwd-bf16-40": lambda: _entry_layernorm(BF16, 40, False),
    "vqa_layernorm_fwd-bf16-64": lambda: _entry_layernorm(BF16, 64, False),
    "vqa_layernorm_bwd-fp32-40": lambda: _entry_layernorm(F32, 40, True), "vqa_layernorm_bwd-bf16-40": lambda: _entry_layernorm(BF16, 40, True),
    "vqa_layernorm_bwd-bf16-64": lambda: _entry_layernorm(BF16, 64, True),
    "vqa_bias_act_bwd-fp32-40": lambda: _entry_bias_act(F32, 40), "vqa_bias_act_bwd-bf16-40": lambda: _entry_bias_act(BF16, 40),
    "vqa_bias_act_bwd-fp32-37": lambda: _entry_bias_act(F32, 37),
}
for _n in ("vqa_attention_fwd", "vqa_attention_fwd_mfma", "vqa_attention_bwd", "vqa_attention_bwd_mfma", "vqa_attention_bwd_dp",
           "vqa_attention_bwd_mfma_dp", "vqa_attention_fwd_idx_train", "vqa_attention_fwd_mfma_idx_train", "vqa_attention_bwd_idx",
           "vqa_attention_bwd_mfma_idx"):
    SEEDED[_n] = (lambda n: (lambda: _entry_attention(n)))(_n)


def test_the_table_covers_every_exported_entry_that_takes_a_seed():
    L = _L()
    seeded = {n for n, sig in L.SIGNATURES.items() if L.ULL in sig} - {"vqa_step_state_set"}
    assert seeded == {k.split("-")[0] for k in SEEDED} and len(seeded) == 16


@pytest.mark.parametrize("case", sorted(SEEDED))
def test_flagged_seed_word_gives_the_plain_seeds_outputs(case):
    SG = _SG()
    run = SEEDED[case]()
    site = 37
    W = SG.seed_step(0, 0x5EED, 4711)
    st = _state(1, W)
    word = SG.seed_word(st.data_ptr() + SG.SEED_STEP_OFFSET, site)
    assert SG.is_indirect(word) and not SG.is_indirect(W | site)
    plain = run(W | site)
    flagged = run(word)
    torch.cuda.synchronize()
    for x, y in zip(plain, flagged):
        assert torch.equal(x, y)
    # rewriting the word changes the mask; the same flagged argument now equals the other step's plain seed
    W2 = SG.seed_step(0, 0x5EED, 4712)
    _L().call("vqa_step_state_set", st.data_ptr(), 2, W2, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0, 0.0, 0)
    flagged2 = run(word)
    plain2 = run(W2 | site)
    torch.cuda.synchronize()
    for x, y in zip(plain2, flagged2):
        assert torch.equal(x, y)
    assert any(not torch.equal(x, y) for x, y in zip(flagged, flagged2))
