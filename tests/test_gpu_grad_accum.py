"""GPU: HipTrainer.accumulate() -- gradient accumulation over micro-batches.

accumulate(...) runs forward, loss and backward into the gradient already in trainer.G and launches nothing else; the step() that
follows k of them applies ONE update with the mean of the k + 1 per-batch mean gradients (tests/_accumref.py is the float64 yardstick,
pinned against a literal torch loop by tests/test_grad_accum_ref_cpu.py).  Small model of tests/test_gpu_param_groups_trainer.py
(embed_dim 32, 10 answers, 64-px images, 10 tokens, B = 4 and B = 2), fp32 and bf16.  Every test that calls accumulate() fails
without it (AttributeError)."""
import json
import math
import multiprocessing as mp
import os
import socket
import time

import pytest
import torch
import torch.distributed as dist

import _accumref as R
import _emaref as E
from _pkg import REPO, pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(vocab_size=100, num_answers=10, embed_dim=32)
CFG = O.full_config(dropout=0.0, answer_dropout=0.0, **SMALL)
CFG_DROP = O.full_config(dropout=0.1, answer_dropout=0.1, **SMALL)
DTYPES = ["fp32", "bf16"]
_CACHE = {}


def _sd():
    if "sd" not in _CACHE:
        _CACHE["sd"] = O.init_state_dict(CFG, 47, jitter=True)
    return _CACHE["sd"]


def _model(dtype="bf16", cfg=CFG):
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(_sd())
    return m.to(DEV).train()


def _batch(seed, B=4):
    key = (seed, B)
    if key not in _CACHE:
        _CACHE[key] = [t.to(DEV) for t in O.synthetic_batch(B, seed=seed, image_size=64, seq_len=10, vocab=100, num_answers=10)]
    return _CACHE[key]


def _trainer(m, **kw):
    return pkg().trainer.HipTrainer(m, **dict(dict(lr=1e-3), **kw))


def _bits(t):
    return t.detach().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _snap(m, tr):
    torch.cuda.synchronize()
    return tuple(t.detach().cpu().clone() for t in (m._flat, tr.m, tr.v))


def _state(m, tr):
    """What a window that never happened leaves alone: the model's state dict (BatchNorm buffers and num_batches_tracked among it),
    both moments and the average."""
    torch.cuda.synchronize()
    out = {"model." + k: v.detach().clone() for k, v in m.state_dict().items()}
    out.update(m=tr.m.clone(), v=tr.v.clone())
    if tr.ema is not None:
        out["ema"] = tr.ema.clone()
    return out


def _assert_state(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert _same(a[k], b[k]), (what, k)


def _buffers_equal(ma, mb):
    for (na, a), (nb, b) in zip(sorted(ma.named_buffers()), sorted(mb.named_buffers())):
        assert na == nb and torch.equal(a, b), na


class _Calls:
    """Names of the launches that go through _lib.call, in order."""

    def __enter__(self):
        L = sub("_lib")
        self.names, self._old = [], L._HOOK[0]
        L._HOOK[0] = lambda name, args: self.names.append(name)
        return self

    def __exit__(self, *a):
        sub("_lib")._HOOK[0] = self._old


def _f32(x):
    """the value a `float` argument of the C ABI carries, as a double"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _check_update(m, tr, snap, n, what=""):
    """The closing step just taken against tests/_accumref.replay fed the window's summed gradient tr.G.  Bounds: those of
    tests/test_gpu_optimizer_ranges.py (|dp| < 2e-6, dm / max|m| < 1e-5, dv / max|v| < 1e-5, norm to 1e-5), which _check_fp64 of
    tests/test_gpu_param_groups_trainer.py uses as well.  Frozen parameters must have kept their bits."""
    torch.cuda.synchronize()
    flat0, m0, v0 = snap
    pe = m._param_entries
    trainable = [p.requires_grad for p in m._param_list()]
    idx = [j for j, t in enumerate(trainable) if t]
    sl = [slice(pe[j].offset, pe[j].offset + pe[j].numel) for j in idx]
    groups = None
    if tr._pg is not None:
        scales, wds = ([_f32(x) for x in vals] for vals in tr._pg.effective(tr.wd))
        groups = [(scales[tr._pg.group_of[j]], wds[tr._pg.group_of[j]]) for j in idx]
    G = tr.G.detach().cpu()
    p, mm, vv, norm = R.replay(flat0, m0, v0, G, n, max_norm=_f32(tr.max_norm), lr=_f32(tr.lr), betas=tuple(_f32(b) for b in tr.betas),
                               eps=_f32(tr.eps), weight_decay=_f32(tr.wd), step=tr.t, slices=sl, groups=groups)
    gsum_norm = math.sqrt(sum(float((G[s].double() ** 2).sum()) for s in sl))
    assert abs(norm - gsum_norm / n) <= 1e-12 * norm
    assert abs(float(tr.grad_norm()) - gsum_norm / n) / (gsum_norm / n) < 1e-5
    flat1, m1, v1 = _snap(m, tr)
    ep = em = ev = mx = vx = 0.0
    for s in sl:
        ep = max(ep, float((flat1[s].double() - p[s]).abs().max()))
        em = max(em, float((m1[s].double() - mm[s]).abs().max()))
        ev = max(ev, float((v1[s].double() - vv[s]).abs().max()))
        mx, vx = max(mx, float(mm[s].abs().max())), max(vx, float(vv[s].abs().max()))
    for j, t in enumerate(trainable):
        if not t:
            s = slice(pe[j].offset, pe[j].offset + pe[j].numel)
            assert _same(flat1[s], flat0[s]) and _same(m1[s], m0[s]) and _same(v1[s], v0[s]), pe[j].name
    print(f"   {what} n = {n}: |dp| {ep:.2e}  dm/max {em / mx:.2e}  dv/max {ev / vx:.2e}  (norm {norm:.3f}, clip {'on' if norm > tr.max_norm else 'off'})")
    assert ep < 2e-6 and em / mx < 1e-5 and ev / vx < 1e-5, what
    assert not torch.equal(flat1, flat0)


# ------------------------------------------------------------------------------- 1. the first micro-batch is the step's gradient
@pytest.mark.parametrize("dtype", DTYPES)
def test_first_micro_batch_leaves_the_gradient_of_a_step(dtype):
    ma, mb = _model(dtype), _model(dtype)
    ta, tb = _trainer(ma), _trainer(mb)
    before, flat0 = _state(ma, ta), ma._flat.detach().clone()
    la, ga = ta.accumulate(*_batch(700))
    lb, gb = tb.step(*_batch(700))
    torch.cuda.synchronize()
    assert _same(ta.G, tb.G) and float(ta.G.abs().max()) > 0
    assert _same(la, lb) and _same(ga, gb)
    after = _state(ma, ta)
    for k in ("m", "v"):
        assert _same(before[k], after[k])
    assert _same(ma._flat, flat0)                                     # (the BatchNorm buffers move: the forward ran)
    assert (ta.calls, ta.t, ta.pending) == (0, 0, 1) and (tb.calls, tb.t, tb.pending) == (1, 1, 0)
    ta.discard_accumulated()
    assert ta.pending == 0


# --------------------------------------------------------------------------------------- 2. the window's gradient is the sum
# N_add of a tensor: the number of separate `+=` it receives in one backward, plus one.  Counted from HipEngine.backward: every
# parameter is written by exactly ONE accumulating launch per backward --
#   conv weights        one weight-gradient launch each (wgrad / wgrad3x3_c64 / _c64_bn / _c128 / the fused stem kernel); conv1, conv2 and
#                       the shortcut conv of a block are three parameters
#   Linear weights      one job of wgrad / wgrad_group each (W_q, W_k, W_v, W_o are four parameters; the odd-width classifier: add_)
#   biases              one fold job each (vqa_bias_act_bwd partial rows -> vqa_fold_group)
#   LayerNorm gamma / beta, the projector's position embedding      one fold job each (vqa_layernorm_bwd -> vqa_fold_group)
#   BatchNorm gamma / beta      one write by vqa_bn_bwd_finalize or vqa_bn_bwd_apply_acc
#   SE fc1 / fc2, the spatial-attention conv      one write by vqa_se_bwd / vqa_spatial_bwd
#   token embedding     one write per row by vqa_embed_bwd (one workgroup owns a block of vocabulary rows)
# -- so N_add = 2, for every tensor but the few whose launch is not ONE fp32 addition onto the destination.  The folds, the BatchNorm,
# SE, spatial and embedding kernels sum first and add once.  The weight gradients' fixed-order reduces do not: wgrad_reduce_kernel and
# wgrad_reduce_group_kernel load dw and add slab after slab onto that running value (nsplit additions), wgrad_reduce2_kernel (32
# slabs or more of a small gradient) and wgrad_c128p_reduce_kernel add their 16 group sums onto it one by one.  Each of those is a
# `+=` with a rounding of its own that falls differently when the chain starts at g1 instead of at 0, so for a weight whose launch
# went through slabs N_add = chained additions + 1.  The chain is read off the closing step's own weight-gradient launches
# (_Chains: the workspace each was handed, wgrad_plan for the grouped Linears), not assumed.  (With N_add = 2 for it, the bf16 stem
# weight -- 16 slabs at B = 2 -- measured 4.47e-7 against 2.93e-7: three roundings' worth, where an overwriting path misses by 2^10
# bounds or more.)
def _chain(nslabs, floats):
    """fp32 additions vqa_slab_reduce / vqa_wgrad's reduce chain onto the destination's running value for `nslabs` slabs of `floats`
    elements (gemm_conv.hip: wgrad_reduce2_kernel from 32 slabs on when the gradient has at most 2^20 elements)."""
    return 16 if (nslabs >= 32 and floats // 4 <= 256 * 1024) else max(1, nslabs)


class _Chains:
    """Hook on _lib.call: {address of dw: chained additions} of every weight-gradient launch while it is installed."""

    def __enter__(self):
        L, K = sub("_lib"), sub("kernels")
        self.at, self._old = {}, L._HOOK[0]

        def hook(name, a):
            if name == "vqa_wgrad":                                    # (dt, loader, dy, x, dw, M, N, Kw, geometry ..., ws, ws floats)
                self.at[a[4]] = _chain(a[-1] // (a[6] * a[7]), a[6] * a[7])
            elif name == "vqa_wgrad_group":                            # (dt, n, dy[], x[], dw[], M[], N[], Kw[], ws, ws floats): wgrad's plan per job
                dtype = torch.bfloat16 if a[0] else torch.float32
                for dw, M, N, Kw in zip(list(a[4]), list(a[5]), list(a[6]), list(a[7])):
                    self.at[dw] = max(1, K.wgrad_plan(dtype, K.LOADER_NHWC, M, N, Kw, *K.linear_geom(M, Kw)[:4], 1, 1)[3])
            elif name in ("vqa_wgrad3x3_c64", "vqa_wgrad3x3_c64_bn"):  # (..., dw, B, H, W, ws, ws floats): at most that many slabs are reduced
                self.at[a[-6]] = min(31, max(1, a[-1] // (64 * 576)))
            elif name == "vqa_wgrad3x3_c128":                          # wgrad_c128p_reduce_kernel: always 16 group sums
                self.at[a[2]] = 16
            elif name.startswith("vqa_stem_wgrad_fused"):              # (img, y, dpool, idx, coef, bc, dw, B, H, W, ws, ws floats[, table])
                self.at[a[6]] = _chain(a[11] // (64 * 147), 64 * 147)
        L._HOOK[0] = hook
        return self

    def __exit__(self, *a):
        sub("_lib")._HOOK[0] = self._old

    def n_add(self, G, entries):
        """{parameter name: N_add}: 2, or chained additions + 1 where a recorded launch wrote the parameter's slice of G."""
        by_offset = {G.data_ptr() + 4 * e.offset: e.name for e in entries}
        out = {e.name: 2 for e in entries}
        for addr, chain in self.at.items():
            if addr in by_offset:                                       # (the odd-width classifier's launch writes a padded copy: add_ is one addition)
                out[by_offset[addr]] = chain + 1
        return out


# tensors whose gradient is round-off only, by name -> the mathematical reason.  (The attention projections of this model carry no
# biases, so the key-projection bias -- whose gradient vanishes because softmax ignores a shift of every score -- does not occur.)
UNCOVERED = {}


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_gradient_is_the_sum_of_the_steps_gradients(dtype):
    mw, m1, m2 = _model(dtype), _model(dtype), _model(dtype)
    tw, t1, t2 = _trainer(mw), _trainer(m1), _trainer(m2)
    b1, b2 = _batch(710), _batch(711, B=2)
    tw.accumulate(*b1)
    with _Chains() as chains:                                          # the launches that add b2's gradient onto g1 (t2 issues the same ones)
        tw.step(*b2)
    t1.step(*b1)
    t2.step(*b2)
    torch.cuda.synchronize()
    n_add = chains.n_add(tw.G, mw._param_entries)
    assert len(chains.at) >= 20 and min(n_add.values()) == 2          # the hook saw the weight gradients; everything else adds once
    Gw, g1, g2 = (t.G.detach().cpu().double() for t in (tw, t1, t2))
    worst, uncovered = 0.0, []
    for e in mw._param_entries:
        s = slice(e.offset, e.offset + e.numel)
        bound = n_add[e.name] * 2.0 ** -24 * float((g1[s].abs() + g2[s].abs()).max())
        err = float((Gw[s] - (g1[s] + g2[s])).abs().max())
        if float(g1[s].abs().max()) < 2.0 ** 10 * bound:
            uncovered.append(e.name)
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
        worst = max(worst, ratio)
        assert err <= bound, (e.name, err, bound, n_add[e.name])
    chained = {k: v for k, v in n_add.items() if v > 2}
    print(f"   {dtype}: worst |G_w - (g1 + g2)| / bound = {worst:.3f} over {len(n_add)} tensors; N_add = 2 but for {chained}")
    assert sorted(uncovered) == sorted(UNCOVERED), uncovered
    _record("sum_check_" + dtype, dict(worst_error_over_bound=round(worst, 4), tensors=len(n_add), n_add_default=2, n_add_chained=chained,
                                       uncovered=sorted(uncovered)))


def _record(key, value):
    """With VQA_RECORD_PROFILES=1 in the environment: keep the measured figure in profiles/grad_accum_bench.json, beside what
    tools/bench_grad_accum.py writes there.  A plain run of the suite prints the figure and leaves the committed file alone."""
    if os.environ.get("VQA_RECORD_PROFILES") != "1":
        return
    path = os.path.join(REPO, "profiles", "grad_accum_bench.json")
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)                                          # (a file that does not parse is an error, not an empty record)
    doc[key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


# ------------------------------------------------------------------------------------------------------------- 3. the update
def _window(tr, n, seed):
    """n - 1 accumulate calls and the closing step; B = 4 then B = 2 (then B = 4)."""
    sizes = [4, 2, 4][:n]
    for i, B in enumerate(sizes[:-1]):
        tr.accumulate(*_batch(seed + i, B))
        assert tr.pending == i + 1
    out = tr.step(*_batch(seed + n - 1, sizes[-1]))
    assert tr.pending == 0
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [2, 3])
def test_closing_step_applies_the_mean_of_the_windows_gradients(dtype, n):
    m = _model(dtype)
    tr = _trainer(m)
    tr.step(*_batch(720))                                            # Adam state that is not zero; the window is update 2
    snap = _snap(m, tr)
    _window(tr, n, 721)
    assert (tr.calls, tr.t) == (2, 2)
    _check_update(m, tr, snap, n, what=dtype)
    tr.check()


def test_closing_step_under_parameter_groups():
    m = _model()
    tr = _trainer(m, weight_decay=0.05, param_groups=sub("finetune").no_weight_decay_groups(m))
    tr.step(*_batch(720))
    snap = _snap(m, tr)
    _window(tr, 2, 721)
    _check_update(m, tr, snap, 2, what="groups")
    tr.check()


def test_closing_step_with_the_text_encoder_frozen():
    m = _model()
    m.text_encoder.requires_grad_(False)
    tr = _trainer(m)
    tr.step(*_batch(720))
    snap = _snap(m, tr)
    _window(tr, 2, 721)
    assert tr._ranges is not None
    _check_update(m, tr, snap, 2, what="frozen text encoder")        # (frozen slices: bits kept, checked inside)
    tr.check()


# ------------------------------------------------------------------------------------------ 4. per-micro-batch forward state
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", [CFG, CFG_DROP], ids=["nodrop", "drop0.1"])
def test_each_micro_batch_runs_the_forward_of_a_plain_step(dtype, cfg):
    mw, mt = _model(dtype, cfg), _model(dtype, cfg)
    tw, tt = _trainer(mw), _trainer(mt, lr=0.0, weight_decay=0.0)       # the twin's plain steps leave the parameters their bits
    batches = [_batch(730), _batch(731, B=2), _batch(732)]
    flat0 = mt._flat.detach().clone()
    for i, b in enumerate(batches):
        lw, gw = (tw.accumulate if i < 2 else tw.step)(*b)
        lw, gw = lw.clone(), gw.clone()
        lt, gt = tt.step(*b)
        torch.cuda.synchronize()
        assert _same(lw, lt) and _same(gw, gt), i
        assert _same(mt._flat, flat0)
    _buffers_equal(mw, mt)
    assert int(mw.state_dict()["image_encoder.stem.1.num_batches_tracked"]) == 3
    assert tw.engine.step_id == tt.engine.step_id and tw.engine.cnn_train_forwards == tt.engine.cnn_train_forwards == 3
    if cfg is CFG_DROP:                                                  # and the masks do differ from call to call
        la = tt.step(*batches[0])[0].clone()
        lc = tt.step(*batches[0])[0]
        assert not _same(la, lc)


# -------------------------------------------------------------------------------------- 5. the mathematics of the large batch
def test_two_halves_give_the_gradient_of_the_whole_batch():
    """fp32, dropout 0, the image encoder frozen and in eval mode: nothing couples the rows of a batch, so the mean of the two halves'
    mean gradients IS the whole batch's mean gradient.  Bound: the per-tensor relative gradient bound of 2e-2 (floor 1e-6) that
    tests/test_gpu_trainer.py::test_hiptrainer_step_matches_reference_golden holds this configuration's fp32 gradients to against the
    oracle -- applied here to the norm of the difference, which is the stricter reading of it."""
    def make():
        m = _model("fp32")
        m.image_encoder.requires_grad_(False)
        m.image_encoder.eval()
        return m, _trainer(m)
    (mw, tw), (mb, tb) = make(), make()
    batch = _batch(740)
    tw.accumulate(*[t[:2].contiguous() for t in batch])
    tw.step(*[t[2:].contiguous() for t in batch])
    tb.step(*batch)
    torch.cuda.synchronize()
    Gw, Gb = tw.G.detach().cpu().double() / 2, tb.G.detach().cpu().double()
    worst = 0.0
    for e, p in zip(mw._param_entries, mw._param_list()):
        if not p.requires_grad:
            continue
        s = slice(e.offset, e.offset + e.numel)
        rel = float((Gw[s] - Gb[s]).norm()) / max(float(Gb[s].norm()), 1e-6)
        worst = max(worst, rel)
        assert rel < 2e-2, (e.name, rel)
    print(f"   halves against the whole batch: worst per-tensor relative difference {worst:.2e}")
    assert abs(float(tw.grad_norm()) - float(tb.grad_norm())) / float(tb.grad_norm()) < 2e-2


# ---------------------------------------------------------------------------------------------------- 6. counters and the average
def test_counters_and_the_average_advance_once_per_window():
    m = _model()
    tr = _trainer(m, ema_decay=0.9)
    torch.cuda.synchronize()
    track = E.Tracker(tr.ema.detach().cpu())
    for w in range(3):
        ema_before = tr.ema.clone()
        tr.accumulate(*_batch(750 + 2 * w))
        torch.cuda.synchronize()
        assert _same(tr.ema, ema_before) and tr.calls == w            # a micro-batch moves neither
        tr.step(*_batch(751 + 2 * w, B=2))
        torch.cuda.synchronize()
        track.step(m._flat.detach().cpu(), 0.9, False, w + 1)
    assert tr.calls == 3 and tr.t == 3 and track.k == 3
    assert tr.engine.step_id == 6                                      # the dropout stream: per micro-batch
    # three updates of decay 0.9 (six would leave 0.9^6 of the start where three leave 0.9^3: far outside the bound)
    track.check(tr.ema.detach().cpu(), "three windows of two")
    tr.check()


# --------------------------------------------------------------------------------- 7. a bad target in a non-closing micro-batch
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_bad_target_in_any_micro_batch_skips_the_windows_update(dtype):
    m = _model(dtype)
    tr = _trainer(m, ema_decay=0.9)
    tr.step(*_batch(760))
    before = _snap(m, tr) + (tr.ema.detach().cpu().clone(),)
    images, ids, mask, answers = _batch(761)
    bad = answers.clone()
    bad[0], bad[3] = 10, -1                                           # two rows outside [0, 10)
    tr.accumulate(images, ids, mask, bad)
    tr.accumulate(*_batch(762, B=2))
    tr.step(*_batch(763))
    after = _snap(m, tr) + (tr.ema.detach().cpu().clone(),)
    assert all(_same(a, b) for a, b in zip(before, after))
    assert tr.calls == 2 and tr.t == 1
    with pytest.raises(IndexError, match=r"^2 target\(s\) out of range .*: 1 step\(s\) were skipped"):
        tr.check()
    tr.check()
    snap = _snap(m, tr)
    _window(tr, 2, 764)                                               # the next window trains
    assert tr.t == 2
    _check_update(m, tr, snap, 2, what="after the skipped window")
    tr.check()


# ---------------------------------------------------------------------------------------------------------------- 8. the guard
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_non_finite_window_never_happened(dtype):
    ma, mb = _model(dtype), _model(dtype)
    ta, tb = _trainer(ma, nonfinite="skip", ema_decay=0.9), _trainer(mb, nonfinite="skip", ema_decay=0.9)
    ta.step(*_batch(770))
    tb.step(*_batch(770))
    before = _state(ma, ta)
    images, ids, mask, answers = _batch(771)
    images = images.clone()
    images[1, 0, 5, 5] = float("nan")                                 # the poison of tests/test_gpu_nonfinite_trainer.py
    with _Calls() as c1:
        lx, _ = ta.accumulate(images, ids, mask, answers)
    assert math.isnan(float(lx))
    with _Calls() as c2:
        ta.step(*_batch(772, B=2))
    assert c1.names.count("vqa_buffers_save") == 1 and "vqa_buffers_restore" not in c1.names
    assert "vqa_buffers_save" not in c2.names and c2.names[-1] == "vqa_buffers_restore"
    _assert_state(before, _state(ma, ta), "the poisoned window")
    assert ta.skipped_nonfinite() == (1, 1) and ta.t == 1 and ta.calls == 2
    rep = ta.nonfinite_report()
    assert rep is not None and rep.parameters and rep.rows.tolist() == []      # the closing micro-batch's rows were finite
    ta.check()
    # a clean window afterwards: as on the twin that never saw the bad one (dropout 0: the stream's position does not matter)
    for t in (ta, tb):
        t.accumulate(*_batch(773))
        t.step(*_batch(774, B=2))
    _assert_state(_state(ma, ta), _state(mb, tb), "the clean window")
    assert _same(ta.G, tb.G) and ta.t == tb.t == 2 and ta.skipped_nonfinite() == (0, 1)


# ------------------------------------------------------------------------------------------------------------ 9. launch lists
def _is_tail(n):
    return n.startswith(("vqa_sumsq", "vqa_adamw")) or n == "vqa_buffers_restore"


@pytest.mark.parametrize("guard", [None, "skip"])
def test_launch_lists(guard):
    m = _model()
    tr = _trainer(m, nonfinite=guard)
    b = _batch(780)
    for _ in range(2):                                                # the packed backward operands and the operand copy settle
        tr.step(*b)
    with _Calls() as plain:
        tr.step(*b)
    with _Calls() as acc:
        tr.accumulate(*b)
    with _Calls() as closing:
        tr.step(*b)
    with _Calls() as again:
        tr.step(*b)
    torch.cuda.synchronize()
    assert sum(map(_is_tail, plain.names)) == (2 if guard is None else 3)
    assert acc.names == [n for n in plain.names if not _is_tail(n)]
    # the closing step: the plain step's launches in order (under the guard the window's buffers were saved by its first call)
    assert closing.names == [n for n in plain.names if guard is None or n != "vqa_buffers_save"]
    assert again.names == plain.names                                 # and no window open: the step as it has always been
    assert tr.pending == 0 and tr.calls == 5


# -------------------------------------------------------------------------------------------------------------- 10. the reducer
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _reducer_worker(port, q):
    """A process of its own, so that no other test of this session sees a process group: one rank over gloo, as
    tests/test_gpu_nonfinite_trainer.py makes it, HipTrainer(force_reducer=True) against a trainer without the reducer."""
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=0, world_size=1)
        torch.cuda.set_device(0)
        mr, mp_ = _model(), _model()
        tr, tp = _trainer(mr, force_reducer=True), _trainer(mp_)
        assert tr.reducer.active and not tp.reducer.active
        grown = []
        for w in range(2):
            for t in (tr, tp):
                b0 = t.reducer.bytes_reduced
                t.accumulate(*_batch(790 + 2 * w))
                assert t.reducer.bytes_reduced == b0                  # nothing is communicated by a micro-batch
                t.step(*_batch(791 + 2 * w, B=2))
            torch.cuda.synchronize()
            grown.append(tr.reducer.bytes_reduced)
            assert _same(mr._flat, mp_._flat) and _same(tr.m, tp.m) and _same(tr.v, tp.v) and _same(tr.G, tp.G), w
            if w == 0:
                tr.step(*_batch(795)); tp.step(*_batch(795))
                plain = tr.reducer.bytes_reduced - grown[0]
        assert plain > 0 and grown[0] == plain and grown[1] - grown[0] - plain == plain and tp.reducer.bytes_reduced == 0
        tr.check()
        dist.destroy_process_group()
        q.put(("ok", ""))
    except BaseException as e:                                        # the parent reports it
        q.put(("failed", f"{type(e).__name__}: {e}"))
        raise


def test_a_window_with_the_forced_one_rank_reducer():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_reducer_worker, args=(_free_port(), q))
    p.start()
    try:
        deadline = time.monotonic() + 240
        while q.empty() and p.is_alive() and time.monotonic() < deadline:      # (returns as soon as the child has answered or died)
            p.join(timeout=0.05)
        status, what = q.get(timeout=5) if (not q.empty() or not p.is_alive()) else ("failed", "no answer within 240 s")
    finally:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()
    assert status == "ok", what
    assert p.exitcode == 0


# ------------------------------------------------------------------------------------------------- 11. refusals and hygiene
def test_refusals_while_a_window_is_open():
    m, twin = _model(), _model()
    tr, tt = _trainer(m), _trainer(twin)
    tr.step(*_batch(800)); tt.step(*_batch(800))
    sd = tr.state_dict()
    tr.accumulate(*_batch(801)); tt.accumulate(*_batch(801))
    before, G0 = _state(m, tr), tr.G.clone()
    eng = tr.engine
    counters = (tr.calls, eng.step_id, eng.cnn_train_forwards, m._feat_epoch, tr.pending)
    with _Calls() as c:
        with pytest.raises(RuntimeError, match="window is open"):
            tr.step_graphed(*_batch(802))
        with pytest.raises(RuntimeError, match="window is open"):
            tr.state_dict()
        with pytest.raises(RuntimeError, match="window is open"):
            tr.load_state_dict(sd)
    assert c.names == [] and counters == (tr.calls, eng.step_id, eng.cnn_train_forwards, m._feat_epoch, tr.pending) and tr.pending == 1
    _assert_state(before, _state(m, tr))
    assert _same(tr.G, G0)
    # a changed trainable set: refused before any launch, nothing counted
    m.text_encoder.requires_grad_(False)
    with _Calls() as c:
        with pytest.raises(RuntimeError, match="trainable set changed"):
            tr.accumulate(*_batch(802))
        with pytest.raises(RuntimeError, match="trainable set changed"):
            tr.step(*_batch(802))
    assert c.names == [] and counters == (tr.calls, eng.step_id, eng.cnn_train_forwards, m._feat_epoch, tr.pending)
    m.text_encoder.requires_grad_(True)
    # and the window can still be closed: as on the twin that was never refused anything
    tr.step(*_batch(802, B=2)); tt.step(*_batch(802, B=2))
    _assert_state(_state(m, tr), _state(twin, tt))
    assert _same(tr.G, tt.G) and tr.pending == 0 and tr.calls == 2
    tr.state_dict()                                                    # at a window boundary: as ever


def test_a_discarded_window_leaves_a_plain_step():
    m, twin = _model(), _model()
    tr, tt = _trainer(m), _trainer(twin)
    images, ids, mask, answers = _batch(810)
    bad = answers.clone()
    bad[1] = 10
    tr.accumulate(images, ids, mask, bad)                             # its bad-target word goes with it
    tr.accumulate(*_batch(811, B=2))
    tr.discard_accumulated()
    assert tr.pending == 0 and tr.calls == 0
    la, ga = tr.step(*_batch(812))
    lb, gb = tt.step(*_batch(812))
    torch.cuda.synchronize()
    assert _same(la, lb) and _same(ga, gb) and _same(tr.G, tt.G)
    assert _same(m._flat, twin._flat) and _same(tr.m, tt.m) and _same(tr.v, tt.v) and tr.t == tt.t == 1
    tr.check()
    tr.discard_accumulated()                                          # no window open: nothing


def test_inference_between_two_calls_leaves_the_window_alone():
    m, twin = _model(), _model()
    tr, tt = _trainer(m, ema_decay=0.9), _trainer(twin, ema_decay=0.9)
    m.graph_inference = False                                         # the eager eval forward: this file captures and replays nothing
    b1, b2 = _batch(820), _batch(821, B=2)
    tr.accumulate(*b1); tt.accumulate(*b1)
    G0 = tr.G.clone()
    m.eval()
    ex = m.explain(b1[0], b1[1], b1[2])
    with torch.no_grad():
        logits, _ = m(b1[0], b1[1], b1[2])
    with tr.ema_weights():
        with torch.no_grad():
            m(b1[0], b1[1], b1[2])
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.accumulate(*b2)
    m.train()
    torch.cuda.synchronize()
    assert ex.logits.shape == logits.shape == (4, 10) and _same(tr.G, G0) and tr.pending == 1
    tr.step(*b2); tt.step(*b2)
    torch.cuda.synchronize()
    assert _same(tr.G, tt.G) and _same(m._flat, twin._flat) and _same(tr.m, tt.m) and _same(tr.v, tt.v) and _same(tr.ema, tt.ema)
