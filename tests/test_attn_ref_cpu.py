"""CPU: the fp64 attention reference, its bounds and its case table (_attnref.py) checked without a GPU: the closed-form backward
against autograd, the mask semantics, fp32 / bf16 stand-ins that must stay inside every bound, mutants that must not, and the
coverage of the case table.  test_gpu_attention_fp64.py then judges the kernels with the same reference and bounds."""
import math

import pytest
import torch

import _attnref as A

F64 = torch.float64
BWD_CASES = [c for c in A.CASES if c.fam == "valu" and c.dname == "fp32" and c.has_bwd]
IDS = lambda cs: [c.id for c in cs]


def _autograd(I):
    """the forward formula in torch fp64 with autograd; loss = sum(ctx dctx) + sum(P dprobs)"""
    B, U, H, Lq, Lk, hd = I.B, I.U, I.H, I.Lq, I.Lk, I.hd
    q = A.heads(I.q, I.ldq, I.qc, B, Lq, H, hd).double().clone().requires_grad_()
    k = A.heads(I.k, I.ldk, I.kc, U, Lk, H, hd).double().clone().requires_grad_()
    v = A.heads(I.v, I.ldv, I.vc, U, Lk, H, hd).double().clone().requires_grad_()
    S = q @ k[I.kv_index].transpose(-1, -2) / math.sqrt(hd)
    if I.kmask is not None:
        S = S.masked_fill((I.kmask[I.kv_index] == 0).view(B, 1, 1, Lk), -math.inf)
    P = torch.softmax(S, -1)
    ctx = (P * I.keep.double() / (1 - I.p)) @ v[I.kv_index]
    loss = (ctx * A.heads(I.dctx, I.ldc, 0, B, Lq, H, hd).double()).sum()
    if I.dprobs is not None:
        loss = loss + (P * I.dprobs.double()).sum()
    dq, dk, dv = torch.autograd.grad(loss, (q, k, v))
    return P.detach(), A.unheads(ctx.detach()), A.unheads(dq), A.unheads(dk), A.unheads(dv)


@pytest.mark.parametrize("case", BWD_CASES, ids=IDS(BWD_CASES))
def test_closed_form_backward_equals_autograd(case):
    """every case shape, mask, dropout rate and entry: the closed form equals torch's fp64 autograd of the forward formula to 1e-12
    (of the largest gradient); the indexed sums equal autograd through a gather; NaN where autograd is NaN."""
    I = A.make_inputs(case)
    R = A.reference(I)
    nanq = torch.tensor([case.mask == "row" and int(u) == I.U - 1 for u in I.kv_index])       # questions on the fully masked image
    nanu = torch.tensor([case.mask == "row" and u == I.U - 1 for u in range(I.U)])
    for name, got, want in zip(("probs", "ctx", "dq", "dk", "dv"), (R.probs, R.ctx, R.dq, R.dk, R.dv), _autograd(I)):
        # (autograd itself gives dq = dk = 0 there: masked_fill's backward zeroes what the NaN softmax sends back.  The kernels and
        # the closed form propagate the NaN probabilities, which is what the reference states.)
        n, L = (nanu, I.Lk) if name in ("dk", "dv") else (nanq, I.Lq)
        rows = n.view(-1, 1, 1, 1).expand_as(got) if name == "probs" else n.repeat_interleave(L).view(-1, 1).expand_as(got)
        assert torch.equal(got.isnan(), rows), name
        fin = ~rows
        scale = max(1.0, float(want[fin].abs().max()))
        assert float((got[fin] - want[fin]).abs().max()) <= 1e-12 * scale, name
    if case.indexed:
        never = sorted(set(range(I.U)) - set(I.kv_index.tolist()))
        assert never == [1]
        rows = slice(never[0] * I.Lk, (never[0] + 1) * I.Lk)
        assert float(R.dk[rows].abs().max()) == 0.0 and float(R.dv[rows].abs().max()) == 0.0


def test_mask_semantics():
    """The reference masks like masked_fill(mask == 0, -inf): -0.0 masks; 0.25, -1 and 2 keep; masked keys get probability exactly 0;
    a fully masked row is NaN.  The modelled cross-attention fills with -1e9 instead: that gives a UNIFORM row where ours is NaN, and
    identical zeros for a partly masked row (exp(-1e9 - m) underflows to 0 in any precision).  The engine passes no key mask to
    cross-attention, and the text encoder never masks every key of a row, so the difference is unreachable from the model."""
    I = A.make_inputs(A.find(Lk=49, hd=64, mask="odd"))
    R = A.reference(I)
    km = I.kmask
    assert bool(((km == 0) & torch.signbit(km)).any()) and {0.25, -1.0, 2.0} <= set(km.flatten().tolist())
    masked = (km == 0).view(I.B, 1, 1, I.Lk).expand_as(R.P)
    assert bool((R.P[masked] == 0).all()) and bool((R.P[~masked] > 0).all())
    S = (R.q @ R.k.transpose(-1, -2)) / math.sqrt(I.hd)
    assert float((R.P - torch.softmax(S.masked_fill(masked, -math.inf), -1)).abs().max()) < 1e-15
    assert float((R.P - torch.softmax(S.masked_fill(masked, -1e9), -1)).abs().max()) < 1e-15   # partly masked rows: the same zeros
    I = A.make_inputs(A.find(Lk=49, hd=64, mask="row", p=0.5))
    R = A.reference(I)
    assert bool(R.P[-1].isnan().all()) and not bool(R.P[:-1].isnan().any())
    assert bool(R.ctx[-I.Lq:].isnan().all()) and bool(R.dq[-I.Lq:].isnan().all()) and bool(R.dk[-I.Lk:].isnan().all())
    assert bool(R.dv[-I.Lk:].isnan().all()) and not bool(R.dk[:-I.Lk].isnan().any())
    S = (R.q @ R.k.transpose(-1, -2)) / math.sqrt(I.hd)
    uni = torch.softmax(S.masked_fill((I.kmask == 0).view(I.B, 1, 1, I.Lk), -1e9), -1)[-1]
    assert float((uni - 1 / I.Lk).abs().max()) < 1e-6                                # the modelled fill: uniform, not NaN


def _ratios(I, fam, got, fwd_ref=None):
    """worst err / bound of each output of `got` (a namespace with probs, ctx[, dq, dk, dv]); the backward against the reference
    that reads got's probs unless fwd_ref's own are to be used"""
    R = A.reference(I)
    bf = A.forward_bounds(I, R, fam)
    out = {"probs": A.worst(got.probs, R.probs, bf["probs"]), "ctx": A.worst(got.ctx, R.ctx, bf["ctx"])}
    if I.case.has_bwd:
        Rb = A.reference(I, probs=fwd_ref)
        bb = A.backward_bounds(I, Rb, fam)
        out.update({n: A.worst(getattr(got, n), getattr(Rb, n), bb[n]) for n in ("dq", "dk", "dv")})
    return out


@pytest.mark.parametrize("case", A.CASES, ids=IDS(A.CASES))
def test_standins_stay_inside_every_bound(case):
    """fp32 evaluation of the formula (for the MFMA family with its bf16 roundings at the sites the bounds name), outputs rounded to
    the compute dtype: err / bound <= 1 for every element of every output, on every case.  The bounds are not too tight."""
    I = A.make_inputs(case)
    got = A.standin(I, case.fam)
    r = _ratios(I, case.fam, got, fwd_ref=got.probs if case.has_bwd else None)
    assert all(x <= 1.0 for x in r.values()), r


def test_c_need_of_the_cpu_standin():
    """what the fp32 stand-in needs of c at the randn / no mask / p = 0 cases: at most half of C_EXP (its docstring records it)"""
    need = -math.inf
    for case in A.CASES:
        if (case.fam, case.dname) == ("valu", "fp32") and case == A.Case("valu", "fp32", case.Lq, case.Lk, case.hd, backward=case.backward):
            I = A.make_inputs(case)
            need = max(need, A.c_need(I, A.reference(I), "valu", A.evaluate(I, prec=torch.float32).probs))
    print(f"c need of the CPU fp32 stand-in: {need:.2f}")
    assert 2 * need <= A.C_EXP


MF = dict(fam="mfma", dname="bf16")
MUTANT_CASES = [
    # mutant, the case that must catch it (MFMA family: the widest bounds), the output that must leave its bound
    ("no_max", dict(MF, Lk=49, hd=64, kind="offset"), "probs"),
    ("no_max", dict(MF, Lq=32, Lk=160, hd=64, kind="offset"), "probs"),
    ("scale", dict(MF), "probs"),
    ("rowsum_tail", dict(MF, Lk=49, hd=64), "probs"),
    ("pv_tail", dict(MF, kind="peaked"), "ctx"),
    ("mask_gt", dict(MF, Lk=49, hd=64, mask="odd"), "probs"),
    ("mask_batch", dict(MF, Lk=49, hd=64, entry="idx_infer", mask="sparse"), "probs"),
    ("drop_swap", dict(MF, Lk=49, hd=64, p=0.1, wide=True), "ctx"),
    ("drop_swap", dict(MF, Lk=49, hd=64, p=0.1, wide=True), "dv"),
    ("dv_scale", dict(MF, p=0.5), "dv"),
    ("t_nodp", dict(MF, Lk=49, hd=64, entry="dp", kind="peaked"), "dq"),
    ("t_nodp", dict(MF, Lk=49, hd=64, entry="dp", kind="peaked"), "dk"),
    ("v_head", dict(MF), "ctx"),
    ("v_head", dict(MF), "dq"),
    ("ld_as_d", dict(MF), "probs"),
    ("dk_pad", dict(MF, Lk=49, hd=64), "dk"),
    ("dk_image", dict(MF, Lk=49, hd=64, entry="idx_train", p=0.1, wide=True), "dk"),
]


@pytest.mark.parametrize("mutant,kw,output", MUTANT_CASES, ids=[f"{m}-{o}-{i}" for i, (m, _, o) in enumerate(MUTANT_CASES)])
def test_mutants_leave_their_bound(mutant, kw, output):
    """each defect, evaluated in fp64 (no max subtraction: in fp32, where it overflows), exceeds the bound on its named case"""
    case = A.find(**kw)
    I = A.make_inputs(case)
    if mutant == "pv_tail":
        assert bool((A.reference(I).P[..., -1] > 0.9).any()), "no row of the case has its mass on the last key"
    got = A.evaluate(I, prec=torch.float32 if mutant == "no_max" else F64, mutant=mutant)
    r = _ratios(I, case.fam, got)
    assert r[output] > 1.0, r


def test_every_mutant_is_listed():
    assert {m for m, _, _ in MUTANT_CASES} == set(A.MUTANTS)


@pytest.mark.parametrize("output", ["probs", "ctx", "dq", "dk", "dv"])
def test_one_element_off_by_twice_its_bound(output):
    """worst() looks at every element: the reference with ONE element moved by twice its bound fails, by 1.5 bounds passes"""
    case = A.find(**dict(MF, Lk=49, hd=64, entry="idx_train", p=0.1, wide=True))
    I = A.make_inputs(case)
    R = A.reference(I)
    b = dict(A.forward_bounds(I, R, case.fam), **A.backward_bounds(I, R, case.fam))[output]
    ref = getattr(R, output)
    assert A.worst(ref, ref, b) == 0.0
    live = (b.flatten() > A.FLT_MIN * 4).nonzero().flatten()
    at = int(live[len(live) // 2])
    for k, inside in ((0.75, True), (2.0, False)):
        got = ref.clone()
        got.view(-1)[at] += k * b.flatten()[at]
        assert (A.worst(got, ref, b) <= 1.0) == inside
    got = ref.clone()
    got.view(-1)[at] = math.nan
    assert A.worst(got, ref, b) == math.inf


def test_case_table_covers_the_code_paths():
    ids = [c.id for c in A.CASES]
    assert len(set(ids)) == len(ids)
    entries = ("plain", "dp", "idx_infer", "idx_train")
    mf = [c for c in A.CASES if c.fam == "mfma"]
    assert all(A.mfma_fits(c.Lq, c.Lk, c.hd) and c.dname == "bf16" for c in mf)
    for e in entries:                                       # every (HD, NKT) instantiation of the MFMA form, in every entry
        assert {(c.hd, A.mfma_nkt(c.Lk)) for c in mf if c.entry == e} == {(32, 2), (64, 2), (32, 5), (64, 5)}, e
    for fam, dn in A.FAMILIES:
        cs = [c for c in A.CASES if (c.fam, c.dname) == (fam, dn)]
        grid = {(c.Lq, c.Lk, c.hd) for c in cs if c == A.Case(fam, dn, c.Lq, c.Lk, c.hd, backward=c.backward)}
        assert grid >= {(Lq, Lk, hd) for Lq, Lk in A.SHAPES for hd in (32, 64)}
        assert {c.kind for c in cs} == {"randn", "peaked", "offset"}
        assert {c.mask for c in cs} == {"none", "prefix", "sparse", "odd", "row"}
        assert {c.p for c in cs} == {0.0, 0.1, 0.5}
        assert {c.entry for c in cs} == set(entries)
        assert any(c.wide for c in cs) and any(c.packed for c in cs) and any(not c.packed and not c.wide for c in cs)
        assert any(c.Lk > 64 for c in cs) and any(c.Lq > 4 for c in cs)        # a second lane trip and a second wave trip (VALU)
        assert {1, 31, 32, 33, 64, 65, 160} <= {c.Lk for c in cs} and {1, 32} <= {c.Lq for c in cs}
        for c in cs:                                        # no case passes an argument an entry refuses or would act on wrongly
            assert A.valu_fits(False, c.Lq, c.Lk, c.hd) and (not c.has_bwd or A.valu_fits(True, c.Lq, c.Lk, c.hd))
            assert not (c.entry == "idx_train" and c.Lk * c.hd > A.IDX_BWD_NKD)
            assert c.mask in ("none", "prefix") or c.Lk >= 20
    valu = {(c.Lq, c.Lk, c.hd) for c in A.CASES if c.fam == "valu"}
    assert {(33, 161, 48), (20, 196, 64), (20, A.LK_FWD_MAX, 64), (20, A.LK_BWD_MAX, 64)} <= valu       # past each MFMA limit
    assert not any(A.mfma_fits(*s) for s in ((33, 161, 48), (33, 20, 32), (20, 161, 32), (20, 20, 48)))


def test_lds_limits_of_the_valu_form():
    """the host mirror of AttnValuLds::floats() * 4 <= 160 KiB at (Lq 20, hd 64): the forward takes Lk up to 264, the backward up to
    225: between them a forward is accepted whose backward is refused"""
    assert (A.LK_FWD_MAX, A.LK_BWD_MAX) == (264, 225)
    assert A.valu_fits(False, 20, 264, 64) and not A.valu_fits(False, 20, 265, 64)
    assert A.valu_fits(True, 20, 225, 64) and not A.valu_fits(True, 20, 226, 64)
    c = [c for c in A.CASES if c.Lk == A.LK_FWD_MAX]
    assert c and all(not x.has_bwd for x in c)
