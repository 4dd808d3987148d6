"""GPU: every attention entry of csrc/attention.hip against the fp64 reference of _attnref.py, element by element, each output
inside the bound derived there from the rounding sites of its form (test_attn_ref_cpu.py proves the bounds have teeth).  The case
table reaches every (HD, NKT) instantiation of the MFMA form and the VALU form past the MFMA limits up to its LDS limits, the packed,
cross and wide layouts, logits that need the max subtraction, one-hot rows, sparse / odd-valued / full masks, dropout, an upstream
gradient on the softmax, and the indexed entries over vqa_index_csr's output.  Every output buffer starts as a sentinel.

The backward is judged from the probs buffer the forward kernel wrote, taken as an exact input, so its bound has no forward error."""
import pytest
import torch

import _attnref as A
from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
EARG = 1000
IDS = [c.id for c in A.CASES]


def _sent(shape, dtype):
    return torch.full(shape, A.SENT, dtype=dtype, device=DEV)


def _untouched(t):
    return bool((t == A.SENT).all())


def launch(case, I):
    """The case's forward launch and, where it has one, the backward launch that reads its probs (indexed: vqa_index_csr in front).
    -> (status of each launch, buffers on the device).  A refused launch returns before any kernel starts."""
    L = sub("_lib")
    mf, dt, d, B, U, H, Lq, Lk, hd = case.fam == "mfma", I.dtype, I.d, I.B, I.U, I.H, I.Lq, I.Lk, I.hd
    raw = lambda name, *a: int(getattr(L.lib(), name)(*a, L.stream()))
    dev = lambda t: None if t is None else t.to(DEV)
    qb = dev(I.q)
    kb = qb if I.k is I.q else dev(I.k)         # packed: one buffer
    q, k, v = qb[:, I.qc:], kb[:, I.kc:], kb[:, I.vc:]
    km, dctx, dprobs = dev(I.kmask), dev(I.dctx), dev(I.dprobs)
    kvi = I.kv_index.to(torch.int32).to(DEV)
    out = {"probs": _sent((B, H, Lq, Lk), A.F32), "ctx": _sent((B * Lq, I.ldc), dt)}
    lead = () if mf else (L.dt(dt),)
    ix = (kvi.data_ptr(), U) if case.indexed else ()
    name = "vqa_attention_fwd_mfma" if mf else "vqa_attention_fwd"
    name += {"plain": "", "dp": "", "idx_infer": "_idx", "idx_train": "_idx_train"}[case.entry]
    ps = () if case.entry == "idx_infer" else (I.p, I.seed)
    st = {"fwd": raw(name, *lead, q.data_ptr(), k.data_ptr(), v.data_ptr(), I.ldq, I.ldk, I.ldv, *ix, L.ptr(km), out["probs"].data_ptr(),
                     out["ctx"].data_ptr(), I.ldc, B, H, Lq, Lk, hd, *ps)}
    if case.has_bwd and st["fwd"] == 0:
        if case.wide:
            out.update(dq=_sent((B * Lq, I.ldc), dt), dk=_sent((U * Lk, I.ldc), dt), dv=_sent((U * Lk, I.ldc), dt))
            g, ldg = (out["dq"], out["dk"], out["dv"]), (I.ldc,) * 3
        elif case.packed:
            out["dqkv"] = _sent((B * Lq, 3 * d), dt)
            g, ldg = (out["dqkv"], out["dqkv"][:, d:], out["dqkv"][:, 2 * d:]), (3 * d,) * 3
        else:
            out.update(dq=_sent((B * Lq, d), dt), dkv=_sent((U * Lk, 2 * d), dt))
            g, ldg = (out["dq"], out["dkv"], out["dkv"][:, d:]), (d, 2 * d, 2 * d)
        mid = ()
        if case.indexed:
            offsets, order = torch.full((U + 1,), -7, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
            st["csr"] = raw("vqa_index_csr", kvi.data_ptr(), B, U, offsets.data_ptr(), order.data_ptr())
            mid = (offsets.data_ptr(), order.data_ptr(), U)
        elif case.entry == "dp":
            mid = (dprobs.data_ptr(),)
        name = ("vqa_attention_bwd_mfma" if mf else "vqa_attention_bwd") + {"plain": "", "dp": "_dp", "idx_train": "_idx"}[case.entry]
        st["bwd"] = raw(name, *lead, dctx.data_ptr(), I.ldc, q.data_ptr(), k.data_ptr(), v.data_ptr(), I.ldq, I.ldk, I.ldv,
                        out["probs"].data_ptr(), *mid, *(t.data_ptr() for t in g), *ldg, B, H, Lq, Lk, hd, I.p, I.seed)
        out["g"] = g
    torch.cuda.synchronize()
    return st, out


def outputs(case, I, out):
    """the five outputs on the CPU in the reference's layout; the gap columns of the wide buffers must still hold the sentinel"""
    d = I.d
    res = {"probs": out["probs"].cpu(), "ctx": out["ctx"][:, :d].cpu()}
    gaps = [out["ctx"][:, d:]]
    if "g" in out:
        res.update({n: t[:, :d].cpu() for n, t in zip(("dq", "dk", "dv"), out["g"])})
        if case.wide:
            gaps += [t[:, d:] for t in out["g"]]
    for t in gaps:
        assert _untouched(t), "a write into the gap a row stride leaves"
    return res


def judge(case, I, got, fam=None):
    """worst err / bound per output, after the exact expectations"""
    fam = fam or case.fam
    R = A.reference(I)
    if I.kmask is not None:                     # masked keys: probability exactly 0 (NaN in a fully masked batch)
        masked = (I.kmask[I.kv_index] == 0).view(I.B, 1, 1, I.Lk).expand_as(R.P)
        pm = got["probs"][masked]
        assert bool(((pm == 0) | R.P[masked].isnan()).all()), "a masked key has a probability"
    bf = A.forward_bounds(I, R, fam)
    r = {n: A.worst(got[n], getattr(R, n), bf[n]) for n in ("probs", "ctx")}
    if case.has_bwd:
        Rb = A.reference(I, probs=got["probs"])
        bb = A.backward_bounds(I, Rb, fam)
        r.update({n: A.worst(got[n], getattr(Rb, n), bb[n]) for n in ("dq", "dk", "dv")})
        for u in sorted(set(range(I.U)) - set(I.kv_index.tolist())):          # an image without questions: exact zeros
            rows = slice(u * I.Lk, (u + 1) * I.Lk)
            assert float(got["dk"][rows].float().abs().max()) == 0.0 and float(got["dv"][rows].float().abs().max()) == 0.0
    if case.mask == "row":                      # the fully masked batch / image is NaN (worst() checks where), every other is finite
        assert bool(got["probs"][I.kv_index == I.U - 1].isnan().all()) and not bool(got["probs"][I.kv_index != I.U - 1].isnan().any())
    return r, R


@pytest.mark.parametrize("case", A.CASES, ids=IDS)
def test_every_element_inside_its_bound(case):
    """err <= bound for every element of probs, ctx, dq, dk, dv.
    Measured on MI355X, worst err / bound over the cases of a family (probs, ctx, dq, dk, dv):
      valu/fp32  0.086  0.066  0.063  0.058  0.384
      valu/bf16  0.042  0.990  0.987  0.992  0.996
      mfma/bf16  0.035  0.847  0.919  0.971  0.938
    and the need behind c at the valu/fp32 randn cases (see _attnref.C_EXP): -141.6 u (the CPU stand-in: -153.7 u).
    The bf16 outputs sit close to 1 by nature, not by fit: the store alone costs up to 2^-8 |out| (half a bf16 ulp just above a power
    of two), that term is most of their bound, and among thousands of elements some land there.  The kernels use no float atomics,
    so these figures are the same on every run."""
    I = A.make_inputs(case)
    st, out = launch(case, I)
    assert all(s == 0 for s in st.values()), st
    got = outputs(case, I, out)
    r, R = judge(case, I, got)
    need = ""
    if case == A.Case("valu", "fp32", case.Lq, case.Lk, case.hd, backward=case.backward):
        need = f" c_need={A.c_need(I, R, 'valu', got['probs']):.2f}"
    print(f"\nRATIO {case.id} " + " ".join(f"{n}={x:.4f}" for n, x in r.items()) + need)
    assert all(x <= 1.0 for x in r.values()), r


BOTH = [dict(Lq=20, Lk=49, hd=64, mask="sparse", p=0.1), dict(Lq=32, Lk=160, hd=64, entry="dp", p=0.1),
        dict(Lq=20, Lk=49, hd=64, entry="idx_train", p=0.1, wide=True)]


@pytest.mark.parametrize("kw", BOTH, ids=[A.find(**kw).id[10:] for kw in BOTH])
def test_both_forms_inside_their_own_bound_of_one_reference(kw):
    """where both forms accept a case they read the same bf16 operands and are judged against the same reference, each with the
    bound of its own rounding sites; the forward outputs of the two forms then differ by no more than the two bounds together"""
    res = {}
    for fam in ("valu", "mfma"):
        case = A.find(fam=fam, dname="bf16", **kw)
        I = A.make_inputs(case)
        st, out = launch(case, I)
        assert all(s == 0 for s in st.values()), st
        got = outputs(case, I, out)
        r, R = judge(case, I, got)
        assert all(x <= 1.0 for x in r.values()), (fam, r)
        res[fam] = (I, got, A.forward_bounds(I, R, fam))
    (Iv, gv, bv), (Im, gm, bm) = res["valu"], res["mfma"]
    assert torch.equal(Iv.q, Im.q) and torch.equal(Iv.k, Im.k) and torch.equal(Iv.dctx, Im.dctx)
    for n in ("probs", "ctx"):
        assert A.worst(gv[n], gm[n].double(), bv[n] + bm[n]) <= 1.0, n


REFUSALS = [
    # case, the launch that must be refused (the ones before it must succeed)
    (A.Case("valu", "fp32", 20, A.LK_FWD_MAX + 1, 64), "fwd"),
    (A.Case("valu", "bf16", 20, A.LK_FWD_MAX + 1, 64, entry="idx_infer"), "fwd"),
    (A.Case("valu", "bf16", 20, A.LK_FWD_MAX + 1, 64, entry="idx_train"), "fwd"),
    (A.Case("valu", "fp32", 20, A.LK_FWD_MAX, 64), "bwd"),               # the forward's top: its backward does not fit
    (A.Case("valu", "bf16", 20, A.LK_BWD_MAX + 1, 64), "bwd"),
    (A.Case("valu", "fp32", 20, A.LK_BWD_MAX + 1, 64, entry="dp"), "bwd"),
    (A.Case("valu", "fp32", 20, A.LK_BWD_MAX + 1, 64, entry="idx_train"), "bwd"),
    (A.Case("valu", "bf16", 5, 161, 64, entry="idx_train"), "bwd"),      # Lk * hd = 10304 > 10240 accumulators, LDS would fit
    (A.Case("mfma", "bf16", 33, 20, 32), "fwd"),
    (A.Case("mfma", "bf16", 20, 161, 32), "fwd"),
    (A.Case("mfma", "bf16", 20, 20, 48), "fwd"),
]


@pytest.mark.parametrize("case,which", REFUSALS, ids=[f"{c.id}-{w}" for c, w in REFUSALS])
def test_refusals_leave_the_outputs_untouched(case, which):
    """One past each limit the entry returns status 1000 before any launch and every output still holds the sentinel.  Between Lk 226
    and 264 at (Lq 20, hd 64) the VALU forward accepts a shape whose backward refuses: both limits come from the host mirror of
    AttnValuLds::floats() * 4 <= 160 KiB, not from literals."""
    assert A.valu_fits(False, 20, A.LK_FWD_MAX, 64) and not A.valu_fits(False, 20, A.LK_FWD_MAX + 1, 64)
    assert A.valu_fits(True, 20, A.LK_BWD_MAX, 64) and not A.valu_fits(True, 20, A.LK_BWD_MAX + 1, 64) and A.LK_BWD_MAX < A.LK_FWD_MAX
    if which == "bwd" and case.fam == "valu":
        assert A.valu_fits(False, case.Lq, case.Lk, case.hd)
        assert not A.valu_fits(True, case.Lq, case.Lk, case.hd) or case.Lk * case.hd > A.IDX_BWD_NKD
    I = A.make_inputs(case)
    st, out = launch(case, I)
    assert st[which] == EARG and all(s == 0 for n, s in st.items() if n != which), st
    if which == "fwd":
        assert _untouched(out["probs"]) and _untouched(out["ctx"]) and "g" not in out
    else:
        assert not bool((out["probs"] == A.SENT).any())
        assert all(_untouched(out[n]) for n in out if n.startswith("d"))
