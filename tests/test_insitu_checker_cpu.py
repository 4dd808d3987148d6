"""CPU: negative controls of the in-situ checker (tests/_insitu.py).  A bf16-stored conv output of a batch large enough that the
global relative norm alone is blind to a one-channel error must pass as stored, and fail with the last image's rows zeroed or
with one channel scaled by 1 + 2^-5.  The grouped references: the indexed attention backward is the expanded one summed per image,
and the checks reject a dK missing one question, a CSR order with two entries swapped and a non-zero row of an image without
questions."""
import pytest
import torch
import torch.nn.functional as F

from _insitu import (T_ATTN, T_ATTN_SLICE, Checker, attn_core_bwd, attn_core_fwd, check_csr, check_zero_rows, empty_images, nchw, rnd,
                     slice_errors)


def _stored_conv(B=96, C=128, H=12, W=12, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(B, C, H, W, generator=g))
    w = rnd(torch.randn(C, C, 3, 3, generator=g) / 24)
    ref = F.conv2d(x, w, padding=1)
    # what a correct bf16 kernel hands out: the fp32 result rounded once, in the engine's [B*H*W, C] layout
    stored = rnd(ref).permute(0, 2, 3, 1).reshape(B * H * W, C).to(torch.bfloat16)
    return stored, ref, (B, H, W)


def test_checker_accepts_a_correctly_rounded_tensor():
    stored, ref, (B, H, W) = _stored_conv()
    ck = Checker()
    ck.check("y", nchw(stored, B, H, W), ref, 4e-3)
    ck.finish("control")


def test_checker_rejects_the_last_image_zeroed():
    stored, ref, (B, H, W) = _stored_conv()
    bad = stored.clone()
    bad[(B - 1) * H * W:] = 0                                        # the last image's rows (a skipped tail round)
    ck = Checker()
    ck.check("y", nchw(bad, B, H, W), ref, 4e-3)
    assert f"dim0[{B - 1}]" in [f[1] for f in ck.fails], ck.fails       # the last image itself is named
    assert float(slice_errors(nchw(bad, B, H, W), ref, 0)[B - 1]) > 0.99


def test_checker_rejects_one_channel_scaled_where_the_global_norm_cannot():
    stored, ref, (B, H, W) = _stored_conv()
    c = 77
    bad = stored.float()
    bad[:, c] *= 1 + 2 ** -5
    bad = bad.to(torch.bfloat16)
    got = nchw(bad, B, H, W)
    glob = float((got - ref).norm() / ref.norm())
    assert glob < 4e-3, glob                                         # the global relative norm alone passes it ...
    ck = Checker()
    ck.check("y", got, ref, 4e-3)
    assert len(ck.fails) == 1 and ck.fails[0][1] == f"dim1[{c}]", ck.fails      # ... the per-channel check does not
    assert ck.fails[0][2] > 2 ** -5 * 0.9


def test_checker_rejects_nan():
    stored, ref, (B, H, W) = _stored_conv()
    bad = stored.clone()
    bad[5, 3] = float("nan")
    ck = Checker()
    ck.check("y", nchw(bad, B, H, W), ref, 4e-3)
    assert ck.fails


def test_near_zero_slices_are_measured_against_the_floor():
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(8, 16, 4, 4, generator=g)
    ref[:, 3] *= 1e-6                                                # a dead channel: relative rounding noise there stays small
    got = ref + 1e-3 * ref.abs().mean() * torch.randn(ref.shape, generator=g) / 1e2
    ck = Checker()
    ck.check("y", got, ref, 4e-3)
    ck.finish("floor")


# ---- grouped (many questions per image): U images, N questions, question b on image IDX[b]; images 0 and U - 1 have none
U, H, LQ, LK, HD = 9, 2, 5, 7, 8
IDX = torch.tensor([3, 1, 1, 7, 2, 3, 5, 1, 6, 4, 2, 3, 1, 5, 4, 6, 2, 7, 3, 3])


def _attn_operands(seed=4):
    g = torch.Generator().manual_seed(seed)
    n = len(IDX)
    Qh = torch.randn(n, H, LQ, HD, generator=g, dtype=torch.float64)
    Kh = torch.randn(U, H, LK, HD, generator=g, dtype=torch.float64)
    Vh = torch.randn(U, H, LK, HD, generator=g, dtype=torch.float64)
    keep = (torch.rand(n, H, LQ, LK, generator=g) > 0.1).double() / 0.9
    P, _ = attn_core_fwd(Qh, Kh, Vh, torch.zeros(n, H, LQ, LK, dtype=torch.float64), keep, index=IDX)
    dC = torch.randn(n, H, LQ, HD, generator=g, dtype=torch.float64)
    return Qh, Kh, Vh, P, keep, dC


def test_indexed_attention_reference_is_the_expanded_one_summed_per_image():
    Qh, Kh, Vh, P, keep, dC = _attn_operands()
    dQ, dK, dV = attn_core_bwd(Qh, Kh, Vh, P, keep, dC, index=IDX, n_kv=U)
    # expanded: every question carries its own copy of its image's K / V (the plain backward), then a plain per-image loop
    Pe, ctxe = attn_core_fwd(Qh, Kh[IDX], Vh[IDX], P, keep)
    Pi, ctxi = attn_core_fwd(Qh, Kh, Vh, P, keep, index=IDX)
    assert torch.equal(Pe, Pi) and torch.equal(ctxe, ctxi)
    dQe, dKe, dVe = attn_core_bwd(Qh, Kh[IDX], Vh[IDX], P, keep, dC)
    assert torch.equal(dQ, dQe)
    for u in range(U):
        mine = (IDX == u).nonzero().flatten().tolist()
        refk = sum((dKe[b] for b in mine), torch.zeros_like(dK[u]))
        refv = sum((dVe[b] for b in mine), torch.zeros_like(dV[u]))
        torch.testing.assert_close(dK[u], refk, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(dV[u], refv, rtol=1e-12, atol=1e-12)
        assert bool(dK[u].abs().sum() > 0) == bool(mine)


def _flat(t):
    return t.transpose(1, 2).reshape(-1, H * HD)


@pytest.mark.parametrize("which", ["first", "last"])
def test_checker_rejects_a_dk_missing_one_question_of_one_image(which):
    Qh, Kh, Vh, P, keep, dC = _attn_operands()
    _, dK, _ = attn_core_bwd(Qh, Kh, Vh, P, keep, dC, index=IDX, n_kv=U)
    ck = Checker()
    ck.check("dK", rnd(_flat(dK).float()), _flat(dK), T_ATTN, cls="attn", slice_tol=T_ATTN_SLICE)     # as a bf16 kernel stores it
    ck.finish("control")
    # the same sum over the image's questions with one of them left out (image 3's first or last question in CSR order)
    q = (IDX == 3).nonzero().flatten()
    drop = int(q[0] if which == "first" else q[-1])
    keep_q = torch.tensor([b for b in range(len(IDX)) if b != drop])
    _, dKb, _ = attn_core_bwd(Qh[keep_q], Kh, Vh, P[keep_q], keep[keep_q], dC[keep_q], index=IDX[keep_q], n_kv=U)
    ck = Checker()
    ck.check("dK", rnd(_flat(dKb).float()), _flat(dK), T_ATTN, cls="attn", slice_tol=T_ATTN_SLICE)
    rows = [int(f[1][5:-1]) for f in ck.fails if f[1].startswith("dim0[")]
    assert rows and all(3 * LK <= r < 4 * LK for r in rows), ck.fails      # only image 3's rows, and they are named


def test_csr_check_accepts_the_contract_and_rejects_two_order_entries_swapped():
    order = torch.argsort(IDX, stable=True)
    offsets = torch.zeros(U + 1, dtype=torch.long)
    offsets[1:] = torch.cumsum(torch.bincount(IDX, minlength=U), 0)
    ck = Checker()
    check_csr(ck, "csr", IDX, U, offsets.int(), order.int())
    ck.finish("control")
    assert order[0] == 1 and order[1] == 2                 # image 1's first two questions
    for i, j in ((0, 1), (3, 12)):                        # within one image (ascending order broken), across two images
        bad = order.clone()
        bad[i], bad[j] = order[j], order[i]
        ck = Checker()
        check_csr(ck, "csr", IDX, U, offsets, bad)
        assert [f[0] for f in ck.fails] == ["csr order"], ck.fails
    bad = offsets.clone()
    bad[4] += 1
    ck = Checker()
    check_csr(ck, "csr", IDX, U, bad, order)
    assert [f[0] for f in ck.fails] == ["csr offsets"], ck.fails


def test_zero_rows_of_images_without_questions():
    empty = empty_images(IDX, U)
    assert empty.tolist() == [0, U - 1]
    t = torch.randn(U * LK, 16).to(torch.bfloat16)
    t[:LK] = 0
    t[(U - 1) * LK:] = 0
    ck = Checker()
    check_zero_rows(ck, "dK", t, U, empty)
    check_zero_rows(ck, "dK cols", t[:, 8:], U, empty)     # a column slice of a fused [rows][2d] buffer
    ck.finish("control")
    for r, val in ((0, 2.0 ** -133), (U * LK - 1, float("nan"))):   # the smallest bf16 subnormal; a NaN
        bad = t.clone()
        bad[r, 11] = val
        ck = Checker()
        check_zero_rows(ck, "dK", bad, U, empty)
        assert [f[0] for f in ck.fails] == ["dK zero rows"], ck.fails
