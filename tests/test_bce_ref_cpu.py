"""CPU: sigmoid BCE on the soft answer scores exists end to end -- the fp64 restatement the GPU tests use (tests/_bceref.py) equals
F.binary_cross_entropy_with_logits on dense targets, vqa_bce_soft is declared with the table's arity, exported by the library built
for gfx950 and refuses bad arguments with 1000 before any HIP call, and HipTrainer documents the option."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _bceref as R
from _pkg import REPO, pkg, sub


@pytest.mark.parametrize("K", [1, 4, 10, 64])
def test_reference_equals_torch_bce_on_dense_targets(K):
    g = torch.Generator().manual_seed(11)
    for B, N in ((512, 1000), (7, 10), (33, 2000)):
        x = (torch.randn(B, N, generator=g) * 3).double()
        if N >= 4:
            x[0, :4] = torch.tensor([90.0, -90.0, 88.7, -104.0], dtype=torch.float64)
        ids, w = R.random_soft(B, N, K, g)
        cnt = torch.randint(0, 5, (B, K), generator=g).int()
        t = R.dense(ids, w, N)
        # the dense targets themselves, slot by slot
        tt = torch.zeros(B, N, dtype=torch.float64)
        for b in range(B):
            for k in range(K):
                if ids[b, k] >= 0:
                    tt[b, ids[b, k]] += float(w[b, k])
        assert torch.equal(t, tt)
        if K > 1:
            assert float(t.max()) > 1.0                                        # duplicates add up and nothing is clamped
        assert bool((t.sum(1) == 0).any())                                     # all-empty rows occur
        xin = x.clone().requires_grad_(True)
        ref = F.binary_cross_entropy_with_logits(xin, t, reduction="sum") / B
        ref.backward()
        loss, grad, bad, thirds = R.bce(x, ids, w, cnt, gscale=1.0)
        assert not bool(bad.any())
        assert abs(float(loss) - float(ref.detach())) < 1e-12 * max(1.0, abs(float(ref.detach())))
        assert float((grad - xin.grad).abs().max()) < 1e-15
        assert torch.isfinite(grad).all() and torch.isfinite(loss)
        _, g2, _, _ = R.bce(x, ids, w, gscale=0.25)
        assert float((g2 - 0.25 * grad).abs().max()) < 1e-15
        empty = (ids < 0).all(1)
        assert float((grad[empty] - torch.sigmoid(x[empty]) / B).abs().max()) < 1e-15 and bool((grad[empty] != 0).all())
        # the thirds: a python loop over the rows
        want = 0
        for b in range(B):
            best = int(x[b].argmax())
            assert float(x[b, best]) == float(x[b].max()) and not bool((x[b, :best] == x[b].max()).any())
            want += min(3, sum(int(cnt[b, k]) for k in range(K) if int(ids[b, k]) == best))
        assert thirds == [want, B]


def test_reference_marks_bad_rows_and_resolves_ties_to_the_lowest_index():
    N = 10
    ids = torch.tensor([[1, -1, -1], [10, 2, -1], [3, 3, -1], [-2, 1, 1], [9, -1, 0], [2, 1 << 30, -1]], dtype=torch.int32)
    w = torch.full((6, 3), 1.0 / 3.0)
    x = torch.randn(6, N, generator=torch.Generator().manual_seed(2))
    loss, grad, bad, _ = R.bce(x, ids, w)
    assert bad.tolist() == [False, True, False, True, False, True]
    assert torch.isnan(loss) and torch.isnan(grad[bad]).all() and torch.isfinite(grad[~bad]).all()
    x = torch.zeros(1, N)
    x[0, 2] = x[0, 7] = 4.0
    _, _, _, thirds = R.bce(x, torch.tensor([[7, 2, -1]], dtype=torch.int32), torch.ones(1, 3), torch.tensor([[3, 1, 0]], dtype=torch.int32))
    assert thirds == [1, 1]                                                    # class 2 (one vote) wins over class 7 (three votes)


def _header_decls():
    txt = open(os.path.join(REPO, "include", "vqa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\bint\s+(vqa_\w+)\s*\((.*?)\)\s*;", txt, flags=re.S)}


def test_header_declares_vqa_bce_soft_with_the_table_arity():
    decls, L, K = _header_decls(), sub("_lib"), sub("kernels")
    assert "vqa_bce_soft" in decls and "vqa_bce_soft" in L.SIGNATURES
    assert decls["vqa_bce_soft"] == len(L.SIGNATURES["vqa_bce_soft"]) == 16
    assert L.SIGNATURES["vqa_bce_soft"] == L.SIGNATURES["vqa_cross_entropy_soft"]        # the same arguments
    a = [1, 1, 1, 1, 10, 1, 1, 1, 512, 1000, 1.0, 1, 1, 1, 1]
    assert K.HBM_BYTES["vqa_bce_soft"][1](a) == K.HBM_BYTES["vqa_cross_entropy_soft"][1](a)


def test_library_exports_vqa_bce_soft():
    import __graft_entry__ as G
    G.build()
    assert hasattr(sub("_lib").lib(), "vqa_bce_soft")


def test_vqa_bce_soft_rejects_bad_arguments_without_a_launch():
    import __graft_entry__ as G
    G.build()
    c = sub("_lib").lib().vqa_bce_soft      # (dtype, logits, ids, weights, K, loss, dlogits, lf32, B, N, gscale, err, ws, counts, acc, stream)
    ok = [0, 1, 1, 1, 10, 1, 1, None, 4, 100, 1.0, None, None, None, None, None]
    cases = ((1, None), (2, None), (3, None),                                  # NULL logits / ids / weights
             (4, 0), (4, -3), (4, 65),                                         # K < 1, K > 64
             (8, 0), (8, -1), (9, 0), (9, -1),                                 # B < 1, N < 1
             (14, 1),                                                          # acc without counts
             (0, 2), (0, -1),                                                  # dtype not 0 / 1
             (10, float("inf")), (10, float("-inf")), (10, float("nan")))      # gscale not finite
    for pos, val in cases:
        a = list(ok)
        a[pos] = val
        assert c(*a) == 1000, (pos, val)


def test_hiptrainer_step_documents_the_loss_option():
    T = sub("trainer")
    doc = T.HipTrainer.step.__doc__
    assert 'loss="bce"' in doc and "vqa_bce_soft" in doc and "loss_kind" in doc
    ST = pkg().load_dropin_soft_targets()
    assert issubclass(ST.SoftTargetBCEWithLogits, torch.nn.Module)
    with pytest.raises(RuntimeError):
        ST.SoftTargetBCEWithLogits()(torch.zeros(4, 10), ST.SoftTargets(torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, 2)))
