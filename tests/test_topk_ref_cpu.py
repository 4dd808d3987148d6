"""The fp64 reference of tests/_topkref.py, pinned without a GPU: against torch.topk on rows of distinct values, and against
hand-written tie, NaN, -inf and nothing-allowed rows (the semantics vqa_softmax_topk states in include/vqa_hip.h)."""
import math

import pytest
import torch

import _topkref as R

INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,N,k", [(4, 50, 5), (3, 200, 200), (1, 1, 1)])
def test_distinct_rows_equal_torch_topk(B, N, k, dtype):
    g = torch.Generator().manual_seed(B * N + k)
    x = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).to(dtype) * 0.125 - 8.0     # distinct in bf16 too (N <= 256)
    assert all(len(set(r.tolist())) == N for r in x)
    idx, p = R.topk_ref(x, k)
    tp, ti = torch.softmax(x.double(), -1).topk(k, dim=-1)
    assert torch.equal(idx, ti)
    assert torch.equal(p, tp)
    if k == N:
        assert (p.sum(-1) - 1).abs().max() < 1e-12


def test_the_documented_order_example():
    y = torch.tensor([[1.0, NAN, 3.0, 3.0, -INF, NAN, 2.0]])
    idx, p = R.topk_ref(y, 7)
    assert idx.tolist() == [[1, 5, 2, 3, 6, 0, 4]]
    assert torch.isnan(p).all()                              # a row holding a NaN: every probability is NaN


def test_ties_go_to_the_lower_index_and_signed_zeros_tie():
    y = torch.tensor([[2.0, 5.0, 2.0, 5.0, 5.0, -1.0], [0.0, -0.0, 0.0, -0.0, -1.0, -0.0]])
    idx, p = R.topk_ref(y, 4)
    assert idx.tolist() == [[1, 3, 4, 0], [0, 1, 2, 3]]
    z = 3 * math.exp(0.0) + 2 * math.exp(-3.0) + math.exp(-6.0)
    assert torch.allclose(p[0], torch.tensor([1 / z, 1 / z, 1 / z, math.exp(-3.0) / z], dtype=torch.float64), rtol=1e-14, atol=0)


def test_minus_inf_entries_have_probability_zero_and_come_last_by_index():
    y = torch.tensor([[-INF, 1.0, -INF, 0.0, -INF]])
    idx, p = R.topk_ref(y, 5)
    assert idx.tolist() == [[1, 3, 0, 2, 4]]
    assert p[0, 2:].tolist() == [0.0, 0.0, 0.0] and abs(float(p[0, :2].sum()) - 1) < 1e-15


def test_mask_shared_per_row_fewer_than_k_and_nothing_allowed():
    x = torch.tensor([[4.0, 3.0, 2.0, 1.0], [1.0, 2.0, 3.0, 4.0], [9.0, 9.0, 9.0, 9.0]])
    shared = torch.tensor([0, 1, 1, 0], dtype=torch.uint8)
    idx, p = R.topk_ref(x, 3, shared)
    assert idx.tolist() == [[1, 2, 0], [2, 1, 0], [1, 2, 0]]        # the tail is the not-allowed entries in index order
    assert (p[:, 2] == 0).all() and torch.allclose(p[:, :2].sum(-1), torch.ones(3, dtype=torch.float64))
    per_row = torch.tensor([[True, False, False, True], [False, False, False, True], [False, False, False, False]])
    idx, p = R.topk_ref(x, 2, per_row)
    assert idx.tolist() == [[0, 3], [3, 0], [0, 1]]
    assert p[1].tolist() == [1.0, 0.0]
    assert torch.isnan(p[2]).all() and not torch.isnan(p[:2]).any()  # nothing allowed: all -inf, NaN like torch.softmax
    assert torch.equal(R.masked(x, per_row)[0], torch.tensor([4.0, -INF, -INF, 1.0], dtype=torch.float64))


def test_all_nan_row_and_scale():
    idx, p = R.topk_ref(torch.full((1, 6), NAN), 3)
    assert idx.tolist() == [[0, 1, 2]] and torch.isnan(p).all()
    x = torch.tensor([[1.0, 3.0, 2.0]])
    i1, p1 = R.topk_ref(x, 3, scale=1.0)
    i2, p2 = R.topk_ref(x, 3, scale=0.5)
    assert torch.equal(i1, i2) and i1.tolist() == [[1, 2, 0]]
    assert torch.equal(p2, torch.softmax(x.double() * 0.5, -1)[:, [1, 2, 0]])
    assert p2[0, 0] < p1[0, 0]                                       # a higher temperature flattens the distribution


def test_prob_error_measures_the_stated_bound():
    ref = torch.tensor([0.5, 0.0, NAN], dtype=torch.float64)
    assert R.prob_error(torch.tensor([0.5, 0.0, NAN]), ref) == (0.0, True)
    e, ok = R.prob_error(torch.tensor([0.5 * (1 + 1e-5), 1e-31, 0.0]), ref)
    assert 0.9e-5 < e < 1.1e-5 and not ok
    assert R.prob_error(torch.tensor([0.5, 1e-20, NAN]), ref)[0] > 1.0
    assert R.prob_error(torch.tensor([NAN, 0.0, NAN]), ref)[0] == INF
