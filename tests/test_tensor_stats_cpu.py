"""CPU: the per-parameter statistics surface exists end to end without a GPU -- the float64 reference (tests/_statsref.py) against
hand-worked cases, kernels.stats_table's refusals and chunk arithmetic, the host logic of monitor.TensorMonitor (due rule, ring wrap,
dropped, constructor errors), the C entry's declaration and its refusals before any HIP call, and the drop-in's registration."""
import inspect
import os
import re

import pytest
import torch

import _statsref as R
from _pkg import REPO, pkg, sub


def _header():
    txt = open(os.path.join(REPO, "include", "vqa_hip.h")).read()
    return txt, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _chunk():
    return int(re.search(r"#define\s+VQA_STATS_CHUNK\s+(\d+)", _header()[0]).group(1))


# ------------------------------------------------------------------------------------------------------------- the reference
def test_reference_on_hand_worked_rows():
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([9.0, 9.0, 9.0, 9.0, 3.0, -4.0, 0.0, -0.0, nan, inf, -inf, 0.5, 7.0, 7.0, 7.0, 7.0])
    assert R.row(x, 4, 8) == (25.0, 4.0, 0, 2)                      # 3^2 + 4^2; 0.0 and -0.0 are both zeros
    assert R.row(x, 8, 12) == (0.25, 0.5, 3, 0)                     # the magnitude of the finite rest, the count says the rest
    assert R.row(x, 8, 11) == (0.0, 0.0, 3, 0)                      # no finite element: 0 and 0
    assert R.row(x, 4, 5) == (9.0, 3.0, 0, 0)
    y = torch.tensor([9.0, 9.0, 9.0, 9.0, 1.0, -4.0, 0.0, 5.0, nan, inf, inf, 0.5, 7.0, 7.0, 7.0, 7.0])
    assert R.row(x, 4, 8, y) == (4.0 + 25.0, 5.0, 0, 2)             # d = {2, 0, 0, -5}
    assert R.row(x, 8, 12, y) == (0.0, 0.0, 3, 1)                   # nan - nan, inf - inf, -inf - inf: three non-finite; 0.5 - 0.5
    t = R.table(x, [(4, 8), (8, 12)])
    assert t["sumsq"].tolist() == [25.0, 0.25] and t["absmax"].tolist() == [4.0, 0.5]
    assert t["nonfinite"].tolist() == [0, 3] and t["zeros"].tolist() == [2, 0]
    # the subtraction is ONE fp32 operation: 1 - 2^-25 rounds to 1 in fp32, the difference is an exact zero
    a, b = torch.tensor([1.0]), torch.tensor([2.0 ** -25])
    assert R.row(a + 0, 0, 1, a - b) == (0.0, 0.0, 0, 1)


def test_unpack_reads_the_words_the_kernel_writes():
    f = torch.tensor([[2.5, 1.5], [0.0, 0.0]], dtype=torch.float32).view(torch.int32)
    c = torch.tensor([[3, -1], [0, 7]], dtype=torch.int32)          # -1: the unsigned word 2^32 - 1
    u = R.unpack(torch.cat([f, c], 1))
    assert u["sumsq"].tolist() == [2.5, 0.0] and u["absmax"].tolist() == [1.5, 0.0]
    assert u["nonfinite"].tolist() == [3, 0] and u["zeros"].tolist() == [2 ** 32 - 1, 7]


def test_rounding_bound_counts_the_kernels_chain():
    C = _chunk()
    assert C == 8192
    assert R.n_add(2359296, C) == 329                               # 288 chunks + 32 in the thread + 6 + 2 + the square
    assert R.n_add(1, C) == 4 + 1 + 6 + 2 + 1 + 1                   # (an upper bound: up to one float4 per 1024 elements, + the tail)
    assert R.n_add(4, C) == 4 + 6 + 2 + 1 + 1
    assert R.n_add(1024, C) == 4 + 9 + 1 and R.n_add(1025, C) == 8 + 1 + 9 + 1
    assert R.n_add(C, C) == 32 + 9 + 1 and R.n_add(C + 1, C) == 32 + 1 + 9 + 2 and R.n_add(3 * C + 5, C, pair=True) == 32 + 1 + 9 + 4 + 1
    assert R.sumsq_bound(C, C) == 42 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------- the table (host logic)
def test_chunk_constant_is_one_number_everywhere():
    C = _chunk()
    assert C % 1024 == 0 and C == sub("kernels").STATS_CHUNK
    src = open(os.path.join(os.path.dirname(sub("kernels").__file__), "csrc", "stats_ops.hip")).read()
    assert int(re.search(r"#define\s+VQA_STATS_CHUNK\s+(\d+)", src).group(1)) == C


def test_stats_table_chunk_arithmetic_and_refusals():
    K = sub("kernels")
    C = K.STATS_CHUNK
    numels = [C - 1, C, C + 1, 1, 3 * C + 5]
    ranges, off = [], 16
    for n in numels:
        ranges.append((off, off + n))
        off += (n + 7) // 8 * 8
    rows, chunks = K.stats_rows(ranges)
    assert [r[:2] for r in rows] == [list(r) for r in ranges]
    assert [r[2] for r in rows] == [0, 1, 2, 4, 5] and chunks == 9
    t = K.stats_table(ranges, device="cpu")
    tab, P, ch = t                                                  # (table, P, chunks), as documented
    assert P == 5 and ch == 9 and tab.dtype == torch.int64 and tab.tolist() == rows and t.extent == ranges[-1][1]
    # the order of the rows is the caller's: first_chunk follows it
    rows2, _ = K.stats_rows(ranges[::-1])
    assert [r[2] for r in rows2] == [0, 4, 5, 7, 8]
    for bad in ([(8, 8)], [(8, 4)], [(2, 10)], [(-4, 4)], [(0, 16), (8, 24)], [(8, 24), (0, 9)], []):
        with pytest.raises(ValueError):
            K.stats_rows(bad)
    with pytest.raises(ValueError):
        K.stats_rows([(8 * i, 8 * i + 1) for i in range(K.STATS_MAX_ROWS + 1)])
    K.stats_rows([(0, 8), (8, 9)])                                  # touching ranges do not overlap
    with pytest.raises(ValueError):                                 # there is no CPU path behind the table
        K.tensor_stats(torch.zeros(64), t)


# ------------------------------------------------------------------------------------------------ the monitor (host logic)
def test_monitor_constructor_refuses_before_anything_is_allocated():
    M = sub("monitor")
    for kw in (dict(every=0), dict(every=-3), dict(slots=0), dict(every=1.5), dict(slots="4"), dict(every=True)):
        with pytest.raises(ValueError):
            M.TensorMonitor(**kw)
    m = M.TensorMonitor()
    assert (m.every, m.slots, m.records, m.dropped) == (100, 64, 0, 0) and m._ring is None and m._snap is None and m.read() == []


def test_monitor_due_rule_ring_wrap_and_dropped():
    M = sub("monitor")
    m = M.TensorMonitor(every=3, slots=2)
    assert [c for c in range(1, 10) if m.due(c)] == [3, 6, 9]
    assert [m._claim(c, 0.5, None) for c in (3, 6)] == [0, 1] and m.dropped == 0
    assert m._claim(9, 0.25, (True, False)) == 0 and m.dropped == 1 and m.records == 3
    assert [(s, c) for s, c, _, _ in m._live] == [(1, 6), (0, 9)] and m._live[-1][2:] == (0.25, (True, False))
    assert m._claim(12, 1.0, None) == 1 and m.dropped == 2 and [c for _, c, _, _ in m._live] == [9, 12]
    m.clear()
    assert len(m._live) == 0 and m.dropped == 2 and m.read() == []
    assert m._claim(15, 1.0, None) == 0                             # records % slots goes on counting
    a, b = object(), object()
    m._attach(a)
    m._attach(a)
    with pytest.raises(ValueError):
        m._attach(b)


def test_records_are_built_from_the_words():
    M = sub("monitor")
    P = 3
    def words(sumsq, absmax, nf, z):
        f = torch.tensor([sumsq, absmax], dtype=torch.float32).t().contiguous().view(torch.int32)
        return torch.cat([f, torch.tensor([nf, z], dtype=torch.int32).t()], 1)
    w = {"grad": words([16.0, 0.0, 4.0], [3.0, 0.0, 2.0], [0, 0, 1], [0, 5, 0]),
         "param": words([4.0, 0.0, 1.0], [2.0, 0.0, 1.0], [0, 0, 0], [0, 5, 0]),
         "update": words([1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0, 0, 0], [1, 5, 7])}
    numel, tr = torch.tensor([4, 5, 7]), torch.tensor([True, False, True])
    r = M.make_record(w, 12, ["a", "b", "c"], numel, tr, gscale=0.5)
    assert r.step == 12 and r.names == ["a", "b", "c"] and r.numel.tolist() == [4, 5, 7] and r.trainable.tolist() == [True, False, True]
    assert r.grad_norm.tolist() == [2.0, 0.0, 1.0] and r.grad_absmax.tolist() == [1.5, 0.0, 1.0] and r.grad_norm.dtype == torch.float64
    assert r.grad_nonfinite.tolist() == [0, 0, 1] and r.grad_zeros.tolist() == [0, 5, 0] and r.grad_zeros.dtype == torch.int64
    assert r.param_norm.tolist() == [2.0, 0.0, 1.0] and r.update_norm.tolist() == [1.0, 0.0, 0.0] and r.update_unchanged.tolist() == [1, 5, 7]
    assert r.update_ratio.tolist() == [0.5, 0.0, 0.0]                # 0 where param_norm is 0
    assert r.moment2_norm is None and r.ema_zeros is None
    assert r.worst("grad_norm", k=2) == ["a", "c"] and r.worst("update_unchanged", k=1) == ["c"] and len(r.worst("grad_norm")) == P
    with pytest.raises(KeyError):
        r.worst("nothing")
    with pytest.raises(ValueError):
        r.worst("ema_norm")
    assert M.check_now_kinds(("grad", "moment2")) == ("grad", "moment2") and M.check_now_kinds("ema") == ("ema",)
    for bad in (("update",), ("grad", "update"), ("grad", "grad"), (), ("weights",)):
        with pytest.raises(ValueError):
            M.check_now_kinds(bad)


# --------------------------------------------------------------------------------------------------------- the C entry, wiring
def test_entry_is_declared_bound_and_refuses_bad_arguments():
    decl = re.search(r"\bint\s+vqa_tensor_stats\s*\((.*?)\)\s*;", _header()[1], flags=re.S)
    assert decl is not None
    L = sub("_lib")
    assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(L.SIGNATURES["vqa_tensor_stats"]) == 8
    import __graft_entry__ as G
    G.build()
    f = L.lib().vqa_tensor_stats                    # (x, y, table, P, chunks, out, scratch, stream)
    ok = [1, None, 1, 4, 4, 1, 1, None]
    for pos, val in ((0, None), (2, None), (5, None), (6, None), (3, 0), (3, -1), (3, 4097), (4, 3), (4, 0), (4, 2 ** 31)):
        a = list(ok)
        a[pos] = val
        assert f(*a) == 1000, (pos, val)
    a = list(ok)
    a[1] = 1                                        # the pair form has the same refusals
    a[0] = None
    assert f(*a) == 1000


def test_dropin_monitor_is_registered_like_the_average():
    B = sub("binding")
    assert B._DROPIN_ONLY["utils.monitor"] == ("utils", "monitor.py")
    spec = B._DropinOnlyFinder().find_spec("utils.monitor")
    assert spec is not None and spec.origin.endswith("dropin/utils/monitor.py")
    PM = pkg().load_dropin_monitor()
    assert pkg().load_dropin_monitor() is PM and hasattr(PM, "ParameterMonitor")
    for kw in (dict(every=0), dict(slots=0)):
        with pytest.raises(ValueError):
            PM.ParameterMonitor(object(), **kw)
    T = sub("trainer")
    sig = inspect.signature(T.HipTrainer.__init__)
    assert sig.parameters["monitor"].default is None and "monitor" in T.HipTrainer.__init__.__doc__
    assert T.HipTrainer.monitor is None
