"""GPU: the frozen-parameter optimizer tail (vqa_sumsq_ranges + vqa_adamw_ranges, csrc/optim_ops.hip) against float64.

The two entries run clip_grad_norm_ + AdamW over a table of trainable ranges {lo, hi, pos, lag index} of a flat buffer
(finetune.range_table_rows builds it).  Checked here, per table shape: elements outside every range are never read (the gradient is NaN
there) and never written (parameters, moments and the bf16 operand copy keep a sentinel bit pattern there); inside, the norm, the
parameters and both moments follow fp64 AdamW at each range's OWN step number  calls - skipped[2] - lag[index]  over three steps; the
lag counters of the frozen parameters advance by one per applied step; a skipped launch changes nothing but the skip counters."""
import math

import pytest
import torch

from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01
SENT32, SENT16 = 0x7FA5A5A5, 0x7FA5                                 # NaN bit patterns: reading one poisons, writing one shows

BIG = [(400_000, 1_900_000, 0), (2_200_000, 4_200_000, 1), (4_549_696, 5_248_000, 2)]        # 4 194 304 + 4 000 trainable elements
TABLES = {
    "whole": (4096, [(0, 4096, 0)]),
    "interior": (4096, [(1000, 3004, 0)]),
    "gaps-4-8-end": (4000, [(8, 1000, 0), (1004, 2000, 1), (2008, 4000, 2)]),
    "r512": (4096, [(8 * r, 8 * r + 4, r) for r in range(512)]),   # the largest table, the deepest binary search
    "two-trips": (5_248_000, BIG),                                  # > 4096 x 256 x 4 (adamw) and > 2048 x 256 x 4 (sumsq) elements
}


class State:
    """Flat buffers with NaN gradients / sentinel parameters outside the ranges, their fp64 mirror, and the device-side counters."""

    def __init__(self, n_buf, ranges, nlag=None, seed=0):
        FT = sub("finetune")
        self.n_buf, self.ranges = n_buf, ranges
        self.rows = FT.range_table_rows(ranges)                     # the producer's format: {lo, hi, pos, lag index}
        self.R, self.n = len(self.rows), sum(hi - lo for lo, hi, _ in ranges)
        self.inside = torch.zeros(n_buf, dtype=torch.bool)
        for lo, hi, _ in ranges:
            self.inside[lo:hi] = True
        assert int(self.inside.sum()) == self.n
        self.g = torch.Generator().manual_seed(seed)
        self.table = torch.tensor(self.rows if self.rows else [[0, 0, 0, 0]], dtype=torch.int64).to(DEV)
        nlag = nlag if nlag is not None else max([j for _, _, j in ranges], default=0) + 1
        self.lag = torch.zeros(nlag, dtype=torch.int32, device=DEV)
        self.skipped = torch.zeros(3, dtype=torch.int32, device=DEV)
        self.sumsq = torch.zeros(2049, device=DEV)
        p0 = torch.randn(n_buf, generator=self.g)
        m0 = torch.randn(n_buf, generator=self.g) * 1e-2
        v0 = torch.rand(n_buf, generator=self.g) * 1e-3 + 1e-6
        self.ref = [t.double() for t in (p0, m0, v0)]               # fp64 mirror (only [inside] is meaningful)
        self.p, self.m, self.v = (self._sentinel(t) for t in (p0, m0, v0))
        self.pb = torch.full((n_buf,), SENT16, dtype=torch.int16).view(torch.bfloat16).to(DEV)

    def _sentinel(self, t):
        out = torch.full((self.n_buf,), SENT32, dtype=torch.int32).view(torch.float32).clone()
        out[self.inside] = t[self.inside]
        return out.to(DEV)

    def grad(self, scale):
        gr = torch.randn(self.n_buf, generator=self.g) * scale
        gr[~self.inside] = float("nan")
        return gr

    def outside_untouched(self):
        o = ~self.inside
        for t in (self.p, self.m, self.v):
            if not (t.cpu().view(torch.int32)[o] == SENT32).all():
                return False
        return bool((self.pb.cpu().view(torch.int16)[o] == SENT16).all())

    def launch(self, gr, calls, *, max_norm=1.0, gscale=1.0, skip=None, frozen=None, lag=True, copy=True):
        L = sub("_lib")
        gd = gr.to(DEV)
        L.call("vqa_sumsq_ranges", gd.data_ptr(), self.table.data_ptr(), self.R, self.n, self.sumsq.data_ptr())
        nf = 0 if frozen is None else frozen.numel()
        L.call("vqa_adamw_ranges", self.p.data_ptr(), gd.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.table.data_ptr(), self.R,
               self.n, LR, B1, B2, EPS, WD, calls, self.sumsq.data_ptr(), max_norm, gscale, L.ptr(skip), self.skipped.data_ptr(),
               self.lag.data_ptr() if lag else None, L.ptr(frozen), nf, self.pb.data_ptr() if copy else None)
        torch.cuda.synchronize()

    def ref_step(self, gr, steps, *, max_norm=1.0, gscale=1.0):
        """fp64 clip + AdamW per range; steps[r] = that range's Adam step number.  Returns (norm, clip active)."""
        p, m, v = self.ref
        gd = gr.double()
        norm = math.sqrt(float((gd[self.inside] ** 2).sum()))
        c = max_norm / (norm * gscale + 1e-6)
        coef = gscale * (c if c < 1 else 1.0)
        for (lo, hi, _), t in zip(self.ranges, steps):
            gq = gd[lo:hi] * coef
            p[lo:hi] *= 1 - LR * WD
            m[lo:hi] = B1 * m[lo:hi] + (1 - B1) * gq
            v[lo:hi] = B2 * v[lo:hi] + (1 - B2) * gq * gq
            p[lo:hi] -= LR / (1 - B1 ** t) * m[lo:hi] / (v[lo:hi].sqrt() / math.sqrt(1 - B2 ** t) + EPS)
        return norm, c < 1

    def check(self, norm=None):
        i = self.inside
        if norm is not None:
            ss = float(self.sumsq[0])
            assert math.isfinite(ss)                                # never read: the gradient is NaN outside the ranges
            assert abs(math.sqrt(ss) - norm) / norm < 1e-5
        assert self.outside_untouched()                             # never written
        p, m, v = (t.cpu().double() for t in (self.p, self.m, self.v))
        rp, rm, rv = self.ref
        ep = float((p[i] - rp[i]).abs().max())
        em = float((m[i] - rm[i]).abs().max() / rm[i].abs().max())
        ev = float((v[i] - rv[i]).abs().max() / rv[i].abs().max())
        print(f"   |dp| {ep:.2e}  dm/max {em:.2e}  dv/max {ev:.2e}")
        assert ep < 2e-6 and em < 1e-5 and ev < 1e-5
        assert torch.equal(self.pb.cpu()[i], self.p.cpu()[i].to(torch.bfloat16))      # the bf16 operand copy of the same launch


@pytest.mark.parametrize("clip_active,gscale", [(True, 1.0), (True, 0.5), (False, 1.0), (False, 0.5)])
@pytest.mark.parametrize("name", ["whole", "interior", "gaps-4-8-end", "r512"])
def test_ranges_match_fp64_adamw_and_touch_nothing_else(name, clip_active, gscale):
    n_buf, ranges = TABLES[name]
    s = State(n_buf, ranges, seed=len(name))
    for t in (1, 2, 3):
        gr = s.grad(0.2 if clip_active else 1e-4)
        norm, active = s.ref_step(gr, [t] * len(ranges), gscale=gscale)
        assert bool(active) == clip_active
        s.launch(gr, t, gscale=gscale)
        s.check(norm)


def test_ranges_grid_stride_loops_take_a_second_trip():
    n_buf, ranges = TABLES["two-trips"]
    s = State(n_buf, ranges, seed=3)
    assert s.n == 4_194_304 + 4_000 and s.inside[-1]
    for t in (1, 2, 3):
        gr = s.grad(2e-3)                                           # norm 4.1, 2.05 after the gradient scale: the clip is active
        norm, active = s.ref_step(gr, [t] * 3, gscale=0.5)
        assert active
        s.launch(gr, t, gscale=0.5)
        s.check(norm)


def test_ranges_step_number_is_per_range_and_lag_advances():
    """calls = 3 with lag = {0, 2}: the first range is at Adam step 3, the second at step 1.  A shared or ignored lag moves p by a large
    fraction of lr = 1e-3, far outside 2e-6."""
    s = State(4000, [(8, 1000, 0), (1004, 4000, 1)], nlag=5, seed=11)
    lag0 = torch.tensor([0, 2, 7, 1, 4], dtype=torch.int32)
    s.lag.copy_(lag0)
    frozen = torch.tensor([2, 4], dtype=torch.int32, device=DEV)
    gr = s.grad(1e-4)
    norm, _ = s.ref_step(gr, [3, 1])
    s.launch(gr, 3, frozen=frozen)
    s.check(norm)
    assert s.lag.tolist() == [0, 2, 8, 1, 5]                        # exactly the frozen entries, by exactly one
    # no lag table: every range at calls - skipped[2]
    gr = s.grad(1e-4)
    norm, _ = s.ref_step(gr, [4, 4])
    s.launch(gr, 4, lag=False)
    s.check(norm)
    assert s.lag.tolist() == [0, 2, 8, 1, 5]


def test_ranges_skipped_launch_changes_nothing_and_does_not_count_as_a_step():
    s = State(4000, [(8, 1000, 0), (1004, 2000, 1), (2008, 4000, 2)], nlag=4, seed=12)
    frozen = torch.tensor([3], dtype=torch.int32, device=DEV)
    for t in (1, 2):
        gr = s.grad(1e-4)
        norm, _ = s.ref_step(gr, [t] * 3)
        s.launch(gr, t, frozen=frozen)
        s.check(norm)
    assert s.lag.tolist() == [0, 0, 0, 2]
    s.skipped.copy_(torch.tensor([5, 3, 0], dtype=torch.int32))
    before = [t.clone() for t in (s.p, s.m, s.v, s.pb, s.lag)]
    skip = torch.tensor([2], dtype=torch.int32, device=DEV)
    s.launch(s.grad(1e-4), 3, skip=skip, frozen=frozen)
    for a, b in zip(before, (s.p, s.m, s.v, s.pb, s.lag)):
        av, bv = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) for t in (a, b))
        assert torch.equal(av, bv)                                  # bit-unchanged (sentinels included)
    assert s.skipped.tolist() == [5 + 2, 3 + 1, 0 + 1]
    gr = s.grad(1e-4)                                               # the next applied launch is Adam step 3, not 4
    norm, _ = s.ref_step(gr, [3] * 3)
    s.launch(gr, 4, skip=torch.zeros(1, dtype=torch.int32, device=DEV), frozen=frozen)
    s.check(norm)
    assert s.lag.tolist() == [0, 0, 0, 3] and s.skipped.tolist() == [7, 4, 1]


def test_ranges_refusals_and_the_empty_table():
    L = sub("_lib")
    n_buf = 4096
    bufs = [torch.full((n_buf,), 2.0, device=DEV) for _ in range(4)]
    p, g, m, v = bufs
    ss = torch.full((2049,), 3.0, device=DEV)
    lag = torch.zeros(4, dtype=torch.int32, device=DEV)
    frozen = torch.tensor([1], dtype=torch.int32, device=DEV)
    table = torch.tensor([[8 * r, 8 * r + 4, 4 * r, 0] for r in range(513)], dtype=torch.int64, device=DEV)

    def adamw(R, n, calls=1, lag_=lag, frozen_=None, nf=0):
        L.call("vqa_adamw_ranges", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), table.data_ptr(), R, n, LR, B1, B2, EPS, WD,
               calls, ss.data_ptr(), 1.0, 1.0, None, None, L.ptr(lag_), L.ptr(frozen_), nf, None)

    def sumsq(R, n):
        L.call("vqa_sumsq_ranges", g.data_ptr(), table.data_ptr(), R, n, ss.data_ptr())

    for R, n in ((513, 513 * 4), (1, 6), (0, 4)):                   # too many ranges, n % 4 != 0, no table for n > 0
        with pytest.raises(RuntimeError):
            sumsq(R, n)
        with pytest.raises(RuntimeError):
            adamw(R, n)
    with pytest.raises(RuntimeError):
        adamw(1, 4, calls=0)                                        # Adam's step number starts at 1
    with pytest.raises(RuntimeError):
        adamw(1, 4, lag_=None, frozen_=frozen, nf=1)                # frozen parameters need the lag table they advance
    torch.cuda.synchronize()
    assert all((t == 2.0).all() for t in bufs) and (ss == 3.0).all() and (lag == 0).all()
    # the empty table is a valid step over nothing
    sumsq(0, 0)
    adamw(0, 0)
    torch.cuda.synchronize()
    assert float(ss[0]) == 0.0
    assert all((t == 2.0).all() for t in bufs) and (lag == 0).all()
