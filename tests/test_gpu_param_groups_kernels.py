"""GPU: the parameter-group optimizer entries (vqa_group_hyper_set, vqa_adamw_groups[_ema][_dev], csrc/optim_ops.hip).

Every range of the table belongs to one of at most 16 groups; a range of group g is updated with lr * lr_scale[g] and wd[g], read
from a device block.  Checked here, on sentinel buffers (NaN gradient and sentinel bit patterns outside the ranges, as
tests/test_gpu_optimizer_ranges.py): neutral groups give the bits of vqa_adamw_ranges[_ema]; per group the update follows
torch.optim.AdamW in float64 with one torch param group per group (lr = LR * lr_scale, that group's weight decay, gradients that carry
the fp64 clip coefficient) within the range-kernel test's bounds; lr_scale 0 keeps the parameter's bits while the moments move; a
skipped launch changes nothing but `skipped`; the _dev entries give the by-value entries' bits and follow a rewritten block; and what
the entries refuse leaves every buffer as it was."""
import ctypes
import math

import pytest
import torch

import _optbits as OB
from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01
SENT32, SENT16 = 0x7FA5A5A5, 0x7FA5                                 # NaN bit patterns: reading one poisons, writing one shows
BIG = [(400_000, 1_900_000, 0), (2_200_000, 4_200_000, 1), (4_549_696, 5_248_000, 2)]
TABLES = {
    "gaps-4-8-end": (4000, [(8, 1000, 0), (1004, 2000, 1), (2008, 4000, 2)]),
    "r512": (4096, [(8 * r, 8 * r + 4, r) for r in range(512)]),   # the largest table, the deepest binary search
    "two-trips": (5_248_000, BIG),                                  # > 4096 blocks x 256 threads x 4 elements: a second grid trip
}
SCALES = (1.0, 0.1, 10.0, 0.0)                                      # group k: lr_scale SCALES[(k + rot) % 4], wd WDS[(k + rot) % 3]
WDS = (0.01, 0.0, 0.1)


def values(G, rot=0):
    return [SCALES[(k + rot) % 4] for k in range(G)], [WDS[(k + rot) % 3] for k in range(G)]


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def floats(v):
    return (ctypes.c_float * len(v))(*v)


def block(scales, wds):
    """a vqa_group_hyper block holding these values"""
    b = torch.zeros(32, dtype=torch.int32, device=DEV)
    sub("_lib").call("vqa_group_hyper_set", b.data_ptr(), len(scales), floats(scales), floats(wds))
    return b


def bits(t):
    return t.cpu().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class GState:
    """Sentinel buffers over a range table with a group per range, and torch.optim.AdamW in float64 as their mirror."""

    def __init__(self, n_buf, ranges, group_of, scales, wds, seed=0):
        FT = sub("finetune")
        self.n_buf, self.ranges, self.group_of, self.scales, self.wds = n_buf, ranges, list(group_of), list(scales), list(wds)
        assert len(group_of) == len(ranges) and max(group_of) < len(scales) == len(wds) <= 16
        rows = FT.range_table_rows(ranges)
        self.R, self.n = len(rows), sum(hi - lo for lo, hi, _ in ranges)
        self.inside = torch.zeros(n_buf, dtype=torch.bool)
        for lo, hi, _ in ranges:
            self.inside[lo:hi] = True
        self.gen = torch.Generator().manual_seed(seed)
        self.table = torch.tensor(rows, dtype=torch.int64).to(DEV)
        self.garr = i32(group_of)
        self.block = block(scales, wds)
        self.skipped = torch.zeros(3, dtype=torch.int32, device=DEV)
        self.sumsq = torch.zeros(2049, device=DEV)
        p0 = torch.randn(n_buf, generator=self.gen)
        m0 = torch.randn(n_buf, generator=self.gen) * 1e-2
        v0 = torch.rand(n_buf, generator=self.gen) * 1e-3 + 1e-6
        self.p, self.m, self.v = (self._sentinel(t) for t in (p0, m0, v0))
        self.pb = torch.full((n_buf,), SENT16, dtype=torch.int16).view(torch.bfloat16).to(DEV)
        # the reference: one fp64 tensor per range, one torch param group per group, Adam's state preset to (step 0, m0, v0)
        self.ref_p = [p0[lo:hi].double().clone().requires_grad_() for lo, hi, _ in ranges]
        groups = []
        for k in range(len(scales)):
            mine = [q for q, g in zip(self.ref_p, group_of) if g == k]
            if mine:
                groups.append({"params": mine, "lr": LR * scales[k], "weight_decay": wds[k], "group": k})
        self.opt = torch.optim.AdamW(groups, lr=LR, betas=(B1, B2), eps=EPS, foreach=False)
        for q, (lo, hi, _) in zip(self.ref_p, ranges):
            self.opt.state[q] = {"step": torch.tensor(0.0), "exp_avg": m0[lo:hi].double().clone(), "exp_avg_sq": v0[lo:hi].double().clone()}

    def _sentinel(self, t):
        out = torch.full((self.n_buf,), SENT32, dtype=torch.int32).view(torch.float32).clone()
        out[self.inside] = t[self.inside]
        return out.to(DEV)

    def set_values(self, scales, wds):
        """new values: into the device block and into the torch groups"""
        self.scales, self.wds = list(scales), list(wds)
        sub("_lib").call("vqa_group_hyper_set", self.block.data_ptr(), len(scales), floats(scales), floats(wds))
        for g in self.opt.param_groups:
            g["lr"], g["weight_decay"] = LR * scales[g["group"]], wds[g["group"]]

    def grad(self, scale):
        gr = torch.randn(self.n_buf, generator=self.gen) * scale
        gr[~self.inside] = float("nan")
        return gr

    def ref_step(self, gr, *, max_norm=1.0, gscale=1.0):
        """fp64: the global norm, the clip coefficient into the gradients, one optimizer step.  Returns (norm, clip active)."""
        gd = gr.double()
        norm = math.sqrt(float((gd[self.inside] ** 2).sum()))
        c = max_norm / (norm * gscale + 1e-6)
        coef = gscale * (c if c < 1 else 1.0)
        for q, (lo, hi, _) in zip(self.ref_p, self.ranges):
            q.grad = gd[lo:hi] * coef
        self.opt.step()
        return norm, c < 1

    def args(self, gd, *, skip=None, lag=None, frozen=None):
        """what follows `calls` / the state block in every grouped entry, and what precedes it"""
        L = sub("_lib")
        head = (self.p.data_ptr(), gd.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.table.data_ptr(), self.R, self.n)
        nf = 0 if frozen is None else frozen.numel()
        tail = (L.ptr(skip), self.skipped.data_ptr(), L.ptr(lag), L.ptr(frozen), nf, self.pb.data_ptr())
        return head, tail

    def launch(self, gr, calls, *, max_norm=1.0, gscale=1.0, skip=None, lag=None, frozen=None, state=None):
        L = sub("_lib")
        gd = gr.to(DEV)
        L.call("vqa_sumsq_ranges", gd.data_ptr(), self.table.data_ptr(), self.R, self.n, self.sumsq.data_ptr())
        head, tail = self.args(gd, skip=skip, lag=lag, frozen=frozen)
        grp = (self.garr.data_ptr(), self.block.data_ptr())
        if state is None:
            L.call("vqa_adamw_groups", *head, LR, B1, B2, EPS, 123.0, calls, self.sumsq.data_ptr(), max_norm, gscale, *tail, *grp)
        else:                                                       # (the launch's own weight decay, 123, is not used with groups)
            L.call("vqa_adamw_groups_dev", *head, state.data_ptr(), self.sumsq.data_ptr(), *tail, *grp)
        torch.cuda.synchronize()

    def outside_untouched(self):
        o = ~self.inside
        return all(bool((bits(t)[o] == SENT32).all()) for t in (self.p, self.m, self.v)) and bool((bits(self.pb)[o] == SENT16).all())

    def check(self, norm=None, only_group=None):
        if norm is not None:
            ss = float(self.sumsq[0])
            assert math.isfinite(ss)                                # never read: the gradient is NaN outside the ranges
            assert abs(math.sqrt(ss) - norm) / norm < 1e-5
        assert self.outside_untouched()                             # never written
        p, m, v = (t.cpu().double() for t in (self.p, self.m, self.v))
        rp, rm, rv = (torch.zeros(self.n_buf, dtype=torch.float64) for _ in range(3))
        sel = torch.zeros(self.n_buf, dtype=torch.bool)
        for q, (lo, hi, _), g in zip(self.ref_p, self.ranges, self.group_of):
            st = self.opt.state[q]
            rp[lo:hi], rm[lo:hi], rv[lo:hi] = q.detach(), st["exp_avg"], st["exp_avg_sq"]
            if only_group is None or g == only_group:
                sel[lo:hi] = True
        ep = float((p[sel] - rp[sel]).abs().max())
        em = float((m[sel] - rm[sel]).abs().max() / rm[sel].abs().max())
        ev = float((v[sel] - rv[sel]).abs().max() / rv[sel].abs().max())
        print(f"   |dp| {ep:.2e}  dm/max {em:.2e}  dv/max {ev:.2e}")
        assert ep < 2e-6 and em < 1e-5 and ev < 1e-5
        i = self.inside
        assert torch.equal(self.pb.cpu()[i], self.p.cpu()[i].to(torch.bfloat16))      # the bf16 operand copy of the same launch


# ------------------------------------------------------------------------------------ 1. neutral groups are the range kernel
def _ranged_buffers(name, ema, grouped):
    """tests/_optbits.ranged_case's inputs (calls = 1000, lagged step numbers, the clip active, gscale 0.5, warm-up on) through
    vqa_adamw_ranges[_ema] or through vqa_adamw_groups[_ema] with every group at lr_scale 1 and wd = WD; every output buffer."""
    L = sub("_lib")
    n_buf, table, R, n = OB._table(name)
    inside = OB._inside(name)
    p0, m0, v0, _, e0 = OB.state(n_buf)
    nlag = max(j for _, _, j in OB.TABLES[name][1]) + 2
    lag0 = torch.tensor([(990 + 37 * j) % 1000 for j in range(nlag)], dtype=torch.int32)
    bufs = {"p": OB._sentinel(p0, inside), "m": OB._sentinel(m0, inside), "v": OB._sentinel(v0, inside), "p_bf16": OB.sent16(n_buf),
            "lag": lag0.to(DEV), "skipped": OB.i32(0, 0, 0)}
    if ema:
        bufs["ema"] = OB._sentinel(e0, inside)
    gd, skip, frozen, sumsq = OB._grad(name), OB.i32(0), OB.i32(nlag - 1), torch.zeros(2049, device=DEV)
    L.call("vqa_sumsq_ranges", gd.data_ptr(), table.data_ptr(), R, n, sumsq.data_ptr())
    head = (bufs["p"].data_ptr(), gd.data_ptr(), bufs["m"].data_ptr(), bufs["v"].data_ptr(), table.data_ptr(), R, n, OB.LR, OB.B1, OB.B2,
            OB.EPS)
    rest = (1000, sumsq.data_ptr(), OB.CLIPS, OB.GSCALE, skip.data_ptr(), bufs["skipped"].data_ptr(), bufs["lag"].data_ptr(),
            frozen.data_ptr(), 1, bufs["p_bf16"].data_ptr()) + ((bufs["ema"].data_ptr(), OB.DECAY, 1) if ema else ())
    if grouped:
        garr = i32(r % 16 for r in range(R))
        blk = block([1.0] * 16, [OB.WD] * 16)
        L.call("vqa_adamw_groups" + ("_ema" if ema else ""), *head, 55.0, *rest, garr.data_ptr(), blk.data_ptr())
    else:
        L.call("vqa_adamw_ranges" + ("_ema" if ema else ""), *head, OB.WD, *rest)
    torch.cuda.synchronize()
    return {k: bits(t) for k, t in bufs.items()}


@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("name", ["gaps-4-8-end", "r512"])
def test_neutral_groups_give_the_range_kernels_bits(name, ema):
    a, b = _ranged_buffers(name, ema, False), _ranged_buffers(name, ema, True)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k                           # p, m, v, bf16 copy, (ema,) lag, skipped: sentinels included
    inside = OB._inside(name)
    assert not torch.equal(a["p"][inside], bits(OB.state(OB.TABLES[name][0])[0])[inside])      # (and the launch did update)
    assert a["skipped"].tolist() == [0, 0, 0] and int(a["lag"][-1]) == (990 + 37 * (a["lag"].numel() - 1)) % 1000 + 1


# ------------------------------------------------------------------------------------------- 2. fp64 per group, three steps
CASES = [("gaps-4-8-end", [0, 1, 0], 2), ("r512", [r % 5 for r in range(512)], 5), ("r512", [r % 16 for r in range(512)], 16)]


@pytest.mark.parametrize("rot", [0, 2])
@pytest.mark.parametrize("clip_active", [True, False])
@pytest.mark.parametrize("name,group_of,G", CASES, ids=["gaps-4-8-end", "r512-mod5", "r512-mod16"])
def test_groups_match_fp64_adamw_per_group(name, group_of, G, clip_active, rot):
    n_buf, ranges = TABLES[name]
    scales, wds = values(G, rot)
    s = GState(n_buf, ranges, group_of, scales, wds, seed=len(name) + G)
    gscale = 0.5 if clip_active else 1.0
    for t in (1, 2, 3):
        gr = s.grad(0.2 if clip_active else 1e-4)
        norm, active = s.ref_step(gr, gscale=gscale)
        assert bool(active) == clip_active
        s.launch(gr, t, gscale=gscale)
        s.check(norm)


def test_every_scale_and_decay_is_exercised():
    used = set()
    for _, group_of, G in CASES:
        for rot in (0, 2):
            sc, wd = values(G, rot)
            used |= {(sc[g], wd[g]) for g in set(group_of)}
    assert {a for a, _ in used} == {0.0, 0.1, 1.0, 10.0} and {b for _, b in used} == {0.0, 0.01, 0.1}


# ------------------------------------------------------------------------------------------------ 3. a second grid trip
def test_two_groups_over_a_second_grid_trip():
    n_buf, ranges = TABLES["two-trips"]
    s = GState(n_buf, ranges, [0, 1, 0], [0.1, 10.0], [0.1, 0.0], seed=3)
    assert s.n == 4_194_304 + 4_000 and s.inside[-1]
    gr = s.grad(2e-3)                                               # norm 4.1, 2.05 after the gradient scale: the clip is active
    norm, active = s.ref_step(gr, gscale=0.5)
    assert active
    s.launch(gr, 1, gscale=0.5)
    s.check(norm)


# ------------------------------------------------------------------------------------------------------- 4. lr_scale = 0
def test_lr_scale_zero_keeps_the_parameter_and_moves_the_moments():
    n_buf, ranges = TABLES["gaps-4-8-end"]
    s = GState(n_buf, ranges, [0, 1, 0], [1.0, 0.0], [0.01, 0.1], seed=4)
    before = [bits(t).clone() for t in (s.p, s.m, s.v)]
    gr = s.grad(1e-4)
    norm, _ = s.ref_step(gr)
    s.launch(gr, 1)
    lo, hi, _ = ranges[1]                                           # the range of group 1
    assert torch.equal(bits(s.p)[lo:hi], before[0][lo:hi])          # lr 0: not a bit of p moves, weight decay 0.1 or not
    assert not torch.equal(bits(s.m)[lo:hi], before[1][lo:hi]) and not torch.equal(bits(s.v)[lo:hi], before[2][lo:hi])
    assert torch.equal(s.pb.cpu()[lo:hi], s.p.cpu()[lo:hi].to(torch.bfloat16))
    s.check(norm)                                                   # both groups follow fp64 (moments of group 1 included)
    s.check(only_group=0)
    lo0, hi0, _ = ranges[0]
    assert not torch.equal(bits(s.p)[lo0:hi0], before[0][lo0:hi0])


# -------------------------------------------------------------------------------------------------- 5. a skipped launch
def test_a_skipped_launch_changes_nothing_but_skipped():
    n_buf, ranges = TABLES["gaps-4-8-end"]
    s = GState(n_buf, ranges, [0, 1, 0], [1.0, 0.1], [0.01, 0.0], seed=5)
    lag = torch.zeros(4, dtype=torch.int32, device=DEV)
    frozen = i32([3])
    gr = s.grad(1e-4)
    norm, _ = s.ref_step(gr)
    s.launch(gr, 1, lag=lag, frozen=frozen)
    s.check(norm)
    assert lag.tolist() == [0, 0, 0, 1]
    s.skipped.copy_(torch.tensor([5, 3, 0], dtype=torch.int32))
    before = [bits(t).clone() for t in (s.p, s.m, s.v, s.pb, lag)]
    s.launch(s.grad(1e-4), 2, skip=i32([2]), lag=lag, frozen=frozen)
    for a, b in zip(before, (s.p, s.m, s.v, s.pb, lag)):
        assert torch.equal(a, bits(b))                              # bit-unchanged (sentinels included)
    assert s.skipped.tolist() == [5 + 2, 3 + 1, 0 + 1]
    gr = s.grad(1e-4)                                               # the next applied launch is Adam step 2, not 3
    norm, _ = s.ref_step(gr)
    s.launch(gr, 3, skip=i32([0]), lag=lag, frozen=frozen)
    s.check(norm)
    assert lag.tolist() == [0, 0, 0, 2] and s.skipped.tolist() == [7, 4, 1]


# ------------------------------------------------------------------------------------------------------ 6. the _dev entries
def _state_block(calls, *, max_norm, gscale, ema_decay=0.0, ema_warmup=0):
    st = torch.zeros(sub("stepgraph").STATE_BYTES // 4, device=DEV, dtype=torch.int32)
    sub("_lib").call("vqa_step_state_set", st.data_ptr(), calls, 0, LR, B1, B2, EPS, 123.0, max_norm, gscale, ema_decay, ema_warmup)
    return st


@pytest.mark.parametrize("ema", [False, True])
def test_dev_entries_give_the_by_value_entries_bits(ema):
    L = sub("_lib")
    name = "r512"
    n_buf, ranges = TABLES[name]
    scales, wds = values(16, 1)
    out = {}
    for dev in (False, True):
        s = GState(n_buf, ranges, [r % 16 for r in range(512)], scales, wds, seed=6)
        lag = i32((7 * j) % 5 for j in range(513))
        frozen, skip = i32([512]), i32([0])                         # (named: the entries get raw pointers, the tensors must outlive the launch)
        e = s._sentinel(torch.randn(n_buf, generator=torch.Generator().manual_seed(60)))
        gd = s.grad(0.2).to(DEV)
        L.call("vqa_sumsq_ranges", gd.data_ptr(), s.table.data_ptr(), s.R, s.n, s.sumsq.data_ptr())
        head, tail = s.args(gd, skip=skip, lag=lag, frozen=frozen)
        grp = (s.garr.data_ptr(), s.block.data_ptr())
        if dev:
            st = _state_block(9, max_norm=1.0, gscale=0.5, ema_decay=0.99 if ema else 0.0, ema_warmup=int(ema))
            L.call("vqa_adamw_groups_ema_dev" if ema else "vqa_adamw_groups_dev", *head, st.data_ptr(), s.sumsq.data_ptr(), *tail,
                   *((e.data_ptr(),) if ema else ()), *grp)
        else:
            L.call("vqa_adamw_groups_ema" if ema else "vqa_adamw_groups", *head, LR, B1, B2, EPS, 123.0, 9, s.sumsq.data_ptr(), 1.0, 0.5,
                   *tail, *((e.data_ptr(), 0.99, 1) if ema else ()), *grp)
        torch.cuda.synchronize()
        assert s.outside_untouched()
        out[dev] = [bits(t) for t in (s.p, s.m, s.v, s.pb, e, lag, s.skipped)]
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)
    assert out[True][5][512] == (7 * 512) % 5 + 1                   # the lag of the frozen parameter advanced
    if ema:
        i = torch.zeros(n_buf, dtype=torch.bool)
        for lo, hi, _ in ranges:
            i[lo:hi] = True
        assert bool((out[True][4][~i] == SENT32).all()) and not bool((out[True][4][i] == SENT32).any())


def test_dev_entry_follows_a_rewritten_block():
    n_buf, ranges = TABLES["gaps-4-8-end"]
    s = GState(n_buf, ranges, [0, 1, 0], [1.0, 0.1], [0.01, 0.0], seed=7)
    for t, vals in ((1, None), (2, ([0.1, 10.0], [0.1, 0.01]))):
        if vals is not None:
            s.set_values(*vals)                                     # vqa_group_hyper_set between the two launches
        gr = s.grad(0.2)
        norm, active = s.ref_step(gr, gscale=0.5)
        assert active
        s.launch(gr, t, gscale=0.5, state=_state_block(t, max_norm=1.0, gscale=0.5))
        s.check(norm)
    blk = sub("stepgraph").GroupHyper.from_buffer_copy(s.block.cpu().numpy().tobytes())
    f32 = lambda x: torch.tensor(x, dtype=torch.float32).item()
    assert list(blk.lr_scale) == [f32(0.1), 10.0] + [0.0] * 14 and list(blk.wd) == [f32(0.1), f32(0.01)] + [0.0] * 14


# -------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_everything_untouched():
    L = sub("_lib")
    n_buf = 4096
    bufs = [torch.full((n_buf,), 2.0, device=DEV) for _ in range(5)]
    p, g, m, v, e = bufs
    ss = torch.full((2049,), 3.0, device=DEV)
    lag = torch.zeros(4, dtype=torch.int32, device=DEV)
    frozen = i32([1])
    table = torch.tensor([[8 * r, 8 * r + 4, 4 * r, 0] for r in range(513)], dtype=torch.int64, device=DEV)
    garr = torch.zeros(513, dtype=torch.int32, device=DEV)
    blk = torch.full((36,), 0x40000000, dtype=torch.int32, device=DEV)             # 2.0f in every word
    st = _state_block(1, max_norm=1.0, gscale=1.0)
    one = floats([1.0] * 17)

    # vqa_group_hyper_set: G = 0 or 17, a null or misaligned block, a null array, a NaN, infinite or negative scale or decay
    for G in (0, 17):
        with pytest.raises(RuntimeError):
            L.call("vqa_group_hyper_set", blk.data_ptr(), G, one, one)
    for bad_ptr in (None, blk.data_ptr() + 4, blk.data_ptr() + 8):
        with pytest.raises(RuntimeError):
            L.call("vqa_group_hyper_set", bad_ptr, 2, one, one)
    with pytest.raises(RuntimeError):
        L.call("vqa_group_hyper_set", blk.data_ptr(), 2, None, one)
    with pytest.raises(RuntimeError):
        L.call("vqa_group_hyper_set", blk.data_ptr(), 2, one, None)
    for bad in (float("nan"), -1.0, float("inf"), -0.5):
        for k in (0, 2):
            vals = [1.0, 1.0, 1.0]
            vals[k] = bad
            with pytest.raises(RuntimeError):
                L.call("vqa_group_hyper_set", blk.data_ptr(), 3, floats(vals), one)
            with pytest.raises(RuntimeError):
                L.call("vqa_group_hyper_set", blk.data_ptr(), 3, one, floats(vals))
    L.call("vqa_group_hyper_set", blk.data_ptr(), 2, floats([1.0, 1.0, float("nan")]), one)     # (only G values are read)
    torch.cuda.synchronize()
    assert blk.view(torch.float32)[:32].tolist() == [1.0, 1.0] + [0.0] * 14 + [1.0, 1.0] + [0.0] * 14
    assert (blk[32:] == 0x40000000).all()                           # 128 bytes, no more
    blk.fill_(0x40000000)

    def adamw(sfx, R, n, calls=1, lag_=lag, frozen_=None, nf=0, garr_=garr, blk_=blk.data_ptr(), ema_=e, decay=0.9):
        hyper = (st.data_ptr(),) if "dev" in sfx else (LR, B1, B2, EPS, WD, calls)
        tail = () if "dev" in sfx else (1.0, 1.0)
        ema_args = () if "ema" not in sfx else ((L.ptr(ema_),) if "dev" in sfx else (L.ptr(ema_), decay, 0))
        L.call("vqa_adamw_groups" + sfx, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), table.data_ptr(), R, n, *hyper,
               ss.data_ptr(), *tail, None, None, L.ptr(lag_), L.ptr(frozen_), nf, None, *ema_args, L.ptr(garr_), blk_)

    for sfx in ("", "_ema", "_dev", "_ema_dev"):
        for R, n in ((513, 513 * 4), (1, 6), (0, 4)):               # too many ranges, n % 4 != 0, no table for n > 0
            with pytest.raises(RuntimeError):
                adamw(sfx, R, n)
        with pytest.raises(RuntimeError):
            adamw(sfx, 1, 4, lag_=None, frozen_=frozen, nf=1)       # frozen parameters need the lag table they advance
        with pytest.raises(RuntimeError):
            adamw(sfx, 1, 4, garr_=None)                            # a null group_of_range
        with pytest.raises(RuntimeError):
            adamw(sfx, 1, 4, blk_=None)                             # a null block
        with pytest.raises(RuntimeError):
            adamw(sfx, 1, 4, blk_=blk.data_ptr() + 8)               # a misaligned block
        if "dev" not in sfx:
            with pytest.raises(RuntimeError):
                adamw(sfx, 1, 4, calls=0)                           # Adam's step number starts at 1
        if "ema" in sfx:
            with pytest.raises(RuntimeError):
                adamw(sfx, 1, 4, ema_=None)
    with pytest.raises(RuntimeError):
        adamw("_ema", 1, 4, decay=1.5)
    torch.cuda.synchronize()
    assert all((t == 2.0).all() for t in bufs) and (ss == 3.0).all() and (lag == 0).all() and (blk == 0x40000000).all()
    # the empty table is a valid step over nothing
    for sfx in ("", "_ema", "_dev", "_ema_dev"):
        adamw(sfx, 0, 0)
    torch.cuda.synchronize()
    assert all((t == 2.0).all() for t in bufs) and (lag == 0).all()
