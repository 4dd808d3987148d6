"""GPU: the weight average inside the optimizer launches (vqa_adamw_ema, vqa_adamw_ranges_ema) and alone (vqa_ema_update),
csrc/optim_ops.hip.

Per case: the parameters, both moments and the bf16 operand copy are BIT-equal to what vqa_adamw / vqa_adamw_ranges give on a twin state
(adding the average must not reorder or contract the optimizer arithmetic); the average follows the float64 reference (tests/_emaref.py)
fed with the kernel's own parameters after each step, within 2^-22 * max(|ema|, |p|) per update (derived and summed there); a skipped
launch leaves all five buffers bit-identical and advances no warm-up; with a range table nothing outside the ranges is read (NaN
gradients) or written (sentinel bit patterns), and each range warms up at its own step number; the stand-alone pass gives the bits
of the fused launch; bad arguments are refused with status 1000 before anything is launched."""
import pytest
import torch

import _emaref as R
from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01
DECAY = 0.999
SENT32, SENT16 = 0x7FA5A5A5, 0x7FA5                                 # NaN bit patterns: reading one poisons, writing one shows

# (tests/test_gpu_optimizer_ranges.py's tables, re-declared)
BIG = [(400_000, 1_900_000, 0), (2_200_000, 4_200_000, 1), (4_549_696, 5_248_000, 2)]        # 4 194 304 + 4 000 trainable elements
TABLES = {
    "whole": (4096, [(0, 4096, 0)]),
    "interior": (4096, [(1000, 3004, 0)]),
    "gaps-4-8-end": (4000, [(8, 1000, 0), (1004, 2000, 1), (2008, 4000, 2)]),
    "r512": (4096, [(8 * r, 8 * r + 4, r) for r in range(512)]),   # the largest table, the deepest binary search
    "two-trips": (5_248_000, BIG),                                  # > 4096 blocks x 256 threads x 4 elements: a second grid trip
}


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def i32(*v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ plain variant
class Plain:
    """Flat optimizer state on the device; `ema` is None for the twin that runs the existing entry."""

    def __init__(self, n, p0, m0, v0, ema0, copy):
        self.n = n
        self.p, self.m, self.v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
        self.ema = None if ema0 is None else ema0.to(DEV)
        self.pb = torch.full((n,), SENT16, dtype=torch.int16).view(torch.bfloat16).to(DEV) if copy else None
        self.skipped = torch.zeros(3, dtype=torch.int32, device=DEV)
        self.sumsq = torch.zeros(2049, device=DEV)

    def buffers(self):
        return [t for t in (self.p, self.m, self.v, self.pb, self.ema) if t is not None]

    def launch(self, gd, calls, skip, warmup=0, decay=DECAY):
        L = sub("_lib")
        L.call("vqa_sumsq", gd.data_ptr(), self.n, self.sumsq.data_ptr())
        args = (self.p.data_ptr(), gd.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n, LR, B1, B2, EPS, WD, calls,
                self.sumsq.data_ptr(), 1.0, 1.0, skip.data_ptr(), self.skipped.data_ptr(), L.ptr(self.pb))
        if self.ema is None:
            L.call("vqa_adamw", *args)
        else:
            L.call("vqa_adamw_ema", *args, self.ema.data_ptr(), decay, warmup)
        torch.cuda.synchronize()


def _plain_states(n, copy, seed):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    m0 = torch.randn(n, generator=g) * 1e-2
    v0 = torch.rand(n, generator=g) * 1e-3 + 1e-6
    ema0 = p0 + 0.05 * torch.randn(n, generator=g)                  # an average some way from the weights: a wrong decay shows
    return g, ema0, Plain(n, p0, m0, v0, None, copy), Plain(n, p0, m0, v0, ema0, copy)


@pytest.mark.parametrize("warmup", [0, 1])
@pytest.mark.parametrize("copy", [False, True])
@pytest.mark.parametrize("n", [4096, 4103, 4096 * 256 + 1028])       # one trip, an odd tail, more than one grid trip
def test_plain_variant_optimizer_bits_and_average(n, copy, warmup):
    g, ema0, a, b = _plain_states(n, copy, seed=n % 97 + 2 * warmup + copy)
    ref = R.Tracker(ema0)
    k = 0
    for calls, skip_rows in ((1, 0), (2, 0), (3, 2), (4, 0)):        # applied, applied, SKIPPED, applied: Adam steps 1, 2, -, 3
        gd = (torch.randn(n, generator=g) * 0.05).to(DEV)           # norm > 3: the clip is active
        skip = i32(skip_rows)
        before = [t.clone() for t in b.buffers()]
        a.launch(gd, calls, skip)
        b.launch(gd, calls, skip, warmup=warmup)
        for x, y in zip(a.buffers(), b.buffers()):                  # p, m, v (and the bf16 copy): the existing kernel's bits
            assert same_bits(x, y)
        assert a.skipped.tolist() == b.skipped.tolist()
        if skip_rows:
            for x, y in zip(before, b.buffers()):                   # all five buffers bit-identical
                assert same_bits(x, y)
            assert b.skipped.tolist() == [2, 1, 1]
            continue
        k += 1                                                      # Adam's step number: the skipped launch did not count
        ref.step(b.p.cpu(), DECAY, bool(warmup), k).check(b.ema.cpu(), f"n={n} step {k}")
    assert k == 3 and ref.k == 3
    if copy:
        assert torch.equal(b.pb, b.p.to(torch.bfloat16))
    if warmup:                                                      # the warm-up moved the average far more than the bound: 2/11 is not 0.999
        cold = R.replay(ema0, [b.p.cpu()] * 3, DECAY, False)
        assert float((ref.ema - cold).abs().max()) > 1e3 * float(ref.err.max())


# ------------------------------------------------------------------------------------------------ ranges variant
class Ranged:
    """test_gpu_optimizer_ranges.State's buffers: NaN gradients and sentinel bit patterns outside the ranges."""

    def __init__(self, n_buf, ranges, p0, m0, v0, ema0, lag0):
        FT = sub("finetune")
        self.n_buf, self.ranges = n_buf, ranges
        rows = FT.range_table_rows(ranges)
        self.R, self.n = len(rows), sum(hi - lo for lo, hi, _ in ranges)
        self.inside = torch.zeros(n_buf, dtype=torch.bool)
        for lo, hi, _ in ranges:
            self.inside[lo:hi] = True
        self.table = torch.tensor(rows, dtype=torch.int64).to(DEV)
        self.lag = lag0.clone().to(DEV)
        self.skipped = torch.zeros(3, dtype=torch.int32, device=DEV)
        self.sumsq = torch.zeros(2049, device=DEV)
        self.p, self.m, self.v = (self._sentinel(t) for t in (p0, m0, v0))
        self.ema = None if ema0 is None else self._sentinel(ema0)
        self.pb = torch.full((n_buf,), SENT16, dtype=torch.int16).view(torch.bfloat16).to(DEV)

    def _sentinel(self, t):
        out = torch.full((self.n_buf,), SENT32, dtype=torch.int32).view(torch.float32).clone()
        out[self.inside] = t[self.inside]
        return out.to(DEV)

    def buffers(self):
        return [t for t in (self.p, self.m, self.v, self.pb, self.lag, self.ema) if t is not None]

    def outside_untouched(self):
        o = ~self.inside
        f32 = [t for t in (self.p, self.m, self.v, self.ema) if t is not None]
        return all(bool((t.cpu().view(torch.int32)[o] == SENT32).all()) for t in f32) and \
            bool((self.pb.cpu().view(torch.int16)[o] == SENT16).all())

    def launch(self, gd, calls, skip, frozen, warmup=0):
        L = sub("_lib")
        L.call("vqa_sumsq_ranges", gd.data_ptr(), self.table.data_ptr(), self.R, self.n, self.sumsq.data_ptr())
        args = (self.p.data_ptr(), gd.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.table.data_ptr(), self.R, self.n, LR, B1, B2,
                EPS, WD, calls, self.sumsq.data_ptr(), 1.0, 1.0, skip.data_ptr(), self.skipped.data_ptr(), self.lag.data_ptr(),
                L.ptr(frozen), 0 if frozen is None else frozen.numel(), self.pb.data_ptr())
        if self.ema is None:
            L.call("vqa_adamw_ranges", *args)
        else:
            L.call("vqa_adamw_ranges_ema", *args, self.ema.data_ptr(), DECAY, warmup)
        torch.cuda.synchronize()


@pytest.mark.parametrize("name,warmup", [("interior", 0), ("interior", 1), ("gaps-4-8-end", 0), ("gaps-4-8-end", 1), ("r512", 1),
                                         ("two-trips", 1)])
def test_ranges_variant_touches_nothing_outside_and_warms_up_per_range(name, warmup):
    n_buf, ranges = TABLES[name]
    g = torch.Generator().manual_seed(len(name) + warmup)
    p0 = torch.randn(n_buf, generator=g)
    m0 = torch.randn(n_buf, generator=g) * 1e-2
    v0 = torch.rand(n_buf, generator=g) * 1e-3 + 1e-6
    ema0 = p0 + 0.05 * torch.randn(n_buf, generator=g)
    nlag = max(j for _, _, j in ranges) + 2                         # one more parameter: the frozen one, whose lag advances
    lag0 = (torch.arange(nlag, dtype=torch.int32) * 2) % 3          # lags 0, 2, 1, 0, ...: neighbouring ranges at different steps
    frozen = i32(nlag - 1)
    a = Ranged(n_buf, ranges, p0, m0, v0, None, lag0)
    b = Ranged(n_buf, ranges, p0, m0, v0, ema0, lag0)
    ref = R.Tracker(ema0)
    i = b.inside
    t0 = 2                                                          # calls start at 3: every range's step number is >= 1
    k = 0
    for calls, skip_rows in ((3, 0), (4, 0), (5, 1), (6, 0)):
        gr = torch.randn(n_buf, generator=g) * 0.01
        gr[~i] = float("nan")                                       # never read outside the ranges
        gd = gr.to(DEV)
        skip = i32(skip_rows)
        before = [t.clone() for t in b.buffers()]
        a.launch(gd, calls, skip, frozen)
        b.launch(gd, calls, skip, frozen, warmup=warmup)
        for x, y in zip(a.buffers(), b.buffers()):                  # p, m, v, bf16 copy, lag: vqa_adamw_ranges' bits (sentinels included)
            assert same_bits(x, y)
        assert b.outside_untouched()                                # the average too: neither read nor written outside
        assert a.skipped.tolist() == b.skipped.tolist()
        if skip_rows:
            for x, y in zip(before, b.buffers()):
                assert same_bits(x, y)
            continue
        t0 += 1
        k += 1
        steps = [t0 - int(lag0[j]) for _, _, j in ranges]           # each range at its OWN step number
        assert min(steps) >= 1 and (len(ranges) == 1 or len(set(steps)) > 1)
        ref.step_ranges(b.p.cpu(), ranges, steps, DECAY, bool(warmup))
        assert bool(torch.isfinite(b.ema.cpu()[i]).all())
        ref.check(b.ema.cpu(), f"{name} step {k}", sel=i)
    assert k == 3 and b.skipped.tolist() == [1, 1, 1] and int(b.lag[nlag - 1]) == int(lag0[nlag - 1]) + 3
    if warmup and len(ranges) > 1:                                  # a shared step number would be far outside the bound
        shared = R.replay(ema0, [b.p.cpu()] * 3, DECAY, True, steps=[3, 4, 5])
        assert float((ref.ema - shared)[i].abs().max()) > 1e2 * float(ref.err[i].max())


# ------------------------------------------------------------------------------------------------ stand-alone pass
@pytest.mark.parametrize("n,off", [(4096, 0), (4103, 0), (4103, 1), (4096 * 256 * 4 + 1031, 0)])
def test_stand_alone_pass_gives_the_fused_launch_its_bits(n, off):
    """vqa_ema_update(ema0, p_after, d) == the average a fused launch produced from the same ema0 (warm-up off).  off = 1: pointers
    that are not 16-byte aligned (the scalar route of the stand-alone pass); the last n: a second trip of its float4 loop."""
    L = sub("_lib")
    g = torch.Generator().manual_seed(n % 89 + off)
    N = n + off
    p, m, v = torch.randn(N, generator=g).to(DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    ema0 = (torch.randn(N, generator=g)).to(DEV)
    gd = (torch.randn(N, generator=g) * 1e-3).to(DEV)
    fused = ema0.clone()
    sl = lambda t: t[off:].data_ptr()
    L.call("vqa_adamw_ema", sl(p), sl(gd), sl(m), sl(v), n, LR, B1, B2, EPS, WD, 1, None, 0.0, 1.0, None, None, None, sl(fused), DECAY, 0)
    alone = ema0.clone()
    L.call("vqa_ema_update", sl(alone), sl(p), n, DECAY)
    torch.cuda.synchronize()
    assert same_bits(alone, fused)
    assert not same_bits(fused[off:], ema0[off:]) and same_bits(fused[:off], ema0[:off])
    R.Tracker(ema0.cpu()[off:]).step(p.cpu()[off:], DECAY, False, 1).check(alone.cpu()[off:], f"alone n={n}")


def test_stand_alone_pass_matches_the_ranges_variant_and_the_decay_ends():
    L = sub("_lib")
    n = 4096
    g = torch.Generator().manual_seed(4)
    p, m, v = torch.randn(n, generator=g).to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ema0 = torch.randn(n, generator=g).to(DEV)
    gd = (torch.randn(n, generator=g) * 1e-3).to(DEV)
    table = torch.tensor(sub("finetune").range_table_rows(TABLES["whole"][1]), dtype=torch.int64).to(DEV)
    fused = ema0.clone()
    L.call("vqa_adamw_ranges_ema", p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), table.data_ptr(), 1, n, LR, B1, B2, EPS, WD, 1,
           None, 0.0, 1.0, None, None, None, None, 0, None, fused.data_ptr(), DECAY, 0)
    alone = ema0.clone()
    L.call("vqa_ema_update", alone.data_ptr(), p.data_ptr(), n, DECAY)
    keep, follow = ema0.clone(), ema0.clone()
    L.call("vqa_ema_update", keep.data_ptr(), p.data_ptr(), n, 1.0)  # d = 1: the average stays, d = 0: it becomes the parameters
    L.call("vqa_ema_update", follow.data_ptr(), p.data_ptr(), n, 0.0)
    torch.cuda.synchronize()
    assert same_bits(alone, fused)
    assert same_bits(keep, ema0) and same_bits(follow, p)


# ------------------------------------------------------------------------------------------------ status
def test_refusals_launch_nothing():
    L = sub("_lib")
    n = 4096
    p, gd, m, v, ema = (torch.full((n,), 2.0, device=DEV) for _ in range(5))
    table = torch.tensor([[0, n, 0, 0]], dtype=torch.int64, device=DEV)
    skipped = torch.zeros(3, dtype=torch.int32, device=DEV)

    def plain(e, d, n_=n):
        L.call("vqa_adamw_ema", p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n_, LR, B1, B2, EPS, WD, 1, None, 0.0, 1.0, None,
               skipped.data_ptr(), None, e, d, 0)

    def ranged(e, d, n_=n):
        L.call("vqa_adamw_ranges_ema", p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), table.data_ptr(), 1, n_, LR, B1, B2, EPS, WD,
               1, None, 0.0, 1.0, None, skipped.data_ptr(), None, None, 0, None, e, d, 0)

    def alone(e, d, n_=n):
        L.call("vqa_ema_update", e, p.data_ptr(), n_, d)

    for fn in (plain, ranged, alone):
        for e, d, n_ in ((None, 0.9, n), (ema.data_ptr(), 1.5, n), (ema.data_ptr(), float("nan"), n), (ema.data_ptr(), -0.25, n),
                         (ema.data_ptr(), 0.9, -4)):
            with pytest.raises(RuntimeError, match="status 1000"):
                fn(e, d, n_)
    with pytest.raises(RuntimeError, match="status 1000"):
        L.call("vqa_ema_update", ema.data_ptr(), None, n, 0.9)
    torch.cuda.synchronize()
    assert all(bool((t == 2.0).all()) for t in (p, gd, m, v, ema)) and skipped.tolist() == [0, 0, 0]
