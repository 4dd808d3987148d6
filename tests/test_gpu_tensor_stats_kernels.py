"""GPU: vqa_tensor_stats (csrc/stats_ops.hip) against the float64 reference of tests/_statsref.py.

One table serves every test: rows of numel 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, CHUNK - 1, CHUNK, CHUNK + 1 and
3 * CHUNK + 5 at 8-aligned offsets, as layout.py lays parameters out.  The padding between the rows and a guard band on both ends
hold NaN and +inf alternately: a read outside a row shows up in `nonfinite` (and, in the pair form, as inf - inf).
sumsq is compared exactly where the data make every partial sum an integer below 2^24, else within N_add * 2^-24 relative of the
float64 sum -- the kernel's own chain of roundings (_statsref.n_add), derived from numel and VQA_STATS_CHUNK, not measured; the counts
and absmax are exact everywhere.  Every test fails without the entry (AttributeError)."""
import pytest
import torch

import _statsref as R
from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
_CACHE = {}


def _K():
    return sub("kernels")


def _numels():
    C = _K().STATS_CHUNK
    return [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, C - 1, C, C + 1, 3 * C + 5]


def _ranges():
    out, off = [], GUARD
    for n in _numels():
        out.append((off, off + n))
        off += (n + 7) // 8 * 8
    return out


def _size():
    return _ranges()[-1][1] + 7 + GUARD


def _table():
    if "table" not in _CACHE:
        _CACHE["table"] = _K().stats_table(_ranges(), DEV)
    return _CACHE["table"]


def _inside():
    """bool mask of the elements that belong to a row"""
    if "inside" not in _CACHE:
        m = torch.zeros(_size(), dtype=torch.bool, device=DEV)
        for lo, hi in _ranges():
            m[lo:hi] = True
        _CACHE["inside"] = m
    return _CACHE["inside"]


def _poison():
    if "poison" not in _CACHE:
        p = torch.full((_size(),), float("nan"), device=DEV)
        p[1::2] = float("inf")
        _CACHE["poison"] = p
    return _CACHE["poison"]


def _buffer(values):
    """`values` inside the rows, NaN / +inf everywhere else"""
    return torch.where(_inside(), values.to(DEV, torch.float32), _poison())


def _randn(seed, sigma):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(_size(), generator=g) * sigma


def _ints(seed, lo=-3, hi=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, (_size(),), generator=g).float()


def _check(words, x, y=None, exact=False, what="", ranges=None):
    """counts and absmax exact; sumsq exact or within the kernel's bound.  Returns the worst observed fraction of the bound."""
    ranges = ranges or _ranges()
    got, ref = R.unpack(words), R.table(x, ranges, y)
    C = _K().STATS_CHUNK
    assert torch.equal(got["nonfinite"], ref["nonfinite"]), (what, got["nonfinite"].tolist(), ref["nonfinite"].tolist())
    assert torch.equal(got["zeros"], ref["zeros"]), (what, got["zeros"].tolist(), ref["zeros"].tolist())
    assert torch.equal(got["absmax"].double(), ref["absmax"]), (what, got["absmax"].tolist(), ref["absmax"].tolist())
    worst = 0.0
    if exact:
        assert torch.equal(got["sumsq"].double(), ref["sumsq"]), (what, got["sumsq"].tolist(), ref["sumsq"].tolist())
        return worst
    for j, (lo, hi) in enumerate(ranges):
        g, r = float(got["sumsq"][j]), float(ref["sumsq"][j])
        bound = R.sumsq_bound(hi - lo, C, pair=y is not None)
        err = abs(g - r) / r if r else abs(g)
        print(f"{what} row {j} numel {hi - lo}: rel err {err:.3e} = {err / bound:.4f} of the bound {bound:.3e}")
        assert err <= bound, (what, j, hi - lo, g, r, err, bound)
        worst = max(worst, err / bound)
    return worst


# ------------------------------------------------------------------------------------------------------------------ exact sums
@pytest.mark.parametrize("pair", [False, True])
def test_small_integers_sum_exactly(pair):
    """Inputs in {-3 ... 3} (differences in {-6 ... 6}): every partial sum is an integer below 2^24, exact in fp32 in any order, so a
    dropped, doubled or misassigned element changes a value -- which the rounding bound would hide on a long row."""
    x = _buffer(_ints(1))
    y = _buffer(_ints(2)) if pair else None
    _check(_K().tensor_stats(x, _table(), y), x, y, exact=True, what="ints")


# ------------------------------------------------------------------------------------------------------------- one-hot sweep
def _positions(n):
    C = _K().STATS_CHUNK
    pos = {0, n - 1, n - (n % 4) - 1, n - (n % 4)}                         # first, last, both sides of the scalar tail's start
    for b in (4, 8):
        pos |= {b - 1, b}
    for b in range(256, n + 1, 256):                                       # every 256-element boundary (1024: a wave's span, C: a chunk)
        pos |= {b - 1, b}
    for b in range(C, n + 1, C):
        pos |= {b - 4, b - 1, b, b + 3, b + 4}
    return sorted(p for p in pos if 0 <= p < n)


@pytest.mark.parametrize("pair", [False, True])
def test_one_hot_sweep(pair):
    """All zeros but a single 1 per row, walked through the first and last element, both sides of 4-element, 256-element and chunk
    boundaries and the scalar tail: sumsq == 1, absmax == 1, zeros == numel - 1 at every position."""
    K, ranges = _K(), _ranges()
    per_row = [_positions(hi - lo) for lo, hi in ranges]
    L = max(len(p) for p in per_row)
    flat_pos = torch.tensor([[lo + p[min(l, len(p) - 1)] for (lo, _), p in zip(ranges, per_row)] for l in range(L)], device=DEV)
    x = _buffer(torch.zeros(_size()))
    y = _buffer(torch.zeros(_size())) if pair else None
    outs = torch.empty((L, len(ranges), 4), device=DEV, dtype=torch.int32)
    for l in range(L):
        x[flat_pos[l]] = 1.0
        K.tensor_stats(x, _table(), y, out=outs[l])
        x[flat_pos[l]] = 0.0
    w = outs.cpu()
    f = w[..., :2].contiguous().view(torch.float32)
    numel = torch.tensor([hi - lo for lo, hi in ranges], dtype=torch.int32)
    bad = ((f[..., 0] != 1) | (f[..., 1] != 1) | (w[..., 2] != 0) | (w[..., 3] != numel - 1)).nonzero().tolist()
    assert not bad, [(l, j, per_row[j][min(l, len(per_row[j]) - 1)], w[l, j].tolist()) for l, j in bad[:8]]


# ------------------------------------------------------------------------------------------------------------------ rounding
@pytest.mark.parametrize("sigma", [0.02, 1e3])
def test_normal_data_within_the_derived_bound(sigma):
    x = _buffer(_randn(3, sigma))
    w1 = _check(_K().tensor_stats(x, _table()), x, what=f"sigma {sigma}")
    y = _buffer(_randn(4, sigma))
    w2 = _check(_K().tensor_stats(x, _table(), y), x, y, what=f"sigma {sigma} pair")
    print(f"worst fraction of the bound, sigma {sigma}: {max(w1, w2):.4f}")


# ------------------------------------------------------------------------------------------------------------ planted values
def _plant(v, value, where):
    C = _K().STATS_CHUNK
    for lo, hi in _ranges():
        n = hi - lo
        spots = {"first": [0], "last": [n - 1], "tail": [n - (n % 4)] if n % 4 else [], "edge": [p for p in (C - 1, C, 2 * C) if p < n]}[where]
        for p in spots:
            v[lo + p] = value


@pytest.mark.parametrize("where", ["first", "last", "tail", "edge"])
def test_planted_nan_inf_and_negative_zero(where):
    """NaN, +inf, -inf and -0.0 at the first element, the last, in the scalar tail and on a chunk edge: the counts are exact, sumsq and
    absmax run over the finite rest."""
    nan, inf = float("nan"), float("inf")
    for value in (nan, inf, -inf, -0.0):
        v = _randn(5, 0.02)
        _plant(v, value, where)
        x = _buffer(v)
        _check(_K().tensor_stats(x, _table()), x, what=f"{value} at {where}")
        ref = R.table(x, _ranges())
        hit = [j for j, n in enumerate(_numels()) if where in ("first", "last") or (where == "tail" and n % 4) or (where == "edge" and n >= _K().STATS_CHUNK)]
        key = "zeros" if value == 0 else "nonfinite"
        assert all(ref[key][j] >= 1 for j in hit) and hit                 # (the plant landed where the test says it does)


def test_pair_form():
    """y = x: every difference is zero.  inf - inf is non-finite.  A random y against float64."""
    K = _K()
    x = _buffer(_randn(6, 0.02))
    u = R.unpack(K.tensor_stats(x, _table(), x.clone()))
    numel = torch.tensor(_numels())
    assert torch.equal(u["zeros"], numel) and not u["nonfinite"].any() and not u["sumsq"].any() and not u["absmax"].any()
    v, w = _randn(7, 0.02), _randn(8, 0.02)
    _plant(v, float("inf"), "last")
    _plant(w, float("inf"), "last")
    _plant(v, float("-inf"), "first")
    _plant(w, float("inf"), "first")
    x, y = _buffer(v), _buffer(w)
    words = K.tensor_stats(x, _table(), y)
    _check(words, x, y, what="inf - inf")
    nf = R.unpack(words)["nonfinite"]
    assert torch.equal(nf, torch.tensor([1 if n == 1 else 2 for n in _numels()]))
    x, y = _buffer(_randn(9, 1.0)), _buffer(_randn(10, 1.0))
    _check(K.tensor_stats(x, _table(), y), x, y, what="random pair")


# ---------------------------------------------------------------------------------------------------------- reproducibility
def test_bits_do_not_depend_on_the_launch_the_table_or_the_position():
    """Two launches are bit-equal; a row's four words are the same when the row stands alone in a table of one and when the table
    lists the rows in another order."""
    K, ranges = _K(), _ranges()
    x, y = _buffer(_randn(11, 0.02)), _buffer(_randn(12, 0.02))
    for yy in (None, y):
        a = K.tensor_stats(x, _table(), yy)
        b = K.tensor_stats(x, _table(), yy)
        assert torch.equal(a, b)
        rev = K.tensor_stats(x, K.stats_table(ranges[::-1], DEV), yy)
        assert torch.equal(rev.flip(0), a)
        rot = ranges[5:] + ranges[:5]
        assert torch.equal(K.tensor_stats(x, K.stats_table(rot, DEV), yy), torch.cat([a[5:], a[:5]]))
        alone = torch.cat([K.tensor_stats(x, K.stats_table([r], DEV), yy) for r in ranges])
        assert torch.equal(alone, a)


def test_rows_of_the_real_layout_keep_their_bits_alone():
    """P = 164, the table of the full-size model's parameters, against P = 1 for a handful of its rows (the largest among them)."""
    K, LY, MON = _K(), sub("layout"), sub("monitor")
    entries = [e for e in LY.build_entries(O.full_config()) if e.is_param]
    assert len(entries) == 164
    ranges = MON.layout_ranges(entries)
    g = torch.Generator(device=DEV).manual_seed(13)
    x = torch.randn(LY.flat_size(entries), device=DEV, generator=g) * 0.02
    full = K.tensor_stats(x, K.stats_table(ranges, DEV))
    again = K.tensor_stats(x, K.stats_table(ranges, DEV))
    assert torch.equal(full, again)
    big = max(range(164), key=lambda j: entries[j].numel)
    picks = sorted({0, 1, 2, big, 80, 162, 163})
    for j in picks:
        assert torch.equal(K.tensor_stats(x, K.stats_table([ranges[j]], DEV))[0], full[j]), entries[j].name
    # and the values: the largest row and the shortest against float64, within the bound
    C = K.STATS_CHUNK
    for j in (big, min(range(164), key=lambda j: entries[j].numel)):
        lo, hi = ranges[j]
        got, ref = R.unpack(full[j:j + 1]), R.row(x, lo, hi)
        assert abs(float(got["sumsq"][0]) - ref[0]) <= R.sumsq_bound(hi - lo, C) * ref[0]
        assert float(got["absmax"][0]) == ref[1] and int(got["nonfinite"][0]) == 0 and int(got["zeros"][0]) == ref[3]


def test_wrappers_refuse_what_the_kernel_must_not_see():
    K = _K()
    x = _buffer(_randn(14, 1.0))
    with pytest.raises(ValueError):
        K.tensor_stats(x[:1000], _table())                          # the table reaches beyond the buffer
    with pytest.raises(ValueError):
        K.tensor_stats(x.double(), _table())
    with pytest.raises(ValueError):
        K.tensor_stats(x, _table(), x[:-8])
    with pytest.raises(ValueError):
        K.tensor_stats(x, _table(), out=torch.empty((3, 4), device=DEV, dtype=torch.int32))
    assert pkg().kernels is K
