"""The device side of HipTrainer's non-finite guard, entry by entry: the guarded norms (vqa_sumsq_guard, vqa_sumsq_ranges_guard)
against the unguarded ones bit for bit and on planted NaN / inf, the BatchNorm buffers' save / restore over a pointer table, and
the per-parameter scan of the flat gradient.  Every expectation is exact: bits, words and integer counts."""
import pytest
import torch

from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [5, 4099, (1 << 20) + 3]          # nearly all scalar tail; no multiple of 4; many partials
NAN, INF = float("nan"), float("inf")


def _call(name, *args):
    sub("_lib").call(name, *args)


def _p(t):
    return None if t is None else t.data_ptr()


def _ints(*v):
    return torch.tensor(v, device=DEV, dtype=torch.int32)


def _grad(n, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, generator=g).to(DEV)


def _plain(g):
    out = torch.full((2049,), -1.0, device=DEV)
    _call("vqa_sumsq", _p(g), g.numel(), _p(out))
    return out


def _guarded(g, bad_step=0, bad=(0, 0), nonfinite=(0, 0)):
    """(out, word, bad, nonfinite) after vqa_sumsq_guard; the word starts at a value no verdict writes."""
    out = torch.full((2049,), -1.0, device=DEV)
    step, word, badc, nf = _ints(bad_step), _ints(77), _ints(*bad), _ints(*nonfinite)
    _call("vqa_sumsq_guard", _p(g), g.numel(), _p(out), _p(step), _p(word), _p(badc), _p(nf))
    torch.cuda.synchronize()
    return out, word.item(), badc.tolist(), nf.tolist()


@pytest.mark.parametrize("n", SIZES)
def test_guarded_norm_of_a_finite_gradient_is_the_plain_norm(n):
    g = _grad(n, seed=n)
    ref = _plain(g)
    out, word, bad, nf = _guarded(g, bad=(5, 2), nonfinite=(4, 9))
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))         # out[0] and every partial
    assert bool(torch.isfinite(out[0])) and out[0] > 0
    assert word == 0 and bad == [5, 2] and nf == [4, 9]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("value", [NAN, INF, -INF])
def test_guarded_norm_flags_a_planted_value_once(n, value):
    for at in (0, n // 2, n - 1):                                            # n - 1 lies in the scalar tail, which block 0 folds
        g = _grad(n, seed=at)
        g[at] = value
        out, word, bad, nf = _guarded(g, bad=(5, 2), nonfinite=(4, 9))
        assert not bool(torch.isfinite(out[0])), at
        assert torch.equal(out.view(torch.int32), _plain(g).view(torch.int32)), at
        assert word == 1 and bad == [5, 2] and nf == [5, 10], at


@pytest.mark.parametrize("n", SIZES)
def test_guarded_norm_flags_an_overflowing_sum_of_finite_elements(n):
    """Four elements of 1.5e19: each square is 2.25e38 (finite in fp32), their sum is inf -- as torch's norm would be."""
    g = _grad(n, seed=3)
    at = [0, n // 3, n // 2, n - 1]
    g[at] = 1.5e19
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(g[at] * g[at]).all())
    out, word, bad, nf = _guarded(g)
    assert bool(torch.isinf(out[0]))
    assert word == 1 and bad == [0, 0] and nf == [1, 1]


@pytest.mark.parametrize("value", [1.0, NAN])
def test_a_bad_target_step_stays_a_bad_target_step(value):
    """Incoming bad-target word 3: the word stays 3, bad_targets take the rows and the step, the non-finite counters rest."""
    g = _grad(4099, seed=7)
    g[17] = value
    out, word, bad, nf = _guarded(g, bad_step=3, bad=(5, 2), nonfinite=(4, 9))
    assert word == 3 and bad == [8, 3] and nf == [4, 9]
    out = torch.full((2049,), -1.0, device=DEV)                              # the bad-target counters are optional
    word, nfc = _ints(77), _ints(4, 9)
    _call("vqa_sumsq_guard", _p(g), g.numel(), _p(out), _p(_ints(3)), _p(word), None, _p(nfc))
    assert word.item() == 3 and nfc.tolist() == [4, 9]
    word, nfc = _ints(77), _ints(4, 9)                                       # ... and so is the incoming word
    _call("vqa_sumsq_guard", _p(g), g.numel(), _p(out), None, _p(word), None, _p(nfc))
    assert word.item() == (1 if value != value else 0)


def test_guarded_norm_refuses_null_outputs():
    g, out, word, nf = _grad(8), torch.zeros(2049, device=DEV), _ints(0), _ints(0, 0)
    for args in ((_p(g), 8, _p(out), None, None, None, _p(nf)), (_p(g), 8, _p(out), None, _p(word), None, None),
                 (_p(g), -1, _p(out), None, _p(word), None, _p(nf))):
        with pytest.raises(RuntimeError, match="1000"):
            _call("vqa_sumsq_guard", *args)


# ------------------------------------------------------------------------------------------------------------- the ranges form
RANGES = [(8, 40), (64, 4160), (4200, 4212)]           # gaps before, between and behind; every bound a multiple of 4
N_FLAT = 4300


def _table():
    rows, pos = [], 0
    for j, (lo, hi) in enumerate(RANGES):
        rows.append([lo, hi, pos, j])
        pos += hi - lo
    return torch.tensor(rows, dtype=torch.int64, device=DEV), len(rows), pos


def _ranges(g, guard):
    table, R, n = _table()
    out = torch.full((2049,), -1.0, device=DEV)
    word, nf = _ints(77), _ints(0, 0)
    if guard:
        _call("vqa_sumsq_ranges_guard", _p(g), _p(table), R, n, _p(out), _p(_ints(0)), _p(word), _p(_ints(0, 0)), _p(nf))
    else:
        _call("vqa_sumsq_ranges", _p(g), _p(table), R, n, _p(out))
    torch.cuda.synchronize()
    return out, word.item(), nf.tolist()


@pytest.mark.parametrize("at,flagged", [(3, False), (50, False), (4180, False), (4299, False), (8, True), (39, True), (2000, True),
                                        (4211, True)])
def test_ranges_norm_judges_only_what_lies_inside_a_range(at, flagged):
    g = _grad(N_FLAT, seed=11)
    g[at] = NAN
    ref, _, _ = _ranges(g, guard=False)
    out, word, nf = _ranges(g, guard=True)
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    assert bool(torch.isfinite(out[0])) != flagged
    assert word == int(flagged) and nf == [int(flagged)] * 2


# ------------------------------------------------------------------------------------------------------------- save / restore
def _buffers():
    a = torch.arange(64, device=DEV, dtype=torch.float32) * 0.37 - 3.0
    b = torch.tensor([NAN, -0.0, 1e-40, INF, 5.0, 6.0, 7.0, 8.0], device=DEV)         # bits, not values: a NaN and a subnormal travel
    c = torch.tensor(0x123456789ABCDEF, device=DEV, dtype=torch.int64)
    rows, off = [], 0
    for t in (a, b, c):
        words = t.numel() * t.element_size() // 4
        rows.append([t.data_ptr(), words, off])
        off += (words + 3) // 4 * 4
    return (a, b, c), torch.tensor(rows, dtype=torch.int64, device=DEV), torch.full((off + 4,), 0x5A5A5A5A, device=DEV, dtype=torch.int32), off


def _bits(t):
    return t.clone().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("word", [0, 1, 3])
def test_buffers_come_back_only_when_the_word_is_set(word):
    bufs, table, scratch, used = _buffers()
    saved = [_bits(t) for t in bufs]
    _call("vqa_buffers_save", _p(table), 3, _p(scratch))
    assert [torch.equal(_bits(t), s) for t, s in zip(bufs, saved)] == [True] * 3         # save reads only
    assert scratch[used:].tolist() == [0x5A5A5A5A] * 4                                   # ... and writes no word past its rows
    bufs[0].fill_(-1.0), bufs[1].fill_(2.0), bufs[2].fill_(99)
    over = [_bits(t) for t in bufs]
    _call("vqa_buffers_restore", _p(table), 3, _p(scratch), _p(_ints(word)))
    torch.cuda.synchronize()
    want = saved if word else over
    assert [torch.equal(_bits(t), s) for t, s in zip(bufs, want)] == [True] * 3


def test_buffers_entries_refuse_bad_arguments():
    bufs, table, scratch, _ = _buffers()
    for name, args in (("vqa_buffers_save", (None, 3, _p(scratch))), ("vqa_buffers_save", (_p(table), 0, _p(scratch))),
                       ("vqa_buffers_save", (_p(table), 3, None)), ("vqa_buffers_restore", (_p(table), 3, _p(scratch), None)),
                       ("vqa_buffers_restore", (_p(table), 65536, _p(scratch), _p(_ints(1))))):
        with pytest.raises(RuntimeError, match="1000"):
            _call(name, *args)


# ------------------------------------------------------------------------------------------------------------------ the scan
def test_scan_counts_per_parameter_and_never_the_padding():
    """Four parameters in 8-element slots: [0, 5) + padding 5..7, [8, 8 + 1030) + padding, one element, and a 3000-element one."""
    params = [(0, 5), (8, 1038), (1040, 1041), (1048, 4048)]
    g = _grad(4056, seed=5)
    planted = {0: [0, 4], 1: [8, 1037, 500, 501], 2: [], 3: [1048, 4047, 2000]}
    for j, idx in planted.items():
        for k, i in enumerate(idx):
            g[i] = (NAN, INF, -INF)[k % 3]
    for i in (5, 6, 7, 1038, 1039, 1041, 1047, 4048, 4055):                  # alignment padding: full of NaN, never counted
        g[i] = NAN
    table = torch.tensor(params, dtype=torch.int64, device=DEV)
    counts = torch.zeros(4, device=DEV, dtype=torch.int32)
    _call("vqa_nonfinite_scan", _p(g), _p(table), 4, _p(counts))
    assert counts.tolist() == [2, 4, 0, 3]
    _call("vqa_nonfinite_scan", _p(g), _p(table), 4, _p(counts))              # it adds: the caller zeroes
    assert counts.tolist() == [4, 8, 0, 6]
    g[1040] = INF
    counts.zero_()
    _call("vqa_nonfinite_scan", _p(g), _p(table), 4, _p(counts))
    assert counts.tolist() == [2, 4, 1, 3]
    with pytest.raises(RuntimeError, match="1000"):
        _call("vqa_nonfinite_scan", _p(g), _p(table), 0, _p(counts))
