"""The outputs of the BatchNorm entries (csrc/batchnorm.hip) as SHA-256 digests: the inputs, the cases and the launches shared by
tests/golden/make_batchnorm_bits.py (which records tests/golden/batchnorm_bits.json) and tests/test_gpu_batchnorm_bits.py (which compares).

Inputs come from _optbits' closed integer formula (bf16 inputs are the fp32 values rounded once); the fixed-point accumulators are
encoded on the host by _bnref.acc_encode from such values.  Every BatchNorm kernel is deterministic -- the slab sums are ordered, the
accumulator sums are integer atomics and are read back as integers -- so every buffer is hashed whole and nothing has a tolerance.
Output buffers start as _optbits' sentinel NaN pattern, one guard row behind them included: a missed or a stray write shows.  The
buffers the kernels add into or update in place (dgamma, dbeta, running_mean, running_var, num_batches_tracked) start from data and
are hashed after the launch.  The shapes are _bnref's tables: the smallest at which these kernels can go wrong.

A case is one table entry and one entry point; it launches every form of that entry (the residual modes, the mask modes, slab and
accumulator), so every reachable instantiation runs at every row case of its dtype, and it records one digest per launch: of all the
buffers that launch may write, whole.  The remaining two-valued arguments (relu, running statistics given or NULL, `training` and
`which` of vqa_bn_bwd_finalize) alternate over the case index.  The status of every launch is recorded with the digests, and a
refused launch (VQA_EARG) must leave every buffer as it was."""
import functools

import numpy as np
import torch

import _bnref as R
from _optbits import DEV, SENT16, SENT32, digest, fill, toolchain, unit  # noqa: F401  (toolchain, unit: for the recorder and the test)
from _pkg import sub

F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64
EARG = 1000
RES = ("none", "add", "bn")                     # RES 0 | 1 | 2 of the forward kernels
MASK = ("none", "outact", "self", "dual")       # plain without / with outact | SELF | DUAL (with outact) of the backward kernels
GUARD64 = 0x5A5A5A5A
NMAX = max(rows * C for _, C, rows in R.ROW_CASES)          # 8195 rows of 2048 channels: 34 MB in bf16


def sent(shape, dtype):
    n = int(np.prod(shape))
    if dtype == BF16:
        return torch.full((n,), SENT16, dtype=torch.int16).view(BF16).to(DEV).view(shape)
    return torch.full((n,), SENT32, dtype=torch.int32).view(F32).to(DEV).view(shape)


def is_sent(t):
    return bool((t.view(torch.int16) == SENT16).all()) if t.dtype == BF16 else bool((t.view(torch.int32) == SENT32).all())


def data(shape, salt, dtype=F32, lo=-1.0, hi=1.0):
    """fill()'s values (element i depends on i and the salt alone, so the cached host copies come in three sizes), rounded once to dtype"""
    n = int(np.prod(shape))
    size = next(s for s in (1 << 20, 1 << 22, NMAX) if n <= s)
    return fill(size, salt, lo, hi)[:n].to(DEV).to(dtype).view(shape).contiguous()


def coefs(C, salt):
    """[4][C] fp32: scale | shift | mean | invstd"""
    return torch.stack([data((C,), salt, F32, -1.5, 1.5), data((C,), salt + 1, F32, -0.3, 0.3), data((C,), salt + 2, F32, -0.5, 0.5),
                        data((C,), salt + 3, F32, 0.5, 1.5)]).contiguous()


def accumulator(K, C, rows, salt, flag=False):
    """a host-encoded accumulator of 9 partials: column k = 0 in [-0.5, 0.5) rows / 9, the others in [1, 2) rows / 9 (as sums of y and
    y^2: the variance stays positive), partial p in replica p % R.  flag: the flag word raised."""
    parts = torch.stack([fill(9 * C, salt + k, -0.5 if k == 0 else 1.0, 0.5 if k == 0 else 2.0).view(9, C) for k in range(K)], 1)
    acc = R.acc_encode((parts * (rows / 9.0)).float(), torch.arange(9) % R.replicas(C), K, C)
    if flag:
        acc[R.replicas(C) * K * C] = 1
    return acc.to(DEV)


class Case:
    """the buffers, the launches and the result of one case: one digest per launch, over every buffer that launch may write -- the
    sentinel outputs and the in-place buffers created for it, whole, in the order they were created"""

    def __init__(self):
        self.bufs, self.new, self.before, self.st = {}, [], [], {}

    def sent(self, name, shape, dtype=F32):
        self.new.append(sent(shape, dtype))
        return self.new[-1]

    def inplace(self, name, t):
        self.new.append(t)
        self.before.append((t, digest(t)))
        return t

    def launch(self, tag, entry, *args):
        L = sub("_lib")
        self.st[tag] = int(getattr(L.lib(), entry)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], L.stream()))
        self.bufs[tag], self.new = self.new, []

    def result(self, refused=False):
        torch.cuda.synchronize()
        if refused:
            inplace = {id(t) for t, _ in self.before}
            assert all(rc == EARG for rc in self.st.values()), f"not refused: {self.st}"
            assert all(is_sent(t) for ts in self.bufs.values() for t in ts if id(t) not in inplace), "a refused launch wrote to its outputs"
            assert all(digest(t) == d for t, d in self.before), "a refused launch changed a buffer it updates in place"
        res = {tag: digest(torch.cat([t.detach().contiguous().view(-1).view(torch.uint8) for t in ts])) for tag, ts in self.bufs.items()}
        res["status"] = " ".join(f"{n}={rc}" for n, rc in sorted(self.st.items()))
        return res


def _dt(d):
    return sub("_lib").dt(R.DT[d])


# --------------------------------------------------------------------------------------------------------------------- forward
def _fwd_in(d, C, rows):
    dtype = R.DT[d]
    return data((rows, C), 1, dtype, -2.0, 2.0), data((rows, C), 2, dtype), coefs(C, 10), coefs(C, 20)


def apply_case(d, C, rows, relu):
    c, dtype = Case(), R.DT[d]
    y, res, coef, rcoef = _fwd_in(d, C, rows)
    for m, mode in enumerate(RES):
        c.launch(mode, "vqa_bn_apply", _dt(d), y, coef, res if m else None, rcoef if m == 2 else None,
                 c.sent(f"out/{mode}", (rows + 1, C), dtype), rows * C, C, relu)
    return c.result()


def apply_pool_case(d, C, B, HW, relu):
    c, dtype = Case(), R.DT[d]
    y, res, coef, rcoef = _fwd_in(d, C, B * HW)
    chunks = R.pool_chunks(HW, C, dtype)
    for m, mode in enumerate(RES):
        c.launch(mode, "vqa_bn_apply_pool", _dt(d), y, coef, res if m else None, rcoef if m == 2 else None,
                 c.sent(f"out/{mode}", (B * HW + 1, C), dtype), B, HW, C, relu, c.sent(f"part/{mode}", (B * chunks + 1, C)))
    return c.result()


def _bn_params(c, tag, C, salt, running):
    """gamma, beta, running_mean, running_var, num_batches_tracked (the last three None without running statistics), coef_out"""
    gamma, beta = data((C,), salt, F32, -1.5, 1.5), data((C,), salt + 1, F32, -0.3, 0.3)
    run = (c.inplace(f"rm/{tag}", data((C,), salt + 2, F32, -0.2, 0.2)), c.inplace(f"rv/{tag}", data((C,), salt + 3, F32, 0.5, 1.5)),
           c.inplace(f"nbt/{tag}", torch.tensor([41, 7], dtype=I64, device=DEV))) if running else (None, None, None)
    return (gamma, beta) + run + (c.sent(f"coef/{tag}", (5, C)),)


def apply_acc_case(d, C, B, HW, relu, running, pool, flag=False):
    """pool: the SE-pooling form (RES 0 | 1; the entry refuses the shortcut's accumulator there)"""
    c, dtype, rows = Case(), R.DT[d], B * HW
    y, res, _, _ = _fwd_in(d, C, rows)
    acc, racc = accumulator(2, C, rows, 30, flag), accumulator(2, C, rows, 40)
    chunks = R.pool_chunks(HW, C, dtype)
    for m, mode in enumerate(RES[:2] if pool else RES):
        own = _bn_params(c, mode, C, 50, running)
        short = (racc,) + _bn_params(c, mode + "/shortcut", C, 60, running) if m == 2 else (None,) * 7
        c.launch(mode, "vqa_bn_apply_acc", _dt(d), y, acc, *own, res if m else None, *short, c.sent(f"out/{mode}", (rows + 1, C), dtype),
                 B, HW, C, relu, float(rows), R.MOM, R.EPS, c.sent(f"part/{mode}", (B * chunks + 1, C)) if pool else None)
    return c.result()


# -------------------------------------------------------------------------------------------------------------------- backward
def _bwd_in(d, C, rows):
    dtype = R.DT[d]
    t = {"dout": data((rows, C), 3, dtype), "y": data((rows, C), 1, dtype, -2.0, 2.0), "y2": data((rows, C), 4, dtype, -1.5, 1.5),
         "outact": torch.relu(data((rows, C), 5, dtype)), "coef": coefs(C, 10), "coef2": coefs(C, 20)}
    return t


def _mask_args(t, mode):
    """(outact, y2, coef2 | None) of a mask mode"""
    return (t["outact"] if mode in ("outact", "dual") else None, t["y2"] if mode == "dual" else None, t["coef2"] if mode == "dual" else None)


def bwd_reduce_case(d, C, rows):
    c, t = Case(), _bwd_in(d, C, rows)
    nb, words = R.bwd_blocks(rows), R.acc_words(3, C)
    for acc_mode in (0, 1):
        for mode in MASK:
            oa, y2, c2 = _mask_args(t, mode)
            if acc_mode:
                buf = c.inplace(f"acc/{mode}", torch.cat([torch.zeros(words, dtype=I64), torch.full((2,), GUARD64, dtype=I64)]).to(DEV))
            else:
                buf = c.sent(f"slab/{mode}", (nb * 3 + 1, C))
            c.launch(f"{'acc' if acc_mode else 'slab'}/{mode}", "vqa_bn_bwd_reduce", _dt(d), t["dout"], oa, t["y"], t["coef"], y2, c2, buf, rows, C,
                     int(mode == "self"), acc_mode)
    return c.result()


def bwd_apply_case(d, C, rows):
    c, dtype, t = Case(), R.DT[d], _bwd_in(d, C, rows)
    bc, bc2 = data((3, C), 70), data((3, C), 71)
    for mode in MASK:
        oa, y2, _ = _mask_args(t, mode)
        dual = mode == "dual"
        c.launch(mode, "vqa_bn_bwd_apply", _dt(d), t["dout"], oa, t["y"], bc, c.sent(f"dy/{mode}", (rows + 1, C), dtype), y2, bc2 if dual else None,
                 c.sent("dy2", (rows + 1, C), dtype) if dual else None, rows * C, C, t["coef"] if mode == "self" else None)
    return c.result()


def bwd_apply_acc_case(d, C, rows, flag=False):
    c, dtype, t = Case(), R.DT[d], _bwd_in(d, C, rows)
    facc = accumulator(3, C, rows, 80, flag)
    gamma, gamma2 = data((C,), 90, F32, -1.5, 1.5), data((C,), 91, F32, -1.5, 1.5)
    for mode in MASK:
        oa, y2, c2 = _mask_args(t, mode)
        dual = mode == "dual"
        g = c.inplace(f"grads/{mode}", data((4, C), 92))                    # dgamma | dbeta | dgamma2 | dbeta2
        c.launch(mode, "vqa_bn_bwd_apply_acc", _dt(d), t["dout"], oa, t["y"], facc, gamma, t["coef"], g[0], g[1],
                 c.sent(f"dy/{mode}", (rows + 1, C), dtype), y2, gamma2 if dual else None, c2, g[2] if dual else None, g[3] if dual else None,
                 c.sent("dy2", (rows + 1, C), dtype) if dual else None, rows * C, C, float(rows), int(mode == "self"))
    return c.result()


# ------------------------------------------------------------------------------------------- statistics, coefficients, counts
def stats_case(tiles, C, running):
    c = Case()
    part = torch.stack([data((tiles, C), 100, F32, -1.5, 1.5), data((tiles, C), 101, F32, 1.0, 4.0)], 1).contiguous()      # [tiles][2][C]
    gamma, beta, rm, rv, nbt, coef = _bn_params(c, "stats", C, 50, running)
    scratch = torch.zeros(64 * 2 * C, dtype=torch.float64, device=DEV)
    c.launch("stats", "vqa_bn_stats_finalize", part, tiles, C, float(tiles * 3), gamma, beta, rm, rv, nbt, R.MOM, R.EPS, scratch, coef)
    return c.result()


def eval_coef_case(C):
    c = Case()
    c.launch("eval", "vqa_bn_eval_coef", C, data((C,), 50, F32, -1.5, 1.5), data((C,), 51, F32, -0.3, 0.3), data((C,), 52, F32, -0.2, 0.2),
             data((C,), 53, F32, 0.0, 1.5), R.EPS, c.sent("coef", (5, C)))
    return c.result()


def bwd_finalize_case(nblk, C, which, training):
    c = Case()
    slab = torch.stack([data((nblk, C), 110 + k, F32, -4.0, 4.0) for k in range(3)], 1).contiguous()                        # [nblk][3][C]
    c.launch("finalize", "vqa_bn_bwd_finalize", slab, nblk, C, which, float(nblk * 7 + 2), data((C,), 90, F32, -1.5, 1.5), coefs(C, 10), training,
             c.inplace("dgamma", data((C,), 92)), c.inplace("dbeta", data((C,), 93)), c.sent("bcoef", (4, C)))
    return c.result()


def counts_case(entry):
    L = sub("_lib")
    if entry == "vqa_bn_acc_words":
        v = [L.count(entry, K, C) for K in (2, 3) for C in sorted({C for _, C, _ in R.ROW_CASES})]
    elif entry == "vqa_bn_bwd_blocks":
        v = [L.count(entry, rows) for rows in sorted({r for _, _, r in R.ROW_CASES})]
    else:
        v = [L.count(entry, _dt(d), HW, C) for d, C in R.POOL_CHANNELS for HW in R.POOL_HW] + [L.count(entry, 1, 49, 96), L.count(entry, 1, 49, 4),
                                                                                                  L.count(entry, 0, 0, 64)]
    return {"values": digest(torch.tensor(v, dtype=I64)), "status": f"n={len(v)}"}


# ------------------------------------------------------------------------------------------------------------ refused launches
def refuse_case(entry, why):
    """One launch that the entry refuses, on buffers of 5 rows of 64 channels (bf16).  why: c96 (12 channel vectors: 256 % 12 != 0) | c4
    (no 16-byte vector) | c0 | self+y2 | self+outact | racc-no-res | pool+racc | b65536 (pool grid) | y2-no-gamma2 | tiles0."""
    c, d, rows = Case(), "bf16", 5
    C = {"c96": 96, "c4": 4, "c0": 0}.get(why, 64)
    B, HW = (65536, 1) if why == "b65536" else (1, rows)
    n = max(rows, B * HW)
    W = max(C, 64)
    t = _bwd_in(d, W, n)
    t["res"] = t["y2"]
    own = lambda tag: _bn_params(c, tag, W, 50, True)
    oa = t["outact"] if why == "self+outact" else None
    y2 = t["y2"] if why in ("self+y2", "y2-no-gamma2") else None
    self_mask = int(why.startswith("self+"))
    out = lambda name: c.sent(name, (n + 1, W), BF16)
    if entry == "vqa_bn_apply":
        c.launch(why, entry, 1, t["y"], t["coef"], None, None, out("out"), rows * C, C, 1)
    elif entry == "vqa_bn_apply_pool":
        c.launch(why, entry, 1, t["y"], t["coef"], None, None, out("out"), B, HW, C, 1, c.sent("part", (n + 1, W)))
    elif entry == "vqa_bn_apply_acc":
        acc = accumulator(2, W, rows, 30)
        short = (acc,) + own("shortcut") if why in ("racc-no-res", "pool+racc") else (None,) * 7
        pool = why in ("pool+racc", "b65536")
        c.launch(why, entry, 1, t["y"], acc, *own("own"), t["res"] if why == "pool+racc" else None, *short, out("out"), B, HW, C, 1, float(rows),
                 R.MOM, R.EPS, c.sent("part", (n + 1, W)) if pool else None)
    elif entry == "vqa_bn_bwd_reduce":
        c.launch(why, entry, 1, t["dout"], oa, t["y"], t["coef"], y2, t["coef2"] if y2 is not None else None, c.sent("slab", (4, W)), rows, C,
                 self_mask, 0)
    elif entry == "vqa_bn_bwd_apply":
        c.launch(why, entry, 1, t["dout"], oa, t["y"], data((3, W), 70), out("dy"), y2, data((3, W), 71) if y2 is not None else None,
                 out("dy2") if y2 is not None else None, rows * C, C, t["coef"] if self_mask else None)
    elif entry == "vqa_bn_bwd_apply_acc":
        g = c.inplace("grads", data((4, W), 92))
        two, gamma2 = y2 is not None, None if why == "y2-no-gamma2" else data((W,), 91)
        c.launch(why, entry, 1, t["dout"], oa, t["y"], accumulator(3, W, rows, 80), data((W,), 90), t["coef"], g[0], g[1], out("dy"), y2,
                 gamma2 if two else None, t["coef2"] if two else None, g[2] if two else None, g[3] if two else None, out("dy2") if two else None,
                 rows * C, C, float(rows), self_mask)
    else:                                                                   # vqa_bn_stats_finalize: no tiles
        gamma, beta, rm, rv, nbt, coef = own("stats")
        c.launch(why, entry, data((1, 2, 64), 100), 0, 64, 3.0, gamma, beta, rm, rv, nbt, R.MOM, R.EPS, torch.zeros(64 * 2 * 64, dtype=torch.float64, device=DEV), coef)
    return c.result(refused=True)


SHAPE_CHECKED = ("vqa_bn_apply", "vqa_bn_apply_pool", "vqa_bn_apply_acc", "vqa_bn_bwd_reduce", "vqa_bn_bwd_apply", "vqa_bn_bwd_apply_acc")
REFUSALS = [(e, w) for e in SHAPE_CHECKED for w in ("c96", "c4")] + \
           [(e, w) for e in ("vqa_bn_bwd_reduce", "vqa_bn_bwd_apply", "vqa_bn_bwd_apply_acc") for w in ("self+y2", "self+outact")] + \
           [("vqa_bn_apply_acc", "racc-no-res"), ("vqa_bn_apply_acc", "pool+racc"), ("vqa_bn_apply_acc", "b65536"), ("vqa_bn_apply_pool", "b65536"),
            ("vqa_bn_bwd_apply_acc", "y2-no-gamma2"), ("vqa_bn_stats_finalize", "tiles0")]


def cases():
    """name -> thunk returning {launch: sha256 of its buffers, "status": the launches' return codes}.  (vqa_bn_eval_coef and vqa_bn_bwd_finalize
    check no argument: they have no refused case.)"""
    c, P = {}, functools.partial
    for i, (d, C, rows) in enumerate(R.ROW_CASES):
        t = f"{d}-{C}-{rows}"
        c[f"vqa_bn_apply/{t}"] = P(apply_case, d, C, rows, i & 1)
        c[f"vqa_bn_apply_pool/rows/{t}"] = P(apply_pool_case, d, C, 1, rows, 1 - (i & 1))
        c[f"vqa_bn_apply_acc/{t}"] = P(apply_acc_case, d, C, 1, rows, i & 1, bool((i >> 1) & 1), False)
        c[f"vqa_bn_apply_acc/pool/rows/{t}"] = P(apply_acc_case, d, C, 1, rows, 1 - (i & 1), not (i >> 1) & 1, True)
        c[f"vqa_bn_bwd_reduce/{t}"] = P(bwd_reduce_case, d, C, rows)
        c[f"vqa_bn_bwd_apply/{t}"] = P(bwd_apply_case, d, C, rows)
        c[f"vqa_bn_bwd_apply_acc/{t}"] = P(bwd_apply_acc_case, d, C, rows)
    for i, (d, C, B, HW) in enumerate(R.pool_cases()):
        t = f"{d}-{C}-{B}-{HW}"
        c[f"vqa_bn_apply_pool/{t}"] = P(apply_pool_case, d, C, B, HW, i & 1)
        c[f"vqa_bn_apply_acc/pool/{t}"] = P(apply_acc_case, d, C, B, HW, 1 - (i & 1), bool((i >> 1) & 1), True)
    i = 0
    for tiles in R.STATS_TILES:
        for C in R.STATS_CHANNELS:
            c[f"vqa_bn_stats_finalize/{tiles}-{C}"] = P(stats_case, tiles, C, bool(i & 1))
            i += 1
    for C in R.STATS_CHANNELS:
        c[f"vqa_bn_eval_coef/{C}"] = P(eval_coef_case, C)
    for i, nblk in enumerate(R.FINALIZE_NBLK):
        for j, C in enumerate((64, 100)):
            c[f"vqa_bn_bwd_finalize/{nblk}-{C}"] = P(bwd_finalize_case, nblk, C, 1 + ((i + j) & 1), 1 - ((i >> 1) & 1))
    for d in ("fp32", "bf16"):                  # the flag word raised: the consumers turn the statistics into NaN
        c[f"vqa_bn_apply_acc/flagged/{d}"] = P(apply_acc_case, d, 64, 1, 33, 1, True, False, flag=True)
        c[f"vqa_bn_apply_acc/pool/flagged/{d}"] = P(apply_acc_case, d, 64, 3, 49, 1, True, True, flag=True)
        c[f"vqa_bn_bwd_apply_acc/flagged/{d}"] = P(bwd_apply_acc_case, d, 64, 33, flag=True)
    for e in ("vqa_bn_acc_words", "vqa_bn_bwd_blocks", "vqa_bn_apply_pool_chunks"):
        c[f"counts/{e}"] = P(counts_case, e)
    for e, w in REFUSALS:
        c[f"refuse/{e}/{w}"] = P(refuse_case, e, w)
    return c
