"""The optimizer tail's outputs as SHA-256 digests: the inputs, the cases and the launches shared by tests/golden/make_optimizer_bits.py
(which records tests/golden/optimizer_bits.json) and tests/test_gpu_optimizer_bits.py (which compares against it).

Every input comes from a closed integer formula (a multiplicative hash of the element index, mapped to a float range in float64 and
rounded once to fp32): the fixture depends on no library's random generator.  Every entry runs once per case on fresh copies of the
inputs; what is hashed are the whole output buffers, sentinels outside the trainable ranges included, so a stray write shows."""
import functools
import hashlib

import numpy as np
import torch

from _pkg import sub

DEV = "cuda"
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01
GSCALE, DECAY = 0.5, 0.99
CLIPS, NO_CLIP = 0.05, 1e9                                          # max_norm; the gradients below have norm * GSCALE > 0.4
SENT32, SENT16 = 0x7FA5A5A5, 0x7FA5                                 # NaN bit patterns: reading one poisons, writing one shows
M32 = np.uint64(0xFFFFFFFF)

# (tests/test_gpu_ema_kernels.py's tables, re-declared)
BIG = [(400_000, 1_900_000, 0), (2_200_000, 4_200_000, 1), (4_549_696, 5_248_000, 2)]        # 4 194 304 + 4 000 trainable elements
TABLES = {
    "gaps-4-8-end": (4000, [(8, 1000, 0), (1004, 2000, 1), (2008, 4000, 2)]),
    "r512": (4096, [(8 * r, 8 * r + 4, r) for r in range(512)]),   # the largest table, the deepest binary search
    "two-trips": (5_248_000, BIG),                                  # > 4096 blocks x 256 threads x 4 elements: a second grid trip
}
N_ODD = 1027                                                        # four full blocks of 256 and one of 3 elements
N_TRIP = 4096 * 256 + 259                                           # the flat AdamW grid (4096 blocks) goes round a second time
N_SUMSQ_TRIP = 2048 * 256 * 4 + 1203                                # vqa_sumsq: a second float4 trip of its 2048 blocks + the scalar tail


def unit(n, salt):
    """u[i] in [0, 1), a multiple of 2^-24: hash of (i, salt), integers only"""
    i = np.arange(n, dtype=np.uint64)
    h = ((i + np.uint64(1)) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(0x9E3779B1)) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & M32
    h ^= h >> np.uint64(16)
    return (h >> np.uint64(8)).astype(np.float64) / 16777216.0


@functools.lru_cache(maxsize=None)
def fill(n, salt, lo, hi):
    """fp32 values in [lo, hi) on the CPU; shared between cases, never written (callers copy to the device)"""
    return torch.from_numpy((lo + (hi - lo) * unit(n, salt)).astype(np.float32))


def state(n):
    """p, m, v, g, ema of n elements"""
    return fill(n, 1, -1.0, 1.0), fill(n, 2, -0.01, 0.01), fill(n, 3, 1e-6, 1e-3), fill(n, 4, -0.05, 0.05), fill(n, 5, -1.0, 1.0)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def i32(*v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def sent16(n):
    return torch.full((n,), SENT16, dtype=torch.int16).view(torch.bfloat16).to(DEV)


def sumsq_blocks(n):
    return min(2048, max(1, (n // 4 + 255) // 256))


def _finish(bufs, before, skip_rows, skipped0, what):
    """digests of the buffers; after a skipped launch: everything but `skipped` unchanged, skipped = [rows, 1, skipped[2] + 1]"""
    torch.cuda.synchronize()
    if skip_rows:
        for k, t in bufs.items():
            if k != "skipped":
                assert digest(t) == before[k], f"{what}: a skipped launch changed {k}"
        assert bufs["skipped"].tolist() == [skip_rows, 1, skipped0 + 1], f"{what}: skipped = {bufs['skipped'].tolist()}"
    return {k: digest(t) for k, t in bufs.items()}


def flat_case(ema, n, calls, skipped2, max_norm, copy, warmup=0, skip_rows=0):
    L = sub("_lib")
    p0, m0, v0, g0, e0 = state(n)
    bufs = {"p": p0.to(DEV), "m": m0.to(DEV), "v": v0.to(DEV), "skipped": i32(0, 0, skipped2)}
    if copy:
        bufs["p_bf16"] = sent16(n)
    if ema:
        bufs["ema"] = e0.to(DEV)
    gd, skip, sumsq = g0.to(DEV), i32(skip_rows), torch.zeros(2049, device=DEV)
    before = {k: digest(t) for k, t in bufs.items()}
    L.call("vqa_sumsq", gd.data_ptr(), n, sumsq.data_ptr())
    args = (bufs["p"].data_ptr(), gd.data_ptr(), bufs["m"].data_ptr(), bufs["v"].data_ptr(), n, LR, B1, B2, EPS, WD, calls, sumsq.data_ptr(),
            max_norm, GSCALE, skip.data_ptr(), bufs["skipped"].data_ptr(), L.ptr(bufs.get("p_bf16")))
    if ema:
        L.call("vqa_adamw_ema", *args, bufs["ema"].data_ptr(), DECAY, warmup)
    else:
        L.call("vqa_adamw", *args)
    return _finish(bufs, before, skip_rows, skipped2, "flat")


def _sentinel(t, inside):
    out = torch.full((t.numel(),), SENT32, dtype=torch.int32).view(torch.float32).clone()
    out[inside] = t[inside]
    return out.to(DEV)


@functools.lru_cache(maxsize=None)
def _inside(name):
    n_buf, ranges = TABLES[name]
    inside = torch.zeros(n_buf, dtype=torch.bool)
    for lo, hi, _ in ranges:
        inside[lo:hi] = True
    return inside


def _table(name):
    n_buf, ranges = TABLES[name]
    rows = sub("finetune").range_table_rows(ranges)
    return n_buf, torch.tensor(rows, dtype=torch.int64).to(DEV), len(rows), sum(hi - lo for lo, hi, _ in ranges)


def _grad(name):
    n_buf = TABLES[name][0]
    g = state(n_buf)[3].clone()
    g[~_inside(name)] = float("nan")                               # never read outside the ranges
    return g.to(DEV)


def ranged_case(ema, name, calls, lagged, warmup=1, skip_rows=0):
    """lagged: parameter j has been frozen for (990 + 37 j) % 1000 applied steps, so with calls = 1000 the ranges run at step numbers
    10, 973, 936, ... (the average's warm-up decay (1 + t) / (10 + t) is below DECAY at the first, above it at the others); one more
    parameter is frozen now, so adamw_lag_kernel runs behind the update."""
    L = sub("_lib")
    n_buf, table, R, n = _table(name)
    inside = _inside(name)
    p0, m0, v0, _, e0 = state(n_buf)
    nlag = max(j for _, _, j in TABLES[name][1]) + 2
    lag0 = torch.tensor([(990 + 37 * j) % 1000 if lagged else 0 for j in range(nlag)], dtype=torch.int32)
    bufs = {"p": _sentinel(p0, inside), "m": _sentinel(m0, inside), "v": _sentinel(v0, inside), "p_bf16": sent16(n_buf),
            "lag": lag0.to(DEV), "skipped": i32(0, 0, 0)}
    if ema:
        bufs["ema"] = _sentinel(e0, inside)
    gd, skip, frozen, sumsq = _grad(name), i32(skip_rows), i32(nlag - 1), torch.zeros(2049, device=DEV)
    before = {k: digest(t) for k, t in bufs.items()}
    L.call("vqa_sumsq_ranges", gd.data_ptr(), table.data_ptr(), R, n, sumsq.data_ptr())
    args = (bufs["p"].data_ptr(), gd.data_ptr(), bufs["m"].data_ptr(), bufs["v"].data_ptr(), table.data_ptr(), R, n, LR, B1, B2, EPS, WD,
            calls, sumsq.data_ptr(), CLIPS, GSCALE, skip.data_ptr(), bufs["skipped"].data_ptr(), bufs["lag"].data_ptr(), frozen.data_ptr(), 1,
            bufs["p_bf16"].data_ptr())
    if ema:
        L.call("vqa_adamw_ranges_ema", *args, bufs["ema"].data_ptr(), DECAY, warmup)
    else:
        L.call("vqa_adamw_ranges", *args)
    return _finish(bufs, before, skip_rows, 0, name)


def sumsq_case(n):
    out = torch.zeros(2049, device=DEV)
    gd = state(n)[3].to(DEV)
    sub("_lib").call("vqa_sumsq", gd.data_ptr(), n, out.data_ptr())
    torch.cuda.synchronize()
    return {"out0": digest(out[:1]), "partials": digest(out[1:1 + sumsq_blocks(n)])}


def sumsq_ranges_case(name):
    _, table, R, n = _table(name)
    out = torch.zeros(2049, device=DEV)
    gd = _grad(name)
    sub("_lib").call("vqa_sumsq_ranges", gd.data_ptr(), table.data_ptr(), R, n, out.data_ptr())
    torch.cuda.synchronize()
    return {"out0": digest(out[:1]), "partials": digest(out[1:1 + sumsq_blocks(n)])}


def ema_update_case(off):
    """off = 1: both pointers one element past a 16-byte boundary (no float4 groups: the scalar route)"""
    n = N_ODD
    p0, _, _, _, e0 = state(n + 1)
    p, e = p0.to(DEV), e0.to(DEV)
    assert p.data_ptr() % 16 == 0 and e.data_ptr() % 16 == 0
    sub("_lib").call("vqa_ema_update", e[off:].data_ptr(), p[off:].data_ptr(), n, DECAY)
    torch.cuda.synchronize()
    return {"ema": digest(e)}


def step_state_case():
    block = torch.full((64,), 0xA5, dtype=torch.uint8, device=DEV)   # the 12 bytes behind the fields must stay as they are
    sub("_lib").call("vqa_step_state_set", block.data_ptr(), 1000, (3 << 44) | (1000 << 12), LR, B1, B2, EPS, WD, CLIPS, GSCALE, DECAY, 1)
    torch.cuda.synchronize()
    return {"state": digest(block)}


def cases():
    """name -> thunk returning {buffer name: sha256}"""
    c = {}
    for ema, entry, warmups in ((False, "vqa_adamw", (0,)), (True, "vqa_adamw_ema", (0, 1))):
        for w in warmups:
            tag = f"{entry}/warmup{w}" if ema else entry
            for calls, s2 in ((1, 0), (1000, 13)):
                for mn, mname in ((CLIPS, "clips"), (NO_CLIP, "noclip")):
                    for copy in (True, False):
                        c[f"{tag}/n{N_ODD}/calls{calls}-skipped{s2}/{mname}/{'copy' if copy else 'nocopy'}"] = \
                            functools.partial(flat_case, ema, N_ODD, calls, s2, mn, copy, warmup=w)
        c[f"{entry}/n{N_ODD}/skipped-launch"] = functools.partial(flat_case, ema, N_ODD, 1000, 13, CLIPS, True, warmup=1, skip_rows=2)
        c[f"{entry}/n{N_TRIP}/second-trip"] = functools.partial(flat_case, ema, N_TRIP, 1000, 13, CLIPS, True, warmup=1)
    for ema, entry in ((False, "vqa_adamw_ranges"), (True, "vqa_adamw_ranges_ema")):
        for name in TABLES:
            c[f"{entry}/{name}/calls1000-lagged"] = functools.partial(ranged_case, ema, name, 1000, True)
        for name in ("gaps-4-8-end", "r512"):
            c[f"{entry}/{name}/calls1-lag0"] = functools.partial(ranged_case, ema, name, 1, False)
        if ema:
            c[f"{entry}/gaps-4-8-end/calls1000-lagged/warmup0"] = functools.partial(ranged_case, ema, "gaps-4-8-end", 1000, True, warmup=0)
        c[f"{entry}/gaps-4-8-end/skipped-launch"] = functools.partial(ranged_case, ema, "gaps-4-8-end", 1000, True, skip_rows=2)
    for n in (N_ODD, N_SUMSQ_TRIP):
        c[f"vqa_sumsq/n{n}"] = functools.partial(sumsq_case, n)
    for name in TABLES:
        c[f"vqa_sumsq_ranges/{name}"] = functools.partial(sumsq_ranges_case, name)
    c["vqa_ema_update/aligned"] = functools.partial(ema_update_case, 0)
    c["vqa_ema_update/offset-by-one"] = functools.partial(ema_update_case, 1)
    c["vqa_step_state_set"] = step_state_case
    return c


def toolchain():
    """the `HIP version` line of hipcc --version (the compiler the library under test was built with, on a box that built it)"""
    import subprocess
    try:
        out = subprocess.run([sub("build").HIPCC, "--version"], capture_output=True, text=True, timeout=60).stdout
        return next((l.strip() for l in out.splitlines() if "HIP version" in l), out.strip().splitlines()[0])
    except Exception as e:                                          # noqa: BLE001  (only ever part of a message)
        return f"unknown ({type(e).__name__})"
