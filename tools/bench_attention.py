"""The attention entries of csrc/attention.hip one by one (bf16, H = 8, hd = 32, p = 0.1), microseconds per launch:

    python tools/bench_attention.py [--out FILE.json] [--reps 5] [--iters 200] [--lib PATH]

Shapes:
    text      B = 512, Lq = Lk = 20, q | k | v packed in one buffer (row strides 768): the benchmarked step's self attention
    cross     B = 512, Lq = 20, Lk = 49, ldq = 256, ldk = ldv = 512: its cross attention
    stress    B = 256, Lq = 20, Lk = 144 (the 384 x 384 stress shape: five key tiles)
    grouped   512 questions over 128 images, Lk = 49 (the _idx entries and vqa_index_csr); stress_grouped: 256 over 64, Lk = 144
Every shape in the MFMA form and in the VALU bf16 form: forward, backward, backward with dprobs (the indexed shapes: inference
forward, training forward, backward).  All rows are warmed up and then timed alternately in one process with device events around
`--iters` back-to-back launches, `--reps` alternations, median per launch.
--lib PATH measures another build of libvqa_hip.so (the binding's LIB_PATH, as tools/ab_lib.py)."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("visual-question-answering-vqa-system_amd")

DEV = "cuda"
H, HD, LQ, P, SEED = 8, 32, 20, 0.1, (3 << 12) | 7
D = H * HD
BF16 = torch.bfloat16


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(fns, reps, n):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, n) * 1e3)
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v} for k, v in t.items()}


def rows_of(L, shape, B, U, Lk, packed, g):
    """name -> launch for one shape; U = B: the plain and _dp entries, U < B: the indexed ones (question i asks about image i % U)"""
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV, BF16)
    if packed:
        qkv, dqkv = rnd(B * LQ, 3 * D), torch.empty(B * LQ, 3 * D, device=DEV, dtype=BF16)
        q, k, v, ldq, ldkv = qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, 3 * D
        dq, dk, dv = dqkv, dqkv[:, D:], dqkv[:, 2 * D:]
    else:
        q, kv = rnd(B * LQ, D), rnd(U * Lk, 2 * D)
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        k, v, ldq, ldkv, dk, dv = kv, kv[:, D:], D, 2 * D, dkv, dkv[:, D:]
    dctx, ctx = rnd(B * LQ, D), torch.empty(B * LQ, D, device=DEV, dtype=BF16)
    probs = torch.empty(B, H, LQ, Lk, device=DEV)
    dprobs = (torch.randn(B, H, LQ, Lk, generator=g) * 1e-3).to(DEV)
    p = L.ptr
    fwd_a = (p(q), p(k), p(v), ldq, ldkv, ldkv)
    bwd_a = (p(dctx), D, p(q), p(k), p(v), ldq, ldkv, ldkv, p(probs))
    grads = (p(dq), p(dk), p(dv), ldq, ldkv, ldkv, B, H, LQ, Lk, HD, P, SEED)
    out = (None, p(probs), p(ctx), D, B, H, LQ, Lk, HD)
    rows = {}
    if U == B:
        for form, dt in (("mfma", ()), ("valu", (1,))):
            m = "_mfma" if form == "mfma" else ""
            rows[f"{shape}/{form}/fwd"] = lambda m=m, dt=dt: L.call(f"vqa_attention_fwd{m}", *dt, *fwd_a, *out, P, SEED)
            rows[f"{shape}/{form}/bwd"] = lambda m=m, dt=dt: L.call(f"vqa_attention_bwd{m}", *dt, *bwd_a, *grads)
            rows[f"{shape}/{form}/bwd_dp"] = lambda m=m, dt=dt: L.call(f"vqa_attention_bwd{m}_dp", *dt, *bwd_a, p(dprobs), *grads)
        L.call("vqa_attention_fwd_mfma", *fwd_a, *out, P, SEED)            # probs for the backward rows
    else:
        idx = (torch.arange(B, dtype=torch.int32) % U).to(DEV)
        offsets, order = torch.empty(U + 1, device=DEV, dtype=torch.int32), torch.empty(B, device=DEV, dtype=torch.int32)
        L.call("vqa_index_csr", p(idx), B, U, p(offsets), p(order))
        for form, dt in (("mfma", ()), ("valu", (1,))):
            m = "_mfma" if form == "mfma" else ""
            rows[f"{shape}/{form}/fwd_idx"] = lambda m=m, dt=dt: L.call(f"vqa_attention_fwd{m}_idx", *dt, *fwd_a, p(idx), U, *out)
            rows[f"{shape}/{form}/fwd_idx_train"] = lambda m=m, dt=dt: L.call(f"vqa_attention_fwd{m}_idx_train", *dt, *fwd_a, p(idx), U, *out, P, SEED)
            rows[f"{shape}/{form}/bwd_idx"] = lambda m=m, dt=dt: L.call(f"vqa_attention_bwd{m}_idx", *dt, *bwd_a, p(offsets), p(order), U, *grads)
        rows[f"{shape}/index_csr"] = lambda: L.call("vqa_index_csr", p(idx), B, U, p(offsets), p(order))
        L.call("vqa_attention_fwd_mfma_idx_train", *fwd_a, p(idx), U, *out, P, SEED)
    rows["_keep"] = (q, k, v, dq, dk, dv, dctx, ctx, probs, dprobs)           # the buffers live as long as the launches
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the figures to this JSON file (default: print only)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    L = pkg._lib
    if a.lib:
        L.LIB_PATH, L._lib = os.path.abspath(a.lib), None
    g = torch.Generator().manual_seed(11)
    rows, keep = {}, []
    for shape, B, U, Lk, packed in (("text", 512, 512, 20, True), ("cross", 512, 512, 49, False), ("stress", 256, 256, 144, False),
                                    ("grouped", 512, 128, 49, False), ("stress_grouped", 256, 64, 144, False)):
        r = rows_of(L, shape, B, U, Lk, packed, g)
        keep.append(r.pop("_keep"))
        rows.update(r)
    torch.cuda.synchronize()
    res = {"dtype": "bf16", "H": H, "hd": HD, "p": P, "reps": a.reps, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(L.LIB_PATH), "kernel_us": alternate(rows, a.reps, a.iters)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    for k, v in res["kernel_us"].items():
        print(f"{k:36s} {v['median']:9.3f} us  (min {v['min']:.3f}, max {v['max']:.3f})")


if __name__ == "__main__":
    main()
