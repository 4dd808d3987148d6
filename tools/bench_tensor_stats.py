"""Per-parameter statistics on the device, measured (bf16, default configuration, B = 512):

    python tools/bench_tensor_stats.py [--out profiles/tensor_stats_bench.json] [--reps 5] [--steps 10] [--only NAME ...]

Device events around `--steps` back-to-back calls, the arms of one comparison alternating in one process (reps alternations; median,
min and max per call -- as profiles/param_groups_bench.json was taken).
    kernels   vqa_tensor_stats over the 164 parameter rows of the model's flat buffer against vqa_sumsq over the same buffer (the
              yardstick: the same bytes read once, one scalar out); the pair form (x - y) against two vqa_sumsq launches.  Also the
              worst observed fraction of the derived rounding bound (tests/_statsref.py) on normal data, sigma 0.02 and 1e3
    step      HipTrainer.step with TensorMonitor(every=1) -- every step records -- against the plain trainer, on images
    features  the same pair on cached image features (image encoder frozen, eval): the host-bound step
    read      monitor.read() of one record and trainer.tensor_stats(("grad", "param")) against the torch loop they replace: per
              parameter vector_norm, abs().max() and isfinite().sum() on two buffers, stacked, one .tolist() -- wall time with a sync
The plain arm is the yardstick, on the same build in the same alternation."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
pkg = importlib.import_module("visual-question-answering-vqa-system_amd")
from oracle import vqa_oracle as O  # noqa: E402

DEV = "cuda"
B = 512


def make_model(sd, cfg, frozen):
    m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    if frozen:
        m.image_encoder.requires_grad_(False)
        m.image_encoder.eval()
    return m


def encode(m, images):
    m.eval()
    with torch.no_grad():
        f = m.encode_features(images)
    m.train()
    m.image_encoder.eval()
    return f


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def walled(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def alternate(fns, reps, n, clock=timed):
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(clock(fn, n))
    return {k: stats(v) for k, v in t.items()}


def run_kernels(cfg, reps, steps):
    import _statsref as R
    L, K, LY, MON = pkg._lib, pkg.kernels, pkg.layout, pkg.monitor
    p = L.ptr
    ent = LY.build_entries(cfg)
    pe = [e for e in ent if e.is_param]
    n = LY.flat_size(ent)
    ranges = MON.layout_ranges(pe)
    covered = sum(hi - lo for lo, hi in ranges)
    gen = torch.Generator().manual_seed(1)
    x, y = (torch.randn(n, generator=gen).to(DEV) * 0.02 for _ in range(2))
    ss = torch.zeros(2049, device=DEV)
    table = K.stats_table(ranges, DEV)
    out = torch.empty((len(pe), 4), device=DEV, dtype=torch.int32)
    fns = {"vqa_sumsq": lambda: L.call("vqa_sumsq", p(x), n, p(ss)),
           "vqa_tensor_stats": lambda: K.tensor_stats(x, table, out=out),
           "vqa_sumsq x2": lambda: (L.call("vqa_sumsq", p(x), n, p(ss)), L.call("vqa_sumsq", p(y), n, p(ss))),
           "vqa_tensor_stats(x - y)": lambda: K.tensor_stats(x, table, y, out=out)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = alternate(fns, reps, steps)
    us = {k: {s: (v[s] * 1e3 if s != "all" else [a * 1e3 for a in v[s]]) for s in v} for k, v in t.items()}
    med = {k: v["median"] for k, v in us.items()}
    res = {"elements": n, "rows": len(pe), "elements_in_rows": covered, "chunks": table[2], "chunk": K.STATS_CHUNK,
           "partials_written_bytes": 16 * table[2], "us_per_call": us,
           "GBps_at_median": {"vqa_sumsq": 4 * n / med["vqa_sumsq"] * 1e-3, "vqa_tensor_stats": 4 * covered / med["vqa_tensor_stats"] * 1e-3,
                              "vqa_sumsq x2": 8 * n / med["vqa_sumsq x2"] * 1e-3,
                              "vqa_tensor_stats(x - y)": 8 * covered / med["vqa_tensor_stats(x - y)"] * 1e-3},
           "stats_over_sumsq_at_median": med["vqa_tensor_stats"] / med["vqa_sumsq"],
           "pair_over_two_sumsq_at_median": med["vqa_tensor_stats(x - y)"] / med["vqa_sumsq x2"]}
    # rounding: the worst observed fraction of the derived bound N_add * 2^-24, over the 164 rows
    worst = {}
    for sigma in (0.02, 1e3):
        a, b = (torch.randn(n, generator=gen).to(DEV) * sigma for _ in range(2))
        for label, yy in (("single", None), ("pair", b)):
            got = R.unpack(K.tensor_stats(a, table, yy))["sumsq"].double()
            ref = R.table(a, ranges, yy)["sumsq"]
            bound = torch.tensor([R.sumsq_bound(hi - lo, K.STATS_CHUNK, yy is not None) for lo, hi in ranges], dtype=torch.float64)
            worst[f"sigma {sigma} {label}"] = float((((got - ref).abs() / ref) / bound).max())
    res["worst_fraction_of_rounding_bound"] = worst
    return res


def run_steps(sd, cfg, reps, steps, features):
    images, ids, mask, answers = (t.to(DEV) for t in O.synthetic_batch(B, seed=7))
    mask[:, 0] = 1
    fns, trainers = {}, {}
    for side in ("plain", "monitor(every=1)"):
        m = make_model(sd, cfg, frozen=features)
        mon = pkg.monitor.TensorMonitor(every=1, slots=8) if side != "plain" else None
        tr = trainers[side] = pkg.trainer.HipTrainer(m, monitor=mon)
        x = encode(m, images) if features else images
        fns[side] = (lambda tr=tr, x=x: tr.step(x, ids, mask, answers))
    for fn in fns.values():
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    res = {"batch": B, "route": "features, step" if features else "images, step", "image_encoder_frozen": features,
           "ms_per_step": alternate(fns, reps, steps)}
    for tr in trainers.values():
        tr.check()
    t = res["ms_per_step"]
    res["monitor_over_plain_at_median"] = t["monitor(every=1)"]["median"] / t["plain"]["median"]
    res["extra_ms_per_recording_step"] = t["monitor(every=1)"]["median"] - t["plain"]["median"]
    return res


def run_read(sd, cfg, reps, steps):
    images, ids, mask, answers = (t.to(DEV) for t in O.synthetic_batch(64, seed=7))
    mask[:, 0] = 1
    m = make_model(sd, cfg, frozen=False)
    mon = pkg.monitor.TensorMonitor(every=1, slots=4)
    tr = pkg.trainer.HipTrainer(m, monitor=mon)
    for _ in range(3):
        tr.step(images, ids, mask, answers)
    views = [[buf[e.offset:e.offset + e.numel] for e in m._param_entries] for buf in (tr.G, m._flat.detach())]

    def torch_loop():
        cols = []
        for vs in views:
            cols += [torch.stack([torch.linalg.vector_norm(v) for v in vs]), torch.stack([v.abs().max() for v in vs]),
                     torch.stack([(~torch.isfinite(v)).sum() for v in vs]).float()]
        return torch.stack(cols).tolist()

    def read_one():
        mon._claim(tr.calls, 1.0, None)                    # (note one slot as live again: read() then copies one record back)
        return mon.read()

    fns = {"torch loop (164 x 3 ops x 2 buffers + tolist)": torch_loop, 'trainer.tensor_stats(("grad", "param"))': lambda: tr.tensor_stats(("grad", "param")),
           "monitor.read() of one record": read_one}
    for fn in fns.values():
        for _ in range(3):
            fn()
    return {"what": "wall ms per call, host synchronised", "parameters": len(m._param_entries), "ms_per_call": alternate(fns, reps, steps, clock=walled)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tensor_stats_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", nargs="*", default=None, choices=["kernels", "step", "features", "read"])
    a = ap.parse_args()
    cfg = O.full_config()
    sd = O.init_state_dict(cfg, 3, jitter=True)
    res = {"dtype": "bf16", "steps_per_rep": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0), "parts": {}}
    for name in (a.only or ["kernels", "step", "features", "read"]):
        if name == "kernels":
            r = run_kernels(cfg, a.reps, a.steps)
            line = {k: [round(v[s], 2) for s in ("median", "min", "max")] for k, v in r["us_per_call"].items()}
            print("kernels us/call [median, min, max]", json.dumps(line), "worst fraction of the bound", r["worst_fraction_of_rounding_bound"], flush=True)
        elif name == "read":
            r = run_read(sd, cfg, a.reps, a.steps)
            print("read ms/call [median, min, max]", json.dumps({k: [round(v[s], 4) for s in ("median", "min", "max")] for k, v in r["ms_per_call"].items()}), flush=True)
        else:
            r = run_steps(sd, cfg, a.reps, a.steps, features=name == "features")
            line = {k: [round(v[s], 4) for s in ("median", "min", "max")] for k, v in r["ms_per_step"].items()}
            print(name, "ms/step [median, min, max]", json.dumps(line), flush=True)
        res["parts"][name] = r
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:                            # written after every part: a partial run still leaves its rows
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
