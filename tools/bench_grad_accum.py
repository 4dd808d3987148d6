"""Gradient accumulation of HipTrainer (accumulate() ... step()), measured (bf16, default configuration):

    python tools/bench_grad_accum.py [--out profiles/grad_accum_bench.json] [--reps 5] [--units 10] [--only NAME ...]

Device events around `--units` back-to-back units of 512 samples (1024 in the third comparison), the arms of one comparison alternating
in one process (reps alternations; median, min and max per unit, so the spread of the yardstick's own repetitions is on record -- as
tools/bench_param_groups.py measures).  The host's enqueue time per unit is the wall clock around the same calls, before the
synchronisation.
    window_4x128     a window of 4 x B = 128 (three accumulate() and the closing step(): ONE update) against four plain B = 128 steps
                     (four updates) and against one B = 512 step (one update of the large batch)
    window_2x512     a window of 2 x B = 512 against two plain B = 512 steps
    features_4x128   the first comparison on cached image features (image encoder frozen, eval): the CNN never runs
The plain arms are the yardsticks, on the same build in the same alternation.  A non-closing micro-batch is a plain step without the
gradient buffer's memset, the norm and AdamW; what a window saves over as many plain steps is that tail, (n - 1) times.
The file also keeps what tests/test_gpu_grad_accum.py records there (the keys sum_check_*) when it runs with VQA_RECORD_PROFILES=1:
    VQA_RECORD_PROFILES=1 python -m pytest tests/test_gpu_grad_accum.py -k window_gradient_is_the_sum"""
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
pkg = importlib.import_module("visual-question-answering-vqa-system_amd")
from oracle import vqa_oracle as O  # noqa: E402

DEV = "cuda"


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
    """(device ms per unit, host enqueue ms per unit)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    h0 = time.perf_counter()
    for _ in range(n):
        fn()
    h1 = time.perf_counter()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n, (h1 - h0) * 1e3 / n


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def alternate(fns, reps, n):
    dev, host = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            d, h = timed(fn, n)
            dev[k].append(d)
            host[k].append(h)
    return {k: stats(v) for k, v in dev.items()}, {k: stats(v) for k, v in host.items()}


def batches(total, size, frozen_model=None):
    """`total` samples cut into batches of `size`: [(images or ImageFeatures, ids, mask, answers), ...]"""
    images, ids, mask, answers = (t.to(DEV) for t in O.synthetic_batch(total, seed=7))
    mask[:, 0] = 1
    out = []
    for lo in range(0, total, size):
        x = images[lo: lo + size].contiguous()
        if frozen_model is not None:
            x = encode(frozen_model, x)
        out.append((x, ids[lo: lo + size].contiguous(), mask[lo: lo + size].contiguous(), answers[lo: lo + size].contiguous()))
    return out


def run(sd, cfg, reps, units, micro, n, features=False, big=False):
    """Arms: `window` (n micro-batches of `micro`, one update), `plain` (n plain steps), and with big=True `large` (one step of n * micro)."""
    total = micro * n
    fns, trainers = {}, {}
    for arm in ("plain", "window") + (("large",) if big else ()):
        m = make_model(sd, cfg, frozen=features)
        tr = trainers[arm] = pkg.trainer.HipTrainer(m)
        bs = batches(total, total if arm == "large" else micro, m if features else None)
        if arm == "window":
            def fn(tr=tr, bs=bs):
                for b in bs[:-1]:
                    tr.accumulate(*b)
                tr.step(*bs[-1])
        else:
            def fn(tr=tr, bs=bs):
                for b in bs:
                    tr.step(*b)
        fns[arm] = fn
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    dev, host = alternate(fns, reps, units)
    for arm, tr in trainers.items():
        tr.check()
        assert tr.pending == 0 and tr.calls == (3 + reps * units) * (n if arm == "plain" else 1)
    res = {"micro_batch": micro, "micro_batches_per_window": n, "samples_per_unit": total, "route": "features" if features else "images",
           "image_encoder_frozen": features, "updates_per_unit": {"plain": n, "window": 1, **({"large": 1} if big else {})},
           "ms_per_unit": dev, "host_enqueue_ms_per_unit": host,
           "samples_per_s_at_median": {k: total / v["median"] * 1e3 for k, v in dev.items()},
           "window_over_plain_at_median": dev["window"]["median"] / dev["plain"]["median"],
           "saved_ms_per_non_closing_micro_batch": (dev["plain"]["median"] - dev["window"]["median"]) / (n - 1)}
    if big:
        res["window_over_large_at_median"] = dev["window"]["median"] / dev["large"]["median"]
    return res


PARTS = {"window_4x128": dict(micro=128, n=4, big=True), "window_2x512": dict(micro=512, n=2), "features_4x128": dict(micro=128, n=4, features=True, big=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grad_accum_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--units", type=int, default=10)
    ap.add_argument("--only", nargs="*", default=None, choices=list(PARTS))
    a = ap.parse_args()
    cfg = O.full_config()
    sd = O.init_state_dict(cfg, 3, jitter=True)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    res = doc["bench"] = {"dtype": "bf16", "units_per_rep": a.units, "reps": a.reps, "device": torch.cuda.get_device_name(0), "parts": {}}
    for name in (a.only or list(PARTS)):
        r = run(sd, cfg, a.reps, a.units, **PARTS[name])
        line = {k: [round(v[s], 3) for s in ("median", "min", "max")] for k, v in r["ms_per_unit"].items()}
        hline = {k: round(v["median"], 3) for k, v in r["host_enqueue_ms_per_unit"].items()}
        print(name, "ms/unit [median, min, max]", json.dumps(line), "host ms/unit", json.dumps(hline), flush=True)
        res["parts"][name] = r
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:                            # written after every part: a partial run still leaves its rows
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
