"""The train step replayed from a captured HIP graph, measured (bf16, default configuration, HipTrainer):

    python tools/bench_step_graph.py [--out profiles/step_graph_bench.json] [--reps 5] [--steps 10] [--only NAME ...]

Every configuration runs step() and step_graphed() on two trainers of their own (two models from one state dict), warmed up -- the
graphed side until its graph is captured -- then timed alternately in one process: device events around `--steps` back-to-back steps
(reps alternations; median, min and max per step, so the spread of the eager step's own repetitions is on record), then the same
steps timed on the host as tools/host_time.py does: the time the call takes to return (enqueue) next to the wall time per step.
    features          B = 512 on cached image features (image encoder frozen, eval)
    grouped_features  N = 512 questions at 5 per image (103 images) on cached features
    frozen_images     B = 512 on images, image encoder frozen and in eval mode
    full_b32          everything trains, B = 32 (the reference's default batch size)
    full_b512         everything trains, B = 512 (GPU-bound: no gain is expected)
step() is the yardstick, on the same build in the same alternation."""
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
PER_IMAGE = 5
CONFIGS = {"features": (512, True, "features"), "grouped_features": (512, True, "grouped"), "frozen_images": (512, True, "images"),
           "full_b32": (32, False, "images"), "full_b512": (512, False, "images")}


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


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def alternate(fns, reps, n):
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, n))
    return {k: stats(v) for k, v in t.items()}


def host_times(fns, reps, n):
    out = {k: {"enqueue_ms": [], "wall_ms": []} for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            host = []
            t0 = time.perf_counter()
            for _ in range(n):
                h0 = time.perf_counter()
                fn()
                host.append(time.perf_counter() - h0)
            torch.cuda.synchronize()
            out[k]["wall_ms"].append((time.perf_counter() - t0) / n * 1e3)
            out[k]["enqueue_ms"].append(statistics.median(host) * 1e3)
    return {k: {s: stats(v) for s, v in d.items()} for k, d in out.items()}


def run_config(name, sd, cfg, reps, steps):
    B, frozen, route = CONFIGS[name]
    images, ids, mask, answers = (t.to(DEV) for t in O.synthetic_batch(B, seed=7))
    mask[:, 0] = 1
    index = None
    if route == "grouped":
        U = (B + PER_IMAGE - 1) // PER_IMAGE
        images, index = images[:U].contiguous(), (torch.arange(B) // PER_IMAGE).to(DEV)
    fns, trainers = {}, {}
    for side in ("eager", "graphed"):
        m = make_model(sd, cfg, frozen)
        tr = trainers[side] = pkg.trainer.HipTrainer(m)
        x = encode(m, images) if route in ("features", "grouped") else images
        call = tr.step if side == "eager" else tr.step_graphed
        fns[side] = (lambda call=call, x=x: call(x, ids, mask, answers, image_index=index))
    for fn in fns.values():                                    # warm-up; the graphed side captures on its third call
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    assert trainers["graphed"].graph_captures == 1
    res = {"batch": B, "route": route, "image_encoder_frozen": frozen, "train_step_ms": alternate(fns, reps, steps), "host_ms": host_times(fns, reps, steps)}
    assert trainers["graphed"].graph_captures == 1
    for tr in trainers.values():
        tr.check()
    # the two sides ran the same number of steps on the same batch from the same weights: they must still agree bit for bit
    res["bit_equal_after_the_run"] = bool(torch.equal(trainers["eager"].model._flat.detach(), trainers["graphed"].model._flat.detach()))
    e, g = res["train_step_ms"]["eager"], res["train_step_ms"]["graphed"]
    res["graphed_over_eager_at_median"] = g["median"] / e["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "step_graph_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", nargs="*", default=None, choices=sorted(CONFIGS))
    a = ap.parse_args()
    cfg = O.full_config()
    sd = O.init_state_dict(cfg, 3, jitter=True)
    res = {"dtype": "bf16", "questions_per_image": PER_IMAGE, "steps_per_rep": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "configs": {}}
    for name in (a.only or list(CONFIGS)):
        r = res["configs"][name] = run_config(name, sd, cfg, a.reps, a.steps)
        torch.cuda.empty_cache()
        t, h = r["train_step_ms"], r["host_ms"]
        print(name, "ms/step [median, min, max]", json.dumps({k: [round(v[s], 4) for s in ("median", "min", "max")] for k, v in t.items()}),
              "host enqueue_ms", json.dumps({k: round(v["enqueue_ms"]["median"], 3) for k, v in h.items()}),
              "wall_ms", json.dumps({k: round(v["wall_ms"]["median"], 3) for k, v in h.items()}),
              "bit-equal", r["bit_equal_after_the_run"], flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:                            # written after every configuration: a partial run still leaves its rows
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
