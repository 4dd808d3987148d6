"""Training from cached image features, measured (bf16, default configuration, HipTrainer, image_encoder frozen and in eval mode):

    python tools/bench_cached_features.py [--out profiles/cached_features_bench.json] [--reps 5] [--steps 10]

Each pair runs on two trainers of their own, warmed up, then timed alternately in one process with device events around `--steps`
back-to-back steps (reps alternations; median, min and max per step, so the spread of the baseline's own repetitions is on record):
    plain     B = 512, one question per image: step(images) -- the existing frozen-CNN route, the yardstick -- against step(features)
    grouped   N = 512 questions at 5 per image (103 images): step(images, image_index=) against step(features, image_index=)
    host      the same four steps timed on the host as tools/host_time.py does: the time step() takes to return (enqueue) next to the
              wall time per step; a step whose enqueue time reaches its wall time is host-bound
Then the pieces alone, alternated the same way:
    encode    encode_features on 512 images (images per second)
    select    ImageFeatures.select of 512 random rows of a 4096-image bank (vqa_gather_rows) against torch.index_select on the same
              tensor with the same device index, at the default row (7 x 7 x 512 bf16, 50 176 B) and the stress row (12 x 12 x 512,
              147 456 B, a 1024-image bank), with the bytes moved (read + write) over the median time"""
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
B, PER_IMAGE = 512, 5


def make_model():
    cfg = O.full_config()
    m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(O.init_state_dict(cfg, 3, jitter=True))
    m = m.to(DEV).train()
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


def alternate(fns, reps, n, warm=3):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, n))
    return {k: stats(v) for k, v in t.items()}


def host_times(fns, reps, n):
    """Per step: host time inside step() (enqueue) and wall time of n back-to-back steps, as tools/host_time.py measures them."""
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


def select_bench(m, shape, bank_rows, reps, iters):
    g = torch.Generator().manual_seed(17)
    bank_t = torch.randn((bank_rows,) + shape, generator=g).to(DEV, torch.bfloat16)
    bank = m.features_from_tensor(bank_t)
    idx = torch.randint(0, bank_rows, (B,), generator=g).to(DEV)
    idx32 = idx.to(torch.int32)
    K = pkg.kernels
    out = torch.empty((B,) + shape, device=DEV, dtype=torch.bfloat16)
    assert torch.equal(bank.select(idx).tensor(), bank_t.index_select(0, idx))
    t = alternate({"index_select": lambda: torch.index_select(bank_t, 0, idx, out=out),
                   "gather_rows": lambda: K.gather_rows(bank_t, idx32, out=out),
                   "select": lambda: bank.select(idx)}, reps, iters)           # select: + the range check's device-to-host read
    nbytes = 2 * B * bank_t[0].numel() * 2
    res = {"row_bytes": bank_t[0].numel() * 2, "rows": B, "bank_rows": bank_rows, "bytes_moved": nbytes}
    for k, d in t.items():
        res[k] = {s: (v * 1e3 if not isinstance(v, list) else [x * 1e3 for x in v]) for s, v in d.items()}      # us
        res[k]["GBps_at_median"] = nbytes / (d["median"] * 1e-3) / 1e9
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cached_features_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel-iters", type=int, default=50)
    a = ap.parse_args()
    images, ids, mask, answers = (t.to(DEV) for t in O.synthetic_batch(B, seed=7))
    mask[:, 0] = 1
    U = (B + PER_IMAGE - 1) // PER_IMAGE
    index = (torch.arange(B) // PER_IMAGE).to(DEV)
    res = {"batch": B, "dtype": "bf16", "questions_per_image": PER_IMAGE, "grouped_images": U, "steps_per_rep": a.steps, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}

    names = ("plain_images", "plain_features", "grouped_images", "grouped_features")
    models = {k: make_model() for k in names}
    trainers = {k: pkg.trainer.HipTrainer(models[k]) for k in names}
    feats = encode(models["plain_features"], images)
    feats_u = encode(models["grouped_features"], images[:U])
    steps = {
        "plain_images": lambda: trainers["plain_images"].step(images, ids, mask, answers),
        "plain_features": lambda: trainers["plain_features"].step(feats, ids, mask, answers),
        "grouped_images": lambda: trainers["grouped_images"].step(images[:U], ids, mask, answers, image_index=index),
        "grouped_features": lambda: trainers["grouped_features"].step(feats_u, ids, mask, answers, image_index=index),
    }
    res["train_step_ms"] = alternate(steps, a.reps, a.steps)
    res["host_ms"] = host_times(steps, a.reps, a.steps)
    for tr in trainers.values():
        tr.check()
    m = models["plain_features"]
    del trainers, steps
    torch.cuda.empty_cache()

    m.eval()
    with torch.no_grad():
        enc = alternate({"encode_features": lambda: m.encode_features(images)}, a.reps, a.steps)["encode_features"]
        enc["images_per_second_at_median"] = B / (enc["median"] * 1e-3)
        res["encode_features_ms"] = enc
        res["select_us"] = {"default_7x7x512": select_bench(m, (7, 7, 512), 4096, a.reps, a.kernel_iters),
                            "stress_12x12x512": select_bench(m, (12, 12, 512), 1024, a.reps, a.kernel_iters)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    short = lambda d: {k: [round(v["median"], 4), round(v["min"], 4), round(v["max"], 4)] for k, v in d.items()}
    print("train_step_ms [median, min, max]", json.dumps(short(res["train_step_ms"])))
    print("host enqueue_ms", json.dumps({k: round(v["enqueue_ms"]["median"], 3) for k, v in res["host_ms"].items()}),
          "wall_ms", json.dumps({k: round(v["wall_ms"]["median"], 3) for k, v in res["host_ms"].items()}))
    print("encode_features ms", round(enc["median"], 3), "images/s", round(enc["images_per_second_at_median"]))
    for k, v in res["select_us"].items():
        print("select", k, json.dumps({n: [round(v[n]["median"], 2), round(v[n]["GBps_at_median"], 1)] for n in ("index_select", "gather_rows", "select")}))


if __name__ == "__main__":
    main()
