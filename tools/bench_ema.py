"""The weight average (EMA) of the fused step, measured (bf16, default configuration, B = 512, HipTrainer):

    python tools/bench_ema.py [--out profiles/ema_bench.json] [--reps 5] [--steps 10] [--lib PATH] [--kernels-only]

Train steps of six set-ups, each on its own trainer, warmed up, then timed alternately in one process with device events around
`--steps` back-to-back steps (reps alternations, median per step):
    plain          HipTrainer(model): vqa_adamw (the bench.py step: the yardstick, same build, same alternation)
    ema            HipTrainer(model, ema_decay=0.999): vqa_adamw_ema, the average kept by the optimizer launch
    plain_lerp     the plain step followed by torch._foreach_lerp_ over the 164 parameter views (what a user does without the feature)
    frozen_plain / frozen_ema / frozen_lerp     the same three with image_encoder.requires_grad_(False): the range-table variants,
                   the foreach over the trainable parameters only
Then the kernels alone over flat buffers of the model's size, alternated the same way over `--kernel-iters` back-to-back launches:
vqa_adamw, vqa_adamw_ema, vqa_adamw_ranges, vqa_adamw_ranges_ema (one range over the whole buffer), vqa_ema_update,
torch._foreach_lerp_ over the 164 views and Tensor.lerp_ over the flat buffer, with the bytes each moves by the byte model of
kernels.HBM_BYTES (the torch ops: 12 B per element) and the rate that follows from the measured time.
--lib PATH measures another build of libvqa_hip.so (the binding's LIB_PATH, as tools/ab_lib.py); --kernels-only leaves the train steps out."""
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
from oracle import vqa_oracle as O  # noqa: E402

DEV = "cuda"
B, DECAY = 512, 0.999
SETUPS = ("plain", "ema", "plain_lerp", "frozen_plain", "frozen_ema", "frozen_lerp")


def make_model(frozen):
    cfg = O.full_config()
    m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(O.init_state_dict(cfg, 3, jitter=True))
    m = m.to(DEV).train()
    if frozen:
        m.image_encoder.requires_grad_(False)
    return m


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
            t[k].append(timed(fn, n))
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v} for k, v in t.items()}


def lerp_lists(m):
    """(averages, parameters) of the trainable parameters: what a torch._foreach_lerp_ EMA keeps."""
    ps = [p.detach() for p in m._param_list() if p.requires_grad]
    return [p.clone() for p in ps], ps


def kernels_alone(m, reps, iters):
    L, FT = pkg._lib, pkg.finetune
    p = L.ptr
    n = m._flat.numel()
    g = torch.Generator().manual_seed(11)
    flat = m._flat.detach().clone()
    gr = (torch.randn(n, generator=g) * 1e-4).to(DEV)
    mo, vo, ema = torch.zeros_like(flat), torch.zeros_like(flat), flat.clone()
    pb = flat.to(torch.bfloat16)
    ss = torch.zeros(2049, device=DEV)
    skip, skipped = torch.zeros(1, device=DEV, dtype=torch.int32), torch.zeros(3, device=DEV, dtype=torch.int32)
    table = torch.tensor(FT.range_table_rows([(0, n, 0)]), dtype=torch.int64).to(DEV)
    lag = torch.zeros(1, device=DEV, dtype=torch.int32)
    L.call("vqa_sumsq", p(gr), n, p(ss))
    adam = (1e-4, 0.9, 0.999, 1e-8, 0.01, 10, p(ss), 1.0, 1.0, p(skip), p(skipped))
    views = [pkg.layout.view_of(flat, e) for e in m._param_entries]
    avgs = [v.clone() for v in views]
    kern = {
        "adamw": (lambda: L.call("vqa_adamw", p(flat), p(gr), p(mo), p(vo), n, *adam, p(pb)), "vqa_adamw"),
        "adamw_ema": (lambda: L.call("vqa_adamw_ema", p(flat), p(gr), p(mo), p(vo), n, *adam, p(pb), p(ema), DECAY, 0), "vqa_adamw_ema"),
        "adamw_ranges": (lambda: L.call("vqa_adamw_ranges", p(flat), p(gr), p(mo), p(vo), p(table), 1, n, *adam, p(lag), None, 0, p(pb)),
                         "vqa_adamw_ranges"),
        "adamw_ranges_ema": (lambda: L.call("vqa_adamw_ranges_ema", p(flat), p(gr), p(mo), p(vo), p(table), 1, n, *adam, p(lag), None, 0, p(pb),
                                            p(ema), DECAY, 0), "vqa_adamw_ranges_ema"),
        "ema_update": (lambda: L.call("vqa_ema_update", p(ema), p(flat), n, DECAY), "vqa_ema_update"),
        "foreach_lerp_164": (lambda: torch._foreach_lerp_(avgs, views, 1.0 - DECAY), None),
        "flat_lerp": (lambda: ema.lerp_(flat, 1.0 - DECAY), None),
    }
    t = alternate({k: fn for k, (fn, _) in kern.items()}, reps, iters)
    # bytes by the byte model (+ 2 B per element for the bf16 operand copy the AdamW launches also write here)
    nbytes = {"adamw": 30 * n, "adamw_ema": 38 * n, "adamw_ranges": 30 * n, "adamw_ranges_ema": 38 * n, "ema_update": 12 * n,
              "foreach_lerp_164": 12 * sum(v.numel() for v in views), "flat_lerp": 12 * n}
    out = {}
    for k, d in t.items():
        out[k] = {s: (v * 1e3 if not isinstance(v, list) else [x * 1e3 for x in v]) for s, v in d.items()}     # us
        out[k]["model_bytes"] = nbytes[k]
        out[k]["model_bytes_over_median_GBps"] = nbytes[k] / (d["median"] * 1e-3) / 1e9
    return n, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ema_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if a.lib:
        pkg._lib.LIB_PATH, pkg._lib._lib = os.path.abspath(a.lib), None
    res = {"batch": B, "dtype": "bf16", "ema_decay": DECAY, "steps_per_rep": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(pkg._lib.LIB_PATH)}
    if a.kernels_only:
        res["flat_elements"], res["kernel_us"] = kernels_alone(make_model(False), a.reps, a.kernel_iters)
        return report(res, a.out)
    images, ids, mask, answers = (t.to(DEV) for t in O.synthetic_batch(B, seed=7))
    mask[:, 0] = 1

    models = {k: make_model(k.startswith("frozen")) for k in SETUPS}
    trainers = {k: pkg.trainer.HipTrainer(models[k], ema_decay=DECAY if k.endswith("ema") else None) for k in SETUPS}
    lerp = {k: lerp_lists(models[k]) for k in SETUPS if k.endswith("lerp")}
    res["lerp_tensors"] = {k: len(v[0]) for k, v in lerp.items()}

    def step_of(k):
        tr = trainers[k]
        if k not in lerp:
            return lambda: tr.step(images, ids, mask, answers)
        avgs, ps = lerp[k]

        def fn():
            tr.step(images, ids, mask, answers)
            torch._foreach_lerp_(avgs, ps, 1.0 - DECAY)
        return fn

    res["train_step_ms"] = alternate({k: step_of(k) for k in SETUPS}, a.reps, a.steps)
    for tr in trainers.values():
        tr.check()
    res["trainable_elements"] = {k: (int(trainers[k]._ranges[2]) if trainers[k]._ranges is not None else models[k]._flat.numel()) for k in SETUPS}
    m = models["plain"]
    del trainers, lerp
    torch.cuda.empty_cache()

    res["flat_elements"], res["kernel_us"] = kernels_alone(m, a.reps, a.kernel_iters)
    report(res, a.out)


def report(res, out):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    short = lambda d: {k: [round(v["median"], 4), round(v["min"], 4), round(v["max"], 4)] for k, v in d.items()}
    if "train_step_ms" in res:
        print("train_step_ms [median, min, max]", json.dumps(short(res["train_step_ms"])))
    print("kernel_us [median, min, max]", json.dumps(short(res["kernel_us"])))
    print("kernel GB/s by the byte model", json.dumps({k: round(v["model_bytes_over_median_GBps"], 1) for k, v in res["kernel_us"].items()}))


if __name__ == "__main__":
    main()
