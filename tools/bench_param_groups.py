"""Parameter groups of HipTrainer, measured (bf16, default configuration, B = 512):

    python tools/bench_param_groups.py [--out profiles/param_groups_bench.json] [--reps 5] [--steps 10] [--only NAME ...]

Device events around `--steps` back-to-back calls, the arms of one comparison alternating in one process (reps alternations; median,
min and max per call, so the spread of the yardstick's own repetitions is on record -- as profiles/step_graph_bench.json was taken).
    step      the full train step on images: HipTrainer(param_groups=finetune.no_weight_decay_groups(model)) against the plain trainer
    graphed   the same pair under step_graphed on cached image features (image encoder frozen, eval)
    kernels   the optimizer tail alone at the model's flat size, each AdamW launch preceded by its sum-of-squares launch:
              vqa_sumsq + vqa_adamw, vqa_sumsq_ranges + vqa_adamw_ranges over a whole-buffer table of one range, and
              vqa_sumsq_ranges + vqa_adamw_groups over the table of the no-decay groups (a few dozen ranges); all with the bf16 copy
The plain arm is the yardstick, on the same build in the same alternation."""
import argparse
import ctypes
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


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def alternate(fns, reps, n):
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, n))
    return {k: stats(v) for k, v in t.items()}


def run_steps(sd, cfg, reps, steps, graphed):
    images, ids, mask, answers = (t.to(DEV) for t in O.synthetic_batch(B, seed=7))
    mask[:, 0] = 1
    fns, trainers = {}, {}
    for side in ("plain", "groups"):
        m = make_model(sd, cfg, frozen=graphed)
        groups = pkg.finetune.no_weight_decay_groups(m) if side == "groups" else None
        tr = trainers[side] = pkg.trainer.HipTrainer(m, param_groups=groups)
        x = encode(m, images) if graphed else images
        call = tr.step_graphed if graphed else tr.step
        fns[side] = (lambda call=call, x=x: call(x, ids, mask, answers))
    for fn in fns.values():                                    # warm-up; step_graphed captures on its third call
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    res = {"batch": B, "route": "features, step_graphed" if graphed else "images, step", "image_encoder_frozen": graphed,
           "ranges": {k: (None if tr._ranges is None else tr._ranges[1]) for k, tr in trainers.items()},
           "ms_per_step": alternate(fns, reps, steps)}
    for tr in trainers.values():
        tr.check()
        assert not graphed or tr.graph_captures == 1
    t = res["ms_per_step"]
    res["groups_over_plain_at_median"] = t["groups"]["median"] / t["plain"]["median"]
    return res


def run_kernels(cfg, reps, steps):
    L, FT, LY = pkg._lib, pkg.finetune, pkg.layout
    p = L.ptr
    ent = LY.build_entries(cfg)
    pe = [e for e in ent if e.is_param]
    n = LY.flat_size(ent)
    gen = torch.Generator().manual_seed(1)
    flat, gr, mo = (torch.randn(n, generator=gen).to(DEV) * s for s in (1.0, 1e-3, 1e-3))
    vo = torch.rand(n, generator=gen).to(DEV) * 1e-4 + 1e-8
    pb = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    ss = torch.zeros(2049, device=DEV)
    lag = torch.zeros(len(pe), dtype=torch.int32, device=DEV)
    whole = FT.trainable_ranges(pe, (True,) * len(pe))

    class M:
        _param_entries = pe
    pg = FT.ParamGroups(pe, [object() for _ in pe], FT.no_weight_decay_groups(M))
    split = FT.trainable_ranges(pe, (True,) * len(pe), None, pg.group_of)
    tables = {k: torch.tensor(FT.range_table_rows(r), dtype=torch.int64, device=DEV) for k, r in (("whole", whole), ("split", split))}
    nn = {k: sum(hi - lo for lo, hi, _ in r) for k, r in (("whole", whole), ("split", split))}
    garr = torch.tensor([pg.group_of[j] for _, _, j in split], dtype=torch.int32, device=DEV)
    block = torch.zeros(32, dtype=torch.int32, device=DEV)
    scales, wds = pg.effective(0.01)
    F = ctypes.c_float * len(scales)
    L.call("vqa_group_hyper_set", p(block), len(scales), F(*scales), F(*wds))
    calls = [0]
    hyper = lambda: (1e-4, 0.9, 0.999, 1e-8, 0.01, calls[0])

    def adamw():
        calls[0] += 1
        L.call("vqa_sumsq", p(gr), n, p(ss))
        L.call("vqa_adamw", p(flat), p(gr), p(mo), p(vo), n, *hyper(), p(ss), 1.0, 1.0, None, None, p(pb))

    def ranges():
        calls[0] += 1
        t = tables["whole"]
        L.call("vqa_sumsq_ranges", p(gr), p(t), len(whole), nn["whole"], p(ss))
        L.call("vqa_adamw_ranges", p(flat), p(gr), p(mo), p(vo), p(t), len(whole), nn["whole"], *hyper(), p(ss), 1.0, 1.0, None, None, p(lag),
               None, 0, p(pb))

    def groups():
        calls[0] += 1
        t = tables["split"]
        L.call("vqa_sumsq_ranges", p(gr), p(t), len(split), nn["split"], p(ss))
        L.call("vqa_adamw_groups", p(flat), p(gr), p(mo), p(vo), p(t), len(split), nn["split"], *hyper(), p(ss), 1.0, 1.0, None, None, p(lag),
               None, 0, p(pb), p(garr), p(block))

    fns = {"vqa_sumsq+vqa_adamw": adamw, "vqa_sumsq_ranges+vqa_adamw_ranges(1 range)": ranges,
           f"vqa_sumsq_ranges+vqa_adamw_groups({len(split)} ranges)": groups}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = alternate(fns, reps, steps)
    res = {"elements": n, "ranges": {"whole": len(whole), "no_decay_groups": len(split)}, "bytes_per_pair": 34 * n,
           "us_per_pair": {k: {s: (v[s] * 1e3 if s != "all" else [x * 1e3 for x in v[s]]) for s in v} for k, v in t.items()}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "param_groups_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", nargs="*", default=None, choices=["step", "graphed", "kernels"])
    a = ap.parse_args()
    cfg = O.full_config()
    sd = O.init_state_dict(cfg, 3, jitter=True)
    res = {"dtype": "bf16", "steps_per_rep": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0), "parts": {}}
    for name in (a.only or ["kernels", "step", "graphed"]):
        if name == "kernels":
            r = run_kernels(cfg, a.reps, a.steps)
            line = {k: [round(v[s], 2) for s in ("median", "min", "max")] for k, v in r["us_per_pair"].items()}
            print("kernels us/pair [median, min, max]", json.dumps(line), flush=True)
        else:
            r = run_steps(sd, cfg, a.reps, a.steps, graphed=name == "graphed")
            line = {k: [round(v[s], 4) for s in ("median", "min", "max")] for k, v in r["ms_per_step"].items()}
            print(name, "ms/step [median, min, max]", json.dumps(line), "ranges", r["ranges"], flush=True)
        res["parts"][name] = r
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:                            # written after every part: a partial run still leaves its rows
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
