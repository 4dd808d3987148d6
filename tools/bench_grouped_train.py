"""Training with many questions per image, measured (bf16, default configuration, HipTrainer):

    python tools/bench_grouped_train.py [--out profiles/grouped_train_bench.json] [--reps 7]
    python tools/bench_grouped_train.py --kernel-run        # workload only, for a separate rocprofv3 --kernel-trace --stats run

N = 512 questions per step at q in {1, 2, 4, 5, 8} questions per image (U = ceil(N / q) images, question i on image i // q):
HipTrainer.step(images[:U], ids, mask, targets, image_index=idx) against the plain HipTrainer.step(images, ids, mask, targets) at
B = 512 on the same trainer.  Both are warmed up at every shape, then timed alternately in one process with device events around
`--steps` back-to-back steps (reps alternations, median per step).  The index is a CPU tensor: its range check is free and it
reaches the device without a sync, like the plain step.  flop_model_speedup is the forward FLOP model of flops.forward_flops with
the image half (CNN, projector, K / V projections) run once per image, the ratio a step should approach."""
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
N = 512
QS = (1, 2, 4, 5, 8)


def make_trainer():
    cfg = O.full_config()
    m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(O.init_state_dict(cfg, 3, jitter=True))
    m = m.to(DEV).train()
    return pkg.trainer.HipTrainer(m), cfg


def inputs(seed=7):
    images, ids, mask, answers = O.synthetic_batch(N, seed=seed)
    mask[:, 0] = 1
    return images.to(DEV), ids.to(DEV), mask.to(DEV), answers.to(DEV)


def index_for(q):
    idx = torch.arange(N) // q
    return idx, int(idx[-1]) + 1


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def flop_ratio(cfg, q):
    f = pkg.flops.forward_flops(cfg)
    img = f["stem"] + f["stages"]
    d, ncl, ntok = cfg["embed_dim"], cfg["num_cross_layers"], 49
    img_extra = 2.0 * ntok * (512 * d + ncl * 2 * d * d)       # projector + every cross layer's K | V projection, per image token
    full = f["total"]
    return full / ((img + img_extra) / q + (full - img - img_extra))


def throughput(tr, cfg, reps, steps):
    x, ids, mask, t = inputs()
    rows = []
    for q in QS:
        idx, U = index_for(q)
        imgs = x[:U].contiguous()
        run_g = lambda: tr.step(imgs, ids, mask, t, image_index=idx)
        run_p = lambda: tr.step(x, ids, mask, t)
        for _ in range(3):                                      # warm-up of both shapes (code objects, allocator)
            run_g(); run_p()
        torch.cuda.synchronize()
        tg, tp = [], []
        for _ in range(reps):                                   # alternate: A B A B ... in one process
            tg.append(timed(run_g, steps))
            tp.append(timed(run_p, steps))
        mg, mp = statistics.median(tg), statistics.median(tp)
        loss = float(tr.step(imgs, ids, mask, t, image_index=idx)[0])
        rows.append(dict(q=q, U=U, N=N, grouped_ms_per_step=round(mg, 3), plain_ms_per_step=round(mp, 3), speedup=round(mp / mg, 3),
                         grouped_pairs_per_s=round(N / mg * 1e3, 1), plain_pairs_per_s=round(N / mp * 1e3, 1),
                         grouped_ms_spread=[round(min(tg), 3), round(max(tg), 3)], plain_ms_spread=[round(min(tp), 3), round(max(tp), 3)],
                         flop_model_speedup=round(flop_ratio(cfg, q), 2), grouped_loss_finite=bool(loss == loss)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def kernel_run(tr):
    """Workload for rocprofv3: five grouped steps at q = 5 and five plain steps (N = 512)."""
    x, ids, mask, t = inputs()
    idx, U = index_for(5)
    imgs = x[:U].contiguous()
    for _ in range(5):
        tr.step(imgs, ids, mask, t, image_index=idx)
        tr.step(x, ids, mask, t)
    torch.cuda.synchronize()
    print("kernel run done", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grouped_train_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--kernel-run", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grouped_train needs the GPU (there is nothing to measure on a CPU)")
    tr, cfg = make_trainer()
    if a.kernel_run:
        return kernel_run(tr)
    t0 = time.time()
    res = dict(device=torch.cuda.get_device_name(0), dtype="bf16", config="default (224x224, 49 image tokens, d=256, 20 tokens)",
               steps_per_timing=a.steps, reps=a.reps, throughput=throughput(tr, cfg, a.reps, a.steps))
    res["wall_s"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}", flush=True)


if __name__ == "__main__":
    main()
