"""Fine-tuning with frozen parts, measured (bf16, default configuration, B = 512, HipTrainer):

    python tools/bench_finetune.py [--out profiles/finetune_bench.json] [--reps 5] [--steps 10]
    python tools/bench_finetune.py --kernel-run        # frozen-eval-CNN steps only, for a separate rocprofv3 --kernel-trace --stats run

Train steps of four set-ups, each on its own trainer, warmed up, then timed alternately in one process with device events around
`--steps` back-to-back steps (reps alternations, median per step):
    full          every parameter trains (the bench.py step)
    cnn_eval      image_encoder frozen and in eval mode (Conv+BN-folded CNN, no CNN backward)
    cnn_train     image_encoder frozen, train mode (batch statistics, running statistics updated, no CNN tape)
    head_fusion   only fusion and answer_head train (the text encoder frozen as well)
torch.cuda.max_memory_allocated is read per set-up over its own steps.  Saliency: a frozen eval model, forward plus
autograd.grad w.r.t. the images at B = 1 / 8 / 64, with the fine-tuning plan against the plain route that computes every
parameter gradient (the route before frozen parameters were honoured), alternated the same way."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("visual-question-answering-vqa-system_amd")
from oracle import vqa_oracle as O  # noqa: E402

DEV = "cuda"
B = 512
SETUPS = ("full", "cnn_eval", "cnn_train", "head_fusion")


def make_model():
    cfg = O.full_config()
    m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(O.init_state_dict(cfg, 3, jitter=True))
    return m.to(DEV).train()


def setup(kind):
    m = make_model()
    if kind in ("cnn_eval", "cnn_train"):
        m.image_encoder.requires_grad_(False)
        if kind == "cnn_eval":
            m.image_encoder.eval()
    elif kind == "head_fusion":
        m.image_encoder.requires_grad_(False)
        m.text_encoder.requires_grad_(False)
    return pkg.trainer.HipTrainer(m)


def inputs(n, seed=7):
    images, ids, mask, answers = O.synthetic_batch(n, seed=seed)
    mask[:, 0] = 1
    return images.to(DEV), ids.to(DEV), mask.to(DEV), answers.to(DEV)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def saliency_fn(m, batch, plain):
    images, ids, mask, _ = batch

    def run():
        x = images.clone().requires_grad_(True)
        if plain:                                  # the route before frozen parameters were honoured: every gradient computed
            m._finetune_plan = lambda *a: None
        try:
            logits, _ = m(x, ids, mask)
            torch.autograd.grad(logits.logsumexp(-1).sum(), x)
        finally:
            m.__dict__.pop("_finetune_plan", None)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "finetune_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel-run", action="store_true")
    a = ap.parse_args()
    batch = inputs(B)
    if a.kernel_run:
        tr = setup("cnn_eval")
        for _ in range(3 + a.steps):
            tr.step(*batch)
        torch.cuda.synchronize()
        return
    res = {"batch": B, "dtype": "bf16", "steps_per_rep": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    trainers = {k: setup(k) for k in SETUPS}
    for tr in trainers.values():
        for _ in range(3):
            tr.step(*batch)
    torch.cuda.synchronize()
    ms = {k: [] for k in SETUPS}
    mem = {}
    for r in range(a.reps):
        for k in SETUPS:
            if r == 0:
                torch.cuda.reset_peak_memory_stats()
            ms[k].append(timed(lambda: trainers[k].step(*batch), a.steps))
            if r == 0:
                mem[k] = torch.cuda.max_memory_allocated()
    res["train_step"] = {k: {"ms_per_step": statistics.median(v), "ms_all": v, "max_memory_allocated_bytes": mem[k]} for k, v in ms.items()}
    del trainers
    torch.cuda.empty_cache()
    m = make_model()
    m.eval()
    m.requires_grad_(False)
    sal = {}
    for n in (1, 8, 64):
        bt = tuple(t[:n] for t in batch)
        fns = {"finetune": saliency_fn(m, bt, False), "plain": saliency_fn(m, bt, True)}
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                t[k].append(timed(fn, a.steps))
        sal[str(n)] = {k: statistics.median(v) for k, v in t.items()}
        sal[str(n)]["all"] = t
    res["saliency_ms"] = sal
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v["ms_per_step"] for k, v in res["train_step"].items()}))
    print(json.dumps({n: {k: v[k] for k in ("finetune", "plain")} for n, v in sal.items()}))


if __name__ == "__main__":
    main()
