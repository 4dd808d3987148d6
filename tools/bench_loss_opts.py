"""Loss options of the fused step, measured (bf16, default configuration, B = 512, HipTrainer):

    python tools/bench_loss_opts.py [--out profiles/loss_opts_bench.json] [--reps 5] [--steps 10] [--lib PATH] [--kernels-only]

Train steps of four set-ups, each on its own trainer, warmed up, then timed alternately in one process with device events around
`--steps` back-to-back steps (reps alternations, median per step):
    plain         HipTrainer(model): vqa_cross_entropy (the bench.py step: the yardstick, same build, same alternation)
    plain_metric  ... with metrics=VQAAccuracy() (one vqa_accuracy_update launch behind the loss)
    opts          HipTrainer(model, label_smoothing=0.1, class_weight=w, ignore_index=-100), ~5 % of the targets ignored
    opts_metric   ... with metrics=VQAAccuracy() (counted inside the loss launch)
Then the kernels alone at [512, 1000] and [256, 2000] bf16 logits, alternated the same way over `--kernel-iters` back-to-back
launches, each with its fold launch: vqa_cross_entropy, vqa_cross_entropy_soft and vqa_bce_soft (K = 10) with and without the fused
challenge accuracy, vqa_cross_entropy_opts with all three options, with and without the fused counters, the same entry with its
options at their defaults, vqa_accuracy_update, vqa_challenge_accuracy_update, vqa_answer_scores and vqa_softmax_topk (K = 5) --
every entry of csrc/loss_ops.hip.
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
B, A = 512, 10
SETUPS = ("plain", "plain_metric", "opts", "opts_metric")


def make_model():
    cfg = O.full_config()
    m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(O.init_state_dict(cfg, 3, jitter=True))
    return m.to(DEV).train()


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


def class_weights(n, seed=5):
    """Inverse-square-root-frequency style weights of a long-tailed answer distribution, mean 1."""
    g = torch.Generator().manual_seed(seed)
    w = (1.0 + torch.arange(n, dtype=torch.float32)).rsqrt()[torch.randperm(n, generator=g)]
    return w / w.mean()


def kernels_alone(L, ST, rows, n, reps, iters):
    g = torch.Generator().manual_seed(rows + n)
    logits = (torch.randn(rows, n, generator=g) * 3).to(DEV).bfloat16()
    lf = logits.float()
    t = torch.randint(0, n, (rows,), generator=g).to(DEV)
    ti = t.clone()
    ti[torch.rand(rows, generator=g).to(DEV) < 0.05] = -100
    w = class_weights(n).to(DEV)
    answers = torch.randint(0, n, (rows, A), generator=g).to(DEV)
    soft = ST.answer_scores(answers, n)
    ids, wts, cnts = torch.empty_like(soft.ids), torch.empty_like(soft.weights), torch.empty_like(soft.counts)
    loss, ws = torch.zeros(1, device=DEV), torch.empty(rows, device=DEV)
    dl, lfo = torch.empty_like(logits), torch.empty_like(lf)
    acc3, empty = torch.zeros(3, device=DEV, dtype=torch.int64), torch.zeros(1, device=DEV, dtype=torch.int32)
    acc2 = torch.zeros(2, device=DEV, dtype=torch.int64)
    tidx, tprob = torch.empty(rows, 5, device=DEV, dtype=torch.int64), torch.empty(rows, 5, device=DEV)
    p = L.ptr

    def opts(tt, cw, has, eps, acc):
        return lambda: L.call("vqa_cross_entropy_opts", 1, p(logits), p(tt), p(loss), p(dl), p(lfo), rows, n, 1.0, None, p(ws), p(cw), -100, has, eps,
                              p(acc), p(empty))

    def soft_loss(entry, acc):
        return lambda: L.call(entry, 1, p(logits), p(soft.ids), p(soft.weights), A, p(loss), p(dl), p(lfo), rows, n, 1.0, None, p(ws),
                              p(soft.counts) if acc else None, p(acc2) if acc else None)
    kern = {
        "cross_entropy": lambda: L.call("vqa_cross_entropy", 1, p(logits), p(t), p(loss), p(dl), p(lfo), rows, n, 1.0, None, p(ws)),
        "cross_entropy_soft": soft_loss("vqa_cross_entropy_soft", False),
        "cross_entropy_soft_acc": soft_loss("vqa_cross_entropy_soft", True),
        "bce_soft": soft_loss("vqa_bce_soft", False),
        "bce_soft_acc": soft_loss("vqa_bce_soft", True),
        "cross_entropy_opts_defaults": opts(t, None, 0, 0.0, None),
        "cross_entropy_opts": opts(ti, w, 1, 0.1, None),
        "cross_entropy_opts_acc": opts(ti, w, 1, 0.1, acc3),
        "accuracy_update": lambda: L.call("vqa_accuracy_update", p(lf), p(t), p(acc3), rows, n),
        "challenge_accuracy_update": lambda: L.call("vqa_challenge_accuracy_update", p(lf), p(soft.ids), p(soft.counts), A, p(acc2), rows, n),
        "answer_scores": lambda: L.call("vqa_answer_scores", p(answers), p(ids), p(wts), p(cnts), rows, A, n, 0, None),
        "softmax_topk": lambda: L.call("vqa_softmax_topk", 1, p(logits), n, None, 0, 1.0, p(tidx), p(tprob), None, rows, n, 5),
    }
    k = alternate(kern, reps, iters)
    return {name: {s: (v * 1e3 if not isinstance(v, list) else [x * 1e3 for x in v]) for s, v in d.items()} for name, d in k.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loss_opts_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    L, M, ST = pkg._lib, pkg.load_dropin_metrics(), pkg.load_dropin_soft_targets()
    if a.lib:
        L.LIB_PATH, L._lib = os.path.abspath(a.lib), None
    if a.kernels_only:
        res = {"dtype": "bf16", "reps": a.reps, "device": torch.cuda.get_device_name(0), "library": os.path.basename(L.LIB_PATH)}
        return report(res, a.out, L, ST, a)
    images, ids, mask, answers = (t.to(DEV) for t in O.synthetic_batch(B, seed=7))
    mask[:, 0] = 1
    N = 1000
    ignored = answers.clone()
    ignored[torch.rand(B, generator=torch.Generator().manual_seed(3)).to(DEV) < 0.05] = -100
    res = {"batch": B, "dtype": "bf16", "steps_per_rep": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(L.LIB_PATH), "options": {"label_smoothing": 0.1, "class_weight": "rsqrt(rank), mean 1", "ignore_index": -100, "ignored_rows": int((ignored == -100).sum())}}

    okw = dict(label_smoothing=0.1, class_weight=class_weights(N), ignore_index=-100)
    trainers = {k: pkg.trainer.HipTrainer(make_model(), **(okw if k.startswith("opts") else {})) for k in SETUPS}
    metrics = {k: (M.VQAAccuracy() if k.endswith("metric") else None) for k in SETUPS}
    step = {k: (lambda k=k: trainers[k].step(images, ids, mask, ignored if k.startswith("opts") else answers, metrics=metrics[k])) for k in SETUPS}
    res["train_step_ms"] = alternate(step, a.reps, a.steps)
    for tr in trainers.values():
        tr.check()
    del trainers, step
    torch.cuda.empty_cache()

    report(res, a.out, L, ST, a)


def report(res, out, L, ST, a):
    # the kernels alone (bf16 logits, as the step hands them over)
    res["kernel_us"] = {f"{rows}x{n}": kernels_alone(L, ST, rows, n, a.reps, a.kernel_iters) for rows, n in ((512, 1000), (256, 2000))}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    short = lambda d: {k: [round(v["median"], 4), round(v["min"], 4), round(v["max"], 4)] for k, v in d.items()}
    if "train_step_ms" in res:
        print("train_step_ms", json.dumps(short(res["train_step_ms"])))
    for shape, d in res["kernel_us"].items():
        print("kernel_us", shape, json.dumps(short(d)))


if __name__ == "__main__":
    main()
