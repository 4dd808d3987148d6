"""Soft answer scores, measured (bf16, default configuration, B = 512, K = 10 annotators, HipTrainer):

    python tools/bench_soft_targets.py [--out profiles/soft_targets_bench.json] [--reps 5] [--steps 10]

Train steps of four set-ups, each on its own trainer, warmed up, then timed alternately in one process with device events around
`--steps` back-to-back steps (reps alternations, median per step):
    hard          a [B] label tensor (the bench.py step: the yardstick, same build, same alternation)
    hard_metric   ... with metrics=VQAAccuracy() (one vqa_accuracy_update launch behind the loss)
    soft          SoftTargets from vqa_answer_scores (ids / weights / counts [B, 10])
    soft_metric   ... with metrics=VQAChallengeAccuracy() (counted inside the loss launch)
Then the kernels alone, alternated the same way over `--kernel-iters` back-to-back launches: the two loss entries (each with its fold
launch), the two metric entries and vqa_answer_scores.  And the autograd loop of training/train.py (model + torch.optim.AdamW, B = 64):
dense torch targets + F.cross_entropy + a reference-style metric that reads its score back every step, against
SoftTargetCrossEntropy + the device metric."""
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
B, A = 512, 10
SETUPS = ("hard", "hard_metric", "soft", "soft_metric")


def make_model():
    cfg = O.full_config()
    m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(O.init_state_dict(cfg, 3, jitter=True))
    return m.to(DEV).train()


def annotators(n, num_answers, seed=11):
    g = torch.Generator().manual_seed(seed)
    pool = torch.randint(0, num_answers, (n, 3), generator=g)
    a = torch.gather(pool, 1, torch.randint(0, 3, (n, A), generator=g) * (torch.rand(n, A, generator=g) < 0.7))
    a[torch.rand(n, A, generator=g) < 0.2] = -1
    return a.to(DEV)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "soft_targets_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--loop-batch", type=int, default=64)
    a = ap.parse_args()
    L, M, ST = pkg._lib, pkg.load_dropin_metrics(), pkg.load_dropin_soft_targets()
    images, ids, mask, answers = (t.to(DEV) for t in O.synthetic_batch(B, seed=7))
    mask[:, 0] = 1
    N = 1000
    ann = annotators(B, N)
    soft = ST.answer_scores(ann, N)
    res = {"batch": B, "annotators": A, "dtype": "bf16", "steps_per_rep": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0)}

    trainers = {k: pkg.trainer.HipTrainer(make_model()) for k in SETUPS}
    metrics = {"hard": None, "hard_metric": M.VQAAccuracy(), "soft": None, "soft_metric": M.VQAChallengeAccuracy()}
    step = {k: (lambda k=k: trainers[k].step(images, ids, mask, soft if k.startswith("soft") else answers, metrics=metrics[k])) for k in SETUPS}
    res["train_step_ms"] = alternate(step, a.reps, a.steps)
    for tr in trainers.values():
        tr.check()
    del trainers, step
    torch.cuda.empty_cache()

    # the kernels alone (bf16 logits [512, 1000], as the step hands them over)
    logits = (torch.randn(B, N, device=DEV) * 3).bfloat16()
    lf = logits.float()
    loss, ws = torch.zeros(1, device=DEV), torch.empty(B, device=DEV)
    dl, lfo = torch.empty_like(logits), torch.empty_like(lf)
    acc3, acc2 = torch.zeros(3, device=DEV, dtype=torch.int64), torch.zeros(2, device=DEV, dtype=torch.int64)
    o_ids, o_w, o_c = torch.empty_like(soft.ids), torch.empty_like(soft.weights), torch.empty_like(soft.counts)
    p = L.ptr
    kern = {
        "cross_entropy": lambda: L.call("vqa_cross_entropy", 1, p(logits), p(answers), p(loss), p(dl), p(lfo), B, N, 1.0, None, p(ws)),
        "cross_entropy_soft": lambda: L.call("vqa_cross_entropy_soft", 1, p(logits), p(soft.ids), p(soft.weights), A, p(loss), p(dl), p(lfo), B, N,
                                             1.0, None, p(ws), None, None),
        "cross_entropy_soft_acc": lambda: L.call("vqa_cross_entropy_soft", 1, p(logits), p(soft.ids), p(soft.weights), A, p(loss), p(dl), p(lfo), B, N,
                                                 1.0, None, p(ws), p(soft.counts), p(acc2)),
        "accuracy_update": lambda: L.call("vqa_accuracy_update", p(lf), p(answers), p(acc3), B, N),
        "challenge_accuracy_update": lambda: L.call("vqa_challenge_accuracy_update", p(lf), p(soft.ids), p(soft.counts), A, p(acc2), B, N),
        "answer_scores": lambda: L.call("vqa_answer_scores", p(ann), p(o_ids), p(o_w), p(o_c), B, A, N, 0, None),
    }
    k = alternate(kern, a.reps, a.kernel_iters)
    res["kernel_us"] = {n: {s: (v * 1e3 if not isinstance(v, list) else [x * 1e3 for x in v]) for s, v in d.items()} for n, d in k.items()}

    # the unchanged train.py-style loop: model + torch.optim, one metric value read per step as train.py:211-212 does
    n = a.loop_batch
    bi, bt, bm, bann = images[:n], ids[:n], mask[:n], ann[:n]
    bsoft = ST.answer_scores(bann, N)
    crit = ST.SoftTargetCrossEntropy()
    loops = {}
    for kind in ("dense_torch", "sparse_hip"):
        m = make_model()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
        metric = M.VQAChallengeAccuracy()

        def run(kind=kind, m=m, opt=opt, metric=metric):
            opt.zero_grad(set_to_none=True)
            logits, _ = m(bi, bt, bm)
            if kind == "dense_torch":
                valid = bann >= 0
                votes = (bann[:, :, None] == bann[:, None, :]).logical_and(valid[:, None, :]).sum(2)
                w = (votes.float() / 3).clamp(max=1.0) / votes.clamp(min=1) * valid          # each annotator carries score / votes
                t = torch.zeros(n, N, device=DEV).scatter_add_(1, bann.clamp(min=0), w)
                loss = F.cross_entropy(logits, t)
                pred = logits.argmax(-1)
                score = ((bann == pred[:, None]).sum(1).float() / 3).clamp(max=1.0).sum().item()   # the reference metric's host value
            else:
                loss = crit(logits, bsoft)
                metric.update(logits, bsoft)
            loss.backward()
            opt.step()
        loops[kind] = run
    res["autograd_loop_ms"] = alternate(loops, a.reps, a.steps)
    res["autograd_loop_batch"] = n
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for sec in ("train_step_ms", "kernel_us", "autograd_loop_ms"):
        print(sec, json.dumps({k: [round(v["median"], 4), round(v["min"], 4), round(v["max"], 4)] for k, v in res[sec].items()}))


if __name__ == "__main__":
    main()
