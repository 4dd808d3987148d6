"""Top-k answers with probabilities, measured (bf16, default configuration, eval mode, no_grad, k = 5):

    python tools/bench_topk.py [--out profiles/topk_bench.json] [--reps 11] [--calls 100]

(a) predict() (graph replay + logits clone + eager softmax + topk) against predict_topk() (one graph that ends in vqa_softmax_topk)
    at B = 1, 8, 64 (graphed) and 512 (eager).
(b) answer() + torch softmax / topk against answer_topk() at N = 1 on a cached context.
(c) the kernel alone (kernels.softmax_topk) against torch.softmax + torch.topk on fp32 [B, 1000] and [B, 2000] logits.
(d) TopK.to_records against the reference's .item() loop (api/inference.py:236-246) at B = 64.

Every pair is warmed up, checked for the same top-1 answers, then timed alternately in one process: `reps` alternations of `calls`
back-to-back calls between two device events (time per call: these paths are host-bound at small B, so this is what a server sees
per request); (d) is host time around a call that ends in its own read-backs.  Reported: the median per call, the min / max over the
alternations, and old / new."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("visual-question-answering-vqa-system_amd")
from oracle import vqa_oracle as O  # noqa: E402

DEV = "cuda"
TOPK = 5


def make_model():
    cfg = O.full_config()
    m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(O.init_state_dict(cfg, 3, jitter=True))
    return m.to(DEV).eval(), cfg


def inputs(B, seed=7):
    images, ids, mask, _ = O.synthetic_batch(B, seed=seed)
    mask[:, 0] = 1
    return images.to(DEV), ids.to(DEV), mask.to(DEV)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def host_timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def alternate(old, new, reps, calls, clock=timed):
    """Medians (ms per call) of `reps` alternations old / new, with the spread of each."""
    for _ in range(3):
        old(); new()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):
        a.append(clock(old, calls))
        b.append(clock(new, calls))
    ma, mb = statistics.median(a), statistics.median(b)
    return {"old_ms": round(ma, 5), "new_ms": round(mb, 5), "old_over_new": round(ma / mb, 3),
            "old_ms_spread": [round(min(a), 5), round(max(a), 5)], "new_ms_spread": [round(min(b), 5), round(max(b), 5)]}


def torch_tail(logits, k=TOPK):
    return F.softmax(logits, dim=-1).topk(k, dim=-1)


def bench_predict(m, reps, calls):
    rows = []
    for B in (1, 8, 64, 512):
        x, ids, mask = inputs(B)
        old = lambda: m.predict(x, ids, mask, top_k=TOPK)
        new = lambda: m.predict_topk(x, ids, mask, top_k=TOPK)
        oi, _ = old()
        t = new()
        agree = int((oi[:, 0] == t.indices[:, 0]).sum())
        r = alternate(old, new, reps, calls if B <= 64 else max(4, calls // 10))
        r.update(B=B, route="graph" if B <= m.graph_max_batch else "eager", top1_agree=f"{agree}/{B}")
        rows.append(r)
        print("predict", r, flush=True)
    return rows


def bench_answer(m, reps, calls):
    x, ids, mask = inputs(1)
    ctx = m.encode_images(x)
    old = lambda: torch_tail(m.answer(ctx, ids, mask)[0])
    new = lambda: m.answer_topk(ctx, ids, mask, top_k=TOPK)
    agree = int((old()[1][:, 0] == new().indices[:, 0]).sum())
    r = alternate(old, new, reps, calls)
    r.update(N=1, top1_agree=f"{agree}/1")
    print("answer", r, flush=True)
    return r


def bench_kernel(reps, calls):
    K = pkg.kernels
    rows = []
    g = torch.Generator().manual_seed(1)
    for N in (1000, 2000):
        for B in (1, 8, 64, 512):
            lg = (torch.randn(B, N, generator=g) * 3).to(DEV)
            old = lambda: torch_tail(lg)
            new = lambda: K.softmax_topk(lg, TOPK)
            agree = int((old()[1][:, 0] == new()[0][:, 0]).sum())
            r = alternate(old, new, reps, calls)
            r.update(B=B, N=N, top1_agree=f"{agree}/{B}")
            rows.append(r)
            print("kernel", r, flush=True)
    return rows


def bench_records(m, reps):
    B = 64
    x, ids, mask = inputs(B)
    decode = lambda i: f"answer-{i}"
    t = m.predict_topk(x, ids, mask, top_k=TOPK)

    def item_loop():                                   # api/inference.py:236-246 per question, 2 * k * B device reads
        out = []
        for b in range(B):
            answers = []
            for i in range(TOPK):
                idx = t.indices[b, i].item()
                prob = t.probs[b, i].item()
                answers.append({"answer": decode(idx), "probability": prob, "index": idx})
            out.append({"answers": answers, "top_answer": answers[0]["answer"], "confidence": answers[0]["probability"]})
        return out

    assert item_loop() == t.to_records(decode)
    r = alternate(item_loop, lambda: t.to_records(decode), reps, 3, clock=host_timed)
    r.update(B=B, k=TOPK, clock="host")
    print("records", r, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "topk_bench.json"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--calls", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk.py measures on the GPU; none found")
    m, cfg = make_model()
    with torch.no_grad():
        res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "k": TOPK, "reps": a.reps, "calls_per_rep": a.calls,
               "config": "default (224x224, 49 image tokens, d=256, 20 tokens, 1000 answers)",
               "old": "predict() / answer() + torch.softmax + torch.topk", "new": "predict_topk() / answer_topk() (vqa_softmax_topk in the graph)",
               "predict": bench_predict(m, a.reps, a.calls), "answer": bench_answer(m, a.reps, a.calls),
               "kernel_fp32_logits": bench_kernel(a.reps, a.calls), "to_records": bench_records(m, a.reps)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
