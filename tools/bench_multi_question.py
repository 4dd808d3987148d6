"""Many questions per image, measured (bf16, default configuration, eval mode, no_grad):

    python tools/bench_multi_question.py [--out profiles/multi_question_bench.json] [--reps 10]
    python tools/bench_multi_question.py --kernel-run        # workload only, for a separate rocprofv3 --kernel-trace --stats run

Throughput: N = 512 questions at q in {1, 2, 5, 10} questions per image (U = ceil(N / q) images, question i on image i // q), the
indexed forward(images, ids, mask, image_index=idx) against the expanded forward(images[idx], ids, mask) at B = 512.  Both are
warmed up at every shape, checked for the same top-1 answers, then timed alternately in one process with device events (reps
alternations, median per call).  Latency: answer() at N = 1 on a cached context (captured graph) against the graphed full forward
at B = 1 (device events around 200 back-to-back calls; both paths are host-bound there, so this is the per-call time a server
sees).  The FLOP model of flops.forward_flops gives the work ratio each q should approach."""
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
QS = (1, 2, 5, 10)


def make_model():
    cfg = O.full_config()
    m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(O.init_state_dict(cfg, 3, jitter=True))
    return m.to(DEV).eval(), cfg


def inputs(seed=7):
    images, ids, mask, _ = O.synthetic_batch(N, seed=seed)
    mask[:, 0] = 1
    return images.to(DEV), ids.to(DEV), mask.to(DEV)


def index_for(q):
    idx = torch.arange(N, device=DEV) // q
    return idx, int(idx[-1]) + 1


def timed(fn, n=1):
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
    # image side once per image: the CNN, the projector and the two cross layers' K / V projections (d x 512 and 2 x (d x 2d) per token)
    d, ncl, ntok = cfg["embed_dim"], cfg["num_cross_layers"], 49
    img_extra = 2.0 * ntok * (512 * d + ncl * 2 * d * d)
    full = f["total"]
    return full / ((img + img_extra) / q + (full - img - img_extra))


def throughput(m, cfg, reps):
    x, ids, mask = inputs()
    rows = []
    with torch.no_grad():
        for q in QS:
            idx, U = index_for(q)
            imgs = x[:U].contiguous()
            expanded = imgs[idx].contiguous()
            run_idx = lambda: m(imgs, ids, mask, image_index=idx)[0]
            run_exp = lambda: m(expanded, ids, mask)[0]
            for _ in range(3):                                  # warm-up of both shapes (code objects, allocator, fold buffers)
                a, b = run_idx(), run_exp()
            torch.cuda.synchronize()
            top_same = int((a.argmax(-1) == b.argmax(-1)).sum())
            max_dl = float((a - b).abs().max())
            if top_same < N:
                print(f"[bench_multi_question] q={q}: top-1 differs on {N - top_same} of {N} questions (max |dlogit| {max_dl:.3g})",
                      file=sys.stderr, flush=True)
            ti, te = [], []
            for _ in range(reps):                               # alternate: A B A B ... in one process
                ti.append(timed(run_idx))
                te.append(timed(run_exp))
            mi, me = statistics.median(ti), statistics.median(te)
            rows.append(dict(q=q, U=U, N=N, indexed_ms=round(mi, 3), expanded_ms=round(me, 3), speedup=round(me / mi, 3),
                             indexed_pairs_per_s=round(N / mi * 1e3, 1), expanded_pairs_per_s=round(N / me * 1e3, 1),
                             indexed_ms_spread=[round(min(ti), 3), round(max(ti), 3)], expanded_ms_spread=[round(min(te), 3), round(max(te), 3)],
                             flop_model_speedup=round(flop_ratio(cfg, q), 2), top1_agree=f"{top_same}/{N}", max_abs_dlogit=round(max_dl, 5)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def latency(m, reps):
    x, ids, mask = inputs(seed=11)
    out = {}
    with torch.no_grad():
        ctx = m.encode_images(x[:1])
        run_ans = lambda: m.answer(ctx, ids[:1], mask[:1])
        run_fwd = lambda: m(x[:1], ids[:1], mask[:1])
        for _ in range(5):
            run_ans(); run_fwd()
        torch.cuda.synchronize()
        a, b = run_ans()[0], run_fwd()[0]
        ta, tf = [], []
        for _ in range(reps):
            ta.append(timed(run_ans, 200))
            tf.append(timed(run_fwd, 200))
        out = dict(answer_graphed_ms=round(statistics.median(ta), 4), forward_graphed_ms=round(statistics.median(tf), 4),
                   answer_ms_spread=[round(min(ta), 4), round(max(ta), 4)], forward_ms_spread=[round(min(tf), 4), round(max(tf), 4)],
                   speedup=round(statistics.median(tf) / statistics.median(ta), 2), same_top1=bool(a.argmax() == b.argmax()),
                   max_abs_dlogit=round(float((a - b).abs().max()), 5), note="per call, 200 back-to-back calls between two device events")
        # the encode cost that answer() amortises: one image, eager (no graph for encode_images)
        for _ in range(3):
            m.encode_images(x[:1])
        out["encode_images_B1_eager_ms"] = round(statistics.median([timed(lambda: m.encode_images(x[:1]), 50) for _ in range(reps)]), 4)
    print(json.dumps(out), flush=True)
    return out


def kernel_run(m):
    """Workload for rocprofv3: the indexed forward at q = 5 (eager, N = 512) and answer() at N = 64 (eager), a few times each."""
    x, ids, mask = inputs()
    idx, U = index_for(5)
    with torch.no_grad():
        m.graph_inference = False
        ctx = m.encode_images(x[:U].contiguous())
        for _ in range(5):
            m(x[:U].contiguous(), ids, mask, image_index=idx)
            m.answer(ctx, ids[:64], mask[:64], image_index=idx[:64])
    torch.cuda.synchronize()
    print("kernel run done", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_question_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-run", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_question needs the GPU (there is nothing to measure on a CPU)")
    m, cfg = make_model()
    if a.kernel_run:
        return kernel_run(m)
    t0 = time.time()
    res = dict(device=torch.cuda.get_device_name(0), dtype="bf16", config="default (224x224, 49 image tokens, d=256, 20 tokens)",
               throughput=throughput(m, cfg, a.reps), latency_b1=latency(m, a.reps))
    res["wall_s"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}", flush=True)


if __name__ == "__main__":
    main()
