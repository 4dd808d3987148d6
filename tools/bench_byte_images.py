"""uint8 images end to end, measured (bf16, default configuration, 224 x 224, one MI355X):

    python tools/bench_byte_images.py [--out profiles/byte_images_bench.json] [--reps 5] [--steps 8] [--batch 512] [--only NAME ...]

Every comparison alternates its sides in one process, `--reps` times, with device events around back-to-back calls; median, min and
max per call are kept, so the spread of a side's own repetitions is on record next to the difference.
    kernels        each *_u8 stem kernel against its fp32 sibling in isolation (the fp32 side reads an already normalised batch)
    step           HipTrainer.step on ByteImages | on the float tensor | vqa_image_normalize + step on the float tensor
    step_graphed   the same three with step_graphed (B = 512 is where the captured step loses to step(): its static image copy)
    predict        VQAModel.predict at B = 1 and B = 64 on ByteImages | on the float tensor | normalize + float
    collate        gpu_collate_fn(output="bytes") against output="float" (resize 256 -> crop 224 -> flip -> jitter)
The float-tensor side is what the parent does once the batch is normalised; normalize + float is what it does from the bytes."""
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
H = W = 224


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(fns, reps, n, warm=2):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, n))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v} for k, v in t.items()}


def byte_batch(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return pkg.load_dropin_byte_images().ByteImages(torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(DEV))


def bench_kernels(args):
    L, K = pkg._lib, pkg.kernels
    B = args.batch
    bi = byte_batch(B)
    f32 = bi.to_float()
    Ho, Wo = H // 2, W // 2
    Hp, Wp = Ho // 2, Wo // 2
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(64, 7, 7, 3, generator=g) * 0.05).to(DEV)
    wst = torch.empty((64, 192), device=DEV, dtype=torch.bfloat16)
    L.call("vqa_stem_pack", w.data_ptr(), wst.data_ptr())
    coef = torch.stack([torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1,
                        torch.rand(64, generator=g) + 0.5]).to(DEV).contiguous()
    bc = (torch.randn(3, 64, generator=g) * 0.1).to(DEV).contiguous()
    y, _, _ = K.stem_conv(f32, wst, B, H, W, True)
    pooled = torch.empty((B * Hp * Wp, 64), device=DEV, dtype=torch.bfloat16)
    idx = torch.empty((B * Hp * Wp, 64), device=DEV, dtype=torch.uint8)
    L.call("vqa_stem_pool_fwd", 1, y.data_ptr(), coef.data_ptr(), pooled.data_ptr(), idx.data_ptr(), B, Ho, Wo, 64)
    dpool = (torch.randn(B * Hp * Wp, 64, generator=g) * 0.1).to(DEV).to(torch.bfloat16)
    dy = torch.randn(B * Ho * Wo, 64, device=DEV).to(torch.bfloat16)
    dw = torch.zeros(64, 7, 7, 3, device=DEV)
    out = {}
    for name, fn in (("stem_conv", lambda im: K.stem_conv(im, wst, B, H, W, True)),
                     ("stem_conv_pool", lambda im: K.stem_conv_pool(im, wst, coef, B, H, W)),
                     ("stem_wgrad", lambda im: K.stem_wgrad(im, dy, dw, B, H, W)),
                     ("stem_wgrad_fused", lambda im: K.stem_wgrad_fused(im, y, dpool, idx, coef, bc, dw, B, H, W))):
        out[name] = alternate({"fp32": lambda fn=fn: fn(f32), "u8": lambda fn=fn: fn(bi)}, args.reps, args.steps)
    out["image_normalize"] = alternate({"normalize": bi.to_float}, args.reps, args.steps)
    return out


def make_model(sd, cfg):
    m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(sd)
    return m.to(DEV)


def bench_steps(args, graphed):
    cfg = O.full_config()
    sd = O.init_state_dict(cfg, 3, jitter=True)
    B = args.batch
    _, ids, mask, answers = (t.to(DEV) for t in O.synthetic_batch(B, seed=5))
    bi = byte_batch(B)
    f32 = bi.to_float()
    T = pkg.trainer.HipTrainer
    trainers = {k: T(make_model(sd, cfg).train(), lr=1e-4) for k in ("bytes", "float", "normalize_float")}
    call = (lambda tr: tr.step_graphed) if graphed else (lambda tr: tr.step)
    fns = {"bytes": lambda: call(trainers["bytes"])(bi, ids, mask, answers),
           "float": lambda: call(trainers["float"])(f32, ids, mask, answers),
           "normalize_float": lambda: call(trainers["normalize_float"])(bi.to_float(), ids, mask, answers)}
    res = alternate(fns, args.reps, args.steps, warm=4)           # (a captured step needs two eager calls and the capture first)
    if graphed:
        res["graph_captures"] = {k: tr.graph_captures for k, tr in trainers.items()}
    return res


def bench_predict(args):
    cfg = O.full_config()
    m = make_model(O.init_state_dict(cfg, 3, jitter=True), cfg).eval()
    out = {}
    for B in (1, 64):
        _, ids, mask, _ = (t.to(DEV) for t in O.synthetic_batch(B, seed=6))
        bi = byte_batch(B, seed=B)
        f32 = bi.to_float()
        out[f"b{B}"] = alternate({"bytes": lambda: m.predict(bi, ids, mask), "float": lambda: m.predict(f32, ids, mask),
                                  "normalize_float": lambda: m.predict(bi.to_float(), ids, mask)}, args.reps, max(args.steps, 20), warm=3)
    return out


def bench_collate(args):
    P = pkg.load_dropin_preprocess()
    B = min(args.batch, 128)                                      # (host-side packing of the decoded images dominates beyond this)
    g = torch.Generator().manual_seed(7)
    items = [(torch.randint(0, 256, (240 + 8 * (i % 5), 320, 3), generator=g, dtype=torch.uint8).to(DEV), torch.arange(20), torch.ones(20, dtype=torch.long), i % 10)
             for i in range(B)]
    rz = P.DeviceImageResizer(size=256, crop=224, jitter=P.DeviceColorJitter(0.2, 0.2, 0.2, 0.1))
    fns = {k: (lambda k=k: P.gpu_collate_fn(items, resizer=rz, flip_p=0.5, generator=torch.Generator().manual_seed(1), output=k))
           for k in ("float", "bytes")}
    res = alternate(fns, args.reps, max(2, args.steps // 4))
    res["batch"] = B
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "byte_images_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_byte_images.py measures on the GPU; there is nothing to measure without one")
    parts = {"kernels": lambda: bench_kernels(args), "step": lambda: bench_steps(args, False), "step_graphed": lambda: bench_steps(args, True),
             "predict": lambda: bench_predict(args), "collate": lambda: bench_collate(args)}
    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "image": [H, W], "dtype": "bf16", "reps": args.reps,
           "calls_per_rep": args.steps}
    for name, fn in parts.items():
        if args.only and name not in args.only:
            continue
        res[name] = fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        print(name, json.dumps(res[name])[:400], flush=True)
        with open(args.out, "w") as f:                             # (rewritten after every part: a later part's failure keeps the earlier ones)
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
