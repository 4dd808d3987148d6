"""Inference-path measurement: forward-only pairs/s and latency of the eval-mode drop-in, Conv+BN folded vs BN as
its own pass; --precision bf16,mxfp8 adds rows for the MXFP8 residual-block convs (set_inference_precision).  Not part of the bench.py
contract; numbers are quoted in DESIGN.md."""
import argparse
import importlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--batches", default="1,8,64,512")
ap.add_argument("--precision", default="bf16", help="comma list of inference precisions: bf16, mxfp8")
args = ap.parse_args()
pkg = importlib.import_module("visual-question-answering-vqa-system_amd")
M = pkg.load_dropin()
dev = torch.device("cuda", 0)
model = M.VQAModel(compute_dtype=args.dtype, seed=1234).to(dev).eval()
for B in [int(b) for b in args.batches.split(",")]:
    images, ids, mask, _ = bench.synth_batch(B, dev, 7)
    for prec in args.precision.split(","):
        model.set_inference_precision(prec)
        tag = "" if prec == "bf16" else f" {prec}"
        for fold in ((True, False) if prec == "bf16" else (True,)):
            model._ensure_engine().fold_eval = fold
            with torch.no_grad():
                for _ in range(5):
                    model(images, ids, mask)
                torch.cuda.synchronize()
                n = 30 if B >= 64 else 100
                t0 = time.perf_counter()
                for _ in range(n):
                    model(images, ids, mask)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / n
            print(f"B={B:4d} fold_bn={int(fold)}{tag}  {dt*1e3:8.3f} ms/forward  {B/dt:10.1f} pairs/s", flush=True)
        if B <= 64:
            model._ensure_engine().fold_eval = True
            with torch.no_grad():
                for _ in range(3):
                    out = model.forward_graphed(images, ids, mask)
                ref, _ = model(images, ids, mask)
                torch.cuda.synchronize()
                err = (out - ref).abs().max().item()
                t0 = time.perf_counter()
                for _ in range(200):
                    model.forward_graphed(images, ids, mask)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / 200
            print(f"B={B:4d} hipGraph{tag}    {dt*1e3:8.3f} ms/forward  {B/dt:10.1f} pairs/s   max|graph - eager| = {err:.2e}", flush=True)
