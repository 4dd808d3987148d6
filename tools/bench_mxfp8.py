"""A/B of the MXFP8 residual-block conv (vqa_conv_mxfp8) against the bf16 vqa_igemm launch it replaces on the folded eval path, per
distinct conv shape at B = 512 (not part of the product; numbers are quoted in DESIGN.md).  The two launches alternate, each timed
with its own event pair, and the medians are reported; operands are random (not zero-filled), epilogues as on the eval path
(conv1: bias + ReLU, MXFP8 output only; conv2: bias + bf16 addend + ReLU after it)."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("visual-question-answering-vqa-system_amd")
K = pkg.kernels

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--json", default="")
args = ap.parse_args()
B, dev = args.batch, "cuda"

# (name, H, Cin, Cout, stride, role): the eval path's residual-block convs at 224^2 (conv1 of block 0 is the strided one)
SHAPES = [("s1 conv1/conv2 3x3 64->64 @56", 56, 64, 64, 1, "conv2"),
          ("s2 conv1 3x3/2 64->128 @56", 56, 64, 128, 2, "conv1"), ("s2 conv2 3x3 128->128 @28", 28, 128, 128, 1, "conv2"),
          ("s3 conv1 3x3/2 128->256 @28", 28, 128, 256, 2, "conv1"), ("s3 conv2 3x3 256->256 @14", 14, 256, 256, 1, "conv2"),
          ("s4 conv1 3x3/2 256->512 @14", 14, 256, 512, 2, "conv1"), ("s4 conv2 3x3 512->512 @7", 7, 512, 512, 1, "conv2")]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


rows = []
g = torch.Generator(device=dev).manual_seed(0)
for name, H, C, N, stride, role in SHAPES:
    Ho = (H + 2 - 3) // stride + 1
    M = B * Ho * Ho
    x = torch.randn((B * H * H, C), device=dev, generator=g).relu_().to(torch.bfloat16)
    w = (torch.randn((N, 9 * C), device=dev, generator=g) * 0.05)
    wb = w.to(torch.bfloat16)
    bias = torch.randn(N, device=dev, generator=g)
    add = torch.randn((M, N), device=dev, generator=g).to(torch.bfloat16) if role == "conv2" else None
    xq, wq = K.mx_quant(x), K.mx_quant(w)
    geom = (B, H, H, C, Ho, Ho, 3, 3, stride, 1)
    relu = 2 if role == "conv2" else 1

    def bf():
        K.igemm(x, wb, M, N, 9 * C, geom, dtype=torch.bfloat16, bias=bias, addend=add, relu=relu)

    def mx():
        K.conv_mxfp8(xq, wq, M, N, geom, bias=bias, addend=add, relu=relu, want_bf16=(role == "conv2"), want_mx=(role == "conv1"))

    for _ in range(3):
        bf(); mx()
    torch.cuda.synchronize()
    ev = {"bf16": [], "mxfp8": []}
    for r in range(args.reps):
        order = (("bf16", bf), ("mxfp8", mx)) if r % 2 == 0 else (("mxfp8", mx), ("bf16", bf))
        for k, fn in order:
            ev[k].append(timed(fn))
    torch.cuda.synchronize()
    med = {k: statistics.median(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in ev.items()}
    fl = 2.0 * M * N * 9 * C
    row = dict(shape=name, M=M, N=N, K=9 * C, bf16_us=round(med["bf16"], 1), mxfp8_us=round(med["mxfp8"], 1),
               speedup=round(med["bf16"] / med["mxfp8"], 3), bf16_tflops=round(fl / med["bf16"] * 1e-6, 1),
               mxfp8_tflops=round(fl / med["mxfp8"] * 1e-6, 1))
    rows.append(row)
    print(f"{name:32s} bf16 {row['bf16_us']:8.1f} us  mxfp8 {row['mxfp8_us']:8.1f} us  x{row['speedup']:.2f}  "
          f"({row['bf16_tflops']:.0f} / {row['mxfp8_tflops']:.0f} TFLOP/s)", flush=True)
    del x, w, wb, add, xq, wq
q = torch.randn((B * 56 * 56, 64), device=dev, generator=g).to(torch.bfloat16)
ts = []
for _ in range(args.reps):
    ts.append(timed(lambda: K.mx_quant(q)))
torch.cuda.synchronize()
tq = statistics.median(a.elapsed_time(b) * 1e3 for a, b in ts)
print(f"mx_quant stage-1 input [{q.shape[0]} x 64] bf16: {tq:.1f} us ({q.numel() * (2 + 1 + 1 / 32) / tq * 1e-3:.0f} GB/s)", flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(batch=B, reps=args.reps, convs=rows, mx_quant_stage1_us=round(tq, 1)), f, indent=1)
