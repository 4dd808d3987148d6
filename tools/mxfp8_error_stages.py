"""Where the MXFP8 eval path loses accuracy: per-residual-block error of the bf16 and the mxfp8 eval against the fp32-compute eval of
the same weights, on tests/test_gpu_mxfp8.py's quality setup (full config, init seed 10 with jitter, 30 HipTrainer steps at B = 64 on
seeded synthetic data, then an eval batch of 32, seed 77).  Per block: relative L2 error and cosine of the block output, and the
relative L2 error that MXFP8 quantization alone puts on the block's fp32 input (the noise one quantized operand carries).  Also the
final image_features cosine and logits relative L2 the test asserts.  Not part of the product; the output is quoted in DESIGN.md."""
import argparse
import importlib
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import vqa_oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default="")
args = ap.parse_args()
pkg = importlib.import_module("visual-question-answering-vqa-system_amd")
K = pkg.kernels
M = pkg.load_dropin()
dev = "cuda"

cfg = O.full_config()
m = M.VQAModel(**cfg, compute_dtype="bf16")
m.load_state_dict(O.init_state_dict(cfg, 10, jitter=True))
m = m.to(dev).train()
tr = pkg.trainer.HipTrainer(m, lr=1e-4)
for step in range(30):
    images, ids, mask, answers = O.synthetic_batch(64, seed=1000 + step)
    tr.step(images.to(dev), ids.to(dev), mask.to(dev), answers.to(dev))
m.eval()
ref = M.VQAModel(**cfg, compute_dtype="fp32")
ref.load_state_dict(m.state_dict())
ref = ref.to(dev).eval()
images, ids, mask, _ = O.synthetic_batch(32, seed=77)
a = (images.to(dev), ids.to(dev), mask.to(dev))


def rel(x, y):
    return float((x.float() - y.float()).norm() / y.float().norm())


def dequant(q, s):
    v = q.view(torch.float8_e4m3fn).float()
    return (v.view(v.shape[0], -1, 32) * torch.exp2(s.float() - 127)[..., None]).view(v.shape)


out = {"setup": "full config, init seed 10 (jitter), 30 HipTrainer steps B=64, eval B=32 seed 77", "blocks": {}, "final": {}}
rec = {}
with torch.no_grad():
    lr_, ar = ref(*a, return_aux=True)
    rf = {}
    ref._ensure_engine().forward(a[0], a[1], a[2].float(), False, False, need_tape=False, record=rf)
    for prec in ("bf16", "mxfp8"):
        m.set_inference_precision(prec)
        lm, am = m(*a, return_aux=True)
        fm, fr = am["image_features"].float().flatten(1), ar["image_features"].float().flatten(1)
        out["final"][prec] = dict(image_features_mean_cosine=round(F.cosine_similarity(fm, fr, dim=1).mean().item(), 4),
                                  logits_rel_l2=round(rel(lm, lr_), 4))
        r = {}
        m._ensure_engine().forward(a[0], a[1], a[2].float(), False, False, need_tape=False, record=r)
        rec[prec] = r
    for k in rf:
        if k.endswith(".a1"):                      # conv1's output of the block: not compared here
            continue
        x32, o32 = rf[k]
        q, s = K.mx_quant(x32)
        row = dict(input_quant_rel_l2=round(rel(dequant(q, s), x32), 4))
        for prec in ("bf16", "mxfp8"):
            o = rec[prec][k][1]
            row[prec] = dict(out_rel_l2=round(rel(o, o32), 4),
                             out_cosine=round(float(F.cosine_similarity(o.float().flatten(), o32.float().flatten(), dim=0)), 5),
                             in_rel_l2=round(rel(rec[prec][k][0], x32), 4))
        out["blocks"][k] = row
        print(k, json.dumps(row), flush=True)
print(json.dumps(out["final"]), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
