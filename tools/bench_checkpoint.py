"""What a checkpoint of HipTrainer costs (bf16, default configuration: 19.3 M parameters), with and without the weight average:

    python tools/bench_checkpoint.py [--out profiles/checkpoint_bench.json] [--reps 5]

    state_dict        trainer.state_dict(): the device-to-host copies of the flat buffers and the per-parameter clones
    torch_save        torch.save of {"model_state_dict", "optimizer_state_dict"} into memory (no disk in the figure)
    torch_load        torch.load(weights_only=True) of those bytes
    load_state_dict   trainer.load_state_dict() of the loaded dict: validation, the copies back, the synchronise that drops the graphs
    model_state_dict / model_load_state_dict   the model's own halves, for scale

A host clock around calls that end in a synchronise; median, min and max of --reps repetitions in ms, and the size of the saved
bytes.  There is no target: saving happens once per epoch, this is a cost to state.
"transfer_control" is the control of tests/test_gpu_trainer_state.py::test_a_transferred_state_continues_like_torch, at its shapes and
seeds: three fused fp32 steps against three steps of the torch loop (cross-entropy, clip_grad_norm_(1.0), torch.optim.AdamW), no
state transferred -- max |p - p_torch| and the share of elements above 1e-6, the two figures that test's bars are read against."""
import argparse
import importlib
import io
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
B = 32


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def run(sd, cfg, ema, reps):
    m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    tr = pkg.trainer.HipTrainer(m, ema_decay=0.999 if ema else None)
    images, ids, mask, answers = (t.to(DEV) for t in O.synthetic_batch(B, seed=7))
    mask[:, 0] = 1
    for _ in range(3):                                     # non-trivial moments, the operand copy in place
        tr.step(images, ids, mask, answers)
    t = {k: [] for k in ("state_dict", "model_state_dict", "torch_save", "torch_load", "load_state_dict", "model_load_state_dict")}
    nbytes = 0
    for _ in range(reps):
        ms, osd = clocked(tr.state_dict)
        t["state_dict"].append(ms)
        ms, msd = clocked(m.state_dict)
        t["model_state_dict"].append(ms)
        buf = io.BytesIO()
        ms, _ = clocked(lambda: torch.save({"model_state_dict": msd, "optimizer_state_dict": osd}, buf))
        t["torch_save"].append(ms)
        nbytes = buf.tell()
        buf.seek(0)
        ms, ck = clocked(lambda: torch.load(buf, weights_only=True))
        t["torch_load"].append(ms)
        ms, _ = clocked(lambda: m.load_state_dict(ck["model_state_dict"]))
        t["model_load_state_dict"].append(ms)
        ms, _ = clocked(lambda: tr.load_state_dict(ck["optimizer_state_dict"]))
        t["load_state_dict"].append(ms)
        tr.step(images, ids, mask, answers)                # the run goes on
    torch.cuda.synchronize()
    tr.check()
    return {"ms": {k: stats(v) for k, v in t.items()}, "saved_bytes": nbytes, "parameters": sum(e.numel for e in m._param_entries)}


def transfer_control():
    cfg = O.full_config(dropout=0.0, answer_dropout=0.0)
    sd = O.init_state_dict(cfg, 17, jitter=True)
    idx = torch.tensor([2, 0, 0, 2, 2, 0, 2])
    models = []
    for _ in range(2):
        m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="fp32")
        m.load_state_dict(sd)
        models.append(m.to(DEV).train())
    mt, mc = models
    opt = torch.optim.AdamW(mt.parameters(), lr=1e-4, weight_decay=0.01)
    tr = pkg.trainer.HipTrainer(mc)
    for k in range(3):
        images, _, _, _ = O.synthetic_batch(3, seed=71 + 10 * k)
        _, ids, mask, answers = O.synthetic_batch(7, seed=72 + 10 * k)
        mask[:, 0] = 1
        x, ids, mask, t = (v.to(DEV) for v in (images, ids, mask, answers))
        opt.zero_grad()
        logits, _ = mt.forward_grouped(x, ids, mask, image_index=idx)
        F.cross_entropy(logits.float(), t).backward()
        torch.nn.utils.clip_grad_norm_(list(mt.parameters()), 1.0)
        opt.step()
        tr.step(x, ids, mask, t, image_index=idx)
    torch.cuda.synchronize()
    d = (mc._flat.detach() - mt._flat.detach()).abs()
    return {"steps": 3, "max_abs_diff": d.max().item(), "share_above_1e-6": (d > 1e-6).float().mean().item(),
            "bars_of_one_step": {"max_abs_diff": 2.5e-4, "share_above_1e-6": 1e-3}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "checkpoint_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    cfg = O.full_config()
    sd = O.init_state_dict(cfg, 3, jitter=True)
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "clock": "time.perf_counter around calls that end in torch.cuda.synchronize",
           "reps": a.reps, "plain": run(sd, cfg, False, a.reps), "ema": run(sd, cfg, True, a.reps)}
    res["transfer_control"] = transfer_control()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for side in ("plain", "ema"):
        print(side, {k: round(v["median"], 2) for k, v in res[side]["ms"].items()}, "ms;", res[side]["saved_bytes"], "bytes")
    print("transfer_control", res["transfer_control"])


if __name__ == "__main__":
    main()
