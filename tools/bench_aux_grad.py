"""Cost of a training step with graph-connected aux outputs (measurement tool): the drop-in's step through autograd at B=512 bf16,
    plain:  logits = model(...);                        CE(logits).backward()
    aux:    logits, aux = model(..., return_aux=True);   (CE(logits) + sum_k <R_k, aux_k>).backward()   (all seven keys)
timed with device events per step, the two variants alternating in blocks after a warm-up of each.  One JSON line.
    python tools/bench_aux_grad.py [--batch 512] [--steps 20] [--warmup 5] [--rounds 3] [--dtype bf16]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("image_features", "text_features", "text_pooled", "fused", "image_projected", "attended_pooled")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    sys.path.insert(0, REPO)
    pkg = importlib.import_module("visual-question-answering-vqa-system_amd")
    model = pkg.load_dropin().VQAModel(compute_dtype=a.dtype, seed=1).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(2)
    B, L = a.batch, 20
    images = torch.randn(B, 3, 224, 224, device="cuda", generator=g)
    ids = torch.randint(1, 10000, (B, L), device="cuda", generator=g)
    mask = torch.ones(B, L, device="cuda", dtype=torch.long)
    answers = torch.randint(0, 1000, (B,), device="cuda", generator=g)
    _, aux = model(images, ids, mask, return_aux=True)
    R = {k: torch.randn(aux[k].shape, device="cuda", generator=g) * 1e-3 for k in KEYS}
    R["cross_attention_weights"] = [torch.randn(w.shape, device="cuda", generator=g) * 1e-3 for w in aux["cross_attention_weights"]]
    del aux
    model.zero_grad(set_to_none=True)

    def step(with_aux):
        if with_aux:
            logits, aux = model(images, ids, mask, return_aux=True)
            loss = torch.nn.functional.cross_entropy(logits.float(), answers)
            loss = loss + sum((aux[k] * R[k]).sum() for k in KEYS)
            loss = loss + sum((w * r).sum() for w, r in zip(aux["cross_attention_weights"], R["cross_attention_weights"]))
        else:
            logits, _ = model(images, ids, mask)
            loss = torch.nn.functional.cross_entropy(logits.float(), answers)
        loss.backward()
        model.zero_grad(set_to_none=True)

    def block(with_aux, n):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        evs[0].record()
        for i in range(n):
            step(with_aux)
            evs[i + 1].record()
        torch.cuda.synchronize()
        return [evs[i].elapsed_time(evs[i + 1]) for i in range(n)]

    for v in (False, True):
        block(v, a.warmup)
    ms = {"plain": [], "aux": []}
    for _ in range(a.rounds):
        for v, name in ((False, "plain"), (True, "aux")):
            ms[name] += block(v, a.steps)
    out = {"batch": B, "dtype": a.dtype, "steps_per_variant": len(ms["plain"]),
           "plain_ms_median": statistics.median(ms["plain"]), "aux_ms_median": statistics.median(ms["aux"]),
           "plain_ms_min": min(ms["plain"]), "aux_ms_min": min(ms["aux"])}
    out["aux_over_plain"] = out["aux_ms_median"] / out["plain_ms_median"]
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
