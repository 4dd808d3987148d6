"""Cost of gradients with respect to the input images (measurement tool), one JSON line:
  kernels:  the stem data gradient in isolation at B=64 and 512 (224x224): the fused bf16 kernel (dy rebuilt from y / dpool /
            argmax), the generic bf16 kernel on a materialised dy, the generic pair vqa_stem_bwd_apply + generic dgrad, and the
            generic fp32 kernel; median of device-event times per launch, with the algorithmic bytes and the rate they imply.
  step:     the drop-in's bf16 training step at B=512 through autograd, with and without images.requires_grad (alternating blocks).
  saliency: a frozen eval model (requires_grad_(False)), forward + torch.autograd.grad(logits[:, c].sum(), images) at B=1/8/64.
    python tools/bench_input_grad.py [--steps 20] [--warmup 5] [--rounds 3] [--skip-step] [--kernels-only]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _time(fn, n, warmup=3):
    for _ in range(warmup):
        fn()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    evs[0].record()
    for i in range(n):
        fn()
        evs[i + 1].record()
    torch.cuda.synchronize()
    return [evs[i].elapsed_time(evs[i + 1]) for i in range(n)]


def kernels(pkg, B, n):
    K, L = pkg.kernels, pkg._lib
    H = W = 224
    Ho = Wo = 112
    Hp = Wp = 56
    g = torch.Generator(device="cuda").manual_seed(B)
    y = torch.randn(B * Ho * Wo, 64, device="cuda", generator=g).to(torch.bfloat16)
    dpool = torch.randn(B * Hp * Wp, 64, device="cuda", generator=g).to(torch.bfloat16)
    idx = torch.randint(0, 9, (B * Hp * Wp, 64), device="cuda", generator=g, dtype=torch.uint8)
    coef = torch.cat([torch.rand(64, device="cuda", generator=g) + 0.5, torch.randn(64, device="cuda", generator=g), torch.zeros(128, device="cuda")])
    bc = torch.randn(3, 64, device="cuda", generator=g)
    w = torch.randn(64, 7, 7, 3, device="cuda", generator=g) * 0.1
    wpk = K.stem_dgrad_pack(w, torch.bfloat16)
    wpk32 = K.stem_dgrad_pack(w, torch.float32)
    dy = torch.empty_like(y)

    def apply(dt=torch.bfloat16, out=dy):
        L.call("vqa_stem_bwd_apply", L.dt(dt), dpool.data_ptr() if dt == torch.bfloat16 else dpool32.data_ptr(), idx.data_ptr(),
               y.data_ptr() if dt == torch.bfloat16 else y32.data_ptr(), coef.data_ptr(), bc.data_ptr(), out.data_ptr(), B, Ho, Wo, 64)
    apply()
    img_bytes = B * 3 * H * W * 4
    res = {}
    t = statistics.median(_time(lambda: K.stem_dgrad_fused(y, dpool, idx, coef, bc, wpk, B, H, W), n))
    nb = y.numel() * 2 + dpool.numel() * 3 + img_bytes
    res["fused_bf16_ms"], res["fused_bf16_GBps"] = t, nb / t / 1e6
    t = statistics.median(_time(lambda: K.stem_dgrad(dy, wpk, B, H, W), n))
    res["generic_bf16_ms"], res["generic_bf16_GBps"] = t, (dy.numel() * 2 + img_bytes) / t / 1e6
    res["apply_plus_generic_bf16_ms"] = statistics.median(_time(lambda: (apply(), K.stem_dgrad(dy, wpk, B, H, W)), n))
    if B <= 64:
        dpool32, y32 = dpool.float(), y.float()
        dy32 = torch.empty_like(y32)
        apply(torch.float32, dy32)
        t = statistics.median(_time(lambda: K.stem_dgrad(dy32, wpk32, B, H, W), n))
        res["generic_fp32_ms"], res["generic_fp32_GBps"] = t, (dy32.numel() * 4 + img_bytes) / t / 1e6
    res["pack_ms"] = statistics.median(_time(lambda: K.stem_dgrad_pack(w, torch.bfloat16), n))
    res["fused_algorithmic_bytes"] = nb
    return res


def step(pkg, a):
    model = pkg.load_dropin().VQAModel(compute_dtype="bf16", seed=1).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(2)
    B, L = 512, 20
    images = torch.randn(B, 3, 224, 224, device="cuda", generator=g)
    ids = torch.randint(1, 10000, (B, L), device="cuda", generator=g)
    mask = torch.ones(B, L, device="cuda", dtype=torch.long)
    answers = torch.randint(0, 1000, (B,), device="cuda", generator=g)

    def one(want):
        img = images.requires_grad_(want)
        logits, _ = model(img, ids, mask)
        torch.nn.functional.cross_entropy(logits.float(), answers).backward()
        model.zero_grad(set_to_none=True)
        img.grad = None

    ms = {False: [], True: []}
    for v in (False, True):
        _time(lambda: one(v), 1, warmup=a.warmup)
    for _ in range(a.rounds):
        for v in (False, True):
            ms[v] += _time(lambda: one(v), a.steps, warmup=0)
    images.requires_grad_(False)
    out = {"batch": B, "plain_ms_median": statistics.median(ms[False]), "input_grad_ms_median": statistics.median(ms[True])}
    out["overhead_ms"] = out["input_grad_ms_median"] - out["plain_ms_median"]
    return out


def saliency(pkg, a):
    model = pkg.load_dropin().VQAModel(compute_dtype="bf16", seed=1).cuda().eval().requires_grad_(False)
    out = {}
    for B in (1, 8, 64):
        g = torch.Generator(device="cuda").manual_seed(3)
        images = torch.randn(B, 3, 224, 224, device="cuda", generator=g)
        ids = torch.randint(1, 10000, (B, 20), device="cuda", generator=g)
        mask = torch.ones(B, 20, device="cuda", dtype=torch.long)

        def one():
            img = images.detach().requires_grad_(True)
            logits, _ = model(img, ids, mask)
            torch.autograd.grad(logits[:, 0].sum(), img)

        def infer():
            with torch.no_grad():
                model(images, ids, mask)
        out[f"B{B}_forward_plus_grad_ms"] = statistics.median(_time(one, a.steps, warmup=a.warmup))
        out[f"B{B}_no_grad_forward_ms"] = statistics.median(_time(infer, a.steps, warmup=a.warmup))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="only the isolated kernels (profiler passes)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    sys.path.insert(0, REPO)
    pkg = importlib.import_module("visual-question-answering-vqa-system_amd")
    importlib.import_module("visual-question-answering-vqa-system_amd.kernels")
    out = {"device": torch.cuda.get_device_name(0), "kernels": {f"B{B}": kernels(pkg, B, a.steps) for B in (64, 512)}}
    torch.cuda.empty_cache()
    if a.kernels_only:
        print(json.dumps(out))
        return out
    if not a.skip_step:
        out["train_step_bf16"] = step(pkg, a)
        torch.cuda.empty_cache()
    out["saliency_bf16"] = saliency(pkg, a)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
