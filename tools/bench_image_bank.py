"""The image bank, measured (one MI355X, bf16, default configuration, B = 512):

    python tools/bench_image_bank.py [--out profiles/image_bank_bench.json] [--reps 5] [--steps 10] [--kernel-iters 50]

Every comparison alternates its arms in one process after a warm-up and reports the median and min - max of `--reps` repetitions.
    kernel    vqa_bank_batch alone: 512 random rows of an 8192-row bank, S = 256 -> O = 224 with random origins and half of the samples
              flipped, and the pure gather O = S = 224; against vqa_gather_rows moving the same output bytes (512 rows of 150 528 B)
              from the same 224-side bank with the same index -- the existing yardstick for a gather of this size.  Device events
              around `--kernel-iters` back-to-back launches; GB/s = (read + write) bytes over the median.
    draw      a whole draw: bank.batch(rows, crop=224, flip_p=0.5, jitter=ColorJitter(0.2, 0.2, 0.2, 0.1)) against
              DeviceImageResizer(256, crop=224, jitter=...) on device-resident decoded 480 x 640 images and against gpu_collate_fn
              on host-resident ones (both output="bytes"); device events, and the host's time inside the call.
    step      HipTrainer.step fed by BankLoader against the same step on one fixed resident ByteImages batch (the ceiling) and
              against the step fed by gpu_collate_fn from host images; ms per step between device events, the host's enqueue time
              (the time the feeding and step() take to return) and the wall time per step.
The default step against the parent is tools/ab_lib.py's job (profiles/image_bank_ab_parent.txt)."""
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
B, BANK_ROWS, S, CROP = 512, 8192, 256, 224
JITTER = (0.2, 0.2, 0.2, 0.1)                       # data/preprocess.py:77-82


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def alternate(fns, reps, n, warm=3):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, n))
    return {k: stats(v) for k, v in t.items()}


def host_times(fns, reps, n):
    """Per call: host time inside fn (enqueue) and wall time of n back-to-back calls."""
    out = {k: {"enqueue_ms": [], "wall_ms": []} for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            host = []
            t0 = time.perf_counter()
            for _ in range(n):
                h0 = time.perf_counter()
                fn()
                host.append(time.perf_counter() - h0)
            torch.cuda.synchronize()
            out[k]["wall_ms"].append((time.perf_counter() - t0) / n * 1e3)
            out[k]["enqueue_ms"].append(statistics.median(host) * 1e3)
    return {k: {s: stats(v) for s, v in d.items()} for k, d in out.items()}


def random_bank(rows, side, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, 256, (rows, side, side, 3), generator=g, dtype=torch.uint8, device=DEV)


def kernel_bench(reps, iters):
    L, K = pkg._lib, pkg.kernels
    g = torch.Generator().manual_seed(11)
    rows = torch.randint(0, BANK_ROWS, (B,), generator=g).to(torch.int32).to(DEV)
    crop = torch.randint(0, S - CROP + 1, (B, 2), generator=g).to(torch.int32).to(DEV)
    flip = (torch.arange(B) % 2).to(torch.uint8)[torch.randperm(B, generator=g)].to(DEV)
    bank256, bank224 = random_bank(BANK_ROWS, S, 1), random_bank(BANK_ROWS, CROP, 2)
    out = torch.empty((B, CROP, CROP, 3), dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    flat224 = bank224.view(BANK_ROWS, -1)
    out_flat = out.view(B, -1)
    fns = {
        "bank_batch_256_to_224": lambda: L.call("vqa_bank_batch", bank256.data_ptr(), BANK_ROWS, S, rows.data_ptr(), crop.data_ptr(),
                                                flip.data_ptr(), out.data_ptr(), B, CROP, err.data_ptr()),
        "bank_batch_224_gather": lambda: L.call("vqa_bank_batch", bank224.data_ptr(), BANK_ROWS, CROP, rows.data_ptr(), None, None,
                                                out.data_ptr(), B, CROP, err.data_ptr()),
        "gather_rows_150528B": lambda: K.gather_rows(flat224, rows, out=out_flat),
    }
    fns["bank_batch_224_gather"]()
    assert torch.equal(out, bank224[rows.long()]) and int(err) == 0
    t = alternate(fns, reps, iters)
    nbytes = 2 * B * CROP * CROP * 3
    res = {"rows": B, "bank_rows": BANK_ROWS, "out_bytes_per_row": CROP * CROP * 3, "bytes_moved": nbytes, "iters": iters}
    for k, d in t.items():
        res[k] = {s: (v * 1e3 if not isinstance(v, list) else [x * 1e3 for x in v]) for s, v in d.items()}      # us
        res[k]["GBps_at_median"] = nbytes / (d["median"] * 1e-3) / 1e9
    y = res["gather_rows_150528B"]["median"]
    res["ratio_to_gather_rows"] = {k: res[k]["median"] / y for k in ("bank_batch_256_to_224", "bank_batch_224_gather")}
    del bank256, bank224
    torch.cuda.empty_cache()
    return res


def decoded_images(n_distinct=64):
    g = torch.Generator().manual_seed(5)
    base = [torch.randint(0, 256, (480, 640, 3), generator=g, dtype=torch.uint8) for _ in range(n_distinct)]
    return [base[i % n_distinct] for i in range(B)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "image_bank_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--draw-iters", type=int, default=4)
    a = ap.parse_args()
    P, IB = pkg.load_dropin_preprocess(), pkg.load_dropin_image_bank()
    res = {"batch": B, "dtype": "bf16", "bank_rows": BANK_ROWS, "bank_side": S, "crop": CROP, "jitter": JITTER, "reps": a.reps,
           "steps_per_rep": a.steps, "device": torch.cuda.get_device_name(0)}
    res["kernel_us"] = kernel_bench(a.reps, a.kernel_iters)

    # ---- a whole draw
    jitter = P.DeviceColorJitter(*JITTER)
    bank = IB.ImageBank(BANK_ROWS, size=S)
    for lo in range(0, BANK_ROWS, 1024):
        bank.append_resized(random_bank(1024, S, 100 + lo))
    res["bank_nbytes"] = bank.nbytes
    host_imgs = decoded_images()
    dev_imgs = [t.to(DEV) for t in host_imgs[:64]]
    dev_imgs = [dev_imgs[i % 64] for i in range(B)]
    items = [(im, torch.zeros(20, dtype=torch.long), torch.ones(20, dtype=torch.long), 0) for im in host_imgs]
    resizer_d = P.DeviceImageResizer(S, crop=CROP, jitter=jitter)
    resizer_h = P.DeviceImageResizer(S, crop=CROP, jitter=jitter)
    gen = torch.Generator().manual_seed(3)
    rows_cpu = torch.randint(0, BANK_ROWS, (B,), generator=gen)

    def resizer_draw():
        flip = torch.rand(B, generator=gen) < 0.5
        crop_yx = torch.randint(0, S - CROP + 1, (B, 2), generator=gen).tolist()
        return resizer_d(dev_imgs, crop_yx=crop_yx, flip=flip, generator=gen, output="bytes")

    draws = {
        "bank_batch": lambda: bank.batch(rows_cpu, crop=CROP, flip_p=0.5, jitter=jitter, generator=gen),
        "bank_batch_no_jitter": lambda: bank.batch(rows_cpu, crop=CROP, flip_p=0.5, generator=gen),
        "resizer_device_images": resizer_draw,
        "gpu_collate_host_images": lambda: P.gpu_collate_fn(items, flip_p=0.5, generator=gen, resizer=resizer_h, output="bytes"),
    }
    res["draw_ms"] = alternate(draws, a.reps, a.draw_iters, warm=2)
    res["draw_host_ms"] = host_times(draws, a.reps, a.draw_iters)

    # ---- a fed step
    cfg = O.full_config()
    sd = O.init_state_dict(cfg, 3, jitter=True)

    def trainer():
        m = pkg.load_dropin().VQAModel(**cfg, compute_dtype="bf16")
        m.load_state_dict(sd)
        return pkg.trainer.HipTrainer(m.to(DEV).train())

    N = 2 * BANK_ROWS
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, 1000, (N, 20), generator=g)
    mask = torch.ones(N, 20, dtype=torch.long)
    answers = torch.randint(0, 1000, (N,), generator=g)
    image_row = torch.randint(0, BANK_ROWS, (N,), generator=g)
    loader = IB.BankLoader(bank, image_row, ids, mask, answers, batch_size=B, drop_last=True, seed=1, crop=CROP, flip_p=0.5, jitter=jitter)

    def batches():
        epoch = 0
        while True:
            loader.set_epoch(epoch)
            yield from loader
            epoch += 1

    feed = batches()
    trainers = {k: trainer() for k in ("resident", "bank_loader", "gpu_collate")}
    fixed = bank.batch(rows_cpu, crop=CROP, flip_p=0.5, jitter=jitter, generator=gen)
    ids_d, mask_d, ans_d = ids[:B].to(DEV), mask[:B].to(DEV), answers[:B].to(DEV)

    def step_bank():
        b = next(feed)
        trainers["bank_loader"].step(b["images"], b["token_ids"], b["attention_mask"], b["answers"])

    def step_collate():
        b = P.gpu_collate_fn(items, flip_p=0.5, generator=gen, resizer=resizer_h, output="bytes")
        trainers["gpu_collate"].step(b["images"], ids_d, mask_d, ans_d)

    steps = {"resident": lambda: trainers["resident"].step(fixed, ids_d, mask_d, ans_d), "bank_loader": step_bank, "gpu_collate": step_collate}
    res["step_ms"] = alternate(steps, a.reps, a.steps)
    res["step_host_ms"] = host_times(steps, a.reps, a.steps)
    for tr in trainers.values():
        tr.check()
    res["bad_rows"] = int(bank.bad_rows)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    k = res["kernel_us"]
    for n in ("bank_batch_256_to_224", "bank_batch_224_gather", "gather_rows_150528B"):
        print("kernel", n, "us [median, min, max]", [round(k[n][s], 2) for s in ("median", "min", "max")], "GB/s", round(k[n]["GBps_at_median"], 1))
    print("ratio to gather_rows", json.dumps({n: round(v, 3) for n, v in k["ratio_to_gather_rows"].items()}))
    short = lambda d: {n: [round(v["median"], 3), round(v["min"], 3), round(v["max"], 3)] for n, v in d.items()}
    print("draw_ms [median, min, max]", json.dumps(short(res["draw_ms"])))
    print("draw host enqueue_ms", json.dumps({n: round(v["enqueue_ms"]["median"], 3) for n, v in res["draw_host_ms"].items()}))
    print("step_ms [median, min, max]", json.dumps(short(res["step_ms"])))
    print("step host enqueue_ms", json.dumps({n: round(v["enqueue_ms"]["median"], 3) for n, v in res["step_host_ms"].items()}),
          "wall_ms", json.dumps({n: round(v["wall_ms"]["median"], 3) for n, v in res["step_host_ms"].items()}))


if __name__ == "__main__":
    main()
