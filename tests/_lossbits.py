"""The outputs of everything that reads the answer logits (csrc/loss_ops.hip) as SHA-256 digests: the inputs, the cases and the launches
shared by tests/golden/make_loss_bits.py (which records tests/golden/loss_bits.json) and tests/test_gpu_loss_bits.py (which compares).

Inputs come from _optbits' closed integer formula (bf16 inputs are the fp32 values rounded once); every entry runs once per case on
fresh buffers.  Output buffers start as _optbits' sentinel NaN patterns (counters, which are added to, as non-zero integers), and the
whole buffers are hashed: a missed or a stray write shows.  With ws == nullptr the loss is a sum of float atomics in arrival order: it
is not hashed there but held against the fp64 sum of the same inputs' ws run (whose row terms are pinned), see _loss_near()."""
import functools

import numpy as np
import torch

from _optbits import DEV, SENT16, SENT32, digest, fill, toolchain, unit  # noqa: F401  (toolchain: for the recorder and the test)
from _pkg import sub

F32, BF16 = torch.float32, torch.bfloat16
# (B, N, K): N below, at and just past one lane trip and several trips with a remainder; B a partly filled workgroup and more than 64
# rows (the opts form's sum over all targets takes a second trip); K slots per row = A annotators
SHAPES = ((1, 1, 1), (4, 63, 3), (5, 64, 10), (70, 65, 64), (4, 200, 10))
MID = (5, 65)                       # the shape of the variants that do not depend on the shape
IGN = -100
DT = {"fp32": F32, "bf16": BF16}


def ints(n, salt, lo, hi):
    """int64 values in [lo, hi) from the integer hash"""
    return torch.from_numpy(lo + np.floor(unit(n, salt) * (hi - lo)).astype(np.int64))


def logits(kind, B, N, dtype):
    """std: [-8, 8); ties: multiples of 0.5 in [-8, 8) (the row maximum and the target's value tie); pm300 / pm90: wide rows"""
    if kind == "pm300":
        x = fill(B * N, 11, -8.0, 8.0).view(B, N) + 300.0 * (1 - 2 * (torch.arange(B) % 2)).float()[:, None]
    elif kind == "pm90":
        x = fill(B * N, 12, -90.0, 90.0).view(B, N)
    else:
        x = fill(B * N, 10, -8.0, 8.0).view(B, N)
        if kind == "ties":
            x = torch.floor(x * 2.0) / 2.0
    return x.to(dtype).to(DEV).contiguous()


def sent(shape, dtype):
    n = int(np.prod(shape))
    if dtype == BF16:
        return torch.full((n,), SENT16, dtype=torch.int16).view(BF16).to(DEV).view(shape)
    t = torch.full((n,), SENT32, dtype=torch.int32)
    return (t.view(F32) if dtype == F32 else t).to(DEV).view(shape)


def counters(n):
    return (torch.arange(n, dtype=torch.int64) * 1000 + 7).to(DEV)          # added to: a plain store would show


def _loss_near(loss, terms, what):
    """loss (float atomics, any order) against t = fp64 sum of the pinned row terms: |loss - t| <= (B - 1) * 2^-24 * sum |term|"""
    t64 = terms.double().cpu()
    if bool(torch.isnan(t64).any()):
        assert bool(torch.isnan(loss).all()), f"{what}: a NaN row term but loss = {loss.item()}"
        return
    d, bound = abs(float(loss.double().cpu()) - float(t64.sum())), (t64.numel() - 1) * 2.0 ** -24 * float(t64.abs().sum())
    assert d <= bound, f"{what}: |loss - sum of the row terms| = {d:.3e} > {bound:.3e}"


def _launch_loss(entry, head, tail, x, B, N, gscale, null):
    """One launch of a loss entry: (dtype, logits, *head, loss, dlogits, logits_f32, B, N, gscale, err, ws, *tail).  Returns the buffers."""
    L = sub("_lib")
    bufs = {"loss": torch.zeros(1, device=DEV), "dlogits": sent((B, N), x.dtype), "logits_f32": sent((B, N), F32),
            "err": torch.zeros(1, dtype=torch.int32, device=DEV), "ws": sent((B,), F32)}
    a = {k: (None if k in null else v.data_ptr()) for k, v in bufs.items()}
    L.call(entry, L.dt(x), x.data_ptr(), *head, a["loss"], a["dlogits"], a["logits_f32"], B, N, gscale, a["err"], a["ws"], *tail)
    return bufs


def _loss_case(entry, head, tail, extra, x, gscale, null):
    """extra: name -> (zeroed or counter buffer, position in tail) that the launch adds to; a fresh copy per launch"""
    B, N = x.shape
    def run(nul):
        ex = {k: v.clone() for k, (v, _) in extra.items()}
        tl = list(tail)
        for k, (_, pos) in extra.items():
            tl[pos] = ex[k].data_ptr()
        bufs = _launch_loss(entry, head, tl, x, B, N, gscale, nul)
        bufs.update(ex)
        torch.cuda.synchronize()
        return bufs
    bufs = run(null)
    if "ws" in null and "loss" not in null:
        _loss_near(bufs.pop("loss"), run(tuple(k for k in null if k != "ws"))["ws"], entry)
    return {k: digest(v) for k, v in bufs.items()}


# ------------------------------------------------------------------------------------------------------------------ hard targets
def targets(kind, B, N):
    t = ints(B, 20, 0, N)
    if kind == "bad":                       # a row with target N and a row with target -1
        t[1], t[3] = N, -1
    elif kind == "ignored":                 # every third row
        t[1::3] = IGN
    elif kind == "all-ignored":
        t[:] = IGN
    elif kind == "bad-among-ignored":
        t[:] = IGN
        t[2] = N
    return t.to(DEV)


def class_weights(N, t):
    """in [0.1, 1.1), one of them zero: the class of the last row's target when that is a class"""
    w = fill(N, 21, 0.1, 1.1).clone()
    z = int(t[-1])
    w[z if 0 <= z < N else N // 2] = 0.0
    return w.to(DEV)


def hard_case(opts, dname, B, N, kind="std", tkind="valid", null=(), gscale=1.0, cw=False, ignore=False, eps=0.0, acc=False):
    x, t = logits(kind, B, N, DT[dname]), targets(tkind, B, N)
    if not opts:
        return _loss_case("vqa_cross_entropy", (t.data_ptr(),), (), {}, x, gscale, null)
    w = class_weights(N, t) if cw else None
    extra = {"empty": (torch.zeros(1, dtype=torch.int32, device=DEV), 5)}
    if acc:
        extra["acc"] = (counters(3), 4)
    out = _loss_case("vqa_cross_entropy_opts", (t.data_ptr(),), [sub("_lib").ptr(w), IGN, int(ignore), eps, None, None], extra, x, gscale, null)
    del w
    return out


# ------------------------------------------------------------------------------------------------------------------ soft targets
def answers(B, A, N, kind="std"):
    """annotator ids [B][A]: -1 (not in the vocabulary) and at most five classes per row, so that annotators agree"""
    a = ints(B * A, 30, -1, min(N, 5)).view(B, A)
    a = torch.where(a >= 0, (a * 37 + torch.arange(B)[:, None]) % N, a)
    if kind == "bad":                       # out-of-range answers reject their rows
        a[0, A - 1] = N + 3
        a[B - 1, 0] = -5
    return a.to(DEV).contiguous()


def _scores(a, N, mode):
    B, A = a.shape
    out = {"ids": sent((B, A), torch.int32), "weights": sent((B, A), F32), "counts": sent((B, A), torch.int32),
           "err": torch.zeros(1, dtype=torch.int32, device=DEV)}
    sub("_lib").call("vqa_answer_scores", a.data_ptr(), out["ids"].data_ptr(), out["weights"].data_ptr(), out["counts"].data_ptr(), B, A, N, mode,
                     out["err"].data_ptr())
    return out


def slots(kind, B, K, N):
    """ids, weights, counts [B][K].  scores: vqa_answer_scores of hashed annotator ids; hand: hashed slots with a duplicate id (row 0)
    and an empty row (row 1); hand-bad: also an id N (row 2, slot 0) and an id -2 (row 3, last slot)"""
    if kind == "scores":
        s = _scores(answers(B, K, N), N, 0)
        return s["ids"], s["weights"], s["counts"]
    ids, w, cnt = ints(B * K, 31, -1, N).view(B, K).int(), fill(B * K, 32, 0.0, 1.0).view(B, K).clone(), ints(B * K, 33, 0, 5).view(B, K).int()
    ids[0, K - 1] = ids[0, 0] = min(2, N - 1)
    ids[1, :] = -1
    if kind == "hand-bad":
        ids[2, 0], ids[3, K - 1] = N, -2
    return ids.to(DEV).contiguous(), w.to(DEV).contiguous(), cnt.to(DEV).contiguous()


def soft_case(entry, dname, B, N, K, skind="scores", kind="std", null=(), gscale=1.0, acc=False):
    x = logits(kind, B, N, DT[dname])
    ids, w, cnt = slots(skind, B, K, N)
    extra = {"acc": (counters(2), 1)} if acc else {}
    return _loss_case(entry, (ids.data_ptr(), w.data_ptr(), K), [cnt.data_ptr() if acc else None, None], extra, x, gscale, null)


# ------------------------------------------------------------------------------------------------------------------ metrics, scores, top-k
def accuracy_case(B, N, kind, tkind):
    x, t, c = logits(kind, B, N, F32), targets(tkind, B, N), counters(3)
    sub("_lib").call("vqa_accuracy_update", x.data_ptr(), t.data_ptr(), c.data_ptr(), B, N)
    torch.cuda.synchronize()
    return {"counters": digest(c)}


def challenge_case(B, N, K, kind, skind):
    x, c = logits(kind, B, N, F32), counters(2)
    ids, _, cnt = slots(skind, B, K, N)
    sub("_lib").call("vqa_challenge_accuracy_update", x.data_ptr(), ids.data_ptr(), cnt.data_ptr(), K, c.data_ptr(), B, N)
    torch.cuda.synchronize()
    return {"acc": digest(c)}


def scores_case(B, A, N, mode, kind):
    out = _scores(answers(B, A, N, kind), N, mode)
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in out.items()}


def topk_case(dname, B, N, K, allowed="none", pad=0, scale=1.0):
    """allowed: none | shared [N] | rows [B][N] (row 0 with nothing allowed); pad: ld = N + pad, the padding holds values that would win"""
    ld = N + pad
    buf = torch.full((B, ld), 1.0e4, dtype=DT[dname], device=DEV)
    buf[:, :N] = logits("std", B, N, DT[dname])
    al, ald = None, 0
    if allowed != "none":
        al = (ints((B if allowed == "rows" else 1) * N, 40, 0, 4) > 0).to(torch.uint8).view(-1, N)
        if allowed == "rows":
            al[0, :], ald = 0, N
        al = al.to(DEV).contiguous()
    out = {"idx": torch.full((B, K), -7777, dtype=torch.int64, device=DEV), "probs": sent((B, K), F32), "logits_f": sent((B, N), F32)}
    L = sub("_lib")
    L.call("vqa_softmax_topk", L.dt(buf), buf.data_ptr(), ld, L.ptr(al), ald, scale, out["idx"].data_ptr(), out["probs"].data_ptr(),
           out["logits_f"].data_ptr(), B, N, K)
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------------ the cases
def cases():
    """name -> thunk returning {buffer name: sha256}.  Every entry runs at the five SHAPES (every N, B and K above); what does not depend
    on the shape runs at MID, and what sums over all B targets also at the 70-row shape."""
    c, P = {}, functools.partial
    for d in DT:
        for opts, e in ((False, "vqa_cross_entropy"), (True, "vqa_cross_entropy_opts")):
            for B, N, _ in SHAPES:
                c[f"{e}/{d}/{B}x{N}/valid"] = P(hard_case, opts, d, B, N)
            B, N = MID
            c[f"{e}/{d}/{B}x{N}/bad-targets"] = P(hard_case, opts, d, B, N, tkind="bad")
            c[f"{e}/{d}/{B}x{N}/ties"] = P(hard_case, opts, d, B, N, kind="ties", acc=opts)
            c[f"{e}/{d}/{B}x{N}/pm300"] = P(hard_case, opts, d, B, N, kind="pm300")
            c[f"{e}/{d}/{B}x{N}/gscale0.5"] = P(hard_case, opts, d, B, N, gscale=0.5)
            for nul in ("dlogits", "logits_f32", "loss", "err", "ws"):
                c[f"{e}/{d}/{B}x{N}/no-{nul}"] = P(hard_case, opts, d, B, N, null=(nul,))
            c[f"{e}/{d}/{B}x{N}/bad-targets/no-ws"] = P(hard_case, opts, d, B, N, tkind="bad", null=("ws",))
        e = "vqa_cross_entropy_opts"
        for B, N in (MID, (70, 65)):
            c[f"{e}/{d}/{B}x{N}/weights"] = P(hard_case, True, d, B, N, cw=True)
            c[f"{e}/{d}/{B}x{N}/ignore"] = P(hard_case, True, d, B, N, tkind="ignored", ignore=True)
            c[f"{e}/{d}/{B}x{N}/smoothing"] = P(hard_case, True, d, B, N, eps=0.1)
            for acc in (False, True):
                c[f"{e}/{d}/{B}x{N}/all-three{'/acc' if acc else ''}"] = P(hard_case, True, d, B, N, tkind="ignored", cw=True, ignore=True, eps=0.1, acc=acc,
                                                                         gscale=0.5)
        B, N = MID
        for cw in (False, True):
            tag = "/weights" if cw else ""
            c[f"{e}/{d}/{B}x{N}/all-ignored{tag}"] = P(hard_case, True, d, B, N, tkind="all-ignored", ignore=True, cw=cw, acc=True)
            c[f"{e}/{d}/{B}x{N}/bad-among-ignored{tag}"] = P(hard_case, True, d, B, N, tkind="bad-among-ignored", ignore=True, cw=cw, acc=True)
        c[f"{e}/{d}/{B}x{N}/all-three/pm300"] = P(hard_case, True, d, B, N, kind="pm300", tkind="ignored", cw=True, ignore=True, eps=0.1)
        c[f"{e}/{d}/{B}x{N}/all-three/no-ws"] = P(hard_case, True, d, B, N, tkind="ignored", cw=True, ignore=True, eps=0.1, null=("ws",))
        for e in ("vqa_cross_entropy_soft", "vqa_bce_soft"):
            for B, N, K in SHAPES:
                for acc in (False, True):
                    c[f"{e}/{d}/{B}x{N}/k{K}/scores{'/acc' if acc else ''}"] = P(soft_case, e, d, B, N, K, acc=acc)
            B, N = MID
            c[f"{e}/{d}/{B}x{N}/k10/ties/acc"] = P(soft_case, e, d, B, N, 10, kind="ties", acc=True)
            for K in (3, 64):
                c[f"{e}/{d}/{B}x{N}/k{K}/hand"] = P(soft_case, e, d, B, N, K, skind="hand")
                c[f"{e}/{d}/{B}x{N}/k{K}/hand-bad/acc"] = P(soft_case, e, d, B, N, K, skind="hand-bad", acc=True)
            c[f"{e}/{d}/{B}x{N}/k3/hand-bad/no-ws"] = P(soft_case, e, d, B, N, 3, skind="hand-bad", null=("ws",))
            c[f"{e}/{d}/{B}x{N}/k10/gscale0.5"] = P(soft_case, e, d, B, N, 10, gscale=0.5)
            c[f"{e}/{d}/{B}x{N}/k10/pm300"] = P(soft_case, e, d, B, N, 10, kind="pm300", acc=True)
            for nul in ("dlogits", "logits_f32", "loss", "err", "ws"):
                c[f"{e}/{d}/{B}x{N}/k10/no-{nul}"] = P(soft_case, e, d, B, N, 10, null=(nul,))
            c[f"{e}/{d}/{B}x{N}/k10/no-dlogits-no-logits_f32/acc"] = P(soft_case, e, d, B, N, 10, null=("dlogits", "logits_f32"), acc=True)
        c[f"vqa_bce_soft/{d}/{B}x{N}/k10/pm90"] = P(soft_case, "vqa_bce_soft", d, B, N, 10, kind="pm90", acc=True)
        for B, N, K in ((1, 1, 1), (4, 63, 5), (5, 64, 64), (70, 65, 5), (4, 200, 64)):
            c[f"vqa_softmax_topk/{d}/{B}x{N}/k{K}"] = P(topk_case, d, B, N, K)
            c[f"vqa_softmax_topk/{d}/{B}x{N}/k{K}/shared-allowed"] = P(topk_case, d, B, N, K, allowed="shared", scale=0.5)
            c[f"vqa_softmax_topk/{d}/{B}x{N}/k{K}/row-allowed/ld+3"] = P(topk_case, d, B, N, K, allowed="rows", pad=3)
    for B, N, K in SHAPES:
        c[f"vqa_accuracy_update/{B}x{N}/ties"] = P(accuracy_case, B, N, "ties", "valid")
        c[f"vqa_challenge_accuracy_update/{B}x{N}/k{K}/ties"] = P(challenge_case, B, N, K, "ties", "scores")
        for mode in (0, 1):
            c[f"vqa_answer_scores/{B}x{N}/a{K}/mode{mode}"] = P(scores_case, B, K, N, mode, "std")
    B, N = MID
    c[f"vqa_accuracy_update/{B}x{N}/bad-targets"] = P(accuracy_case, B, N, "std", "bad")
    c[f"vqa_challenge_accuracy_update/{B}x{N}/k3/hand-bad"] = P(challenge_case, B, N, 3, "std", "hand-bad")
    for A in (3, 64):
        for mode in (0, 1):
            c[f"vqa_answer_scores/{B}x{N}/a{A}/mode{mode}/out-of-range"] = P(scores_case, B, A, N, mode, "bad")
    return c
