"""The outputs of the attention entries (csrc/attention.hip) as SHA-256 digests: the inputs, the cases and the launches shared by
tests/golden/make_attention_bits.py (which records tests/golden/attention_bits.json) and tests/test_gpu_attention_bits.py (which compares).

Inputs come from _optbits' closed integer formula (bf16 inputs are the fp32 values rounded once).  Every output buffer starts as
_optbits' sentinel NaN pattern and is hashed whole, the gaps a row stride leaves between rows included: a missed or a stray write
shows.  No attention kernel uses float atomics, so every buffer is hashed and none has a tolerance.  A case is one forward launch and,
where it has one, the backward launch that reads its probs (the indexed backward also the vqa_index_csr launch in front of it); the
status of every launch is recorded with the digests, and a refused launch (VQA_EARG) must leave every buffer as it was."""
import functools

import numpy as np
import torch

from _optbits import DEV, SENT16, SENT32, digest, fill, toolchain, unit  # noqa: F401  (toolchain: for the recorder and the test)
from _pkg import sub

F32, BF16 = torch.float32, torch.bfloat16
DT = {"fp32": F32, "bf16": BF16}
FAMILIES = (("valu", "fp32"), ("valu", "bf16"), ("mfma", "bf16"))
B0, H0 = 3, 3                                   # 9 (batch, head) problems: odd against 4, 2 and 1 waves per workgroup
# (Lq, Lk): Lq 1 / 5 (a second trip of the VALU form's four waves) / 20 / 32 (the full tile); Lk 1 / 20 / 49 / 64 | 65 (two -> five key
# tiles, a second lane trip of the VALU form) / 144 / 160 (the top).  (20, 20) and (20, 49) are the model's own shapes.
SHAPES = ((1, 1), (5, 20), (20, 20), (20, 49), (32, 64), (20, 65), (5, 144), (32, 160))
REPEATS = (3, 3, 0, 2, 0, 3, 2)                 # 7 questions over 4 images: repeats, out of order, image 1 never asked about
EARG = 1000


def sent(shape, dtype):
    n = int(np.prod(shape))
    if dtype == BF16:
        return torch.full((n,), SENT16, dtype=torch.int16).view(BF16).to(DEV).view(shape)
    t = torch.full((n,), SENT32, dtype=torch.int32)
    return (t.view(F32) if dtype == F32 else t).to(DEV).view(shape)


def data(shape, salt, dtype, lo=-1.0, hi=1.0):
    return fill(int(np.prod(shape)), salt, lo, hi).view(shape).to(dtype).to(DEV).contiguous()


def _raw(name, *args):
    """status of one launch (L.call raises on a non-zero one; here the status is part of what is pinned)"""
    L = sub("_lib")
    return int(getattr(L.lib(), name)(*args, L.stream()))


def _kmask(kind, U, Lk):
    if kind == "none":
        return None
    m = (unit(U * Lk, 50) >= 0.25).astype(np.float32).reshape(U, Lk)         # about a quarter of the keys masked
    m[:, 0] = 1.0
    if kind == "row":
        m[U - 1, :] = 0.0                       # every key of the last batch / image: its probs and ctx rows are NaN
    return torch.from_numpy(m).to(DEV).contiguous()


def _seed(kind):
    """(seed argument, what has to stay alive).  flagged: bit 63 set, the word points at the seed_step of a step-state block."""
    SG = sub("stepgraph")
    W = SG.seed_step(0, 0x5EED, 4711)
    if kind == "plain":
        return W | 37, None
    st = torch.zeros(SG.STATE_BYTES // 4, device=DEV, dtype=torch.int32)
    sub("_lib").call("vqa_step_state_set", st.data_ptr(), 1, W, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0, 0.0, 0)
    return SG.seed_word(st.data_ptr() + SG.SEED_STEP_OFFSET, 37), st


def _index(kind, B):
    """(kv_index or None, images U)"""
    if kind is None:
        return None, B
    if kind == "identity":
        return torch.arange(B, dtype=torch.int32, device=DEV), B
    idx = list(REPEATS)
    assert B == len(idx)
    if kind == "bad":
        idx[3] = 7                              # outside [0, 4): the forwards write NaN rows, the CSR is all -1, dK / dV are NaN
    return torch.tensor(idx, dtype=torch.int32, device=DEV), 4


def attn_case(fam, dname, Lq, Lk, hd, B=B0, H=H0, layout="cross", p=0.0, seed="plain", kmask="none", dp=None, index=None, train=True,
              wide=False, ldq_off=0, backward=True):
    """layout packed: q | k | v are the column blocks of one [rows][3 H hd] buffer, and dq | dk | dv of another (the model's self
    attention); cross: q [B Lq][H hd (+ ldq_off)], k | v the column blocks of [U Lk][2 H hd], gradients alike (its cross attention).
    wide: ctx / dctx, dq, dk, dv in buffers of their own with 8 columns more than H hd.  dp: None | "data" | "zero" | "null" (the _dp
    entries).  index: None | "identity" | "repeats" | "bad" (the _idx entries; train = False: the inference forward, no backward)."""
    L = sub("_lib")
    dtype, mf, d = DT[dname], fam == "mfma", H * hd
    kv_index, U = _index(index, B)
    if layout == "packed":
        rows = max(B * Lq, U * Lk)
        qkv = data((rows, 3 * d), 1, dtype)
        q, k, v, ldq, ldk, ldv = qkv, qkv[:, d:], qkv[:, 2 * d:], 3 * d, 3 * d, 3 * d
    else:
        qb, kvb = data((B * Lq, d + ldq_off), 2, dtype), data((U * Lk, 2 * d), 3, dtype)
        q, k, v, ldq, ldk, ldv = qb, kvb, kvb[:, d:], d + ldq_off, 2 * d, 2 * d
    ldc = d + 8 if wide else d
    out = {"probs": sent((B, H, Lq, Lk), F32), "ctx": sent((B * Lq, ldc), dtype)}
    km = _kmask(kmask, U, Lk)
    sd, keep = _seed(seed)
    head = (() if mf else (L.dt(dtype),)) + (q.data_ptr(), k.data_ptr(), v.data_ptr(), ldq, ldk, ldv)
    tail = (L.ptr(km), out["probs"].data_ptr(), out["ctx"].data_ptr(), ldc, B, H, Lq, Lk, hd)
    name = "vqa_attention_fwd_mfma" if mf else "vqa_attention_fwd"
    if index is None:
        st = {"fwd": _raw(name, *head, *tail, p, sd)}
    elif train:
        st = {"fwd": _raw(name + "_idx_train", *head, kv_index.data_ptr(), U, *tail, p, sd)}
    else:
        st = {"fwd": _raw(name + "_idx", *head, kv_index.data_ptr(), U, *tail)}
    if backward and (index is None or train):
        dctx = data((B * Lq, ldc), 4, dtype)
        if wide:
            out.update(dq=sent((B * Lq, ldc), dtype), dk=sent((U * Lk, ldc), dtype), dv=sent((U * Lk, ldc), dtype))
            g = (out["dq"].data_ptr(), out["dk"].data_ptr(), out["dv"].data_ptr(), ldc, ldc, ldc)
        elif layout == "packed":
            out["dqkv"] = sent((rows, 3 * d), dtype)
            g = (out["dqkv"].data_ptr(), out["dqkv"][:, d:].data_ptr(), out["dqkv"][:, 2 * d:].data_ptr(), 3 * d, 3 * d, 3 * d)
        else:
            out.update(dq=sent((B * Lq, d), dtype), dkv=sent((U * Lk, 2 * d), dtype))
            g = (out["dq"].data_ptr(), out["dkv"].data_ptr(), out["dkv"][:, d:].data_ptr(), d, 2 * d, 2 * d)
        bhead = (() if mf else (L.dt(dtype),)) + (dctx.data_ptr(), ldc, q.data_ptr(), k.data_ptr(), v.data_ptr(), ldq, ldk, ldv,
                                                    out["probs"].data_ptr())
        btail = g + (B, H, Lq, Lk, hd, p, sd)
        name = "vqa_attention_bwd_mfma" if mf else "vqa_attention_bwd"
        if index is not None:
            out.update(offsets=sent((U + 1,), torch.int32), order=sent((B,), torch.int32))
            st["csr"] = _raw("vqa_index_csr", kv_index.data_ptr(), B, U, out["offsets"].data_ptr(), out["order"].data_ptr())
            st["bwd"] = _raw(name + "_idx", *bhead, out["offsets"].data_ptr(), out["order"].data_ptr(), U, *btail)
        elif dp is not None:
            dpr = None if dp == "null" else data((B, H, Lq, Lk), 5, F32, -0.05, 0.05) if dp == "data" else torch.zeros(B, H, Lq, Lk, device=DEV)
            st["bwd"] = _raw(name + "_dp", *bhead, L.ptr(dpr), *btail)
        else:
            st["bwd"] = _raw(name, *bhead, *btail)
    torch.cuda.synchronize()
    del keep
    if st["fwd"] == EARG:
        assert all(bool((out[n].view(torch.int16 if out[n].dtype == BF16 else torch.int32) == (SENT16 if out[n].dtype == BF16 else SENT32)).all())
                   for n in ("probs", "ctx")), "a refused forward wrote to its outputs"
    if st.get("bwd") == EARG:
        assert all(bool((t.view(torch.int16 if t.dtype == BF16 else torch.int32) == (SENT16 if t.dtype == BF16 else SENT32)).all())
                   for n, t in out.items() if n.startswith("d")), "a refused backward wrote to its outputs"
    res = {n: digest(t) for n, t in out.items()}
    res["status"] = " ".join(f"{n}={c}" for n, c in sorted(st.items()))
    return res


def csr_case(N, U, kind):
    """kv_index: sorted (ascending), reversed (descending) or repeated (the hash, any order); N = 0 passes no index and no order"""
    v = np.floor(unit(max(N, 1), 60)[:N] * U).astype(np.int32)
    if kind != "repeated":
        v = np.sort(v)[::(1 if kind == "sorted" else -1)].copy()
    idx = torch.from_numpy(v).to(DEV) if N else None
    out = {"offsets": sent((U + 1,), torch.int32), "order": sent((max(N, 1),), torch.int32)}
    rc = _raw("vqa_index_csr", sub("_lib").ptr(idx), N, U, out["offsets"].data_ptr(), out["order"].data_ptr() if N else None)
    torch.cuda.synchronize()
    res = {n: digest(t) for n, t in out.items()}
    res["status"] = f"csr={rc}"
    return res


def csr_refuse_case(kind):
    """what vqa_index_csr refuses: more than 32768 images, no offsets, an index but no order, a negative N"""
    N, U = (-1 if kind == "n-1" else 7), (32769 if kind == "u32769" else 4)
    idx = torch.tensor(REPEATS, dtype=torch.int32, device=DEV)
    out = {"offsets": sent((U + 1,), torch.int32), "order": sent((7,), torch.int32)}
    rc = _raw("vqa_index_csr", idx.data_ptr(), N, U, None if kind == "null-offsets" else out["offsets"].data_ptr(),
              None if kind == "null-order" else out["order"].data_ptr())
    torch.cuda.synchronize()
    assert rc == EARG and all(bool((t == SENT32).all()) for t in out.values()), f"vqa_index_csr {kind}: status {rc}"
    res = {n: digest(t) for n, t in out.items()}
    res["status"] = f"csr={rc}"
    return res


def cases():
    """name -> thunk returning {buffer name: sha256, "status": the launches' return codes}"""
    c, P = {}, functools.partial
    for fam, d in FAMILIES:
        t = f"{fam}/{d}"
        for hd in (32, 64):
            for Lq, Lk in SHAPES:               # plain forward + backward: dropout at the longer query counts, the key mask and the packed layout in self attention
                self_attn = Lq == Lk
                c[f"{t}/plain/{Lq}x{Lk}x{hd}"] = P(attn_case, fam, d, Lq, Lk, hd, layout="packed" if self_attn else "cross",
                                                   p=0.1 if Lq >= 20 else 0.0, kmask="zeros" if self_attn else "none")
            for Lk in (49, 144):                # the _dp entries, both key-tile counts
                for dp in ("data", "zero"):
                    c[f"{t}/dp-{dp}/20x{Lk}x{hd}"] = P(attn_case, fam, d, 20, Lk, hd, p=0.1, dp=dp)
            for Lk in (49, 64, 144, 160):       # indexed: Lk * hd on both sides of 4096 (16 -> 40 accumulators of the VALU backward)
                c[f"{t}/idx-repeats/20x{Lk}x{hd}"] = P(attn_case, fam, d, 20, Lk, hd, B=7, p=0.1, index="repeats")
            c[f"{t}/idx-identity/20x49x{hd}"] = P(attn_case, fam, d, 20, 49, hd, p=0.1, index="identity")
            c[f"{t}/idx-infer/5x65x{hd}"] = P(attn_case, fam, d, 5, 65, hd, B=7, index="repeats", train=False, kmask="zeros")
        # the model's shapes, hd = 32: masks, the flagged seed word, wide output strides, p = 0, an index out of range
        c[f"{t}/self/mask-row"] = P(attn_case, fam, d, 20, 20, 32, layout="packed", p=0.1, kmask="row")
        c[f"{t}/self/no-mask-p0"] = P(attn_case, fam, d, 20, 20, 32, layout="packed")
        c[f"{t}/self/flagged-seed"] = P(attn_case, fam, d, 20, 20, 32, layout="packed", p=0.1, seed="flagged", kmask="zeros")
        c[f"{t}/cross/mask-zeros-144"] = P(attn_case, fam, d, 20, 144, 32, p=0.1, kmask="zeros")
        c[f"{t}/cross/mask-row"] = P(attn_case, fam, d, 20, 49, 32, kmask="row")
        c[f"{t}/cross/wide"] = P(attn_case, fam, d, 20, 49, 32, p=0.1, wide=True)
        c[f"{t}/cross/dp-wide"] = P(attn_case, fam, d, 5, 65, 64, dp="data", wide=True)
        c[f"{t}/idx-repeats/flagged-seed-wide"] = P(attn_case, fam, d, 20, 49, 32, B=7, p=0.1, seed="flagged", index="repeats", wide=True)
        c[f"{t}/idx-repeats/p0-mask"] = P(attn_case, fam, d, 20, 49, 32, B=7, index="repeats", kmask="row")
        c[f"{t}/idx-bad/20x49x32"] = P(attn_case, fam, d, 20, 49, 32, B=7, p=0.1, index="bad")
        c[f"{t}/idx-bad/infer"] = P(attn_case, fam, d, 20, 49, 32, B=7, index="bad", train=False)
        # The MFMA limits (Lq <= 32, Lk <= 160, hd in {32, 64}, row strides % 8) and p = 1, for the plain, _dp and indexed entries.
        # The MFMA entries refuse all of them and the indexed entries refuse p = 1 (refuse/); the VALU entries have no such limits and
        # no p check outside the indexed ones: there the same arguments are launches whose bits are pinned like any other (limits/).
        for tag, kw in (("Lq33", dict(Lq=33)), ("Lk161", dict(Lk=161)), ("hd48", dict(hd=48)), ("ldq+4", dict(ldq_off=4)), ("p1", dict(p=1.0))):
            a = dict(dict(Lq=5, Lk=20, hd=32, p=0.1), **kw)
            g = "refuse" if fam == "mfma" and tag != "p1" else "limits"     # (no plain or _dp entry checks p)
            c[f"{t}/{g}/{tag}/plain"] = P(attn_case, fam, d, **a)
            c[f"{t}/{g}/{tag}/dp"] = P(attn_case, fam, d, dp="data", **a)
            c[f"{t}/{'refuse' if tag == 'p1' else g}/{tag}/idx"] = P(attn_case, fam, d, B=7, index="repeats", **a)
            if tag != "p1":                     # the inference forwards take no p
                c[f"{t}/{g}/{tag}/idx-infer"] = P(attn_case, fam, d, B=7, index="repeats", train=False, **a)
        c[f"{t}/refuse/null-dprobs"] = P(attn_case, fam, d, 5, 20, 32, p=0.1, dp="null")
        c[f"{t}/refuse/idx-Lk161xhd64"] = P(attn_case, fam, d, 5, 161, 64, B=7, p=0.1, index="repeats")     # Lk * hd > 10240
    for N in (0, 1, 7, 1024, 1025):             # 1025: a second chunk of 1024
        for U in (1, 4, 300):
            for kind in ("sorted", "reversed", "repeated"):
                c[f"vqa_index_csr/n{N}/u{U}/{kind}"] = P(csr_case, N, U, kind)
    for kind in ("u32769", "null-offsets", "null-order", "n-1"):
        c[f"vqa_index_csr/refuse/{kind}"] = P(csr_refuse_case, kind)
    return c
