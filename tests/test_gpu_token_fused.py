"""Round-4 launch mergers of the fusion tail (models/fusion.py:281-296): both masked means / both backward broadcasts in one launch.

Below them: the small token-side kernels of csrc/token_ops.hip against float64 at the branches the model-level tests never isolate --
embedding forward / backward (bf16, id-list tails, a second pass over the id list, a workgroup owning one table row), bias / ReLU /
dropout backward (several column blocks, fewer rows than a block has in flight, the scalar kernel), the single-tensor masked mean
(no mask, a column window, an addend) and the cross entropy on rows that need the max subtraction."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _dropmask import keep_mask
from _pkg import sub

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(5, 20, 256), (64, 20, 256), (3, 7, 512), (512, 20, 256)])
def test_masked_pool_pair_equals_two_single_launches(shape, dtype):
    L = sub("_lib")
    B, T, D = shape
    g = torch.Generator().manual_seed(B + T)
    x0 = torch.randn(B, T, D, generator=g).to(DEV, dtype)
    x1 = torch.randn(B, T, D, generator=g).to(DEV, dtype)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = 0                                                  # an all-padding row: the count clamps to 1 (models/fusion.py:289)
    mask = (torch.arange(T)[None, :] < lens[:, None]).float().to(DEV)
    d = L.dt(dtype)
    pair = torch.empty(B, 2 * D, device=DEV, dtype=dtype)
    L.call("vqa_masked_pool_pair_fwd", d, x0.data_ptr(), x1.data_ptr(), mask.data_ptr(), pair.data_ptr(), B, T, D)
    two = torch.empty_like(pair)
    L.call("vqa_masked_pool_fwd", d, x0.data_ptr(), mask.data_ptr(), two.data_ptr(), 2 * D, 0, B, T, D)
    L.call("vqa_masked_pool_fwd", d, x1.data_ptr(), mask.data_ptr(), two.data_ptr(), 2 * D, D, B, T, D)
    torch.cuda.synchronize()
    assert torch.equal(pair, two)
    cnt = mask.sum(1, keepdim=True).clamp(min=1.0)
    ref = torch.cat([(x0.float() * mask[..., None]).sum(1) / cnt, (x1.float() * mask[..., None]).sum(1) / cnt], 1)
    assert (pair.float() - ref).abs().max().item() < (1e-5 if dtype == torch.float32 else 2e-2)
    assert (pair[0] == 0).all()

    dcat = torch.randn(B, 2 * D, generator=g).to(DEV, dtype)
    dq, de = torch.full_like(x0, 7.0), torch.full_like(x1, 7.0)
    L.call("vqa_masked_pool_pair_bwd", d, dcat.data_ptr(), mask.data_ptr(), dq.data_ptr(), de.data_ptr(), B, T, D)
    dq2, de2 = torch.empty_like(x0), torch.empty_like(x1)
    L.call("vqa_masked_pool_bwd", d, dcat.data_ptr(), 2 * D, 0, mask.data_ptr(), None, dq2.data_ptr(), B, T, D)
    L.call("vqa_masked_pool_bwd", d, dcat.data_ptr(), 2 * D, D, mask.data_ptr(), None, de2.data_ptr(), B, T, D)
    torch.cuda.synchronize()
    assert torch.equal(dq, dq2) and torch.equal(de, de2)
    ref_q = dcat[:, None, :D].float() * mask[..., None] / cnt[..., None]
    assert (dq.float() - ref_q).abs().max().item() < (1e-6 if dtype == torch.float32 else 2e-2)
    assert (dq[mask == 0] == 0).all() and (de[mask == 0] == 0).all()


def test_pair_entries_refuse_missing_operands():
    L = sub("_lib")
    x = torch.zeros(2, 4, 8, device=DEV)
    with pytest.raises(RuntimeError):
        L.call("vqa_masked_pool_pair_fwd", 0, x.data_ptr(), None, None, x.data_ptr(), 2, 4, 8)
    with pytest.raises(RuntimeError):
        L.call("vqa_linear_dgrad_act", 0, x.data_ptr(), x.data_ptr(), x.data_ptr(), None, None, 0.1, 8, 8, 8)


# ---------------------------------------------------------------------------------------------------------------------------
# kernel edges against float64 (every reference: plain torch on the CPU in fp64, from the rounded inputs the kernel receives)
# ---------------------------------------------------------------------------------------------------------------------------
BF16_HALF_ULP = 2.0 ** -8


def _keep(seed, shape, p):
    n = int(np.prod(shape))
    return torch.from_numpy(keep_mask(seed, n, p)).view(*shape) if p > 0 else torch.ones(*shape, dtype=torch.bool)


def _edge_ids(rows, V, g):
    ids = torch.randint(0, V, (rows,), generator=g)
    edge = [0, V - 1, V + 3, -2] if rows >= 4 else [0, V - 1, -2]   # padding row, last row, out of range on both sides
    ids[:len(edge)] = torch.tensor(edge)
    if rows >= 8:
        ids[-1] = V - 1                                             # the id list's last (tail) entry lands in the second workgroup
    return ids


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embed_forward_matches_fp64(dtype, p):
    L = sub("_lib")
    rows, Lq, D, V, seed = 1027, 13, 40, 17, 606
    g = torch.Generator().manual_seed(rows + D)
    ids = _edge_ids(rows, V, g)
    emb, pe = torch.randn(V, D, generator=g), torch.randn(Lq, D, generator=g)
    scale = float(np.float32(math.sqrt(D)))
    ok = (ids >= 0) & (ids < V)
    ref = emb.double()[ids.clamp(0, V - 1)] * ok[:, None] * scale + pe.double()[torch.arange(rows) % Lq]
    keep = _keep(seed, (rows, D), p)
    ref = ref * keep / (1 - float(np.float32(p)))
    out = torch.full((rows, D), 7.0, device=DEV, dtype=dtype)
    idd, embd, ped = ids.to(DEV), emb.to(DEV), pe.to(DEV)
    L.call("vqa_embed_fwd", L.dt(dtype), idd.data_ptr(), embd.data_ptr(), ped.data_ptr(), out.data_ptr(), rows, Lq, D, V, scale, p, seed)
    torch.cuda.synchronize()
    tol = 1e-6 + 1e-5 * ref.abs() + (BF16_HALF_ULP * ref.abs() if dtype == torch.bfloat16 else 0)
    assert bool(((out.cpu().double() - ref).abs() <= tol).all())
    assert (out.cpu()[~keep] == 0).all()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [40, 512])
@pytest.mark.parametrize("rows", [3, 1027, 2050])
def test_embed_backward_matches_fp64(rows, D, dtype, p):
    """rows % 4 != 0: the scalar id-load tail; rows > 1024 and rows % 1024 != 0: more than one pass; V = 17: the second workgroup owns
    a single table row."""
    L = sub("_lib")
    V, seed = 17, 707
    g = torch.Generator().manual_seed(rows + D)
    ids = _edge_ids(rows, V, g)
    dout = torch.randn(rows, D, generator=g).to(dtype)
    scale = float(np.float32(math.sqrt(D)))
    keep = _keep(seed, (rows, D), p)
    ok = (ids > 0) & (ids < V)                                      # padding_idx = 0 and out-of-range ids receive nothing
    src = dout.double() * scale * keep / (1 - float(np.float32(p)))
    ref = torch.zeros(V, D, dtype=torch.float64).index_add_(0, ids[ok], src[ok])
    idd, dd = ids.to(DEV), dout.to(DEV)
    res = []
    for rep in range(2):
        demb = torch.zeros(V + 4, D, device=DEV)                    # four guard rows behind the table
        L.call("vqa_embed_bwd", L.dt(dtype), idd.data_ptr(), dd.data_ptr(), demb.data_ptr(), rows, D, V, scale, p, seed)
        res.append(demb)
    torch.cuda.synchronize()
    got = res[0].cpu().double()
    assert float(ref.abs().max()) > 0
    assert float((got[:V] - ref).abs().max() / ref.abs().max()) < 1e-5
    assert (got[0] == 0).all() and (got[V:] == 0).all()
    assert torch.equal(res[0], res[1])
    L.call("vqa_embed_bwd", L.dt(dtype), idd.data_ptr(), dd.data_ptr(), res[1].data_ptr(), rows, D, V, scale, p, seed)
    torch.cuda.synchronize()
    assert torch.allclose(res[1], 2 * res[0], rtol=1e-6, atol=0)    # += semantics


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N", [(1, 256), (3, 2048), (37, 4096), (5, 24), (300, 2048)])
def test_bias_act_backward_matches_fp64(M, N, dtype):
    """dz = dout * [out > 0] * keep-scale, dbias += column sums of dz, in the three operand modes, with and without the fixed-order
    scratch and with dz = NULL.  The keep-scale is the fp32 number each kernel forms: the vectorised kernel multiplies by
    1 / (1 - p) (as torch.dropout does), the scalar kernel (N / VEC does not divide 256) divides by (1 - p); the two differ by an ulp
    of fp32 on some elements, so the exact reference follows the kernel's form."""
    L, K = sub("_lib"), sub("kernels")
    d, p, seed = L.dt(dtype), 0.1, 808
    g = torch.Generator().manual_seed(M + N)
    dout = torch.randn(M, N, generator=g).to(dtype)
    act = torch.relu(torch.randn(M, N, generator=g)).to(dtype)
    vecn = 8 if dtype == torch.bfloat16 else 4
    vec = N % vecn == 0 and 256 % min(N // vecn, 256) == 0
    one_minus_p = np.float32(1) - np.float32(p)
    ks = float(np.float32(1) / one_minus_p)
    scaled = dout.double() * ks if vec else dout.double() / float(one_minus_p)
    modes = {"relu": (act, 0.0, dout.double() * (act > 0)),
             "relu+dropout": (act, p, scaled * (act > 0)),
             "dropout": (None, p, scaled * _keep(seed, (M, N), p)),
             "plain": (None, 0.0, dout.double())}
    dd, ad = dout.to(DEV), act.to(DEV)
    wsf = K.reduce_ws("vqa_bias_act_bwd_ws", d, M, N)
    for name, (outact, pp, ref) in modes.items():
        ref_dz = ref.float().to(dtype)                              # one rounding to fp32 (the kernel's register), then to the dtype
        ref_db = ref.float().double().sum(0)
        bound = 1e-3 * max(1.0, float(ref_db.abs().max()))
        for use_ws, want_dz in ((True, True), (False, True), (True, False)):
            ws = torch.empty(wsf, device=DEV) if use_ws else None
            dz = torch.full((M, N), 7.0, device=DEV, dtype=dtype) if want_dz else None
            db = torch.full((N,), 0.25, device=DEV)
            L.call("vqa_bias_act_bwd", d, dd.data_ptr(), ad.data_ptr() if outact is not None else None, L.ptr(dz), db.data_ptr(), M, N,
                   pp, seed, L.ptr(ws), 0)
            torch.cuda.synchronize()
            if want_dz:
                assert torch.equal(dz.cpu(), ref_dz), (name, use_ws)
            assert float((db.cpu().double() - 0.25 - ref_db).abs().max()) < bound, (name, use_ws, want_dz)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("masked", [False, True])
def test_masked_pool_single_entries_window_addend_and_no_mask(masked, dtype):
    L = sub("_lib")
    B, T, D = 5, 7, 40
    g = torch.Generator().manual_seed(B + T + D)
    x = torch.randn(B, T, D, generator=g).to(dtype)
    mask = None
    w = torch.ones(B, T, dtype=torch.float64)
    if masked:
        lens = torch.tensor([0, 7, 1, 4, 6])                        # an all-padding row: the count clamps to 1
        mask = (torch.arange(T)[None, :] < lens[:, None]).float()
        w = mask.double()
    cnt = w.sum(1, keepdim=True).clamp(min=1.0)
    d = L.dt(dtype)
    maskd = mask.to(DEV) if masked else None
    out = torch.full((B, 3 * D), 7.0, device=DEV, dtype=dtype)
    xd = x.to(DEV)
    L.call("vqa_masked_pool_fwd", d, xd.data_ptr(), L.ptr(maskd), out.data_ptr(), 3 * D, D, B, T, D)
    torch.cuda.synchronize()
    ref = (x.double() * w[..., None]).sum(1) / cnt                  # mask = NULL: the plain mean
    out = out.cpu()
    assert float((out[:, D:2 * D].double() - ref).abs().max()) < (1e-5 if dtype == torch.float32 else 2e-2)
    assert (out[:, :D] == 7.0).all() and (out[:, 2 * D:] == 7.0).all()      # outside the window: untouched

    dpool = torch.randn(B, 3 * D, generator=g).to(dtype)
    addend = torch.randn(B, T, D, generator=g).to(dtype)
    dx = torch.full((B, T, D), 7.0, device=DEV, dtype=dtype)
    dpd, addd = dpool.to(DEV), addend.to(DEV)
    L.call("vqa_masked_pool_bwd", d, dpd.data_ptr(), 3 * D, D, L.ptr(maskd), addd.data_ptr(), dx.data_ptr(), B, T, D)
    torch.cuda.synchronize()
    ref_dx = addend.double() + dpool[:, None, D:2 * D].double() * w[..., None] / cnt[..., None]
    assert float((dx.cpu().double() - ref_dx).abs().max()) < (1e-6 if dtype == torch.float32 else 2e-2)
    if masked:
        assert torch.equal(dx.cpu()[mask == 0], addend[mask == 0])  # padding positions: exactly the addend


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [3, 70, 1000])
def test_cross_entropy_rows_that_need_the_max_subtraction(N, dtype):
    """Rows offset by +300 / -300 (expf overflows / flushes without the max subtraction) and a row with one logit 60 above the rest."""
    L = sub("_lib")
    B = 5
    g = torch.Generator().manual_seed(N)
    logits = torch.randn(B, N, generator=g) * 3
    logits[1] += 300.0
    logits[2] -= 300.0
    logits[3, N // 2] = logits[3].max() + 60.0
    logits = logits.to(dtype)
    tgt = torch.randint(0, N, (B,), generator=g)
    tgt[3] = (N // 2 + 1) % N                                       # the target is NOT the dominant logit: a loss of about 60
    ref_in = logits.double().requires_grad_(True)
    ref = F.cross_entropy(ref_in, tgt)
    ref.backward()
    ld, td = logits.to(DEV), tgt.to(DEV)
    loss = torch.zeros(1, device=DEV)
    dl = torch.empty(B, N, device=DEV, dtype=dtype)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    L.call("vqa_cross_entropy", L.dt(dtype), ld.data_ptr(), td.data_ptr(), loss.data_ptr(), dl.data_ptr(), None, B, N, 1.0, err.data_ptr(), None)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(dl.float()).all()
    e_loss, e_dl = abs(loss.item() - ref.item()), float((dl.cpu().double() - ref_in.grad).abs().max())
    print(f"CE B={B} N={N} {dtype}: loss err {e_loss:.2e} (ref {ref.item():.3f})  dlogits err {e_dl:.2e}")
    assert e_loss < 1e-5 * max(1.0, abs(ref.item()))
    assert e_dl < (1e-6 if dtype == torch.float32 else 4e-3 * float(ref_in.grad.abs().max()))
    assert int(err.item()) == 0
