"""Checker of the in-situ tests (test_gpu_insitu.py): a tensor of a live step against its high-precision reference, judged by the
relative norm of the whole tensor AND of every slice along the given dimensions (per image, per output channel).

A global relative norm over 1.6 M rows cannot see an error confined to one image (the last, partial tile round) or one channel:
zeroing one of 512 images moves it by 1/sqrt(512) ~ 0.044 at most, scaling one of 128 channels by 1 + 2^-5 by 0.0028 -- under the
4e-3 bound of a bf16-stored tensor.  Each slice is held to the same bound, relative to its own norm; a slice whose reference norm
is below FLOOR of its fair share (||ref|| / sqrt(number of slices)) is measured against that floor instead, so a near-zero slice (a
dead ReLU channel, a vanishing BatchNorm-gradient entry) cannot turn rounding noise into a large relative error.

Also here: the bounds of the in-situ test (documented and measured there), the fp64 attention core of a live step, plain or indexed
(many questions per image: question b attends to image index[b], dK / dV are per image), and the checks of the image index's CSR and
of the all-zero image-token gradient of an image without questions."""
import math

import torch

FLOOR = 0.1
T_BF16, T_WGRAD, T_BNPARAM, T_FP32 = 4e-3, 2e-4, 1e-3, 1e-4
T_SIGMA = 5e-4                             # batch mean / BN shift error in standard deviations (measured 2.5e-4: stage-1 bn1 shift)
T_PROBS = 1e-6                             # fp32 attention probabilities from bf16 Q / K (measured 1.5e-7)
T_ATTN, T_ATTN_SLICE = 4e-3, 8e-3         # dQ / dK / dV of the attention backward: the kernel also feeds P and dS to its MFMAs in bf16
                                           # (measured 2.6e-3 globally, 5.2e-3 in one feature column of cross-attention dQ;
                                           # dK / dV summed per image: 2.0e-3 / 4.4e-3)


def rnd(t):
    """bf16 rounding in fp32 (what a bf16 kernel reads of an fp32 value)."""
    return t.to(torch.bfloat16).float()


def slice_errors(got, ref, dim):
    """Relative error of every slice of `got` along `dim` (see the module docstring for the floor)."""
    d = (got - ref).double()
    r = ref.double()
    others = [k for k in range(ref.dim()) if k != dim]
    dn = torch.linalg.vector_norm(d, dim=others) if others else d.abs()
    rn = torch.linalg.vector_norm(r, dim=others) if others else r.abs()
    floor = FLOOR * float(torch.linalg.vector_norm(r)) / ref.shape[dim] ** 0.5
    return dn / rn.clamp(min=max(floor, 1e-30))


class Checker:
    """Collects every comparison of one step; finish() prints the worst error per tag and per class and raises on any violation
    (all of them listed, so one run shows every failing layer)."""

    def __init__(self):
        self.worst = {}
        self.by_class = {}
        self.fails = []

    def _record(self, tag, cls, e):
        self.worst[tag] = max(self.worst.get(tag, 0.0), e) if e == e else float("nan")
        self.by_class[cls] = max(self.by_class.get(cls, 0.0), e) if e == e else float("nan")

    def check(self, tag, got, ref, tol, dims=(0, 1), cls="bf16", slice_tol=None, assert_=True):
        """Global relative norm <= tol and every slice along `dims` <= slice_tol (default: tol).  assert_=False: measured and
        reported only."""
        got, ref = got.float(), ref.float()
        assert got.shape == ref.shape, (tag, tuple(got.shape), tuple(ref.shape))
        e = float(torch.linalg.vector_norm((got - ref).double()) / torch.linalg.vector_norm(ref.double()).clamp(min=1e-30))
        if assert_ and not e <= tol:               # (NaN included)
            self.fails.append((tag, "all", e, tol))
        self._record(tag, cls, e)
        st = tol if slice_tol is None else slice_tol
        for dim in dims:
            es = slice_errors(got, ref, dim)
            i = int(torch.nan_to_num(es, nan=float("inf")).argmax())
            ei = float(es[i])
            self._record(tag + " /slice", cls + " /slice", ei)
            if assert_ and not ei <= st:
                self.fails.append((tag, f"dim{dim}[{i}]", ei, st))
        return e

    def check_abs(self, tag, err, tol, cls):
        """An error already in units of its natural scale (e.g. a batch mean's error in standard deviations)."""
        e = float(err.abs().max()) if err.numel() else 0.0
        if not e == e:
            e = float("nan")
        self._record(tag, cls, e)
        if not e <= tol:
            self.fails.append((tag, "max", e, tol))

    def expect(self, tag, ok, detail=""):
        """A property that is not an error norm (an argmax that points at a maximum, a mask that matches)."""
        if not ok:
            self.fails.append((tag, detail, None, None))

    def report(self, title):
        print(f"{title}: worst relative error per class:", {k: float("%.3g" % v) for k, v in sorted(self.by_class.items())})
        print(f"{title}: worst relative error per tensor:", {k: float("%.3g" % v) for k, v in sorted(self.worst.items())})

    def finish(self, title):
        self.report(title)
        assert not self.fails, f"{len(self.fails)} checks failed: {self.fails[:40]}"


def nchw(t, B, H, W, sel=None):
    """engine layout [B*H*W, C] (NHWC) -> float32 NCHW on the CPU (only the images `sel`, if given)."""
    v = t.view(B, H, W, -1)
    if sel is not None:
        v = v[sel]
    return v.cpu().float().permute(0, 3, 1, 2).contiguous()


def bn_bwd(g, y, coef, gamma):
    """nn.BatchNorm2d training-mode backward on NCHW fp32 tensors; coef rows: scale, shift, batch mean, 1/sqrt(var + eps)."""
    mean, inv = coef[2].view(1, -1, 1, 1), coef[3].view(1, -1, 1, 1)
    xhat = (y - mean) * inv
    n = g.numel() / g.shape[1]
    dbeta = g.sum((0, 2, 3))
    dgamma = (g * xhat).sum((0, 2, 3))
    dy = gamma.view(1, -1, 1, 1) * inv * (g - dbeta.view(1, -1, 1, 1) / n - xhat * dgamma.view(1, -1, 1, 1) / n)
    return dy, dgamma, dbeta


def channel_moments(y):
    """fp64 batch mean and biased variance per channel of an NCHW tensor (two-pass)."""
    y = y.double()
    mean = y.mean((0, 2, 3))
    var = ((y - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    return mean, var


def attn_core_fwd(Qh, Kh, Vh, P, keep, kmask=None, index=None):
    """fp64 attention core in head layout: (softmax(Q K^T / sqrt(hd)) from Q / K, ctx from the STORED probabilities P and the dropout
    keep scale).  Qh, P, keep: per question [Bq][H][Lq][.]; Kh, Vh [Bk][H][Lk][hd] -- per question, or per image with `index`
    (long [Bq]: question b attends to image index[b]).  kmask [Bq][Lk]: 0 = masked key."""
    if index is not None:
        Kh, Vh = Kh[index], Vh[index]
    sc = Qh @ Kh.transpose(-1, -2) / math.sqrt(Qh.shape[-1])
    if kmask is not None:
        sc = sc.masked_fill(kmask[:, None, None, :] == 0, float("-inf"))
    return torch.softmax(sc, -1), (P * keep) @ Vh


def attn_core_bwd(Qh, Kh, Vh, P, keep, dC, index=None, n_kv=None):
    """fp64 closed form of the attention core backward on the stored probabilities (dP = dctx V^T * keep, dS = P (dP - sum(dP P)) /
    sqrt(hd), dQ = dS K, dK = dS^T Q, dV = (P keep)^T dctx), shapes as attn_core_fwd.  With `index`, Kh / Vh hold n_kv images and
    dK / dV are per IMAGE: the per-question closed forms summed over the image's questions (an image without questions gets zeros)."""
    Kq, Vq = (Kh, Vh) if index is None else (Kh[index], Vh[index])
    dP = (dC @ Vq.transpose(-1, -2)) * keep
    dS = P * (dP - (dP * P).sum(-1, keepdim=True)) / math.sqrt(Qh.shape[-1])
    dQ, dK, dV = dS @ Kq, dS.transpose(-1, -2) @ Qh, (P * keep).transpose(-1, -2) @ dC
    if index is not None:
        dK = torch.zeros((n_kv,) + tuple(dK.shape[1:]), dtype=dK.dtype).index_add_(0, index, dK)
        dV = torch.zeros((n_kv,) + tuple(dV.shape[1:]), dtype=dV.dtype).index_add_(0, index, dV)
    return dQ, dK, dV


def check_csr(ck, tag, index, n_img, offsets, order):
    """vqa_index_csr's result against its contract: offsets = exclusive prefix sum of the questions per image ([U+1]), order = the
    questions of each image in ascending order (a stable argsort of the index)."""
    index = index.cpu().long()
    ref_off = torch.zeros(n_img + 1, dtype=torch.long)
    ref_off[1:] = torch.cumsum(torch.bincount(index, minlength=n_img), 0)
    ck.expect(tag + " offsets", torch.equal(offsets.cpu().long(), ref_off), "not the prefix sum of the questions per image")
    ck.expect(tag + " order", torch.equal(order.cpu().long(), torch.argsort(index, stable=True)),
              "not the stable argsort of the image index")


def empty_images(index, n_img):
    """Images without a question (long [k])."""
    return (torch.bincount(index.cpu().long(), minlength=n_img) == 0).nonzero().flatten()


def check_zero_rows(ck, tag, t, n_img, images):
    """The rows of `images` in t ([n_img * rows per image][cols], rows of one image contiguous) are exactly zero (NaN is not)."""
    v = t.reshape(n_img, -1)[images.to(t.device)]
    bad = int((v != 0).sum())
    ck.expect(tag + " zero rows", bad == 0, f"{bad} non-zero entries in the rows of images without questions {images.tolist()}")
