"""fp64 CPU reference of vqa_softmax_topk (include/vqa_hip.h): mask, stable descending sort, softmax gathered at the picks.

    y[j]   = logits[j] where allowed (or without a mask), else -inf
    order  : a before b when y[a] > y[b], or y[a] == y[b] and a < b; NaN above every number, NaNs among themselves by index
             (torch.sort(y, descending=True, stable=True))
    probs  = softmax(y * scale) in fp64, gathered at the first k of the order (IEEE on special rows: a row that holds a NaN, or
             nothing but -inf, is all NaN)
The logits come in whatever dtype the kernel was given and are widened exactly, so the reference sees the dtype-rounded values."""
import torch


def masked(logits, allowed=None):
    """fp64 [B][N] copy of the logits with -inf where `allowed` ([N] or [B][N], bool / uint8) is zero."""
    y = logits.detach().cpu().double().clone()
    if allowed is not None:
        a = allowed.detach().cpu() != 0
        y[~a.expand_as(y)] = float("-inf")
    return y


def topk_ref(logits, k, allowed=None, scale=1.0):
    """(indices int64 [B][k], probs fp64 [B][k]) of the semantics above."""
    y = masked(logits, allowed)
    order = torch.sort(y, dim=-1, descending=True, stable=True).indices[:, :k]
    p = torch.softmax(y * float(scale), dim=-1)
    return order, p.gather(1, order)


def prob_error(got, ref):
    """(e, nan_ok): e = max over the non-NaN reference entries of max(|got - ref| - 1e-30, 0) / |ref|, so e <= 2e-5 is the bound
    "relative 2e-5 plus absolute 1e-30" (a reference of exactly 0 tolerates 1e-30 and nothing more); nan_ok: every entry whose
    reference is NaN is NaN in `got`."""
    got, ref = got.detach().cpu().double(), ref.double()
    nan = torch.isnan(ref)
    ok = ~nan
    err = ((got[ok] - ref[ok]).abs() - 1e-30).clamp_min(0.0) / ref[ok].abs().clamp_min(1e-300)
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    return (float(err.max()) if err.numel() else 0.0), bool(torch.isnan(got[nan]).all())
