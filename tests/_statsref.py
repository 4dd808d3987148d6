"""float64 yardstick of vqa_tensor_stats (include/vqa_hip.h), plain torch on whatever device the data lives on: the four values of a
table row from x[lo:hi] (and y), the unpacking of the kernel's 32-bit words, and the rounding bound the kernel source states."""
import torch

TWO_M24 = 2.0 ** -24


def row(x, lo, hi, y=None):
    """(sumsq float, absmax float, nonfinite int, zeros int) of d = x[lo:hi] (- y[lo:hi], ONE fp32 subtraction): sumsq and absmax over
    the finite d in float64 (0 when there is none), nonfinite = #NaN or +-inf, zeros = #(d == 0) (-0.0 counts)."""
    d = x[lo:hi].float()
    if y is not None:
        d = d - y[lo:hi].float()
    fin = torch.isfinite(d)
    f = d[fin].double()
    sumsq = float((f * f).sum()) if f.numel() else 0.0
    absmax = float(f.abs().max()) if f.numel() else 0.0
    return sumsq, absmax, int((~fin).sum()), int((d == 0).sum())


def table(x, ranges, y=None):
    """{"sumsq", "absmax": float64 [P]; "nonfinite", "zeros": int64 [P]} on the CPU, one row() per range."""
    rows = [row(x, lo, hi, y) for lo, hi in ranges]
    return {"sumsq": torch.tensor([r[0] for r in rows], dtype=torch.float64), "absmax": torch.tensor([r[1] for r in rows], dtype=torch.float64),
            "nonfinite": torch.tensor([r[2] for r in rows], dtype=torch.int64), "zeros": torch.tensor([r[3] for r in rows], dtype=torch.int64)}


def unpack(words):
    """The kernel's int32 [P][4] rows as the reference's dict: the two fp32 words as they are (float32), the counts as unsigned."""
    w = words.detach().cpu()
    f = w[:, :2].contiguous().view(torch.float32)
    c = w[:, 2:].long() & 0xffffffff
    return {"sumsq": f[:, 0].clone(), "absmax": f[:, 1].clone(), "nonfinite": c[:, 0].clone(), "zeros": c[:, 1].clone()}


def n_add(numel, chunk, pair=False):
    """The longest chain of roundings a term of sumsq goes through (csrc/stats_ops.hip): T additions in its thread -- four per float4,
    at most chunk / 1024 float4 per thread, plus one for a tail element --, 6 in the wave butterfly, 2 across the four waves, one per
    chunk of the row in the fold, 1 for the square, and 1 more for the subtraction of the pair form."""
    per_thread = min(chunk // 256, 4 * -(-min(numel, chunk) // 1024)) + (1 if numel % 4 else 0)
    return per_thread + 6 + 2 + -(-numel // chunk) + 1 + (1 if pair else 0)


def sumsq_bound(numel, chunk, pair=False):
    """Relative bound on |sumsq - exact| (all terms are non-negative): n_add * 2^-24."""
    return n_add(numel, chunk, pair) * TWO_M24
