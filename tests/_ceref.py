"""fp64 reference of cross entropy with nn.CrossEntropyLoss's options (weight, ignore_index, label_smoothing; reduction "mean"):
torch's own F.cross_entropy plus autograd on the CPU, the closed-form restatement the HIP kernel implements, and VQAAccuracy's
counters over the rows that are not ignored (rank rule: the lowest index wins ties)."""
import torch
import torch.nn.functional as F

NO_IGNORE = -100        # torch's default ignore_index: "nothing is ignored" as long as no target holds it


def torch_ce(x, t, w=None, ii=None, eps=0.0, dtype=torch.float64):
    """(loss, d loss / d x) of F.cross_entropy in `dtype` on the CPU; ii None: no target is ignored."""
    if ii is None:
        assert not bool((t == NO_IGNORE).any())
    x = x.detach().to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(x, t, weight=None if w is None else w.to(dtype), ignore_index=NO_IGNORE if ii is None else ii,
                           label_smoothing=eps, reduction="mean")
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


def closed_form(x, t, w=None, ii=None, eps=0.0, gscale=1.0):
    """The restatement in include/vqa_hip.h, fp64:  W = sum_b wy[b], Sw = sum_c w[c],
    loss = [(1-eps) sum_b wy[b] (-lp[b][t_b]) + eps/N sum_b keep[b] sum_c w[c] (-lp[b][c])] / W,
    dx[b][c] = [(1-eps) wy[b] (p[b][c] - [c == t_b]) + eps/N keep[b] (Sw p[b][c] - w[c])] gscale / W;
    W == 0: NaN loss and a ZERO gradient (torch's unweighted behaviour; the kernel's in both cases)."""
    x = x.double()
    B, N = x.shape
    w = torch.ones(N, dtype=torch.float64) if w is None else w.double()
    keep = torch.ones(B, dtype=torch.bool) if ii is None else t != ii
    ts = torch.where(keep, t, torch.zeros_like(t))
    wy = keep.double() * w[ts]
    W, Sw = wy.sum(), w.sum()
    lp = torch.log_softmax(x, 1)
    p = lp.exp()
    onehot = F.one_hot(ts, N).double()
    if float(W) == 0.0:
        return torch.tensor(float("nan"), dtype=torch.float64), torch.zeros_like(x)
    loss = ((1 - eps) * (wy * -lp.gather(1, ts[:, None])[:, 0]).sum() + eps / N * (keep.double() * (-(lp * w).sum(1))).sum()) / W
    g = ((1 - eps) * wy[:, None] * (p - onehot) + eps / N * keep.double()[:, None] * (Sw * p - w[None, :])) * gscale / W
    return loss, g


def accuracy_counts(x, t, ii=None):
    """[correct, correct_top5, total] over the kept rows: rank of the target = #{j: x[j] > x[t]} + #{j < t: x[j] == x[t]}; a target
    outside [0, N) counts in total as wrong."""
    B, N = x.shape
    out = [0, 0, 0]
    for b in range(B):
        tb = int(t[b])
        if ii is not None and tb == ii:
            continue
        out[2] += 1
        if not 0 <= tb < N:
            continue
        row = x[b]
        rank = int((row > row[tb]).sum()) + int((row[:tb] == row[tb]).sum())
        out[0] += rank == 0
        out[1] += rank < 5
    return out
