"""fp64 reference of vqa_bce_soft on the CPU: the contract in include/vqa_hip.h restated from (logits, ids, weights, counts) -- loss,
gradient, which rows are bad, the challenge accuracy in integer thirds -- and BCEOracleTrainer, the CPU oracle's train step with
F.binary_cross_entropy_with_logits(reduction="sum") / B in the place of F.cross_entropy."""
import torch
import torch.nn.functional as F

from oracle import vqa_oracle as O


def random_soft(B, N, K, g):
    """tests/test_gpu_soft_targets.py::_random_soft: ids with duplicates, -1 slots and all-empty rows; weights as the scores come:
    1/3, 2/3, 1 in fp32."""
    ids = torch.randint(0, N, (B, K), generator=g)
    if K > 1:
        ids[:, K // 2] = ids[:, 0]                                         # a duplicate in every row: the weights add up
        ids[torch.rand(B, K, generator=g) < 0.25] = -1
    ids[torch.arange(B) % 5 == 3] = -1                                     # rows without any answer
    w = (torch.randint(1, 4, (B, K), generator=g).float() / 3.0).clamp(max=1.0)
    return ids.int(), w


def bad_rows(ids, N):
    """bool [B]: the row holds an id < -1 or >= N."""
    ids = ids.cpu().long()
    return ((ids < -1) | (ids >= N)).any(1)


def dense(ids, weights, N):
    """t[b, c] = sum of weights[b, k] over ids[b, k] == c in fp64; -1 slots are skipped, duplicates add up, nothing is clamped.  Slots
    with an id outside [-1, N) are skipped too (their rows are bad: bad_rows)."""
    ids, w = ids.cpu().long(), weights.cpu().double()
    ok = (ids >= 0) & (ids < N)
    return torch.zeros(ids.shape[0], N, dtype=torch.float64).scatter_add_(1, torch.where(ok, ids, torch.zeros_like(ids)), w * ok)


def bce(logits, ids, weights, counts=None, gscale=1.0):
    """(loss, dlogits, bad, thirds) in fp64:
    loss = (1/B) sum_b sum_c [max(x,0) + log1p(exp(-|x|)) - x t], NaN when any row is bad;
    dlogits = (sigmoid(x) - t) gscale / B, NaN rows where bad;
    thirds = [sum_b min(3, votes for the lowest index holding row b's maximum), B] (None without counts)."""
    x = logits.detach().cpu().double()
    B, N = x.shape
    t = dense(ids, weights, N)
    bad = bad_rows(ids, N)
    terms = (x.clamp(min=0) + torch.log1p(torch.exp(-x.abs())) - x * t).sum(1) / B
    terms[bad] = float("nan")
    g = (torch.sigmoid(x) - t) * gscale / B
    g[bad] = float("nan")
    thirds = None
    if counts is not None:
        idl, cnt = ids.cpu().long(), counts.cpu().long()
        best = (x == x.max(1, keepdim=True).values).long().argmax(1)       # argmax of a 0/1 row: the first 1 = the lowest index
        votes = ((idl == best[:, None]) * cnt).sum(1).clamp(0, 3)
        thirds = [int(votes.sum()), B]
    return terms.sum(), g, bad, thirds


class BCEOracleTrainer(O.OracleTrainer):
    """OracleTrainer with the loss of HipTrainer(loss="bce"): `targets` is the dense [B, N] soft-score matrix."""

    def step(self, images, token_ids, attention_mask, targets):
        self.opt.zero_grad()
        nb = {}
        logits, _ = O.vqa_forward(images, token_ids, attention_mask, self.sd, self.cfg, True, nb)
        loss = F.binary_cross_entropy_with_logits(logits, targets, reduction="sum") / logits.shape[0]
        loss.backward()
        gnorm = torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
        self.opt.step()
        self.sd.update(nb)
        return loss.detach(), logits.detach(), gnorm
