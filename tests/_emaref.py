"""float64 reference of the weight average the optimizer launches keep (vqa_adamw_ema, vqa_adamw_ranges_ema, vqa_ema_update;
include/vqa_hip.h):   ema <- d * ema + (1 - d) * p_new,   d = decay, or min(decay, (1 + t) / (10 + t)) with warm-up, t = the Adam step
number of the element (per range when parameters are frozen); a skipped launch changes nothing and advances no t.

Bound on what the fp32 kernels may differ by: ONE update adds at most 2^-22 * max(|ema|, |p|) of ITS operands, per element -- it rounds
1 - d, the product (1 - d) * p and the final sum (an fma); with the fp32 rounding of d itself that is at most 3.5 * 2^-24 of the
larger operand, and 4 * 2^-24 = 2^-22 also covers the e + (1 - d)(p - e) form -- and the error of the earlier updates is carried
with the factor d <= 1.  After k updates:  err_k <= d_k * err_{k-1} + 2^-22 * max(|ema_{k-1}|, |p_k|)  <=  k * 2^-22 * max(|ema|, |p|),
the max taken over the k updates.  Tracker keeps the recurrence (the tighter form); it must be evaluated on each update's own operands,
not on the last ones alone: AdamW moves every parameter by about lr per step, so a small parameter (a bias near zero) changes sign and
magnitude between updates, the average of it cancels, and the rounding error made on the larger earlier operands stays."""
import torch

ULP4 = 2.0 ** -22


def decay_at(decay, warmup, t):
    """The decay of the update at step t >= 1 (python floats, i.e. float64)."""
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def ema_step(ema, p_new, decay, warmup, t, skip=False):
    """One update of a float64 average `ema` (returned, not modified) at step t; skip: the launch was skipped."""
    if skip:
        return ema.clone()
    d = decay_at(decay, warmup, t)
    return d * ema + (1.0 - d) * p_new.double()


def ema_step_ranges(ema, p_new, ranges, steps, decay, warmup, skip=False):
    """The same over trainable ranges [(lo, hi, lag index)] of a flat buffer, range r at its own step steps[r]; elements outside
    every range keep their value."""
    out = ema.clone()
    if skip:
        return out
    for (lo, hi, _), t in zip(ranges, steps):
        out[lo:hi] = ema_step(ema[lo:hi], p_new[lo:hi], decay, warmup, t)
    return out


def replay(ema0, snapshots, decay, warmup, steps=None):
    """The average after the parameter snapshots p_1 ... p_k (one per applied update), started at ema0; steps: their step numbers
    (1 ... k when None)."""
    ema = ema0.double()
    for i, p in enumerate(snapshots):
        ema = ema_step(ema, p, decay, warmup, (i + 1) if steps is None else steps[i])
    return ema


class Tracker:
    """The float64 average next to the kernels' one, with its error bound (module docstring): .ema, .err (per element), .k updates."""

    def __init__(self, ema0):
        self.ema = ema0.double().clone()
        self.err = torch.zeros_like(self.ema)
        self.k = 0

    def _one(self, sl, p_new, d):
        e, p = self.ema[sl], p_new[sl].double()
        self.err[sl] = d * self.err[sl] + ULP4 * torch.maximum(e.abs(), p.abs())
        self.ema[sl] = d * e + (1.0 - d) * p

    def step(self, p_new, decay, warmup, t, skip=False):
        """One update with the parameters p_new at step t (skip: the launch was skipped, nothing moves)."""
        if not skip:
            self._one(slice(None), p_new, decay_at(decay, warmup, t))
            self.k += 1
        return self

    def step_ranges(self, p_new, ranges, steps, decay, warmup, skip=False):
        """One update over trainable ranges [(lo, hi, lag index)], range r at its own step steps[r]; nothing moves outside."""
        if not skip:
            for (lo, hi, _), t in zip(ranges, steps):
                self._one(slice(lo, hi), p_new, decay_at(decay, warmup, t))
            self.k += 1
        return self

    def check(self, got, what="", sel=None):
        """Assert |got - ema| <= err elementwise (sel: a boolean mask of the elements to look at); prints the worst ratio first."""
        sel = slice(None) if sel is None else sel
        e = (got.double() - self.ema).abs()[sel]
        b = self.err[sel]
        ratio = float((e / b.clamp_min(1e-300)).max()) if e.numel() else 0.0
        print(f"   ema {what}: max |err| {float(e.max()) if e.numel() else 0.0:.3e}, worst err / bound {ratio:.3f} (k = {self.k})")
        assert bool((e <= b).all()), (what, ratio)
