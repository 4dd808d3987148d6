"""float64 replay of one gradient-accumulation window of HipTrainer (accumulate() ... step()): the yardstick of
tests/test_gpu_grad_accum.py, pinned against a literal torch loop by tests/test_grad_accum_ref_cpu.py.

A window of n micro-batches leaves the SUM of their per-batch mean gradients in the flat gradient buffer; its one update is what

    for batch_i in window:  (loss_i / n).backward()
    clip_grad_norm_(trainable parameters, max_norm)
    torch.optim.AdamW(...).step()

applies: the gradient is sum / n, the norm is taken over every trainable element (global, also with parameter groups), the clip
coefficient is min(1, max_norm / (norm + 1e-6)), and AdamW is torch's decoupled form

    p <- p * (1 - lr * wd);  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2;  p <- p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

Everything is computed in float64 from the values handed in: give the hyper-parameters as the fp32 values the C ABI carries (as
doubles), see tests/test_gpu_param_groups_trainer.py on why that matters for beta2."""
import math

import torch


def replay(p0, m0, v0, gsum, n, *, max_norm, lr, betas, eps, weight_decay, step, slices=None, groups=None):
    """The window's update.  p0, m0, v0, gsum: flat tensors of one length (parameter snapshot, both moments, the window's summed
    gradient); n: micro-batches in the window; step: Adam's step number t of this update (an int, or one per slice);
    slices: the trainable parameters as slices of the flat buffers (None: everything is one trainable slice) -- what lies outside
    keeps its values; groups: None, or one (lr_scale, weight_decay) per slice (weight_decay None: the trainer's).
    Returns (p, m, v, norm): float64 flats and the global norm of gsum / n over the trainable slices."""
    p, m, v = (t.detach().double().clone() for t in (p0, m0, v0))
    g = gsum.detach().double() / n
    if slices is None:
        slices = [slice(0, p.numel())]
    norm = math.sqrt(sum(float((g[s] ** 2).sum()) for s in slices))
    coef = 1.0
    if max_norm is not None and max_norm > 0:
        coef = min(1.0, max_norm / (norm + 1e-6))
    b1, b2 = betas
    for i, s in enumerate(slices):
        t = step[i] if isinstance(step, (list, tuple)) else step
        scale, wd = (1.0, None) if groups is None else groups[i]
        wd = weight_decay if wd is None else wd
        lr_i = lr * scale
        gi = g[s] * coef
        pi = p[s] * (1.0 - lr_i * wd)
        mi = b1 * m[s] + (1.0 - b1) * gi
        vi = b2 * v[s] + (1.0 - b2) * gi * gi
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        p[s] = pi - (lr_i / bc1) * mi / (vi.sqrt() / math.sqrt(bc2) + eps)
        m[s], v[s] = mi, vi
    return p, m, v, norm
