"""CPU: tests/_accumref.replay -- the float64 yardstick of a gradient-accumulation window -- against the literal torch loop it stands
for, on a small torch.nn module in float64:  (loss_i / n).backward() for the n batches, clip_grad_norm_, torch.optim.AdamW.step().
n = 1, 2, 3 with unequal batch sizes, the clip on and off, one and two parameter groups, a frozen parameter; equality to 1e-12."""
import pytest
import torch

import _accumref as R

SIZES = {1: (5,), 2: (4, 2), 3: (3, 5, 2)}
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)


def _net():
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.LayerNorm(8), torch.nn.Tanh(), torch.nn.Linear(8, 4)).double()
    return net


def _batches(n):
    g = torch.Generator().manual_seed(100 + n)
    return [(torch.randn(b, 6, generator=g, dtype=torch.float64), torch.randint(0, 4, (b,), generator=g)) for b in SIZES[n]]


def _flatten(ts):
    return torch.cat([t.detach().reshape(-1).double() for t in ts])


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("max_norm", [0.05, 100.0])                     # the clip on (the norm here is ~1) and off
@pytest.mark.parametrize("grouped,frozen", [(False, False), (True, False), (True, True)])
def test_replay_equals_the_torch_loop(n, max_norm, grouped, frozen):
    net = _net()
    params = list(net.parameters())
    if frozen:
        params[2].requires_grad_(False)                                  # the LayerNorm weight keeps its values
    train = [p for p in params if p.requires_grad]
    if grouped:                                                          # biases and norms: no decay, twice the rate
        spec = [(2.0, 0.0) if p.dim() == 1 else (1.0, None) for p in train]
        opt = torch.optim.AdamW([{"params": [p], "lr": HYPER["lr"] * s, "weight_decay": HYPER["weight_decay"] if w is None else w}
                                 for p, (s, w) in zip(train, spec)], lr=HYPER["lr"], betas=HYPER["betas"], eps=HYPER["eps"], foreach=False)
    else:
        spec = None
        opt = torch.optim.AdamW(train, **HYPER, foreach=False)
    loss_fn = torch.nn.CrossEntropyLoss()
    # one plain step first: the window starts from Adam state that is not zero, at step 2
    x, y = _batches(1)[0]
    loss_fn(net(x), y).backward()
    opt.step()
    opt.zero_grad()
    sizes = [p.numel() for p in params]
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    slices = [slice(o, o + k) for o, k, p in zip(offs, sizes, params) if p.requires_grad]
    zeros = lambda p: torch.zeros_like(p)
    p0 = _flatten(params)
    m0 = _flatten([opt.state[p]["exp_avg"] if p.requires_grad else zeros(p) for p in params])
    v0 = _flatten([opt.state[p]["exp_avg_sq"] if p.requires_grad else zeros(p) for p in params])
    # the window's SUMMED gradient, as HipTrainer's flat buffer holds it: each batch's mean-loss gradient, added up unscaled
    gsum = torch.zeros_like(p0)
    for x, y in _batches(n):
        gs = torch.autograd.grad(loss_fn(net(x), y), train)
        for s, g in zip(slices, gs):
            gsum[s] += g.reshape(-1)
    # the literal loop
    for x, y in _batches(n):
        (loss_fn(net(x), y) / n).backward()
    norm_t = float(torch.nn.utils.clip_grad_norm_(train, max_norm))
    opt.step()
    p, m, v, norm = R.replay(p0, m0, v0, gsum, n, max_norm=max_norm, step=2, slices=slices, groups=spec, **HYPER)
    assert (norm > max_norm) == (max_norm < 1.0)                          # the case is what its name says
    assert abs(norm - norm_t) <= 1e-12 * norm_t
    p1 = _flatten(params)
    m1 = _flatten([opt.state[q]["exp_avg"] if q.requires_grad else zeros(q) for q in params])
    v1 = _flatten([opt.state[q]["exp_avg_sq"] if q.requires_grad else zeros(q) for q in params])
    for got, want, what in ((p, p1, "p"), (m, m1, "m"), (v, v1, "v")):
        assert float((got - want).abs().max()) <= 1e-12, what
    assert not torch.equal(p1, p0)
    if frozen:
        s = slice(offs[2], offs[2] + sizes[2])
        assert torch.equal(p[s], p0[s]) and torch.equal(p1[s], p0[s])


def test_replay_takes_a_step_number_per_slice_and_leaves_the_rest():
    p0, m0, v0, g = (torch.full((8,), x, dtype=torch.float64) for x in (1.0, 0.1, 0.01, 0.5))
    sl = [slice(0, 2), slice(4, 8)]
    p, m, v, norm = R.replay(p0, m0, v0, g, 2, max_norm=0.0, step=[1, 3], slices=sl, **HYPER)
    one = R.replay(p0, m0, v0, g, 2, max_norm=0.0, step=1, slices=sl, **HYPER)[0]
    three = R.replay(p0, m0, v0, g, 2, max_norm=0.0, step=3, slices=sl, **HYPER)[0]
    assert torch.equal(p[0:2], one[0:2]) and torch.equal(p[4:8], three[4:8]) and not torch.equal(one[4:8], three[4:8])
    assert torch.equal(p[2:4], p0[2:4]) and torch.equal(m[2:4], m0[2:4]) and torch.equal(v[2:4], v0[2:4])
    assert abs(norm - (6 * 0.25 ** 2) ** 0.5) < 1e-15
