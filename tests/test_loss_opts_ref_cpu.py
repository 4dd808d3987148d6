"""CPU: the closed-form restatement of cross entropy with class weights, ignore_index and label smoothing (tests/_ceref.py, the
formulas of vqa_cross_entropy_opts in include/vqa_hip.h) equals torch's F.cross_entropy and its autograd gradient in fp64; the
drop-in CrossEntropyLoss validates its arguments in the constructor and refuses CPU logits."""
import math

import pytest
import torch

import _ceref as R
from _pkg import pkg

# both sides are fp64 evaluations of the same mathematical expression through different summation trees: B * N <= 9000 terms of
# relative rounding 1.1e-16 give about 1e-12 of (1 + |ref|); 1e-10 leaves two orders for the softmax's own rounding
TOL = 1e-10


def _inputs(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, generator=g, dtype=torch.float64) * 3
    t = torch.randint(0, N, (B,), generator=g)
    w = torch.rand(N, generator=g, dtype=torch.float64) + 0.1
    return x, t, w


@pytest.mark.parametrize("eps", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("ignore", [None, -100, 2])
@pytest.mark.parametrize("weighted", [False, True])
def test_closed_form_equals_torch(weighted, ignore, eps):
    for B, N in ((1, 5), (5, 65), (9, 1000)):
        x, t, w = _inputs(B, N, 100 * B + N)
        if ignore == 2:
            t[t == 2] = 3                                      # only the rows set below hold the ignored class id
        if ignore is not None and B > 1:
            t[B // 2] = ignore
        if weighted and B > 1:
            z = int(t[B - 1])
            w[z] = 0.0                                         # a class of weight 0 that is a row's target
            t[0] = (z + 1) % N if (z + 1) % N != ignore else (z + 2) % N       # row 0 keeps a positive weight: W > 0
        ww = w if weighted else None
        ref_l, ref_g = R.torch_ce(x, t, ww, ignore, eps)
        l, g = R.closed_form(x, t, ww, ignore, eps)
        assert math.isfinite(float(ref_l))
        assert abs(float(l) - float(ref_l)) <= TOL * (1 + abs(float(ref_l))), (B, N)
        assert float(((g - ref_g).abs() / (1 + ref_g.abs())).max()) <= TOL, (B, N)
        gs = R.closed_form(x, t, ww, ignore, eps, gscale=0.25)[1]
        assert torch.allclose(gs, 0.25 * ref_g, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_all_rows_ignored_is_nan_with_a_zero_gradient_like_torch(eps):
    x, t, _ = _inputs(4, 7, 5)
    t[:] = -100
    ref_l, ref_g = R.torch_ce(x, t, None, -100, eps)
    l, g = R.closed_form(x, t, None, -100, eps)
    assert math.isnan(float(ref_l)) and math.isnan(float(l))
    assert torch.equal(ref_g, torch.zeros_like(x)) and torch.equal(g, torch.zeros_like(x))


def test_accuracy_counts_rank_rule():
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0, 0.0, 0.0, 0.0], [5.0, 1.0, 2.0, 3.0, 4.0, 0.0, 6.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 9.0],
                      [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]])
    assert R.accuracy_counts(x, torch.tensor([1, 1, 6, 0])) == [2, 2, 4]          # tie at row 0: index 1 wins; row 1 rank 5; row 3 rank 6
    assert R.accuracy_counts(x, torch.tensor([2, 3, 6, 0])) == [1, 3, 4]          # index 2 loses the tie (rank 1)
    assert R.accuracy_counts(x, torch.tensor([2, -100, 6, 9]), ii=-100) == [1, 2, 3]   # an ignored row and a bad target


def test_criterion_validates_in_the_constructor_and_refuses_cpu_logits():
    CE = pkg().load_dropin_losses().CrossEntropyLoss
    for kw in (dict(reduction="sum"), dict(reduction="none"), dict(label_smoothing=-0.1), dict(label_smoothing=1.5),
               dict(label_smoothing=float("nan")), dict(weight=[1.0, -1.0]), dict(weight=[1.0, float("inf")]),
               dict(weight=torch.ones(2, 2)), dict(ignore_index=1.5)):
        with pytest.raises(ValueError):
            CE(**kw)
    c = CE(weight=[1.0, 2.0, 0.0], ignore_index=1, label_smoothing=0.1)
    assert c.weight.dtype == torch.float32 and c.ignore_index == 1 and c.label_smoothing == 0.1 and c.reduction == "mean"
    assert CE().ignore_index == -100 and CE().weight is None
    with pytest.raises(RuntimeError, match="no CPU path"):
        c(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))


def test_trainer_constructor_rejects_bad_options():
    T = pkg().trainer.HipTrainer

    class _M:                                                  # _check_loss_opts reads nothing but these two
        num_answers = 4
        _flat = torch.zeros(1)
    chk = lambda **kw: T._check_loss_opts(type("S", (), {"model": _M})(), kw.get("label_smoothing", 0.0), kw.get("class_weight"), kw.get("ignore_index"))
    for kw in (dict(label_smoothing=-0.01), dict(label_smoothing=1.01), dict(label_smoothing=float("nan")), dict(class_weight=[1.0, 1.0]),
               dict(class_weight=[1.0, 1.0, -1.0, 1.0]), dict(class_weight=[1.0, float("nan"), 1.0, 1.0]), dict(ignore_index=0.5)):
        with pytest.raises(ValueError):
            chk(**kw)
    eps, ii, w = chk(label_smoothing=0.1, class_weight=[1, 2, 0, 4], ignore_index=-100)
    assert eps == 0.1 and ii == -100 and w.dtype == torch.float32 and w.tolist() == [1.0, 2.0, 0.0, 4.0]
    assert chk() == (0.0, None, None)


def test_a_bound_project_imports_utils_losses_and_keeps_its_own_utils(tmp_path):
    """A fresh interpreter (the binding lives in sys.modules and sys.meta_path): a project laid out like the reference, whose utils
    package has no losses.py, gets the drop-in's; its own utils.config stays its own; a project WITH a utils/losses.py keeps that."""
    import json
    import os
    import subprocess
    import sys
    import textwrap
    from _pkg import REPO
    code = textwrap.dedent("""
        import sys, importlib, json
        sys.path.insert(0, %r)
        binding = importlib.import_module("visual-question-answering-vqa-system_amd.binding")
        binding.bind(sys.argv[1], "fp32")
        sys.path.insert(0, sys.argv[1])
        from utils.config import WHO
        import utils.losses as UL
        print(json.dumps(dict(who=WHO, file=UL.__file__, has=hasattr(UL, "CrossEntropyLoss"), own=getattr(UL, "WHO", None))))
    """) % REPO
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("PYTHONPATH", None)
    outs = []
    for own in (False, True):
        root = tmp_path / ("own" if own else "plain")
        (root / "utils").mkdir(parents=True)
        (root / "utils" / "__init__.py").write_text("")
        (root / "utils" / "config.py").write_text("WHO = 'project utils.config'\n")
        if own:
            (root / "utils" / "losses.py").write_text("WHO = 'project utils.losses'\n")
        r = subprocess.run([sys.executable, "-c", code, str(root)], cwd=str(root), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    plain, kept = outs
    assert plain["who"] == "project utils.config" and plain["has"] and plain["file"].endswith(os.path.join("dropin", "utils", "losses.py"))
    assert kept["own"] == "project utils.losses" and not kept["has"]
