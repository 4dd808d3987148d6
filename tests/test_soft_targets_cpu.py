"""CPU: the soft-answer-score surface exists end to end -- the three C entries are declared with the table's arity, exported by the
library built for gfx950 and refuse bad arguments with 1000 before any HIP call; SoftTargets.validate is pure host logic; the
drop-in VQAChallengeAccuracy reproduces the reference's recorded result (tests/golden/soft_targets.npz, written by the real
utils.metrics.VQAChallengeAccuracy) on the reference's own call form, two lists of strings."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from _pkg import REPO, pkg, sub

NEW = ("vqa_answer_scores", "vqa_cross_entropy_soft", "vqa_challenge_accuracy_update")


def _header_decls():
    txt = open(os.path.join(REPO, "include", "vqa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\bint\s+(vqa_\w+)\s*\((.*?)\)\s*;", txt, flags=re.S)}


def test_header_declares_the_new_entries_with_the_table_arity():
    decls, L = _header_decls(), sub("_lib")
    for name in NEW:
        assert name in decls, name
        assert name in L.SIGNATURES, name
        assert decls[name] == len(L.SIGNATURES[name]), (name, decls[name], len(L.SIGNATURES[name]))
    # the soft loss is the hard one with (ids, weights, K) in place of targets, plus (counts, acc) before the stream
    S, P, I = L.SIGNATURES, ctypes.c_void_p, ctypes.c_int
    hard = S["vqa_cross_entropy"]
    assert S["vqa_cross_entropy_soft"] == hard[:2] + [P, P, I] + hard[3:-1] + [P, P, P]
    K = sub("kernels")
    for name in NEW:
        assert name in K.HBM_BYTES, name
    # B = 512, N = 1000, K = 10, bf16, with counts: the hard kernel's logits traffic plus B * K * 12 bytes
    a = [1, 1, 1, 1, 10, 1, 1, 1, 512, 1000, 1.0, 1, 1, 1, 1]
    assert K.HBM_BYTES["vqa_cross_entropy_soft"][1](a) == K.HBM_BYTES["vqa_cross_entropy"][1]([1, 1, 1, 1, 1, 1, 512, 1000]) + 512 * 10 * 12


def test_library_exports_the_new_entries_and_they_reject_bad_arguments():
    import __graft_entry__ as G
    G.build()
    lib = sub("_lib").lib()
    for name in NEW:
        assert hasattr(lib, name), name
    s = lib.vqa_answer_scores                      # (answers, ids, weights, counts, B, A, N, mode, err, stream)
    assert s(None, 1, 1, 1, 4, 10, 100, 0, None, None) == 1000
    assert s(1, None, 1, 1, 4, 10, 100, 0, None, None) == 1000
    assert s(1, 1, None, 1, 4, 10, 100, 0, None, None) == 1000
    assert s(1, 1, 1, None, 4, 10, 100, 0, None, None) == 1000
    assert s(1, 1, 1, 1, 0, 10, 100, 0, None, None) == 1000
    assert s(1, 1, 1, 1, 4, 0, 100, 0, None, None) == 1000
    assert s(1, 1, 1, 1, 4, 65, 100, 0, None, None) == 1000
    assert s(1, 1, 1, 1, 4, 10, 0, 0, None, None) == 1000
    assert s(1, 1, 1, 1, 4, 10, 100, 2, None, None) == 1000
    c = lib.vqa_cross_entropy_soft                 # (dtype, logits, ids, weights, K, loss, dlogits, lf32, B, N, gscale, err, ws, counts, acc, stream)
    ok = [0, 1, 1, 1, 10, 1, 1, None, 4, 100, 1.0, None, None, None, None, None]
    for pos, val in ((1, None), (2, None), (3, None), (4, 0), (4, 65), (8, 0), (9, -1), (14, 1)):      # (14: acc without counts)
        a = list(ok)
        a[pos] = val
        assert c(*a) == 1000, (pos, val)
    m = lib.vqa_challenge_accuracy_update          # (logits, ids, counts, K, acc, B, N, stream)
    ok = [1, 1, 1, 10, 1, 4, 100, None]
    for pos, val in ((0, None), (1, None), (2, None), (3, 0), (3, 65), (4, None), (5, 0), (6, 0)):
        a = list(ok)
        a[pos] = val
        assert m(*a) == 1000, (pos, val)


def test_soft_targets_validate_is_host_logic():
    ST = pkg().load_dropin_soft_targets()
    assert pkg().load_dropin_soft_targets() is ST
    B, K = 6, 10
    ids, w, cnt = torch.full((B, K), -1, dtype=torch.int32), torch.zeros(B, K), torch.zeros(B, K, dtype=torch.int32)
    cpu = torch.device("cpu")
    s = ST.SoftTargets(ids, w, cnt)
    assert s.validate(B, cpu) is s
    assert ST.SoftTargets(ids, w).counts is None
    ST.SoftTargets(ids, w).validate(B, "cpu")                              # counts are optional
    ST.SoftTargets(ids[:, :1].contiguous(), w[:, :1].contiguous()).validate(B, cpu)
    bad = [
        (ST.SoftTargets(ids, w, cnt), B + 1, cpu),                         # wrong batch
        (ST.SoftTargets(ids.long(), w, cnt), B, cpu),                      # dtypes
        (ST.SoftTargets(ids, w.double(), cnt), B, cpu),
        (ST.SoftTargets(ids, w, cnt.long()), B, cpu),
        (ST.SoftTargets(ids, w[:, :4].contiguous(), cnt), B, cpu),         # shapes that disagree
        (ST.SoftTargets(ids, w, cnt[:, :4].contiguous()), B, cpu),
        (ST.SoftTargets(ids[:, 0], w[:, 0], None), B, cpu),                # not 2-D
        (ST.SoftTargets(torch.zeros(B, 65, dtype=torch.int32), torch.zeros(B, 65), None), B, cpu),      # more slots than lanes
        (ST.SoftTargets(torch.zeros(B, 0, dtype=torch.int32), torch.zeros(B, 0), None), B, cpu),
        (ST.SoftTargets(ids, w, cnt), B, torch.device("cuda:0")),          # wrong device
        (ST.SoftTargets(ids.t().contiguous().t(), w, cnt), B, cpu) if B != K else None,                   # not contiguous
        (ST.SoftTargets(ids.tolist(), w, cnt), B, cpu),                    # not a tensor
    ]
    for case in bad:
        if case is None:
            continue
        s, b, dev = case
        with pytest.raises(ValueError):
            s.validate(b, dev)
    with pytest.raises(RuntimeError):
        ST.answer_scores(torch.zeros(B, K, dtype=torch.int64), 100)        # host tensor: there is no CPU path
    with pytest.raises(RuntimeError):
        ST.SoftTargetCrossEntropy()(torch.zeros(B, 100), s)


def test_challenge_accuracy_on_string_lists_reproduces_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "soft_targets.npz"))
    M = pkg().load_dropin_metrics()
    m = M.VQAChallengeAccuracy()
    assert m.count == 0 and m.total_score == 0.0 and m.compute() == 0.0
    answers, pred = g["answers"].astype(np.int64), g["pred"].astype(np.int64)
    for lo in range(0, len(pred), 300):                                    # several updates of uneven size
        m.update([str(int(v)) for v in pred[lo:lo + 300]], [[str(int(v)) for v in row] for row in answers[lo:lo + 300]])
    assert m.count == int(g["count"]) == len(pred)
    assert abs(m.compute() - float(g["compute"])) < 1e-9
    assert abs(m.total_score - float(g["total_score"])) < 1e-9 * len(pred)
    # thirds are exact: the recorded per-question scores are k/3 with k the capped vote count
    thirds = np.minimum(3, (answers == pred[:, None]).sum(1))
    assert np.abs(g["scores"] - thirds / 3.0).max() < 1e-15
    assert round(m.total_score * 3) == int(thirds.sum())
    m.reset()
    assert m.count == 0 and m.compute() == 0.0
    with pytest.raises(RuntimeError):
        m.update(torch.zeros(4, 10), torch.zeros(4, 10, dtype=torch.int64))   # host logits: there is no CPU path


def test_hiptrainer_step_documents_soft_targets():
    """The TypeError cases of HipTrainer.step need a built engine (a device): they are in tests/test_gpu_soft_targets.py.  Here: the
    recogniser the step uses accepts the drop-in's SoftTargets and nothing else."""
    T = sub("trainer")
    ST = pkg().load_dropin_soft_targets()
    s = ST.SoftTargets(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3))
    assert T._is_soft(s) and not T._is_soft(torch.zeros(2, dtype=torch.int64)) and not T._is_soft((s.ids, s.weights, None))
    assert "SoftTargets" in T.HipTrainer.step.__doc__
