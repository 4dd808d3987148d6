"""GPU: everything that reads the answer logits (csrc/loss_ops.hip) computes the bits it computed before the four loss kernels were
folded into two templates.

tests/golden/loss_bits.json holds the SHA-256 of every output buffer of vqa_cross_entropy, vqa_cross_entropy_opts,
vqa_cross_entropy_soft, vqa_bce_soft, vqa_accuracy_update, vqa_challenge_accuracy_update, vqa_answer_scores and vqa_softmax_topk over
the cases of tests/_lossbits.py, recorded by tests/golden/make_loss_bits.py on an MI355X with the library of the commit BEFORE that
change.  Here the product library runs the same cases and every digest must match.  Without ws the loss is a sum of float atomics in
arrival order: it is not hashed but held within (B - 1) * 2^-24 * sum |term| of the fp64 sum of the ws run's row terms, which are
pinned (tests/_lossbits._loss_near)."""
import json
import os

import pytest

import _lossbits as LB

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_bits.json")
CASES = LB.cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_holds_exactly_the_cases(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_output_bits_are_those_of_the_parent_commit(case, golden):
    got, want = CASES[case](), golden["cases"][case]
    assert sorted(got) == sorted(want), f"{case}: buffers {sorted(got)} against recorded {sorted(want)}"
    for buf in sorted(want):
        if got[buf] != want[buf]:
            import torch
            pytest.fail(f"{case}: buffer {buf}: sha256 {got[buf]} differs from the recorded {want[buf]}\n"
                        f"  recorded with: {golden['hipcc']} on {golden['device']}\n"
                        f"  this run:      {LB.toolchain()} on {torch.cuda.get_device_name(0)}")
