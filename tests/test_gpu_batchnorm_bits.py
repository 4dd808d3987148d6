"""GPU: the twelve BatchNorm entries (csrc/batchnorm.hip) compute the bits they computed before their kernels were folded into one
forward text, one backward-apply text and one masked gradient and moved out of csrc/cnn_ops.hip.

tests/golden/batchnorm_bits.json holds one SHA-256 per launch, over every buffer the launch may write, and the status of every launch, of the nine vqa_bn_* entries
that launch and the values of the three that return counts over the cases of tests/_bnbits.py, recorded by
tests/golden/make_batchnorm_bits.py on an MI355X with the library of the commit BEFORE that change.  Here the product library runs the
same cases and every digest and status must match.  Every BatchNorm kernel is deterministic (ordered slab sums, integer atomics):
nothing has a tolerance."""
import json
import os

import pytest

import _bnbits as BB

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batchnorm_bits.json")
CASES = BB.cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_holds_exactly_the_cases(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_output_bits_are_those_of_the_parent_commit(case, golden):
    got, want = CASES[case](), golden["cases"][case]
    assert sorted(got) == sorted(want), f"{case}: launches {sorted(got)} against recorded {sorted(want)}"
    for buf in sorted(want):
        if got[buf] != want[buf]:
            import torch
            pytest.fail(f"{case}: {buf}: {got[buf]} differs from the recorded {want[buf]}\n"
                        f"  recorded with: {golden['hipcc']} on {golden['device']}\n"
                        f"  this run:      {BB.toolchain()} on {torch.cuda.get_device_name(0)}")


@pytest.mark.parametrize("entry", BB.SHAPE_CHECKED)
def test_zero_channels_are_refused(entry):
    """C = 0 is refused by the shared shape check (common.h bn_vec_ok) and nothing is written.  The library of the commit before
    divided by it on the host, so the golden cannot hold this case: the status and the untouched buffers are asserted here."""
    BB.refuse_case(entry, "c0")
