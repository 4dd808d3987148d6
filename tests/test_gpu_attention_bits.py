"""GPU: the thirteen attention entries (csrc/attention.hip) compute the bits they computed before their kernels were folded into one
forward and one backward text per family and moved out of csrc/token_ops.hip.

tests/golden/attention_bits.json holds the SHA-256 of every output buffer, and the status of every launch, of vqa_attention_fwd / _bwd
in their plain, _mfma, _dp, _idx and _idx_train forms and of vqa_index_csr over the cases of tests/_attnbits.py, recorded by
tests/golden/make_attention_bits.py on an MI355X with the library of the commit BEFORE that change.  Here the product library runs the
same cases and every digest and status must match.  No attention kernel uses float atomics: nothing has a tolerance."""
import json
import os

import pytest

import _attnbits as AB

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_bits.json")
CASES = AB.cases()


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
            pytest.fail(f"{case}: {buf}: {got[buf]} differs from the recorded {want[buf]}\n"
                        f"  recorded with: {golden['hipcc']} on {golden['device']}\n"
                        f"  this run:      {AB.toolchain()} on {torch.cuda.get_device_name(0)}")
