"""GPU: the optimizer tail (csrc/optim_ops.hip) computes the bits it computed before its AdamW kernels were folded into one.

tests/golden/optimizer_bits.json holds the SHA-256 of every output buffer of vqa_sumsq, vqa_sumsq_ranges, vqa_adamw, vqa_adamw_ema,
vqa_adamw_ranges, vqa_adamw_ranges_ema, vqa_ema_update and vqa_step_state_set over the cases of tests/_optbits.py, recorded by
tests/golden/make_optimizer_bits.py on an MI355X with the library of the commit BEFORE that change.  Here the product library runs
the same cases and every digest must match.  The EMA and _dev entries are tied to vqa_adamw / vqa_adamw_ranges by
tests/test_gpu_ema_kernels.py and tests/test_gpu_step_graph_kernels.py; this test ties those two, and the sums of squares, to the past.
A skipped launch is also checked directly: no buffer changes and skipped becomes [rows, 1, skipped[2] + 1] (tests/_optbits._finish)."""
import json
import os

import pytest

import _optbits as OB

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optimizer_bits.json")
CASES = OB.cases()


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
                        f"  this run:      {OB.toolchain()} on {torch.cuda.get_device_name(0)}")
