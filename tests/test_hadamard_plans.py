"""CPU-only: plan_hadamard, plan_hadamard_k and plan_hadamard_perm return or raise what the record holds (tests/hadamard_plans.json, written by
tools/record_hadamard.py on the commit before the three planners moved onto one core): the plan tuple field by field, or the exception's type and
full message.  The sweep (tests/_hadamard_record_cases.py) covers the shapes (), (n,), (n, 1), (3, n), (n, 3), (2, n, 3), (2, 3, 2n) with every dim
in and out of range, the sizes 0, 1, 2, 12, 96 and every cap and the step past it with k in {1, 3, 12} and at the caps of k, the three float dtypes
and an integer one, the four precisions, a CPU tensor, a non-contiguous one, every `form`, and inputs that trip two conditions at once."""
import json
import os

import pytest

import _hadamard_record_cases as C

RECORD = dict(json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "hadamard_plans.json"))))
CASES = C.plan_cases()
FNS = ("plan_hadamard", "plan_hadamard_k", "plan_hadamard_perm")


def test_record_is_the_sweep_and_reaches_every_answer():
    assert [c["id"] for c in CASES] == list(RECORD)  # nothing dropped, added or reordered by hand
    for fn in FNS:
        mine = [RECORD[c["id"]] for c in CASES if c["fn"] == fn]
        assert {r["raises"][0] for r in mine if "raises" in r} == {"ValueError", "IndexError", "NotImplementedError"}, fn
        plans = [r["plan"] for r in mine if "plan" in r]
        assert {"rows", "cols"} <= {v for p in plans for v in (p if fn != "plan_hadamard_perm" else p[2]) if isinstance(v, str)}, fn
    assert {r["plan"][1] for r in RECORD.values() if "plan" in r and r["plan"][0] == "HadamardPermPlan"} == {"fused", "composed"}
    assert {"butterfly", "mfma", "valu"} <= {r["plan"][2] for r in RECORD.values() if "plan" in r and r["plan"][0] == "HadamardKPlan"}
    assert len({r["raises"][1] for r in RECORD.values() if "raises" in r}) >= 30


@pytest.mark.parametrize("fn", FNS)
def test_planner_answers_the_record(fn):
    from compressed_tensors_amd import codec

    for case in (c for c in CASES if c["fn"] == fn):
        assert C.run_plan(codec, case) == RECORD[case["id"]], case["id"]
