"""CPU-only: the six `ct_hadamard*` row / column entries and ct_hadamard_k_workspace_bytes answer the recorded sweep of bad arguments
(tests/hadamard_refusals.json, written by tools/record_hadamard.py on the commit before the launchers moved onto the shared host path of
csrc/ct_hadamard.h) with the same return code and the same text of ct_last_error: one case per CT_REQUIRE / CT_UNSUPPORTED line of check_had,
check_hadk, check_hadp, the column driver and the row dispatch, and pairs that trip two lines at once, so the order of the checks is pinned.
Every case is refused before the first launch; the addresses are made up (tests/_hadamard_record_cases.py)."""
import json
import os

import pytest

import _hadamard_record_cases as C

RECORD = dict(json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "hadamard_refusals.json"))))
CASES = C.refusal_cases()
ENTRIES = tuple(C.ENTRIES) + ("ct_hadamard_k_workspace_bytes",)


@pytest.fixture(scope="module")
def lib():
    from compressed_tensors_amd import _lib

    return _lib.load()


def test_record_is_the_sweep_and_holds_refusals_only():
    assert [c["id"] for c in CASES] == list(RECORD)  # nothing dropped, added or reordered by hand
    assert {c["entry"] for c in CASES} == set(ENTRIES)
    for c in CASES:
        r = RECORD[c["id"]]
        if c["entry"] == "ct_hadamard_k_workspace_bytes":
            assert r["error"] is None and r["ret"] >= -1, c["id"]
        else:  # CT_ERR_INVALID_ARG or CT_ERR_UNSUPPORTED with a reason: no case reached a launch (CT_ERR_HIP) or passed
            assert r["ret"] in (1, 2) and r["error"], c["id"]
    texts = {r["error"] for r in RECORD.values() if r["error"]}
    assert len(texts) >= 35, len(texts)  # the sweep reaches the lines it names, not one line forty ways


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_answers_the_record(lib, entry):
    for case in (c for c in CASES if c["entry"] == entry):
        assert C.run_refusal(lib, case) == RECORD[case["id"]], case["id"]
