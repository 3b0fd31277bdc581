"""CPU-only: the seventeen `ct_*_plan` entries answer the recorded sweep (tests/plan_tables.json, written by tools/record_plan_tables.py on the commit
before the planners moved onto csrc/ct_plan.h) byte for byte: the return value, every derived field of every item after the call — fields the planner
leaves alone included, they hold a sentinel — and the full text of ct_last_error on a refusal.  Per entry: an admitted table, one table per refusal
branch with the offending item not first, n = 0, (NULL, 0), (NULL, 1), n = -1, bad extra arguments, and a table past 2^31 workgroups (or the entry's
own cap).  The tables are tests/_plan_table_cases.py's; the record holds what the library answered.  Left out because they are no pure function of
the input: `gen` of ct_bitmask_item (a process-wide counter), and `tpw` / `nwg` and the count ct_bitmask_batch_plan returns (they follow the
device's CU count; its sign is kept)."""
import json
import os

import pytest

import _plan_table_cases as C

RECORD = dict(json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_tables.json"))))
CASES = json.loads(json.dumps(C.cases()))
ENTRIES = ("ct_w4_batch_plan", "ct_rtn_w4_batch_plan", "ct_q8_batch_plan", "ct_rtn_channel8_batch_plan", "ct_rtn_block8_batch_plan", "ct_rtn_group8_batch_plan",
           "ct_rtn_wb_batch_plan", "ct_fp4_batch_plan", "ct_mx_scale_batch_plan", "ct_rtn_mxfp4_batch_plan", "ct_rtn_nvfp4_batch_plan", "ct_zp4_batch_plan",
           "ct_bitmask_batch_plan", "ct_bitmask_decompress_batch_plan", "ct_copy_batch_plan", "ct_awq_repack_plan", "ct_fp8block_dequant_plan")
# the three entries whose (NULL, 0) / n = 0 answers differ from the rest: recorded as they are
REFUSE_NULL0 = ("ct_fp4_batch_plan", "ct_mx_scale_batch_plan", "ct_rtn_nvfp4_batch_plan")


@pytest.fixture(scope="module")
def lib():
    from compressed_tensors_amd import _lib

    return _lib.load()


def test_record_covers_every_plan_entry_and_is_the_sweep():
    assert {c["entry"] for c in CASES} == set(ENTRIES)
    assert [c["id"] for c in CASES] == list(RECORD)  # nothing dropped, added or reordered by hand
    for e in ENTRIES:
        mine = [(c["id"].split("/", 1)[1], RECORD[c["id"]]) for c in CASES if c["entry"] == e]
        assert {"admitted", "n0", "null0", "null1", "nneg", "cross", "refuse"} <= {k.split(":")[0] for k, _ in mine}, e
        for kind, r in mine:
            if kind.startswith(("refuse", "cross", "nneg", "null1", "badarg")):
                assert r["ret"] == -1 and r["error"], (e, kind)
            elif kind == "admitted":
                assert r["ret"] >= 0 and r["error"] is None, (e, kind)
            elif kind == "null0":
                assert (r["ret"] == -1) == (e in REFUSE_NULL0), (e, kind)
            elif kind == "n0":
                assert (r["ret"] == -1) == (e == "ct_rtn_nvfp4_batch_plan"), (e, kind)


@pytest.mark.parametrize("entry", ENTRIES)
def test_plan_answers_the_record(lib, entry):
    from compressed_tensors_amd import _lib

    for case in (c for c in CASES if c["entry"] == entry):
        assert C.run_case(lib, _lib, case) == RECORD[case["id"]], case["id"]


def test_plan_header_under_the_host_sanitizers(tmp_path):
    """csrc/ct_plan.h in a stand-alone program with its own main (tests/native/plan_check.cpp), built with -fsanitize=address,undefined: magic_div for every
    divisor in 1..2^16 and around every power of two up to 2^31 against plain division (it shifts by up to 62), and the plan loop on a dummy item type up to
    and past the 2^31 refusal (its sum saturates).  No kernel is launched and nothing is loaded into python."""
    import shutil
    import subprocess

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "plan_check")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "plan_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr  # a sanitizer report ends the program with a non-zero status
