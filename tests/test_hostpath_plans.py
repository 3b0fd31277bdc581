"""CPU-only: the twelve module-loop entries of csrc/host/ct_hostpath.cpp (w4 / q8 / mx8 / w8 / fp4 `_plan_compress` and `_plan_decompress`, `wb_compress_modules`,
`wb_decompress_modules`) and its five finish functions, called directly on the trees of tests/_hostpath_plan_cases.py, do what tests/hostpath_plans.json
holds — written by tools/record_hostpath_plans.py on the commit BEFORE the loops moved onto one plan driver, one row builder and one finish driver.  Compared
word for word: the batch keys in returned order, both tables' row counts, every word of every row (pointers by the entry they belong to, allocations by the
entry that holds them after the finish), which modules come back in `rest`, every job tuple's elements (the keep-alive references among them), and every
module's entries — names, ORDER, kinds, trainability, shapes, dtypes — and status after the finish."""
import json
import os

import pytest

import _hostpath_plan_cases as C

RECORD = C.unpack(json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostpath_plans.json"))))
CASES = C.cases()


@pytest.fixture(scope="module")
def hostpath():
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import _lib

    hp = _lib.hostpath()
    assert hp is not None, "the host extension was not built (python -c 'import __graft_entry__ as g; g.build()')"
    yield cta, hp
    C.restore()


def test_record_is_the_sweep_and_reaches_every_entry():
    assert [c["id"] for c in CASES] == list(RECORD)  # nothing dropped, added or reordered by hand
    assert {c["family"] for c in CASES} == {"w4", "q8", "mx8", "w8", "fp4", "wb"}
    for c in CASES:
        calls = RECORD[c["id"]]
        assert [r["call"] for r in calls] == [f"{d}{k}" for k in range(c.get("rounds", 1)) for d in ("compress", "decompress")]
    # more than one batch key somewhere in every table family and direction (float16 next to bfloat16), a second table, and taken as well as refused modules
    for fam in ("w4", "q8", "w8", "fp4"):
        mine = [r for c in CASES if c["family"] == fam for r in RECORD[c["id"]]]
        assert any(len(r["keys"]) > 1 for r in mine if r["call"].startswith("compress")), fam
        assert any(r["rest"] for r in mine) and any(b["n"] for r in mine for b in r["batches"]), fam
    assert any(b["aux_n"] for c in CASES if c["family"] == "w4" for r in RECORD[c["id"]] for b in r["batches"])
    assert all(b["aux_n"] == b["n"] for c in CASES if c["family"] == "mx8" for r in RECORD[c["id"]] for b in r["batches"])
    wb = [r for c in CASES if c["family"] == "wb" for r in RECORD[c["id"]]]
    assert any(r["rest"] for r in wb) and any(len(r["rest"]) < len(C.SHAPES) for r in wb)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_hostpath_plans(hostpath, case):
    cta, hp = hostpath
    got = json.loads(json.dumps(C.run_case(cta, hp, case)))
    want = RECORD[case["id"]]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for key in w:
            assert g[key] == w[key], (case["id"], w["call"], key)
        assert g == w
