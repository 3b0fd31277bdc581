"""Record what the rotation family answers on the sweeps of tests/_hadamard_record_cases.py: the six `ct_hadamard*` row / column entries and
ct_hadamard_k_workspace_bytes on bad arguments into tests/hadamard_refusals.json (return code, ct_last_error's text), and plan_hadamard,
plan_hadamard_k and plan_hadamard_perm into tests/hadamard_plans.json (the plan, or the exception's type and message).  With --check compare the
built tree against the two records.  CPU only: no case reaches a launch.  Record on the commit whose behaviour is the yardstick, BEFORE changing
the launchers or the planners; tests/test_hadamard_refusals.py and tests/test_hadamard_plans.py replay the files."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _hadamard_record_cases as C  # noqa: E402
from compressed_tensors_amd import _lib, codec  # noqa: E402

REFUSALS = os.path.join(ROOT, "tests", "hadamard_refusals.json")
PLANS = os.path.join(ROOT, "tests", "hadamard_plans.json")


def main():
    lib = _lib.load()
    refusals = {c["id"]: C.run_refusal(lib, c) for c in C.refusal_cases()}
    for k, r in refusals.items():  # a refusal of the entry's own checks: CT_ERR_INVALID_ARG or CT_ERR_UNSUPPORTED, never a HIP status
        assert k.startswith("ct_hadamard_k_workspace_bytes/") or (r["ret"] in (_lib.CT_ERR_INVALID_ARG, _lib.CT_ERR_UNSUPPORTED) and r["error"]), (k, r)
    plans = {c["id"]: C.run_plan(codec, c) for c in C.plan_cases()}
    bad = []
    for path, got in ((REFUSALS, refusals), (PLANS, plans)):
        if "--check" in sys.argv:
            want = dict(json.load(open(path)))
            bad += sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
            continue
        with open(path, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps([k, g], separators=(",", ":")) for k, g in got.items()) + "\n]\n")
        print(f"{len(got)} cases -> {path} ({os.path.getsize(path)} bytes)")
    if "--check" in sys.argv:
        print(f"{len(refusals)} + {len(plans)} cases, {len(bad)} differ" + "".join("\n  " + b for b in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
