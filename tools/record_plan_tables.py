"""Record what the seventeen `ct_*_plan` entries of the built library answer on the sweep of tests/_plan_table_cases.py into tests/plan_tables.json
(return value, derived fields of every item, ct_last_error's text), or with --check compare the built library against that record.  CPU only.
Record on the commit whose behaviour is the yardstick, BEFORE changing the planners; tests/test_plan_tables.py replays the file."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _plan_table_cases as C  # noqa: E402
from compressed_tensors_amd import _lib  # noqa: E402

RECORD = os.path.join(ROOT, "tests", "plan_tables.json")


def main():
    lib = _lib.load()
    got = {case["id"]: C.run_case(lib, _lib, case) for case in json.loads(json.dumps(C.cases()))}
    if "--check" in sys.argv:
        want = dict(json.load(open(RECORD)))
        bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
        print(f"{len(got)} cases, {len(bad)} differ" + "".join("\n  " + b for b in bad))
        return 1 if bad else 0
    with open(RECORD, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps([k, g], separators=(",", ":")) for k, g in got.items()) + "\n]\n")
    entries = {k.split("/")[0].split("[")[0] for k in got}
    print(f"{len(got)} cases over {len(entries)} entries -> {RECORD} ({os.path.getsize(RECORD)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
