"""CPU-only: which kernel ct_quant_pack's lean W4 branch launches is a pure function of the value of CT_W4_COMPRESS (diagnostics build), the number of lanes
(elements / 32) and the input's address (csrc/ct_w4_variant.h).  The function is called from a stand-alone program with its own main
(tests/native/w4_variant_check.cpp) built with -fsanitize=address,undefined (runtimes linked in statically): no kernel is launched and nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND = 256 * 8 * 256  # lanes in one residency round of the chip (kW4RoundLanes)

# (environment value or "-" for unset, lanes, address) -> decision
CASES = [
    # plain is plain at every size
    ("plain", 64, 0x1000, "plain"), ("plain", 16 * ROUND, 0x1000, "plain"),
    # lds: whole waves exist and the loads are 16-byte aligned, else the plain kernel (which guards every lane)
    ("lds", 64, 0x1000, "lds"), ("lds", 65, 0x1010, "lds"), ("lds", 63, 0x1000, "plain"), ("lds", 1, 0x1000, "plain"), ("lds", 0, 0x1000, "plain"),
    ("lds", 4 * ROUND, 0x1008, "plain"), ("lds", 4 * ROUND, 0x7F0000001230, "lds"), ("lds", 1 << 38, 0x1000, "lds"),
    # auto (also unset and empty; all the product library ever passes): the LDS form from four residency rounds of lanes
    ("auto", 64, 0x1000, "plain"), ("auto", ROUND, 0x1000, "plain"), ("auto", 4 * ROUND - 1, 0x1000, "plain"), ("auto", 4 * ROUND, 0x1000, "lds"),
    ("auto", 7 * ROUND, 0x1000, "lds"), ("auto", 4 * ROUND, 0x1004, "plain"), ("-", 4 * ROUND, 0x1000, "lds"), ("", 16 * ROUND, 0x1000, "lds"),
    ("-", 25 * ROUND // 16, 0x1000, "plain"),
    # anything else is an error, never a guess
    ("LDS", 64, 0x1000, "bad"), ("ld", 64, 0x1000, "bad"), ("ldss", 64, 0x1000, "bad"), ("1", 64, 0x1000, "bad"), ("auto ", 64, 0x1000, "bad"),
]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("w4_variant") / "w4_variant_check")
    src = os.path.join(ROOT, "tests", "native", "w4_variant_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_variant_rule_under_the_host_sanitizers(checker):
    args = [str(a) for c in CASES for a in c[:3]]
    r = subprocess.run([checker, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr  # a sanitizer report ends the program with a non-zero status
    assert r.stdout.split() == [c[3] for c in CASES]
