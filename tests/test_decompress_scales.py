"""The decompress-side scale fixture on the CPU (tests/_decompress_scale_cases.py, tools/gen_golden_decompress_scales.py): the pinned oracle's
`dequantize` against what the reference recorded for every case, and the conditions the GPU tests rely on — asserted, not assumed: every 16-bit
pattern is a scale of each `sweep16` case, every (edge scale, zero point, code) triple occurs in each `cross` case, and the recorded outputs hold
NaN, inf, subnormal and ordinary values in numbers that an all-NaN comparison could not pass."""
import os
import subprocess
import sys

import pytest
import torch

import _decompress_scale_cases as C
import oracle as O

CASES = dict(C.case_list())
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def manifest():
    return C.load_fixture()[1]


def test_the_manifest_lists_exactly_the_case_matrix(manifest):
    assert sorted(manifest["cases"]) == sorted(CASES)
    assert all(manifest["cases"][k]["recipe"] == r for k, r in CASES.items())
    assert {k for k, e in manifest["cases"].items() if e["out"]["whole"]} == set(C.load_fixture()[0])
    assert all(CASES[k]["scales"] == "cross" for k in C.load_fixture()[0])


@pytest.mark.parametrize("key", list(CASES))
def test_oracle_matches_the_recorded_reference(manifest, key):
    r = CASES[key]
    t = C.inputs(r)
    assert C.input_sha(t) == manifest["cases"][key]["inputs_sha256"]
    assert C.fixture_mismatch(key, C.oracle_output(O, r, t)) == ""


def test_the_comparison_sees_one_bit_and_the_sign_of_a_zero_but_no_nan_payload():
    """what `fixture_mismatch` (and `eq` on the GPU side) can and cannot tell apart, on a case kept whole and on one kept as a hash"""
    for key in ("w4.cross.g128.i4.bf16", "w4.g32.i8.f16"):
        out = C.oracle_output(O, CASES[key])
        assert C.fixture_mismatch(key, out) == ""
        raw = out.view(torch.int16).reshape(-1)
        zero = int((raw == 0).nonzero()[0])  # a +0.0
        nan = int(torch.isnan(out.reshape(-1)).nonzero()[0])
        ordinary = int(((out.reshape(-1).float().abs() > 1) & torch.isfinite(out.reshape(-1).float())).nonzero()[0])
        for at, flip, seen in ((zero, -32768, True), (ordinary, 1, True), (nan, 1, False), (nan, -32768, False)):
            bad = out.clone()
            bad.view(torch.int16).reshape(-1)[at] ^= flip
            assert (C.fixture_mismatch(key, bad) != "") is seen, (key, at, flip)
    a, b = C.sweep16("bf16"), C.sweep16("bf16", 1)
    assert not torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(torch.sort(a.view(torch.int16)).values, torch.sort(b.view(torch.int16)).values)
    assert C.sweep32().dtype is torch.float32 and int(torch.isnan(C.sweep32()).sum()) == 2 * 3  # exponent 255 with a non-zero mantissa, both signs


def test_the_edge_scales_are_the_patterns_they_claim():
    for dt, td in (("bf16", C.BF16), ("f16", C.F16)):
        e = torch.tensor([p - 65536 if p >= 32768 else p for p in C.edge(dt)], dtype=torch.int16).view(td).float()
        fi = torch.finfo(td)
        sub = fi.tiny * fi.eps  # the smallest subnormal: the smallest normal's last mantissa bit
        want = [0.0, sub, fi.tiny - sub, fi.tiny, 1.0, fi.max, float("inf")]
        assert e[:14:2].tolist() == want and e[1:14:2].tolist() == [-v for v in want]
        assert torch.signbit(e[1]) and not torch.signbit(e[0]) and bool(torch.isnan(e[14:]).all()) and len(set(C.edge(dt))) == 17


@pytest.mark.parametrize("key", [k for k, r in CASES.items() if C.is_sweep16(r)])
def test_every_16_bit_pattern_is_a_scale(manifest, key):
    r = CASES[key]
    every = C.scale_bits(r).reshape(-1)
    assert torch.equal(C.scale(r).view(torch.int16).reshape(-1).to(torch.int64) & 0xFFFF, every)
    copies = r["sweeps"] or every.numel() // C.SWEEP  # (`sweeps`: the cross follows that many copies)
    bits = every[:copies * C.SWEEP]
    assert copies >= 1 and (r["sweeps"] or bits.numel() == every.numel())
    for copy in bits.reshape(-1, C.SWEEP):  # each copy of the sweep holds each pattern exactly once
        assert torch.equal(torch.sort(copy).values, torch.arange(C.SWEEP))
    # neighbouring groups hold unrelated patterns: never the same, never adjacent ones
    assert int((bits[1:] - bits[:-1]).abs().min()) > 1
    # the recorded output holds every class of value, and NaN is rare: a pass cannot come from an all-NaN comparison
    out = manifest["cases"][key]["out"]
    ordinary = out["numel"] - out["nans"] - out["infs"] - out["subnormals"]
    assert min(out["nans"], out["infs"], out["subnormals"], ordinary) > 0
    if not r["sweeps"]:  # (a cross behind the sweep brings its own NaN scales: three of seventeen)
        assert out["nans"] < out["numel"] * (0.02 if r["sdt"] == "bf16" else 0.065)


def test_the_fp32_sweep_holds_every_exponent():
    b = C.sweep32_bits()
    assert len(set(b.tolist())) == 2048
    assert {(int(v) >> 23) & 255 for v in b} == set(range(256)) and {int(v) & 0x7FFFFF for v in b} == {0, 1, 0x400000, 0x7FFFFF}
    for key, r in CASES.items():
        if r["scales"] == "sweep32":
            assert torch.equal(torch.sort(C.scale_bits(r).reshape(-1)).values, torch.sort(b).values), key


@pytest.mark.parametrize("key", [k for k, r in CASES.items() if r["scales"] == "cross" or r["sweeps"]])
def test_every_edge_scale_meets_every_zero_point_and_code(key):
    r = CASES[key]
    t = C.inputs(r)
    rows, cols, g, G = C.layout(r)
    lo, n = C._zp_range(r) if r["zp"] else (0, 1)
    ncodes = 1 << r["bits"]
    sb = C.scale_bits(r)
    z = (t["zero_point"].view(torch.int8).to(torch.int64) - lo) if r["zp"] else torch.zeros_like(sb)
    q = t["q"].view(torch.int8).to(torch.int64) + ncodes // 2
    col_group = t["g_idx"].to(torch.int64) if t["g_idx"] is not None else torch.arange(cols) // g
    edges = C.edge(r["sdt"])
    which = torch.full((65536,), len(edges), dtype=torch.int64)  # pattern -> its place among the edge scales; the last slot: any other pattern
    which[torch.tensor(edges)] = torch.arange(len(edges))
    seen = torch.zeros((len(edges) + 1, n, ncodes), dtype=torch.bool)
    seen[which[sb][:, col_group], z[:, col_group], q] = True
    seen = seen[:-1]
    if g >= ncodes:  # a group holds every code
        assert bool(seen.all())
    else:  # rows of fewer columns than codes (the any-layout kernels): every pair, and every code under every edge scale
        assert bool(seen.any(dim=2).all()) and bool(seen.any(dim=1).all())


def test_the_e8m0_case_holds_every_exponent_byte_and_code():
    r = CASES["mxfp8.e8m0"]
    t = C.inputs(r)
    assert sorted(t["scale"][:, 0].tolist()) == list(range(256)) and bool((t["scale"] == t["scale"][:, :1]).all())
    assert all(len(set(row.tolist())) == 256 for row in t["q"].view(torch.uint8)[::37])


def test_generator_check_where_the_reference_is():
    """the committed fixture is what the reference produces (the generator imports it; skipped where its sources are not present)"""
    import ref_import

    if not ref_import.available():
        pytest.skip("upstream reference sources not present on this machine")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_decompress_scales.py"), "--check"], capture_output=True, text=True, env=env)
    assert done.returncode == 0 and "fixture matches" in done.stdout, done.stdout + done.stderr
