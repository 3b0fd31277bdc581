"""The compress-side scale fixture on the CPU (tests/_compress_scale_cases.py, tools/gen_golden_compress_scales.py): the pinned oracle's `quantize`,
`fake_quantize` and packed words against what the reference recorded, and the conditions that keep the GPU tests from passing vacuously —
asserted, not assumed: every 16-bit pattern is a scale of each `sweep16` case, every code of the width occurs in every integer case, most groups
take many distinct codes (a group under a NaN, zero or overflowing scale cannot, and says so), both sides of every guard end point meet in every
window of groups a wave can hold, and the one masked property (the int32 cast of a NaN) covers no more than the NaN quotients."""
import os
import subprocess
import sys

import pytest
import torch

import _compress_scale_cases as C
import oracle as O

CASES = dict(C.case_list())
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# rebuilt with the oracle here (the whole matrix is rebuilt where the reference is: test_generator_check...; on the GPU machine every case is)
REBUILT = ["w4.cross.g128.i8.bf16", "w4.guard.g128.ib.f16", "q8.f32.guard.i8", "f8.cross.g256.f8.f16", "w4.cross.chan20.i8.bf16", "w4.f32.g128.i8.xbf16",
           "q8.f32.cross.g256.i8", "fp4.nv.lo_out.bf16", "fp4.nv.hi.f16", "fp4.mx.bf16"]
# the least share of groups that take min(2^bits, G / 4) distinct codes: the groups that do not are those whose scale is non-finite, zero or
# subnormal, or overflows (qmax + 2) |s| — about 1 / 64 of the bfloat16 patterns and 1 / 8 of the float16 ones, more at 8 bits
SHARE = {"bf16": 3 / 4, "f16": 2 / 3}


@pytest.fixture(scope="module")
def manifest():
    return C.load_fixture()[1]


def test_the_manifest_lists_exactly_the_case_matrix(manifest):
    assert sorted(manifest["cases"]) == sorted(CASES)
    assert all(manifest["cases"][k]["recipe"] == r for k, r in CASES.items())
    whole = {f"{k}/{op}" for k, e in manifest["cases"].items() for op, o in e["out"].items() if o["whole"]}
    assert whole == set(C.load_fixture()[0]) and whole
    assert all(CASES[k.split("/")[0]]["scales"] == "cross" for k in whole)
    assert all(sorted(e["out"]) == sorted(CASES[k]["ops"]) for k, e in manifest["cases"].items())


@pytest.mark.parametrize("key", REBUILT)
def test_oracle_matches_the_recorded_reference(manifest, key):
    r = CASES[key]
    t = C.inputs(r)
    assert C.input_sha(t) == manifest["cases"][key]["inputs_sha256"]
    for op, out in C.oracle_outputs(O, r, t).items():
        assert C.fixture_mismatch(key, op, C.masked(r, t, op, out)) == "", op
    assert manifest["cases"][key]["scales"] == C.scale_stats(r, t)
    if r["qtype"] == "int":
        assert manifest["cases"][key]["codes"] == C.code_stats(r, t, C.oracle_outputs(O, r, t, ops=("q",))["q"])


def test_the_comparison_sees_one_code_one_bit_and_the_sign_of_a_zero_but_no_nan_payload():
    key = "w4.cross.g128.i8.bf16"
    r = CASES[key]
    t = C.inputs(r)
    outs = C.oracle_outputs(O, r, t)
    bad = outs["pack"].clone()
    bad[5, 7] ^= 1 << 12
    assert C.fixture_mismatch(key, "pack", outs["pack"]) == "" and C.fixture_mismatch(key, "pack", bad) != ""
    fq = outs["fq"]
    raw = fq.view(torch.int16).reshape(-1)
    zero, nan = int((raw == 0).nonzero()[0]), int(torch.isnan(fq.reshape(-1)).nonzero()[0])
    ordinary = int((torch.isfinite(fq.reshape(-1).float()) & (fq.reshape(-1).float().abs() > 1)).nonzero()[0])
    for at, flip, seen in ((zero, -32768, True), (ordinary, 1, True), (nan, 1, False), (nan, -32768, False)):
        bad = fq.clone()
        bad.view(torch.int16).reshape(-1)[at] ^= flip
        assert (C.fixture_mismatch(key, "fq", bad) != "") is seen, (at, flip)


def test_the_guard_patterns_are_the_end_points_and_their_neighbours():
    for dt, td in C.DTYPES.items():
        vals = C._as_float(torch.tensor(C.guard_bits(dt), dtype=torch.int64), dt).double()
        lo, hi = (2.0 ** e for e in C.GUARD_ENDS[dt])
        assert vals[1] == lo and vals[4] == hi and vals[0] < lo < vals[2] and vals[3] < hi < vals[5] and torch.equal(vals[6:], -vals[:6])
        eps = torch.finfo(td).eps
        below = eps if lo == torch.finfo(td).tiny else eps / 2  # one ulp below 2^e: half the spacing above it, unless a subnormal lies below (fp16's 2^-14)
        assert vals[2] == lo * (1 + eps) and vals[0] == lo * (1 - below) and vals[5] == hi * (1 + eps) and vals[3] == hi * (1 - eps / 2)
        inside = [(lo <= abs(v) <= hi) for v in vals.tolist()]
        assert inside == C.guard_inside(dt) and len(set(C.guard_bits(dt))) == 12


@pytest.mark.parametrize("key", [k for k, r in CASES.items() if r["scales"] == "guard"])
def test_both_sides_of_every_guard_end_point_meet_in_every_wave(key):
    """a wave of 64 lanes holds at least 16 consecutive groups in every kernel form (the lean W4 kernels: 32 elements per lane, groups of 128; every
    other form holds more): every window of 16 consecutive groups holds all 12 guard patterns, so a scale on either side of each end point, of
    either sign, sits next to one on the other side"""
    r = CASES[key]
    bits = C.scale_bits(r).reshape(-1)
    want = sorted(C.guard_bits(r["sdt"]))
    assert bits.numel() >= 64
    windows = bits.unfold(0, 16, 1)
    assert torch.equal(torch.sort(windows, dim=1).values[:, [0, -1]], torch.tensor([want[0], want[-1]]).expand(windows.shape[0], 2))
    assert all(len(set(w)) == 12 for w in windows.tolist())  # every window, not a sample: twelve distinct patterns, all of them guard patterns
    assert set(bits.tolist()) == set(want)
    assert int((bits[1:] == bits[:-1]).sum()) == 0
    raw = C.scale(r).reshape(-1)
    mask = 0xFFFF if r["sdt"] != "f32" else 0xFFFFFFFF
    assert torch.equal(raw.view(torch.int16 if r["sdt"] != "f32" else torch.int32).to(torch.int64) & mask, bits)


@pytest.mark.parametrize("key", [k for k, r in CASES.items() if C.is_sweep16(r)])
def test_every_16_bit_pattern_is_a_scale_exactly_once(manifest, key):
    r = CASES[key]
    every = C.scale_bits(r).reshape(-1)
    assert every.numel() == C.SWEEP and torch.equal(torch.sort(every).values, torch.arange(C.SWEEP))
    assert torch.equal(C.scale(r).view(torch.int16).reshape(-1).to(torch.int64) & 0xFFFF, every)
    assert int((every[1:] - every[:-1]).abs().min()) > 1  # neighbouring groups hold unrelated patterns
    st = manifest["cases"][key]["scales"]
    nan_patterns = 2 * ((1 << (7 if r["sdt"] == "bf16" else 10)) - 1)
    assert st["groups"] == C.SWEEP and st["nan_scales"] == nan_patterns and st["inf_scales"] == 2


def test_the_fp32_cases_hold_every_exponent(manifest):
    import _decompress_scale_cases as D

    b = D.sweep32_bits()
    for key, r in CASES.items():
        if r["scales"] == "sweep32":
            assert torch.equal(torch.sort(C.scale_bits(r).reshape(-1)).values, torch.sort(b).values), key
            assert manifest["cases"][key]["scales"]["nan_scales"] == 6 and manifest["cases"][key]["scales"]["inf_scales"] == 2


@pytest.mark.parametrize("key", [k for k, r in CASES.items() if r["qtype"] == "int"])
def test_every_code_occurs_and_most_groups_take_many(manifest, key):
    r = CASES[key]
    codes = manifest["cases"][key]["codes"]
    assert len(codes["histogram"]) == 1 << r["bits"] and min(codes["histogram"]) > 0
    rows, cols, g, G = C.layout(r)
    assert sum(codes["groups_by_distinct_codes"].values()) == rows * G
    if C.is_sweep16(r):
        need = min(1 << r["bits"], g // 4)
        share = sum(n for d, n in codes["groups_by_distinct_codes"].items() if int(d) >= need) / (rows * G)
        print(f"{key}: {share:.4f} of the groups take at least {need} distinct codes")
        assert share >= SHARE[r["sdt"]]


@pytest.mark.parametrize("key", ["w4.g128.ib.f16", "q8.g128.i8.bf16"])
def test_the_groups_of_few_codes_are_the_ones_whose_scale_leaves_no_room(key):
    """rebuilt with the oracle: a group that takes fewer than min(2^bits, G / 4) distinct codes has a scale that is non-finite, zero or subnormal,
    or whose largest target (qmax + 2 + |z|) |s| overflows the weight's dtype"""
    r = CASES[key]
    t = C.inputs(r)
    q = C.oracle_outputs(O, r, t, ops=("q",))["q"]
    rows, cols, g, G = C.layout(r)
    u = (q.to(torch.int64) + (1 << (r["bits"] - 1))).reshape(rows, G, g)
    seen = torch.zeros((rows, G, 1 << r["bits"]), dtype=torch.bool)
    seen.scatter_(2, u, torch.ones_like(u, dtype=torch.bool))
    few = seen.sum(dim=2) < min(1 << r["bits"], g // 4)
    s = t["scale"].double().abs()
    fi = torch.finfo(t["scale"].dtype)
    room = (1 << (r["bits"] - 1)) + 2 + t["zero_point"].double().abs()
    no_room = ~torch.isfinite(s) | (s < fi.tiny) | (room * s > fi.max)
    assert bool((~few | no_room).all()), int((few & ~no_room).sum())
    assert 0 < int(few.sum()) < few.numel() // 3


@pytest.mark.parametrize("key", [k for k, r in CASES.items() if r["scales"] == "cross"])
def test_every_edge_scale_meets_every_zero_point(key):
    import _decompress_scale_cases as D

    r = CASES[key]
    lo, n = D._zp_range(C._drec(r)) if r["zp"] and r["zp"] != "f8z" else (0, 1)
    edges = C.edge_bits(r["sdt"])
    assert len(edges) == 17 == len(set(edges))
    sb = C.scale_bits(r).reshape(-1)
    z = C.zero_point(r)
    zi = (z.view(torch.int8).to(torch.int64).reshape(-1) - lo) if n > 1 else torch.zeros_like(sb)
    place = {b: i for i, b in enumerate(edges)}
    which = torch.tensor([place[b] for b in sb.tolist()])  # (KeyError: a scale that is no edge scale)
    seen = torch.zeros((len(edges), n), dtype=torch.bool)
    seen[which, zi] = True
    assert bool(seen.all())
    if r["qtype"] == "fp8":  # and every edge scale meets every float8 target
        rows, cols, g, G = C.layout(r)
        gi = C.group_index(r)[:, :, None].expand(rows, G, g)
        ti = C.target_index(r, gi, torch.arange(g)[None, None, :].expand(rows, G, g))
        met = torch.zeros((len(edges), C.F8_TARGETS), dtype=torch.bool)
        met[which.reshape(rows, G, 1).expand(rows, G, g), ti] = True
        assert bool(met.all()), int((~met).sum())


def test_the_fp32_edge_scales_are_the_patterns_they_claim():
    e = C._as_float(torch.tensor(C.edge_bits("f32"), dtype=torch.int64), "f32").double()
    fi = torch.finfo(torch.float32)
    sub = fi.tiny * fi.eps
    want = [0.0, sub, fi.tiny - sub, fi.tiny, 1.0, fi.max, float("inf")]
    assert e[:14:2].tolist() == want and e[1:14:2].tolist() == [-v for v in want] and bool(torch.isnan(e[14:]).all())


@pytest.mark.parametrize("key", [k for k, r in CASES.items() if r["qtype"] in ("fp8", "fp4")])
def test_every_float_target_is_reached(key):
    """the step through the target table is prime to its length: a group of at least that many positions holds every target, and a shorter one
    holds as many distinct targets as it has positions"""
    import math

    r = CASES[key]
    rows, cols, g, G = C.layout(r)
    n = C.F8_TARGETS if r["qtype"] == "fp8" else len(C.FP4_TARGETS)
    assert math.gcd(C._step(n), n) == 1
    gi = C.group_index(r)[::7, :, None]
    ti = C.target_index(r, gi.expand(gi.shape[0], G, g), torch.arange(g)[None, None, :].expand(gi.shape[0], G, g))
    distinct = torch.zeros((gi.shape[0], G, n), dtype=torch.bool).scatter_(2, ti, True).sum(dim=2)
    assert bool((distinct == min(g, n)).all())
    whole = torch.zeros(n, dtype=torch.bool)
    whole[C.target_index(r, C.group_index(r)[:, :, None].expand(rows, G, g), torch.arange(g)[None, None, :].expand(rows, G, g)).reshape(-1)] = True
    assert bool(whole.all())


# ---- FP4 with given scales ----------------------------------------------------------------------------------------------------------------------
def test_the_fp4_global_scales_put_s_eff_where_they_claim():
    """over the 126 finite positive float8 values (2^-9 .. 448): inside the guard [2^-20, 2^10] for all, exactly at an end for one byte, one fp32
    ulp outside an end, or outside for all"""
    lo, hi = (2.0 ** e for e in C.FP4_GUARD)
    vals = torch.arange(256, dtype=torch.int64).to(torch.uint8).view(C.F8).float()
    pos = vals[(vals > 0) & ~torch.isnan(vals)]
    assert pos.numel() == 126 and float(pos.min()) == 2.0 ** -9 and float(pos.max()) == 448.0
    s_eff = {name: (pos / C.global_scale(dict(gs=bits))).double() for name, bits in C.FP4_GLOBALS.items()}
    inside = {name: (v >= lo) & (v <= hi) for name, v in s_eff.items()}
    ulp_lo, ulp_hi = lo * 2.0 ** -24, hi * 2.0 ** -23  # the fp32 spacing just below 2^-20 and just above 2^10
    assert bool(inside["one"].all()) and bool(inside["odd"].all())
    assert float(s_eff["lo"].min()) == lo and bool(inside["lo"].all())
    # (the smallest global scale above 2^11 is 2^11 (1 + 2^-23): the quotient lands two places below 2^-20, the nearest this byte can come from outside)
    assert float(s_eff["lo_out"].min()) == lo - 2 * ulp_lo and int((~inside["lo_out"]).sum()) == 1
    assert sorted(s_eff["lo2"].tolist())[:2] == [lo / 2, lo] and int((~inside["lo2"]).sum()) == 1
    assert bool((s_eff["hi"] == hi).any()) and int((~inside["hi"]).sum()) == int((pos > 256).sum()) == 6
    assert float(s_eff["hi_in"][pos == 256]) == hi - 2 * hi * 2.0 ** -24 and int((~inside["hi_in"]).sum()) == 6
    assert float(s_eff["hi_out"][pos == 256]) == hi + ulp_hi and int((~inside["hi_out"]).sum()) == 7
    assert not bool(inside["far_lo"].any()) and not bool(inside["far_hi"].any())
    assert sorted(k.split(".")[2] for k in CASES if k.startswith("fp4.nv.") and k.endswith(".bf16")) == sorted(C.FP4_GLOBALS)


@pytest.mark.parametrize("key", [k for k, r in CASES.items() if r["qtype"] == "fp4"])
def test_every_fp4_scale_meets_every_target(manifest, key):
    """NVFP4: all 256 float8 bytes are a scale, each in 16 groups; MXFP4: every positive power of two of the dtype.  Each of them meets every one
    of the 34 targets, and neighbouring groups hold different scales"""
    r = CASES[key]
    rows, cols, g, G = C.layout(r)
    sb = C.scale_bits(r)
    s = C.scale(r)
    if r["scales"] == "f8bytes":
        by = s.to(C.F8).view(torch.uint8)
        assert torch.equal(by.view(C.F8).to(s.dtype).view(torch.int16)[~torch.isnan(s)], s.view(torch.int16)[~torch.isnan(s)])  # float8 values, held exactly
        assert torch.equal(torch.bincount(((C.group_index(r) * 77 + 5) % 256).reshape(-1), minlength=256), torch.full((256,), rows * G // 256))
        assert int(torch.isnan(s).sum()) == 2 * rows * G // 256 and int((s == 0).sum()) == 2 * rows * G // 256
        ids, n = ((C.group_index(r) * 77 + 5) % 256), 256
    else:
        p = C.pow2_bits(r["sdt"])
        v = C._as_float(torch.tensor(p, dtype=torch.int64), r["sdt"]).double()
        fi = torch.finfo(C.DTYPES[r["sdt"]])
        assert bool((torch.log2(v) == torch.round(torch.log2(v))).all()) and float(v.min()) == fi.tiny * fi.eps and float(v.max()) == 2.0 ** int(torch.log2(torch.tensor(fi.max)))
        assert len(p) == len(set(p)) == int(torch.log2(v.max()) - torch.log2(v.min())) + 1  # every one of them
        place = {b: i for i, b in enumerate(p)}
        ids, n = torch.tensor([place[b] for b in sb.reshape(-1).tolist()]).reshape(rows, G), len(p)
        assert bool((torch.bincount(ids.reshape(-1), minlength=n) >= rows * G // n).all())
    assert int((sb.reshape(-1)[1:] == sb.reshape(-1)[:-1]).sum()) == 0
    gi = C.group_index(r)[:, :, None].expand(rows, G, g)
    ti = C.target_index(r, gi, torch.arange(g)[None, None, :].expand(rows, G, g))
    met = torch.zeros((n, len(C.FP4_TARGETS)), dtype=torch.bool)
    met[ids[:, :, None].expand(rows, G, g)[:, :, : g - 5], ti[:, :, : g - 5]] = True  # (the last five positions hold the special values)
    assert bool(met.all()), int((~met).sum())
    out = manifest["cases"][key]["out"]["fp4"]
    assert out["dtype"] == "uint8" and out["shape"] == [rows, cols // 2]


def test_the_masked_share_is_at_most_the_share_of_nan_quotients(manifest):
    """what is left uncompared — the int32 cast of a NaN and the sign bit of an FP4 code of a NaN (`_compress_scale_cases.masked`) — covers exactly
    the elements whose quotient is NaN, in the int32-typed and the FP4 outputs alone; everything else is compared whole"""
    any_masked = 0
    for key, e in manifest["cases"].items():
        st = e["scales"]
        assert sorted(st["masked"]) == sorted(op for op in CASES[key]["ops"] if op in C.MASKED_OPS), key
        for op, n in st["masked"].items():
            # (FP4 under the global scale 2^-30: float16 weights overflow to inf, and an inf moved one place up is a NaN — a third of that case)
            assert op in ("q32", "fp4") and n <= st["nan_quotients"] < st["numel"] // (8 if op == "q32" else 2), key
            any_masked += n
        # NaN is present in every case, and no case is mostly NaN (7 of the 17 edge scales of a cross make every quotient of their groups NaN: three
        # NaNs, +-0 under which the weights are 0 (0 / 0), +-inf under which they are inf or NaN)
        assert 0 < st["nan_quotients"] < st["numel"] // (2 if CASES[key]["scales"] == "cross" or CASES[key]["qtype"] == "fp4" else 4), key
    assert any_masked > 0


def test_the_float8_targets_hold_every_value_and_every_midpoint():
    t = C.f8_targets()
    vals = torch.arange(256, dtype=torch.int64).to(torch.uint8).view(C.F8).float()
    assert torch.equal(t[:256].view(torch.int32), vals.view(torch.int32)) and int(torch.isnan(t).sum()) == 2
    finite = torch.sort(torch.unique(vals[~torch.isnan(vals)])).values
    assert finite.numel() == 253 and torch.equal(t[256:508], (finite[1:] + finite[:-1]) / 2) and float(t[508]) > 448 > 0 > -448 > float(t[509])
    # a midpoint is a tie of the float8 rounding: it is no float8 value itself
    assert not bool(torch.isin(t[256:508], finite).any())


def test_generator_check_where_the_reference_is():
    """the committed fixture is what the reference produces, and the pinned oracle is the reference on every case (the generator imports it;
    skipped where its sources are not present)"""
    import ref_import

    if not ref_import.available():
        pytest.skip("upstream reference sources not present on this machine")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_compress_scales.py"), "--check"], capture_output=True, text=True, env=env)
    assert done.returncode == 0 and "fixture matches" in done.stdout, done.stdout + done.stderr
