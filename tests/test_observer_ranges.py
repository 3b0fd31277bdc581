"""The observer-range fixture on the CPU (tests/_observer_range_cases.py, tools/gen_golden_observer_ranges.py): the pinned oracle's
`calculate_qparams_minmax`, `calculate_qparams_float` and `generate_gparam` against what the reference recorded, and the conditions that keep the
GPU tests from passing vacuously — asserted, not assumed: every 16-bit pattern is the extreme of exactly one group of each `sweep16` case, every
group's min and max are its two planted values, most scales are finite, the eps substitution occurs, the zero points cover their range, and the
one masked property (the MX scale of a group that holds a NaN) covers exactly the groups that hold one."""
import os
import subprocess
import sys

import pytest
import torch

import _observer_range_cases as R
import oracle as O

CASES = dict(R.case_list())
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# rebuilt with the oracle here (the whole matrix is rebuilt where the reference is: test_generator_check...; on the GPU machine every case is)
REBUILT = ["s16.g32.bf16", "s16.g16.f16", "e16.chan2056.f16", "e16.g2048.bf16", "ties.g32.f16", "c16.g48.bf16", "c16.g32.f16", "c16.blk16x64.bf16",
           "s16.blk4x16.f16", "s32.g32", "c32.g8"]
NAN_PATTERNS = {"bf16": 254, "f16": 2046}  # 2 (2^mantissa - 1)


@pytest.fixture(scope="module")
def manifest():
    return R.load_fixture()[1]


def test_the_manifest_lists_exactly_the_case_matrix(manifest):
    assert sorted(manifest["cases"]) == sorted(CASES)
    assert all(manifest["cases"][k]["recipe"] == r for k, r in CASES.items())
    assert all(sorted(e["out"]) == sorted(CASES[k]["ops"]) for k, e in manifest["cases"].items())
    whole = {f"{k}/{op}" for k, e in manifest["cases"].items() for op, o in e["out"].items() if o["whole"]}
    assert whole and whole == {k.rsplit("/", 1)[0] for k in R.load_fixture()[0]}
    assert all(CASES[k.split("/")[0]]["pat"] == "cross" for k in whole)
    assert sorted(manifest["gparam"]) == sorted(f"{dt}.{a}x{b}" for dt in ("bf16", "f16") for a, b in R.gparam_shapes())


def test_each_fixture_file_stays_under_one_mebibyte():
    for name in ("observer_ranges.safetensors", "observer_ranges_manifest.json"):
        assert os.path.getsize(os.path.join(R.GOLDEN, name)) < 1 << 20, name


@pytest.mark.parametrize("key", sorted(CASES))
def test_every_group_holds_exactly_its_two_planted_values(manifest, key):
    """torch.aminmax of every group is (the smaller, the larger) of the planted extreme and partner — up to the sign of a zero — and NaN exactly
    where one of them is a NaN; the two sit at different positions of the group"""
    r = CASES[key]
    x = R.weight(r)
    assert R.sha(x) == manifest["cases"][key]["input_sha256"] and list(x.shape) == r["shape"] and x.dtype is R.DTYPES[r["dt"]]
    whole_nan = int(R.nan_groups(r, x).sum())
    r, x = R.built(r), x.reshape(R.built(r)["shape"])  # (the `tensor` case: the groups it was built of)
    mn, mx = R.group_minmax(r, x)
    E, P = R.planted(r)
    nan = torch.isnan(E) | torch.isnan(P)
    assert torch.equal(torch.isnan(mn), nan) and torch.equal(torch.isnan(mx), nan)
    assert torch.equal(mn[~nan], torch.minimum(E, P)[~nan]) and torch.equal(mx[~nan], torch.maximum(E, P)[~nan])
    assert manifest["cases"][key]["nan_groups"] == whole_nan and (CASES[key]["built"] or manifest["cases"][key]["groups"] == nan.numel())
    pe, pp, glen = R.positions(r)
    m = R.to_groups(r, x)
    rows, cols, g, G = R.layout(r)
    raw = m.view(torch.int32 if r["dt"] == "f32" else torch.int16).to(torch.int64) & ((1 << (32 if r["dt"] == "f32" else 16)) - 1)
    Eb, Pb = R.planted_bits(r)
    at = torch.arange(G)[None, :] * g
    assert torch.equal(torch.gather(raw, 1, at + pe), Eb) and torch.equal(torch.gather(raw, 1, at + pp), Pb)
    if g >= 32:  # half a group plus 5 further: in another 16-byte unit (a lane of the per-unit kernels), whatever the extreme's position
        assert bool(((pe // 8 != pp // 8) | (glen < 32)).all())
    elif g == 16:  # two units: 13 further is the other unit for the positions 3 .. 7 and 11 .. 15 of the partner
        assert 0 < int((pe // 8 != pp // 8).sum()) < pe.numel()


@pytest.mark.parametrize("key", [k for k, r in CASES.items() if R.is_sweep16(r)])
def test_every_16_bit_pattern_is_the_extreme_of_exactly_one_group(manifest, key):
    r = CASES[key]
    E, P = R.planted_bits(r)
    assert E.numel() == R.SWEEP and torch.equal(torch.sort(E.reshape(-1)).values, torch.arange(R.SWEEP))
    assert int((E.reshape(-1)[1:] - E.reshape(-1)[:-1]).abs().min()) > 1  # neighbouring groups hold unrelated patterns
    sign, inf, _, _ = R.fmt(r["dt"])
    assert bool(((E ^ P) & sign == sign).all()) and bool(((P & (sign - 1)) < inf).all())  # the partner: the other sign, finite
    assert torch.equal(torch.bincount(torch.tensor([R.finite_edges(r["dt"]).index(int(v)) for v in (P.reshape(-1)[:600] & (sign - 1))]), minlength=6),
                       torch.full((6,), 100))
    assert manifest["cases"][key]["nan_groups"] == NAN_PATTERNS[r["dt"]]


def test_the_other_patterns_are_what_they_claim():
    for dt in ("bf16", "f16"):
        e, m = R._FMT[dt]
        b = R.exp16_bits(dt)
        assert b.numel() == len(set(b.tolist())) == 1 << (e + 3)
        assert set(((b >> m) & ((1 << e) - 1)).tolist()) == set(range(1 << e)) and set((b >> 15).tolist()) == {0, 1}
        assert set((b & ((1 << m) - 1)).tolist()) == {0, 1, 1 << (m - 1), (1 << m) - 1}
        ext, par = R.pattern("cross", dt)
        assert len(set(zip(ext.tolist(), par.tolist()))) == 289 and set(ext.tolist()) == set(R.edge(dt)) == set(par.tolist())
    assert torch.equal(torch.sort(R.sweep32_perm()).values, torch.sort(R.D.sweep32_bits()).values)
    assert torch.equal(R.as_float(R.D.sweep32_bits(), "f32").view(torch.int32), R.sweep32().view(torch.int32))
    assert torch.equal(R.as_float(R.sweep16_bits(0), "bf16").view(torch.int16), R.sweep16("bf16").view(torch.int16))
    e32, _ = R.pattern("cross", "f32")
    assert set(e32.tolist()) == set(R.C.edge_bits("f32"))
    for key, r in CASES.items():  # every pattern of a case's table occurs in it
        n = len(R.pattern(r["pat"], r["dt"])[0])
        assert R.layout(R.built(r))[0] * R.layout(R.built(r))[3] >= n, key


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_the_ties_put_the_zero_point_at_a_half_integer(dt):
    """before the rounding to the dtype: mn / ((mx - mn) / (2^b - 1)) = -(2 k + 1) / 2 for every k < 2^b; and most of them survive the rounding
    (they are small integers times a power of two: exact until 2 k + 1 needs more than the significand)"""
    mn, mx = (R.as_float(t, dt).double() for t in R.tie_pairs(dt))
    at, exact = 0, 0
    for b in range(1, 9):
        n = 3 * (1 << b)
        k = torch.arange(1 << b, dtype=torch.float64).repeat_interleave(3)
        e = torch.tensor(R.TIE_EXPONENTS, dtype=torch.float64).repeat(1 << b)
        want_mn, want_mx = -(2 * k + 1) * 2 ** e, (2 * ((1 << b) - 1) - (2 * k + 1)) * 2 ** e
        assert bool(((want_mn / ((want_mx - want_mn) / ((1 << b) - 1))) == -(2 * k + 1) / 2).all())
        same = (mn[at:at + n] == want_mn) & (mx[at:at + n] == want_mx)
        exact += int(same.sum())
        if b <= (7 if dt == "bf16" else 8):
            assert bool(same.all()), b
        at += n
    assert at == mn.numel() == 1530 and exact >= 1530 - 3 * 256


@pytest.mark.parametrize("key", [k for k, r in CASES.items() if R.is_sweep16(r)])
def test_most_scales_are_finite_the_eps_occurs_and_the_zero_points_cover_their_range(manifest, key):
    r = CASES[key]
    e = manifest["cases"][key]
    for op, o in e["out"].items():
        share = (o["nans"] + o["infs"]) / e["groups"]
        print(f"{key}/{op}: non-finite {share:.4f}, eps {o.get('eps')}, distinct zero points {o.get('zps')}")
        assert share <= 1 / 4, op  # a cap, not a measurement
        p = R.parse_op(op)
        if p["kind"] != "int":
            continue
        assert o["eps"] >= 1, op
        if p["symmetric"]:
            assert o["zps"] == 1
        elif p["bits"] <= 4:
            assert o["zps"] == 1 << p["bits"], op
        elif p["bits"] == 8:
            assert o["zps"] >= 200, op


@pytest.mark.parametrize("key", REBUILT)
def test_oracle_matches_the_recorded_reference(manifest, key):
    r = CASES[key]
    x = R.weight(r)
    for op in r["ops"]:
        s, z = R.oracle_output(O, r, x, op)
        assert R.fixture_mismatch(key, op, r, x, s, z) == "", op
        if op == "nv.gen":
            assert int(R.global_scale(O, r, x, op).view(torch.int32)) == manifest["cases"][key]["global_scales"][op]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_oracle_generate_gparam_matches_the_recorded_reference(manifest, dt):
    for shape in R.gparam_shapes():
        xs = R.weight(R.gparam_case(dt, shape)).reshape(-1, *shape)
        assert R.sha(xs) == manifest["gparam"][f"{dt}.{shape[0]}x{shape[1]}"]["input_sha256"]
        n_exp = len(R.exp16_bits(dt))
        last = xs.reshape(xs.shape[0], -1)[:, -1].view(torch.int16).to(torch.int64) & 0xFFFF
        assert torch.equal(last[:n_exp], R.exp16_bits(dt)) and last[n_exp:].tolist() == R.edge(dt)  # the extreme is the last element
        got = torch.cat([O.generate_gparam(t).reshape(1) for t in xs])
        assert R.gparam_mismatch(dt, shape, got) == ""
        assert 0 < manifest["gparam"][f"{dt}.{shape[0]}x{shape[1]}"]["ones"] < xs.shape[0] // 2  # non-finite -> 1 occurs, and is not the rule


def test_the_comparison_sees_one_bit_one_zero_point_and_the_sign_of_a_zero_but_no_nan_payload():
    key = "c16.g32.bf16"
    r = CASES[key]
    x = R.weight(r)
    s, z = R.oracle_output(O, r, x, "i4a")
    assert R.fixture_mismatch(key, "i4a", r, x, s, z) == ""
    flat = s.reshape(-1)
    nan = int(torch.isnan(flat).nonzero()[0])
    ordinary = int((torch.isfinite(flat.float()) & (flat.float() > 1)).nonzero()[0])
    for at, flip, seen in ((ordinary, 1, True), (ordinary, -32768, True), (nan, 1, False), (nan, -32768, False)):
        bad = s.clone()
        bad.view(torch.int16).reshape(-1)[at] ^= flip
        assert (R.fixture_mismatch(key, "i4a", r, x, bad, z) != "") is seen, (at, flip)
    bad = z.clone()
    bad.reshape(-1)[3] += 1
    assert R.fixture_mismatch(key, "i4a", r, x, s, bad) != ""
    # the sign of a zero scale: an MX scale is never zero, so take the masked zero of a group that holds a NaN — and a sha-only case
    for key in ("c16.g32.bf16", "s16.g32.bf16"):
        r = CASES[key]
        x = R.weight(r)
        s, _ = R.oracle_output(O, r, x, "mxfp4")
        assert R.fixture_mismatch(key, "mxfp4", r, x, s, None) == ""
        zero = R.masked(r, x, "mxfp4", s)
        assert int((zero == 0).sum()) == int(R.nan_groups(r, x).sum()) > 0
        neg = zero.clone()
        neg.view(torch.int16).reshape(-1)[int((zero.reshape(-1) == 0).nonzero()[0])] = -32768
        rec, want = R.record(r, "mxfp4", neg, None), R.load_fixture()[1]["cases"][key]["out"]["mxfp4"]
        assert rec["zeros"] == want["zeros"] and rec["sha256"] != want["sha256"]
        fin = int(torch.isfinite(s.reshape(-1).float()).nonzero()[0])
        bad = s.clone()
        bad.view(torch.int16).reshape(-1)[fin] ^= 1 << 7
        assert R.fixture_mismatch(key, "mxfp4", r, x, bad, None) != ""


@pytest.mark.parametrize("key", [k for k, r in CASES.items() if any(op in R.MASKED_OPS for op in r["ops"])])
def test_the_mask_covers_exactly_the_groups_that_hold_a_nan(manifest, key):
    """the MX scale of a group that holds a NaN is the one property not compared with the reference's record; the oracle gives +inf there (the
    project's pinned choice, compared with the kernel whole), and the mask touches nothing else"""
    r = CASES[key]
    x = R.weight(r)
    nang = R.nan_groups(r, x)
    E, P = R.planted(r)
    assert torch.equal(nang, (torch.isnan(E) | torch.isnan(P)).reshape(nang.shape))
    if R.is_sweep16(r):
        assert int(nang.sum()) == NAN_PATTERNS[r["dt"]]
    for op in r["ops"]:
        s, _ = R.oracle_output(O, r, x, op)
        m = R.masked(r, x, op, s)
        if op not in R.MASKED_OPS:
            assert m is s
            continue
        assert bool(torch.isposinf(s[nang]).all()) and bool((m[nang] == 0).all())
        assert torch.equal(R.canonical(m)[~nang], R.canonical(s)[~nang]) and not bool(torch.isnan(s).any())
        assert manifest["cases"][key]["out"][op]["zeros"] == int(nang.sum()) and manifest["cases"][key]["out"][op]["nans"] == 0


def test_generator_check_where_the_reference_is():
    """the committed fixture is what the reference produces, and the pinned oracle is the reference on every case (the generator imports it;
    skipped where its sources are not present)"""
    import ref_import

    if not ref_import.available():
        pytest.skip("upstream reference sources not present on this machine")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_observer_ranges.py"), "--check"], capture_output=True, text=True, env=env)
    assert done.returncode == 0 and "fixture matches" in done.stdout, done.stdout + done.stderr
