"""The non-finite round-to-nearest fixture without a GPU: the case matrix of tests/_nonfinite_rtn_cases.py places what its recipes say and leaves
every other group alone; the pinned oracle's composition reproduces what the reference recorded (tests/golden/nonfinite_rtn.safetensors and
its manifest) outside the listed MX groups; that list holds MX kinds and NaN-holding groups only; and the codec's eligibility helpers send every
case down the kernel path it is named after, so that a moved threshold cannot silently move a case."""
import os
import subprocess
import sys

import pytest
import torch

import _nonfinite_rtn_cases as C
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = C.case_list()


@pytest.fixture(scope="module")
def fixture():
    return C.load_fixture()


def test_the_matrix_has_every_family_plant_and_dtype():
    cases = dict(CASES)
    assert len(cases) == len(CASES)  # the keys are unique
    assert {r["family"] for r in cases.values()} == {"pack", "channel8", "block8", "group8", "fp4"}
    for family in ("pack", "channel8", "block8", "group8", "fp4"):
        for dtype in ("bf16", "f16"):
            plants = {p["plant"] for r in cases.values() if r["family"] == family and r["dtype"] == dtype for p in r["plants"]}
            assert plants == set(C.PLANTS), (family, dtype, set(C.PLANTS) - plants)
    assert {k for r in cases.values() for k in C.kinds_of(r)} == set(C.PACK_KINDS) | set(C.KINDS8) | {"mxfp8", "mxfp4", "nvfp4"}
    assert {tuple(r["shape"]) for r in cases.values() if r["family"] == "pack"} >= {(1, 8224)} and cases["pack.e.bf16"]["plants"][0]["region"][2] == 8192
    assert max(r["shape"][1] for r in cases.values()) == 16384 + 4 * 256 * 8 + 8
    for dtype, pats in C.PATTERNS.items():  # the patterns are what they are called
        as_float = {n: torch.tensor([C._signed(b)], dtype=torch.int16).view(C.DTYPES[dtype]) for n, b in pats.items()}
        assert all(bool(torch.isnan(as_float[n])) for n in ("nan", "neg_nan", "nan_min", "nan_ones"))
        assert float(as_float["inf"]) == float("inf") and float(as_float["neg_inf"]) == -float("inf")
        assert pats["nan_min"] == pats["inf"] + 1 and pats["nan_ones"] == 0xFFFF and pats["neg_nan"] == pats["nan"] | 0x8000


@pytest.mark.parametrize("key,r", CASES, ids=[k for k, _ in CASES])
def test_make_weight_plus_plant_is_deterministic_and_places_what_the_recipe_says(fixture, key, r):
    base, x = C.make_weight(r), C.weight(r)
    raw, pats = x.view(torch.int16), C.PATTERNS[r["dtype"]]
    assert x.dtype == C.DTYPES[r["dtype"]] and list(x.shape) == r["shape"] and bool(torch.isfinite(base.float()).all())
    assert torch.equal(raw, C.weight(r).view(torch.int16)) and C.sha(x) == fixture[1]["cases"][key]["x_sha256"]
    mask = C.planted_mask(r)
    assert torch.equal(raw[~mask], base.view(torch.int16)[~mask]) and bool(torch.isfinite(x[~mask].float()).all())  # nothing else moved
    for p in r["plants"]:
        r0, r1, c0, c1 = p["region"]
        region, spots = raw[r0:r1, c0:c1], []
        for name, which in C.PLANTS[p["plant"]]:
            if which == "all":
                assert bool((region == C._signed(pats[name])).all()), (key, p)
                continue
            dr, dc = p["at"] if which == 0 else p["partner"]
            assert 0 <= dr < r1 - r0 and 0 <= dc < c1 - c0 and int(region[dr, dc]) == C._signed(pats[name]), (key, p, name)
            spots.append((dr, dc))
        if spots:  # a point plant: the rest of its region is the finite base
            rest = torch.ones(region.shape, dtype=torch.bool)
            for dr, dc in spots:
                rest[dr, dc] = False
            assert len(set(spots)) == len(spots) and bool(torch.isfinite(x[r0:r1, c0:c1][rest].float()).all()), (key, p)
        assert bool(torch.isnan(x[r0:r1, c0:c1].float()).any()) == (p["plant"] in C.HOLDS_NAN)
        # the neighbours: the regions of the same size to the left and right (and, for a block, above and below) hold no plant
        h, w = r1 - r0, c1 - c0
        bh = r["block"][0] if r["family"] == "block8" else 1
        for a0, a1, b0, b1 in ((r0, r1, c0 - w, c0), (r0, r1, c1, c1 + w), (r0 - bh, r0, c0, c1), (r1, r1 + bh, c0, c1)):
            if r["family"] != "block8" and (a0, a1) != (r0, r1):
                continue  # rows are independent of each other outside the block family
            if a0 >= 0 and b0 >= 0 and a1 <= x.shape[0] and b1 <= x.shape[1]:
                assert not bool(mask[a0:a1, b0:b1].any()), (key, p, (a0, a1, b0, b1))
    if r["family"] == "block8":
        assert not bool(C.planted_regions(r).all())  # a clean block
    elif x.shape[0] > 1 and r["plants"]:
        assert bool((~mask.any(dim=1)).any()) and len({p["region"][0] for p in r["plants"]}) == len(r["plants"])  # a clean row, one plant per row
    if r["family"] in ("pack", "group8", "fp4") and r["group"] and r["shape"][1] == 3 * r["group"]:
        assert all(p["region"][2:] == [r["group"], 2 * r["group"]] for p in r["plants"])  # the middle group of three
    flat = C.plant(base, r, value=0.25)
    assert bool(torch.isfinite(flat.float()).all()) and torch.equal(flat[~mask], base[~mask])
    assert all(float(flat[p["region"][0] + p["at"][0], p["region"][2] + p["at"][1]]) == 0.25 for p in r["plants"])


@pytest.mark.parametrize("key,r", CASES, ids=[k for k, _ in CASES])
def test_oracle_composition_reproduces_the_fixture_outside_the_listed_groups(fixture, key, r):
    x = C.weight(r)
    for kind in C.kinds_of(r):
        outs = C.oracle_outputs(O, x, r, kind)
        mask = C.fp4_sign_mask(O, x, r, kind) if r["family"] == "fp4" else None
        assert set(f"{kind}.{n}" for n in outs) == {n for n in fixture[1]["cases"][key]["out"] if n.split(".")[0] == kind}
        assert C.fixture_mismatches(fixture, key, kind, outs, mask) == [], (key, kind)


def test_the_fixture_holds_nothing_else_and_stays_small(fixture):
    tensors, manifest = fixture
    cases = dict(CASES)
    assert set(manifest["cases"]) == set(cases)
    want = {f"{key}.{name}" for key, e in manifest["cases"].items() for name, m in e["out"].items() if m["whole"]}
    assert set(tensors) == want
    for key, e in manifest["cases"].items():
        assert {n.split(".")[0] for n in e["out"]} == set(C.kinds_of(cases[key]))
        for name, m in e["out"].items():
            nbytes = int(torch.tensor(m["shape"]).prod()) * {"float32": 4, "int32": 4, "bfloat16": 2, "float16": 2}.get(m["dtype"], 1)
            assert m["whole"] == (nbytes <= C.WHOLE_MAX), (key, name)
    size = os.path.getsize(os.path.join(GOLDEN, "nonfinite_rtn.safetensors"))
    others = [os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.endswith("_rtn.safetensors") and f != "nonfinite_rtn.safetensors"]
    assert size < max(others) and size < (1 << 20) and os.path.getsize(os.path.join(GOLDEN, "nonfinite_rtn_manifest.json")) < (1 << 20)


def test_the_exception_list_holds_mx_kinds_and_nan_groups_only(fixture):
    """the cap: only MX kinds, only groups that hold a NaN — no group of infinities, no finite group, no INT, FP8 or NVFP4 case at all"""
    tensors, manifest = fixture
    cases = dict(CASES)
    listed = manifest["mx_exceptions"]
    assert len({tuple(e) for e in listed}) == len(listed)
    for key, kind, row, g in listed:
        r = cases[key]
        assert kind in C.MX_KINDS and kind in C.kinds_of(r), (key, kind)
        group = C.weight(r)[row, 32 * g:32 * g + 32]
        assert group.numel() == 32 and bool(torch.isnan(group).any()), (key, kind, row, g)
    # and a listed result is stored whole, or its groups could not be cut out of the comparison
    for key, kind in {(k, kd) for k, kd, _, _ in listed}:
        assert all(m["whole"] for n, m in manifest["cases"][key]["out"].items() if n.split(".")[0] == kind)


def test_the_references_answers_are_the_documented_ones(fixture):
    """the non-finite contract of DESIGN section 2, read off the fixture: NaN -> scale NaN and the code 0 (INT) or NaN codes (FP8); inf -> scale inf,
    the inf element the code 0 (INT) or the NaN code (FP8), the group's other elements the zero-point code; NVFP4's global scale 1 (NaN), 0 (+inf)"""
    tensors, manifest = fixture
    cases = dict(CASES)
    r = cases["group8.g32.bf16"]
    rows = {(p["plant"], tuple(p["at"])): i for i, p in enumerate(r["plants"])}
    nan_row, inf_row = rows[("nan", (0, 0))], rows[("inf", (0, 0))]
    s, z, q = (tensors[f"group8.g32.bf16.int8_zp.{n}"] for n in ("scale", "zero_point", "q"))
    assert bool(torch.isnan(s[nan_row, 1])) and int(z[nan_row, 1]) == 0 and not q[nan_row, 32:64].any()
    assert float(s[inf_row, 1]) == float("inf") and int(z[inf_row, 1]) == -128 and int(q[inf_row, 32]) == 0 and bool((q[inf_row, 33:64] == -128).all())
    s, q = tensors["group8.g32.bf16.fp8.scale"], tensors["group8.g32.bf16.fp8.q"]
    assert bool(torch.isnan(s[nan_row, 1])) and bool(torch.isnan(q[nan_row, 32:64].float()).all())
    assert float(s[inf_row, 1]) == float("inf") and bool(torch.isnan(q[inf_row, 32].float())) and not q[inf_row, 33:64].view(torch.uint8).any()
    for s in (tensors["group8.g32.bf16.int8.scale"], tensors["group8.g32.bf16.fp8.scale"]):  # the neighbours and the clean row are finite
        assert bool(torch.isfinite(s[:, 0].float()).all()) and bool(torch.isfinite(s[:, 2].float()).all()) and bool(torch.isfinite(s[-1].float()).all())
    for dtype in ("bf16", "f16"):
        assert float(tensors[f"fp4.last_nan.{dtype}.nvfp4.global_scale"]) == 1.0 and float(tensors[f"fp4.g32.{dtype}.nvfp4.global_scale"]) == 1.0
        assert float(tensors[f"fp4.last_inf.{dtype}.nvfp4.global_scale"]) == 0.0  # 448 * 6 / inf is finite: nan_to_num has nothing to replace
        assert float(tensors[f"fp4.last_nan_gs.{dtype}.nvfp4.global_scale"]) == C.EXPLICIT_GLOBAL_SCALE
        assert 1.0 < float(tensors[f"fp4.clean.{dtype}.nvfp4.global_scale"]) < float("inf")


def test_every_case_takes_the_kernel_path_it_is_named_after():
    from compressed_tensors_amd import codec

    for key, r in CASES:
        shape, family, form = r["shape"], r["family"], r["form"]
        if family == "pack":
            lanes = {"a": 1, "b": 4, "c": 64, "d": 8, "e": 1}[form]
            assert codec.rtn_w4_group(shape, r["group"]) == 32 * lanes, key
            assert form != "e" or (shape[0] * shape[1] // 32 == 257 and r["plants"][0]["region"][2] // 32 == 256)  # the one live lane of workgroup 2
        elif family == "group8":
            assert codec.rtn_group8_group(shape, r["group"]) == r["group"] and r["group"] // 16 == {"g32": 2, "g128": 8, "g1024": 64}[form], key
        elif family == "block8":
            bh, bw = r["block"]
            assert codec.rtn_block8_group(shape, r["block"]) == -((bh << 24) | bw) and shape[1] % bw == 0, key
            assert (shape[0] % bh != 0) == form.startswith("b128x128"), key  # the ragged last row of blocks
        elif family == "channel8":
            want = {"wave": ("wave", "wave"), "sym_wave_last": ("wave", "wave"), "sym_row_first": ("row", "wave"), "asym_wave_last": ("row", "wave"),
                    "asym_row_first": ("row", "row"), "row": ("row", "row"), "long1": ("long", "long"), "long2": ("long", "long")}[form]
            assert (codec.rtn_channel8_form(shape, True), codec.rtn_channel8_form(shape, False)) == want, key
            one_less = [shape[0], shape[1] - 8]
            if form == "sym_row_first":
                assert codec.rtn_channel8_form(one_less, True) == "wave"
            if form == "asym_row_first":
                assert codec.rtn_channel8_form(one_less, False) == "wave"
            if form == "long1":
                assert codec.rtn_channel8_form(one_less, True) == codec.rtn_channel8_form(one_less, False) == "row"
            if form == "long2":  # the streamed part: one whole trip of 4 x 256 units and one unit of a second trip
                assert shape[1] // 8 - 2048 == 4 * 256 + 1
        else:
            assert shape[1] % 32 == 0 and r["group"] == 32, key


def test_generator_check_mode_matches_the_reference():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_import

    if not ref_import.available():
        pytest.skip("the reference sources are not on this machine")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_nonfinite_rtn.py"), "--check"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
