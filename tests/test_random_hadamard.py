"""The host side of the random-hadamard rotation, without a GPU: the plan (shapes and dtypes only), the factoriser, the location
table, apply_transform_config's argument checks, the fixtures' own consistency, and the untouched ISA of the two objects the new
kernels share helpers with."""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _random_hadamard_cases as C  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "random_hadamard_manifest.json")) as _f:
    _M = json.load(_f)
MANIFEST, SIZES_IN_FIXTURE = _M["cases"], _M["sizes"]


@pytest.fixture(scope="module")
def golden_tensors():
    from safetensors.torch import load_file

    return load_file(os.path.join(GOLDEN, "random_hadamard.safetensors"))


def _weight(golden_tensors, n, dtype=torch.float32):
    return C.weight_from_factors(n, golden_tensors.get(f"had_k.{n}"), golden_tensors[f"signs.{n}"], dtype)


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------------
def test_the_case_matrix_is_the_one_the_fixtures_were_generated_from():
    cases = dict(C.case_list())
    assert sorted(cases) == sorted(MANIFEST)
    assert all(MANIFEST[k]["recipe"] == r for k, r in cases.items())
    assert {int(n): (e["k"], e["m"]) for n, e in SIZES_IN_FIXTURE.items()} == C.SIZES
    ks = {k for k, _ in C.SIZES.values()}
    assert {224, 160, 192} <= ks and {172, 148, 140} <= ks and {m for k, m in C.SIZES.values() if k > 1 and m >= 8} == {8, 16, 32, 64, 128}
    assert set(C.REAL) <= set(C.SIZES)
    for tier, dt, inv in ((t, d, i) for t in "AB" for d in C.DTYPES for i in (False, True)):
        for n in C.SIZES:
            assert any(r["tier"] == tier and r["dtype"] == dt and r["inverse"] == inv and r["size"] == n and r["location"] == "input" for r in cases.values())


def test_inputs_synthesise_to_the_recorded_digests():
    for key, entry in MANIFEST.items():
        if entry["recipe"]["size"] <= 5120:
            assert C.sha(C.synth(entry["recipe"])) == entry["x_sha256"], key


def test_the_stored_weights_are_their_factors(golden_tensors):
    for n in (40, 96):
        assert torch.equal(_weight(golden_tensors, n, torch.int8), golden_tensors[f"weight.{n}"])
    assert "weight.1376" not in golden_tensors and os.path.getsize(os.path.join(GOLDEN, "random_hadamard.safetensors")) < (1 << 20)


@pytest.mark.parametrize("key", sorted(k for k, e in MANIFEST.items() if e["stored"]))
def test_evaluation_from_the_factors_gives_the_stored_reference_outputs(key, golden_tensors):
    """`structured` (the restatement the GPU tests lean on for tier B and the graph test) against upstream's own stored outputs"""
    r = MANIFEST[key]["recipe"]
    n = r["size"]
    got = C.structured(C.synth(r), n, golden_tensors.get(f"had_k.{n}"), golden_tensors[f"signs.{n}"], C.transposed_of(r), C.dim_of(r), C.precision_of(r))
    assert torch.equal(got + 0.0, golden_tensors[f"{key}.out"] + 0.0)


@pytest.mark.parametrize("n", [40, 96])
@pytest.mark.parametrize("transposed", [False, True])
def test_structured_is_the_matrix_product(n, transposed, golden_tensors):
    w = golden_tensors[f"weight.{n}"].to(C.F64)
    x = C.synth(dict(gen="ints", dtype="f32", shape=[4, n], salt=n))
    want = (x.to(C.F64) @ (w.t() if transposed else w)) / torch.tensor(n, dtype=C.F64).sqrt()
    assert torch.equal(C.structured(x, n, golden_tensors[f"had_k.{n}"], golden_tensors[f"signs.{n}"], transposed, cast=False), want)


# ---- the factoriser ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(n for n in C.SIZES if n <= 5120))
def test_factoriser_round_trips_every_fixture_weight(n, golden_tensors):
    from compressed_tensors_amd.transform import factor_hadamard_weight

    w = _weight(golden_tensors, n, torch.float64 if n % 3 else torch.float32)
    f = factor_hadamard_weight(w)
    assert f is not None and (f.n, f.k, f.m) == (n, *C.SIZES[n])
    assert f.signs.dtype is torch.int8 and torch.equal(f.signs, golden_tensors[f"signs.{n}"])
    if C.SIZES[n][0] == 1:
        assert f.had_k is None  # Sylvester: dropped
    else:
        assert f.had_k.dtype is torch.int8 and torch.equal(f.had_k, golden_tensors[f"had_k.{n}"])
    assert torch.equal(C.weight_from_factors(n, f.had_k, f.signs, w.dtype), w)


@pytest.mark.parametrize("n", [96, 128, 1376, 1792])
def test_factoriser_returns_none_on_a_perturbed_weight(n, golden_tensors):
    from compressed_tensors_amd.transform import factor_hadamard_weight

    w = _weight(golden_tensors, n)
    for change in ("flip", "scale", "zero"):
        p = w.clone()
        p[n // 3, n // 2] = {"flip": -p[n // 3, n // 2], "scale": 0.5, "zero": 0.0}[change]
        assert factor_hadamard_weight(p) is None, change
    assert factor_hadamard_weight(w[:-1]) is None and factor_hadamard_weight(w[0]) is None
    assert factor_hadamard_weight(w / n ** 0.5) is None  # a normalised matrix is not the +-1 weight upstream keeps


def test_a_sylvester_weight_of_size_2_to_the_m_has_no_mix():
    from compressed_tensors_amd.transform import factor_hadamard_weight

    f = factor_hadamard_weight(C.sylvester(256, torch.float32))
    assert (f.k, f.m) == (1, 256) and f.had_k is None and bool((f.signs == 1).all())


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
def test_plan_forms():
    from compressed_tensors_amd.codec import plan_hadamard_k

    p = plan_hadamard_k((1, 8192, 14336), C.BF16, 14336, 224)
    assert (p.entry, p.form, p.k, p.m, p.blocks, p.acc64, p.workspace) == ("rows", "mfma", 224, 64, 8192, False, 0)
    for n, (k, m) in C.SIZES.items():
        want = "butterfly" if k == 1 else "mfma" if m >= 8 else "valu"
        for dt in (C.BF16, C.F16):
            assert plan_hadamard_k((3, n), dt, n, k).form == want, n
        assert plan_hadamard_k((3, n), C.F32, n, k).form == ("butterfly" if k == 1 else "valu")  # float32 activations
        assert plan_hadamard_k((3, n), C.BF16, n, k, precision=torch.float64).form == ("butterfly" if k == 1 else "valu")
    p = plan_hadamard_k((3, 14336), C.BF16, 14336, 224, precision=torch.float64)
    assert p.acc64 and p.workspace == 3 * 14336 * 8
    p = plan_hadamard_k((14336, 16), C.F16, 14336, 224, dim=0, precision=torch.float64)  # Linear weight_output: the weight's twin of the online size
    assert (p.entry, p.form, p.rows, p.cols, p.blocks) == ("cols", "valu", 14336, 16, 16) and p.workspace == 14336 * 16 * (2 + 8)
    assert plan_hadamard_k((1376, 1), C.BF16, 1376, 172, dim=0, precision=torch.float64).entry == "rows"  # a bias column
    assert plan_hadamard_k((2, 3, 2752), C.BF16, 1376, 172).blocks == 12  # head_dim blocks


def test_plan_raises_upstreams_errors_first_then_declines():
    from compressed_tensors_amd.codec import plan_hadamard_k

    for size, k in ((0, 1), (1376, 0), (1376, 171), (1376, 32), (96, 32)):  # 96 / 32 = 3 is not a power of two
        with pytest.raises(ValueError, match="Cannot construct random hadamard matrix of size"):
            plan_hadamard_k((2, 1376), C.F64, size, k, device_type="cpu")  # before any dtype / device complaint
    with pytest.raises(ValueError, match="must divide"):
        plan_hadamard_k((2, 1000), C.BF16, 1376, 172)
    with pytest.raises(IndexError):
        plan_hadamard_k((2, 1376), C.BF16, 1376, 172, dim=2)
    with pytest.raises(NotImplementedError, match="upstream would run its GEMM in that dtype"):
        plan_hadamard_k((2, 1376), C.BF16, 1376, 172, precision=C.BF16)
    with pytest.raises(NotImplementedError, match="bfloat16, float16 and float32"):
        plan_hadamard_k((2, 1376), C.F64, 1376, 172)
    with pytest.raises(NotImplementedError, match="GPU tensors"):
        plan_hadamard_k((2, 1376), C.BF16, 1376, 172, device_type="cpu")
    with pytest.raises(NotImplementedError, match="contiguous"):
        plan_hadamard_k((2, 1376), C.BF16, 1376, 172, contiguous=False)
    with pytest.raises(NotImplementedError, match="exceeds the supported maximum 32768"):
        plan_hadamard_k((1, 57344), C.BF16, 57344, 224)
    with pytest.raises(NotImplementedError, match="k <= 256"):
        plan_hadamard_k((1, 4160), C.BF16, 4160, 260)
    with pytest.raises(NotImplementedError, match="exceeds the supported maximum 16384"):
        plan_hadamard_k((1, 32768), C.BF16, 32768, 1)
    with pytest.raises(NotImplementedError, match="runs of up to 4096"):
        plan_hadamard_k((1, 32768), C.F32, 32768, 4)
    with pytest.raises(NotImplementedError, match="neither the first nor the last"):
        plan_hadamard_k((2, 1376, 3), C.BF16, 1376, 172, dim=1)
    # M = 128 with K close to 256: the staged row passes 64 KiB, the call goes to the vector form
    assert plan_hadamard_k((1, 32256), C.BF16, 32256, 252).form == "valu"


# ---- locations ---------------------------------------------------------------------------------------------------------------------------
def test_location_table():
    from compressed_tensors_amd.transform import transform_dim, transform_transposed

    L, E = torch.nn.Linear, torch.nn.Embedding
    table = {("input", L): (-1, False), ("output", L): (-1, False), ("weight_input", L): (-1, True), ("weight_output", L): (0, False),
             ("weight_input", E): (0, True), ("weight_output", E): (-1, False)}
    for (location, module), (dim, transposed) in table.items():
        assert transform_dim(location, module) == dim
        assert transform_transposed(location, module, False) == transposed and transform_transposed(location, module, True) == (not transposed)
    for key, entry in MANIFEST.items():
        r = entry["recipe"]
        module = getattr(torch.nn, r["module"])
        assert transform_dim(r["location"], module) == C.dim_of(r) and transform_transposed(r["location"], module, r["inverse"]) == C.transposed_of(r), key


def test_the_module_holds_factors_not_a_weight(golden_tensors):
    import compressed_tensors_amd as cta
    from compressed_tensors_amd.transform import HadamardFactors, HadamardTransform, RandomHadamardTransform

    n = 1376
    f = HadamardFactors(n, 172, 8, golden_tensors[f"had_k.{n}"], golden_tensors[f"signs.{n}"])
    t = RandomHadamardTransform(f, cta.TransformScheme("random-hadamard"), cta.TransformArgs(["x"], "weight_input", inverse=True), torch.nn.Linear)
    assert not isinstance(t, HadamardTransform)  # fuse_input_quantization looks for that class
    assert sum(b.numel() * b.element_size() for b in t.buffers()) == n + 172 * 172 and not list(t.parameters())
    assert (t.dim, t.transposed, t.precision) == (-1, False, torch.float64)
    with pytest.raises(NotImplementedError, match="GPU tensors"):
        t(torch.zeros(2, n, dtype=C.BF16))  # no quiet CPU path


# ---- apply_transform_config ----------------------------------------------------------------------------------------------------------------
def test_apply_checks_everything_before_it_draws_or_changes_anything():
    import compressed_tensors_amd as cta

    drawn = []

    def hadamard_weights(size, dtype, device, gen):
        drawn.append(size)
        return C.sylvester(size, dtype)

    m = C.model()
    before = C.sha(m[0].weight.data)
    with pytest.raises(NotImplementedError, match="type='random-hadamard' is not built here"):
        cta.apply_transform_config(m, C.MODEL_CONFIG)
    for field, value, match in (("randomize", True, "randomize=True"), ("requires_grad", True, "requires_grad=True"), ("type", "random-matrix", "random-matrix")):
        cfg = json.loads(json.dumps(C.MODEL_CONFIG))
        cfg["config_groups"]["w"][field] = value
        with pytest.raises(NotImplementedError, match=match):
            cta.apply_transform_config(m, cfg, hadamard_weights=hadamard_weights)
    cfg = json.loads(json.dumps(C.MODEL_CONFIG))
    cfg["config_groups"]["v"]["apply"][0]["location"] = "q_attn"
    with pytest.raises(NotImplementedError, match="q_attn"):
        cta.apply_transform_config(m, cfg, hadamard_weights=hadamard_weights)
    assert drawn == [] and C.sha(m[0].weight.data) == before and not hasattr(m, "transform_config")


def test_apply_rejects_a_weight_without_the_structure():
    import compressed_tensors_amd as cta

    m = C.model()
    with pytest.raises(ValueError, match="config group 'u': the weight of size 1376"):
        cta.apply_transform_config(m, C.MODEL_CONFIG, hadamard_weights=lambda size, dtype, device, gen: torch.ones(size, size, dtype=dtype))


def test_install_flag_needs_patch_transforms():
    import inspect

    import compressed_tensors_amd.install as ct_amd

    sig = inspect.signature(ct_amd.install)
    assert sig.parameters["patch_random_hadamard"].default is False
    try:
        import compressed_tensors  # noqa: F401
    except ImportError:
        return  # the argument check sits behind upstream's import
    with pytest.raises(ValueError, match="needs patch_transforms=True"):
        ct_amd.install(patch_random_hadamard=True)


# ---- the objects the new kernels share a header with ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("obj", ["ct_hadamard.o", "ct_rotated.o"])
def test_the_parent_objects_keep_their_isa(obj):
    """csrc/ct_hadamard_k.hip includes ct_hadamard.h and ct_hadamard.hip gained one host function for it: the gfx950 code of the
    existing kernels is, instruction for instruction, what it was before (tests/golden/random_hadamard_parent_isa.json holds the
    sha256 of the disassembly of the objects built without this file's feature)"""
    import __graft_entry__ as ge

    path = os.path.join(ge.BUILD, obj)
    if not os.path.exists(path) or not os.path.exists(ge.LLVM_OBJDUMP):
        pytest.skip("the build's object files or llvm-objdump are not on this machine")
    with open(os.path.join(GOLDEN, "random_hadamard_parent_isa.json")) as f:
        want = json.load(f)[obj]
    text = "\n".join(line for line in ge.disassemble_device_code(path).splitlines() if "file format" not in line)
    assert hashlib.sha256(text.encode()).hexdigest() == want
