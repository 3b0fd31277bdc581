"""Host side of the fused rotation + dynamic QDQ (quantization/dynamic.py: plan_rotated_dynamic, the hand-off between the fused
pre-hook of transform.fuse_input_quantization and forward_quantize) and the fixtures of tools/gen_golden_rotated.py.  No GPU needed."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rotated_cases as C  # noqa: E402

import compressed_tensors_amd as cta  # noqa: E402
from compressed_tensors_amd import _lib, transform  # noqa: E402
from compressed_tensors_amd.quantization import QuantizationArgs, QuantizationScheme  # noqa: E402
from compressed_tensors_amd.quantization import dynamic  # noqa: E402
from compressed_tensors_amd.quantization.dynamic import plan_rotated_dynamic  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "rotated_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
FORMS = ("in_wave", "block", "block_row", "head_row")
TORCH_NAME = {"bf16": "bfloat16", "f16": "float16", "f32": "float32"}


@pytest.fixture(autouse=True)
def every_form_enabled(request, monkeypatch):
    """The dispatch rule and the hand-off are tested for every form the kernels compute.  Which of them the plan dispatches as
    shipped (dynamic.MEASURED_FASTER: the forms measured faster than the two launches) has the test_as_shipped_* tests."""
    if not request.node.name.startswith("test_as_shipped"):
        monkeypatch.setattr(dynamic, "MEASURED_FASTER", dynamic.ALL_FORMS)


def _args(preset):
    return QuantizationArgs(**C.PRESETS[preset])


def _plan(r):
    gs = C.D.global_scale_of(r["gs"]) if r["gs"] else None
    return plan_rotated_dynamic(tuple(r["shape"]), C.DTYPES[r["dtype"]], r["size"], _args(r["preset"]), gs)


# ---- the dispatch rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,shape,n,form,launches", [
    ("fp8_group128", (1, 8192, 8192), 128, "in_wave", 1), ("nvfp4", (2, 4, 64), 8, "in_wave", 1), ("mxfp4", (3, 64), 2, "in_wave", 1),
    ("fp8_token", (2, 4, 512), 512, "in_wave", 1), ("fp8_token", (2, 2, 4, 64), 64, "in_wave", 1),
    ("fp8_group128", (1, 9, 4096), 4096, "block", 1), ("nvfp4", (9, 8192), 8192, "block", 1), ("mxfp4", (3, 2, 2, 2048), 1024, "block", 1),
    ("fp8_token", (1, 9, 1024), 1024, "block_row", 1), ("int8_token_asym", (2, 3, 8192), 8192, "block_row", 1),
    ("fp8_token", (1, 9, 14336), 128, "head_row", 1), ("int8_token", (1, 9, 14336), 512, "head_row", 1), ("fp8_token", (1, 2, 32768), 256, "head_row", 1),
    ("fp8_token", (2, 4, 192), 64, "head_row", 1),
    ("fp8_token", (9, 4096), 128, None, 3),  # token on a 2-D input: one segment, the tensor form (two launches of its own)
    ("fp8_tensor", (1, 9, 1024), 64, None, 3),
    ("fp8_tensor", (2, 4, 16), 8, "in_wave", 1),  # one segment of <= 512 elements is an ordinary in-wave segment
    ("fp8_token", (2, 3, 16384), 16384, None, 2), ("fp8_group128", (9, 16384), 16384, None, 2),  # n = 16384: measured slower in one launch
    ("fp8_token", (1, 9, 4096), 1024, None, 2),  # 1024 <= n < L
    ("fp8_token", (1, 2, 65536), 128, None, 2),  # longer than the staged form
    ("fp8_token", (2, 4, 516), 4, None, 2),  # rows that are not whole 16-byte units
])
def test_plan_forms(preset, shape, n, form, launches):
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        gs = torch.tensor([37.5]) if preset == "nvfp4" else None
        plan = plan_rotated_dynamic(shape, dtype, n, _args(preset), gs)
        assert plan.fused == (form is not None) and plan.form == form, (plan.form, plan.reason)
        assert plan.launches() == launches
        assert (plan.reason is None) == plan.fused
        assert plan.hadamard.size == n and plan.dynamic.segs * plan.dynamic.seg_len == torch.Size(shape).numel()


@pytest.mark.parametrize("shape,dtype,n,preset,err", [
    ((2, 4, 96), torch.bfloat16, 24, "fp8_token", ValueError),  # not a power of two (upstream's message)
    ((2, 4, 96), torch.bfloat16, 64, "fp8_token", ValueError),  # does not divide the dimension
    ((2, 4, 64), torch.bfloat16, 0, "fp8_token", ValueError),
    ((2, 4, 64), torch.float64, 64, "fp8_token", NotImplementedError),
    ((1, 2, 32768), torch.bfloat16, 32768, "fp8_token", NotImplementedError),  # n > 16384: plan_hadamard declines
    ((2, 4, 192), torch.bfloat16, 64, "fp8_group128", NotImplementedError),  # plan_dynamic: columns are not whole groups
    ((2, 4, 0), torch.bfloat16, 8, "fp8_token", NotImplementedError),
])
def test_plan_errors_come_through(shape, dtype, n, preset, err):
    with pytest.raises(err):
        plan_rotated_dynamic(shape, dtype, n, _args(preset))


def test_plan_passes_the_strategy_error_through():
    with pytest.raises(ValueError):
        plan_rotated_dynamic((2, 4, 64), torch.bfloat16, 64, QuantizationArgs(num_bits=8, type="float", strategy="channel", dynamic=True))
    with pytest.raises(NotImplementedError):  # a global scale outside NVFP4
        plan_rotated_dynamic((2, 4, 64), torch.bfloat16, 64, _args("fp8_token"), torch.ones(1))


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_plan_of_every_case(key):
    entry = MANIFEST[key]
    plan = _plan(entry["recipe"])
    if key in C.DECLINED:
        assert not plan.fused and plan.launches() == C.DECLINED[key], plan.reason
    else:
        assert plan.fused and plan.form in FORMS and plan.launches() == 1, plan.reason
    assert list(plan.dynamic.scale_shape) == entry["scale"]["shape"] == entry["zp"]["shape"]
    assert str(plan.dynamic.scale_dtype).replace("torch.", "") == entry["scale"]["dtype"]
    assert str(plan.dynamic.zp_dtype).replace("torch.", "") == entry["zp"]["dtype"]
    assert entry["out"]["dtype"] == entry["rotated"]["dtype"] == TORCH_NAME[entry["recipe"]["dtype"]]
    assert entry["out"]["shape"] == entry["rotated"]["shape"] == entry["recipe"]["shape"]


def test_the_cases_cover_the_matrix():
    plans = {k: _plan(r) for k, r in C.case_list()}
    assert {p.form for p in plans.values() if p.fused} == set(FORMS)
    assert {k for k, p in plans.items() if not p.fused} == set(C.DECLINED) and len(C.DECLINED) >= 2
    recipes = [r for _, r in C.case_list()]
    for form in FORMS:  # every form in every dtype
        assert {r["dtype"] for (k, r) in C.case_list() if plans[k].form == form} == set(C.DTYPES), form
    assert {r["preset"] for r in recipes} >= {"fp8_token", "int8_token", "fp8_group128", "nvfp4", "mxfp4", "mxfp8", "int8_token_asym", "int4_group32_asym"}
    assert {r["gs"] for r in recipes if r["preset"] == "nvfp4"} >= {"nogs", "gs"}
    assert {len(r["shape"]) for r in recipes} >= {3, 4}
    assert {r["size"] for r in recipes} >= {8, 64, 128, 512, 1024, 4096, 8192}
    assert {r["size"] for r in recipes if r["preset"] == "mxfp4"} >= {8, 16, 32, 128, 1024, 4096}
    assert any(r["shape"] == [1, 9, 14336] and r["size"] == 128 for r in recipes) and any(r["shape"] == [1, 9, 14336] and r["size"] == 512 for r in recipes)


# ---- what is dispatched as shipped: only what tools/rotated_bench.py measured faster ---------------------------------------------------
def test_as_shipped_the_plan_follows_the_measurements(monkeypatch):
    shipped = dynamic.MEASURED_FASTER
    assert shipped <= dynamic.ALL_FORMS
    monkeypatch.setattr(dynamic, "MEASURED_FASTER", dynamic.ALL_FORMS)
    computable = {k: _plan(r) for k, r in C.case_list()}
    monkeypatch.setattr(dynamic, "MEASURED_FASTER", shipped)
    for key, recipe in C.case_list():
        plan, could = _plan(recipe), computable[key]
        want = could.fused and dynamic._measure_key(could.form, recipe["size"]) in shipped
        assert plan.fused == want and plan.launches() == (1 if want else 1 + plan.dynamic.launches())
        assert (plan.form == could.form) if want else (plan.form is None and plan.reason)


def test_as_shipped_every_dispatched_form_is_measured_faster():
    """MEASURED_FASTER holds only keys whose every row of profiles/rotated_bench.jsonl has the verdict "faster" """
    path = os.path.join(ROOT, "profiles", "rotated_bench.jsonl")
    if not dynamic.MEASURED_FASTER:
        return  # nothing is dispatched to the fused launch: nothing to justify
    with open(path) as f:
        verdicts = [v for v in map(json.loads, f) if "verdict" in v]
    for key in dynamic.MEASURED_FASTER:
        rows = [v for v in verdicts if v["key"] == key]
        assert rows and all(v["faster"] for v in rows), (key, rows)


# ---- the fixtures -----------------------------------------------------------------------------------------------------------------
def test_manifest_is_complete():
    cases = dict(C.case_list())
    assert set(MANIFEST) == set(cases)
    for key, recipe in cases.items():
        entry = MANIFEST[key]
        assert entry["recipe"] == recipe and entry["stored"] == C.stored(recipe)
        for name in ("rotated", "out", "scale", "zp"):
            assert set(entry[name]) == {"dtype", "shape", "sha256"}


def test_fixture_size_cap():
    total = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.startswith("rotated"))
    assert total <= C.MAX_FIXTURE_BYTES, total


def test_stored_tensors_match_their_hashes():
    from safetensors.torch import load_file

    g = load_file(os.path.join(GOLDEN, "rotated.safetensors"))
    want = {f"{k}.{n}" for k, e in MANIFEST.items() if e["stored"] for n in ("rotated", "out", "scale", "zp")}
    assert set(g) == want and want
    for name, t in g.items():
        key, part = name.rsplit(".", 1)
        assert C.sha(t) == MANIFEST[key][part]["sha256"], name
        assert list(t.shape) == MANIFEST[key][part]["shape"]


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_recipes_resynthesise_the_inputs(key):
    entry = MANIFEST[key]
    x = C.synth(entry["recipe"])
    assert C.sha(x) == entry["x_sha256"]
    rows = x.reshape(-1, x.shape[-1])
    if rows.shape[0] >= C.EDGE_ROWS:
        assert not rows[0].any() and int((rows[1] != 0).sum()) == 1
        assert torch.signbit(rows[2][0]) and rows[2][0] == 0
        nan_row = entry["recipe"]["nan_row"]  # false only for MX behind n < 32 (tests/_rotated_cases.py)
        assert nan_row == (not (entry["recipe"]["preset"].startswith("mx") and entry["recipe"]["size"] < 32))
        if entry["recipe"].get("finite"):  # the twins of the tensor-form cases: +128 and -128 where the others hold +inf and NaN
            assert bool(torch.isfinite(x).all()) and rows[3][x.shape[-1] // 2] == 128 and rows[4][-1] == -128
        else:
            assert int(torch.isinf(rows[3]).sum()) == 1
            assert int(torch.isnan(rows[4]).sum()) == int(nan_row) and int(torch.isinf(rows[4]).sum()) == int(not nan_row)
        assert bool((rows[5] == 3).all())


def test_finite_twins_of_the_tensor_form_cases():
    """the tensor-form cases with a +inf and a NaN row expect an all-NaN output; each has a finite twin that expects anything else"""
    twins = {k for k, e in MANIFEST.items() if e["recipe"].get("finite")}
    assert twins and all(_plan(MANIFEST[k]["recipe"]).dynamic.tensor_form for k in twins)
    for key, entry in MANIFEST.items():
        if not _plan(entry["recipe"]).dynamic.tensor_form:
            continue
        all_nan = {n: C.sha(torch.full(entry[n]["shape"], float("nan"), dtype=C.DTYPES[entry["recipe"]["dtype"]])) for n in ("out", "scale")}
        if key in twins:
            assert all(entry[n]["sha256"] != all_nan[n] for n in all_nan), key
        else:
            assert all(entry[n]["sha256"] == all_nan[n] for n in all_nan) and key + ".finite" in twins, key


def test_by_value_comparison():
    a = torch.tensor([0.0, -0.0, 1.0, float("nan")], dtype=torch.bfloat16)
    b = torch.tensor([-0.0, 0.0, 1.0, float("nan")], dtype=torch.bfloat16)
    b.view(torch.int16)[3] |= -0x8000  # another NaN
    assert C.equal_by_value(a, b) and C.sha(a) == C.sha(b)
    assert not C.equal_by_value(a, torch.tensor([0.0, 0.0, -1.0, float("nan")], dtype=torch.bfloat16))
    f8 = torch.tensor([0.0, -0.0, 2.0], dtype=torch.float32).to(torch.float8_e4m3fn)
    assert C.by_value(f8).tolist() == [0, 0, 0x40]


# ---- C ABI surface ----------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared():
    argtypes, restype = _lib._PROTOTYPES["ct_hadamard_dynamic_qdq"]
    assert len(argtypes) == 15 and restype is _lib._PROTOTYPES["ct_dynamic_qdq"][1]
    with open(os.path.join(ROOT, "include", "ct_hip.h")) as f:
        header = f.read()
    assert "int ct_hadamard_dynamic_qdq(const void* x, int xdt, int64_t numel, int64_t n, int64_t seg_len, int kind, int bits" in header
    assert callable(cta.codec.hadamard_dynamic_qdq) and callable(transform.fuse_input_quantization)


# ---- the hand-off between the fused pre-hook and forward_quantize, with the launches replaced by stand-ins ----------------------------
ONLINE = {"config_groups": {"v": {"type": "hadamard", "apply": [{"targets": ["Linear"], "location": "input", "inverse": False, "ignore": []}],
                                  "randomize": False, "requires_grad": False, "head_dim": 16, "precision": "torch.float32"}}}


class _Calls:
    def __init__(self, monkeypatch):
        self.rotate, self.fused, self.quantize = [], [], []
        monkeypatch.setattr(cta.codec, "hadamard_transform", lambda x, size, **kw: self.rotate.append(size) or x + 1)
        monkeypatch.setattr(dynamic, "rotated_fake_quantize", lambda x, size, args, gs=None, **kw: self.fused.append(size) or (x + 1) * 2)
        monkeypatch.setattr(dynamic, "dynamic_fake_quantize", lambda x, args, gs=None, **kw: self.quantize.append(1) or x * 2)

    def counts(self):
        return len(self.rotate), len(self.fused), len(self.quantize)


def _quantized_forward(module, x):
    """shaped like upstream's quantized_forward (quantization/lifecycle/forward.py:244-289) for the input side"""
    scheme = getattr(module, "quantization_scheme", None)
    if getattr(module, "quantization_enabled", True) and scheme is not None and getattr(module, "quantization_status", None) is not None \
            and scheme.input_activations is not None:
        x = dynamic.forward_quantize(module, x, "input", scheme.input_activations)
    return x


def _model(preset="fp8_token", fuse=True):
    m = torch.nn.Sequential(torch.nn.Linear(32, 8, bias=False), torch.nn.ReLU())
    cta.apply_transform_config(m, cta.TransformConfig.from_dict(ONLINE))
    lin = m[0]
    if preset is not None:
        lin.quantization_scheme = QuantizationScheme(targets=["Linear"], input_activations=_args(preset))
        lin.quantization_status = "frozen"
    lin.forward = lambda x: _quantized_forward(lin, x)
    names = transform.fuse_input_quantization(m) if fuse else None
    return m, lin, names


def test_handoff_identity_hit(monkeypatch):
    calls = _Calls(monkeypatch)
    m, lin, names = _model()
    assert names == ["0"]
    x = torch.ones(2, 3, 32, dtype=torch.bfloat16)
    out = lin(x)
    assert calls.counts() == (0, 1, 0) and calls.fused == [16]  # one fused call, no rotation of its own, no second QDQ
    assert torch.equal(out, (x + 1) * 2)
    assert dynamic._PREQUANTIZED not in lin.__dict__  # cleared after use


def test_without_the_opt_in_nothing_changes(monkeypatch):
    calls = _Calls(monkeypatch)
    m, lin, names = _model(fuse=False)
    out = lin(torch.ones(2, 3, 32, dtype=torch.bfloat16))
    assert calls.counts() == (1, 0, 1) and torch.equal(out, torch.full((2, 3, 32), 4.0, dtype=torch.bfloat16))


def test_handoff_identity_miss(monkeypatch):
    calls = _Calls(monkeypatch)
    m, lin, _ = _model()
    lin.register_forward_pre_hook(lambda _, inputs: inputs[0].clone())  # another hook replaces the input after ours
    out = lin(torch.ones(2, 3, 32, dtype=torch.bfloat16))
    assert calls.counts() == (0, 1, 1)  # any other tensor is quantized as always
    assert torch.equal(out, torch.full((2, 3, 32), 8.0, dtype=torch.bfloat16))
    assert dynamic._PREQUANTIZED not in lin.__dict__
    # and a call nobody pre-quantized
    v = torch.ones(2, 3, 32, dtype=torch.bfloat16)
    assert dynamic.forward_quantize(lin, v, "input", lin.quantization_scheme.input_activations) is not v
    assert calls.counts() == (0, 1, 2)


def test_handoff_is_for_the_input_only(monkeypatch):
    calls = _Calls(monkeypatch)
    _, lin, _ = _model()
    v = torch.ones(2, 3, 32, dtype=torch.bfloat16)
    dynamic.remember_prequantized(lin, v)
    assert not dynamic.take_prequantized(lin, v, "output") and dynamic._PREQUANTIZED in lin.__dict__
    assert dynamic.take_prequantized(lin, v, "input") and dynamic._PREQUANTIZED not in lin.__dict__
    dynamic.remember_prequantized(lin, v)
    assert dynamic.forward_quantize(lin, v, "input", lin.quantization_scheme.input_activations) is v
    assert calls.counts() == (0, 0, 0)


@pytest.mark.parametrize("how", ["disabled", "no_status", "no_scheme"])
def test_predicate_false_rotates_only(monkeypatch, how):
    calls = _Calls(monkeypatch)
    m, lin, names = _model()
    assert names == ["0"]
    if how == "disabled":
        lin.quantization_enabled = False
    elif how == "no_status":
        del lin.quantization_status
    else:
        del lin.quantization_scheme
    x = torch.ones(2, 3, 32, dtype=torch.bfloat16)
    assert torch.equal(lin(x), x + 1)  # rotated, nothing quantized
    assert calls.counts() == (1, 0, 0) and dynamic._PREQUANTIZED not in lin.__dict__


def test_a_plan_that_does_not_fuse_rotates_only(monkeypatch):
    calls = _Calls(monkeypatch)
    m, lin, names = _model()
    out = lin(torch.ones(3, 32, dtype=torch.bfloat16).repeat(32, 1))  # 2-D token input of 96 x 32: the tensor form
    assert calls.counts() == (1, 0, 1) and bool((out == 4).all())


def test_which_modules_qualify():
    assert _model(preset=None)[2] == []  # no scheme
    static = QuantizationArgs(num_bits=8, type="float", strategy="tensor", symmetric=True, dynamic=False)
    m, lin, _ = _model(preset=None, fuse=False)
    lin.quantization_scheme = QuantizationScheme(targets=["Linear"], input_activations=static)
    assert transform.fuse_input_quantization(m) == []
    lin.quantization_scheme = QuantizationScheme(targets=["Linear"], input_activations=_args("nvfp4"))
    assert transform.fuse_input_quantization(m) == ["0"]
    plain = torch.nn.Sequential(torch.nn.Linear(32, 8))  # no input transform
    plain[0].quantization_scheme = QuantizationScheme(targets=["Linear"], input_activations=_args("fp8_token"))
    assert transform.fuse_input_quantization(plain) == []
