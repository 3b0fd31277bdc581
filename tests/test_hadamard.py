"""The Hadamard rotation without a GPU: the fixtures re-synthesise, the butterfly arithmetic the kernels implement equals the
reference's stored outputs, the host-side plan, the transform configuration surface and apply_transform_config's plumbing."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hadamard_cases as C  # noqa: E402
import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "hadamard_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
with open(os.path.join(GOLDEN, "hadamard_transform_config.json")) as _f:
    UPSTREAM_DUMP = json.load(_f)


def _golden_tensors():
    from safetensors.torch import load_file

    return load_file(os.path.join(GOLDEN, "hadamard.safetensors"))


def test_manifest_covers_the_case_matrix():
    cases = dict(C.case_list())
    assert sorted(cases) == sorted(MANIFEST)
    assert all(MANIFEST[k]["recipe"] == cases[k] for k in cases)
    for tier, location in (("A", "input"), ("C", "weight_input"), ("C", "weight_output")):
        assert any(r["tier"] == tier and r["location"] == location for r in cases.values())
    for n in C.SIZES:  # every power of two 2 ... 8192 in every dtype, exact and bounded
        for dt in C.DTYPES:
            assert any(r["tier"] == "A" and r["size"] == n and r["dtype"] == dt for r in cases.values()), (n, dt)
            assert any(r["tier"] == "B" and r["size"] == n and r["dtype"] == dt for r in cases.values()), (n, dt)
    assert sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.startswith("hadamard")) < 512 * 1024


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_recipes_resynthesise_their_inputs(key):
    entry = MANIFEST[key]
    assert C.sha(C.synth(entry["recipe"])) == entry["x_sha256"]


def test_sha_compares_by_value():
    a = torch.tensor([0.0, -0.0, 1.5, -2.0], dtype=torch.bfloat16)
    b = torch.tensor([-0.0, 0.0, 1.5, -2.0], dtype=torch.bfloat16)
    assert torch.equal(a, b) and C.sha(a) == C.sha(b)
    assert C.sha(a) != C.sha(torch.tensor([0.0, 0.0, 1.5, 2.0], dtype=torch.bfloat16))


def test_butterfly_restatement_equals_every_stored_reference_output():
    """pins the arithmetic on the CPU, independent of the kernels: float32 (online) / float64 (offline) butterfly in any bit
    order, ONE division by sqrt(n), one cast — equal to upstream's GEMM result in every element of tiers A and C"""
    g = _golden_tensors()
    seen = 0
    for key, entry in MANIFEST.items():
        if not entry["stored"]:
            continue
        r = entry["recipe"]
        got = C.butterfly(C.synth(r), r["size"], C.dim_of(r), C.precision_of(r))
        ref = g[f"{key}.out"]
        assert got.dtype == ref.dtype and torch.equal(got, ref), key
        assert C.sha(got) == entry["out"]["sha256"], key
        seen += 1
    assert seen >= 40


def test_reciprocal_instead_of_division_is_not_the_reference():
    """why the kernels divide: x * (1 / sqrt(n)) differs from the stored reference where n is not a power of 4"""
    g = _golden_tensors()
    differs = 0
    for key, entry in MANIFEST.items():
        r = entry["recipe"]
        if entry["stored"] and r["tier"] == "A" and r["dtype"] == "f32" and r["size"] in (2, 8, 32, 128):
            x = C.synth(r)
            s = torch.tensor(r["size"], dtype=torch.float64).sqrt().to(torch.float32)
            differs += int(not torch.equal(C.butterfly(x, r["size"]) * s * (1.0 / s), g[f"{key}.out"]))
    assert differs > 0


# ---- plan_hadamard -------------------------------------------------------------------------------------------------------------
def test_plan_forms_blocks_and_accumulators():
    from compressed_tensors_amd.codec import plan_hadamard

    p = plan_hadamard((1, 8192, 4096), torch.bfloat16, 4096)  # online
    assert (p.form, p.size, p.blocks, p.acc64) == ("rows", 4096, 8192, False)
    p = plan_hadamard((65, 8192), torch.float16, 128)  # head_dim blocks
    assert (p.form, p.size, p.blocks, p.acc64) == ("rows", 128, 65 * 64, False)
    p = plan_hadamard((4096, 1024), torch.bfloat16, 1024, -1, torch.float64)  # Linear weight_input
    assert (p.form, p.blocks, p.acc64) == ("rows", 4096, True)
    p = plan_hadamard((4096, 1024), torch.bfloat16, 4096, 0, torch.float64)  # Linear weight_output
    assert (p.form, p.size, p.blocks, p.acc64, p.rows, p.cols) == ("cols", 4096, 1024, True, 4096, 1024)
    p = plan_hadamard((4096, 1024), torch.bfloat16, 128, 0, torch.float64)  # ... with head_dim
    assert (p.form, p.size, p.blocks) == ("cols", 128, 32 * 1024)
    p = plan_hadamard((4096, 1), torch.bfloat16, 128, 0, torch.float64)  # bias.unsqueeze(-1): contiguous along dim 0
    assert (p.form, p.size, p.blocks, p.acc64) == ("rows", 128, 32, True)
    p = plan_hadamard((4096,), torch.float32, 4096, 0)
    assert (p.form, p.blocks) == ("rows", 1)
    assert plan_hadamard((3, 16384), torch.bfloat16, 16384).form == "rows"
    assert plan_hadamard((3, 16384), torch.bfloat16, 16384, precision=torch.float64).form == "rows"


def test_plan_raises_upstreams_value_errors():
    from compressed_tensors_amd.codec import plan_hadamard

    with pytest.raises(ValueError, match="Cannot construct deterministic hadamard of size <= 0"):
        plan_hadamard((4, 8), torch.bfloat16, 0)
    with pytest.raises(ValueError, match="Cannot construct deterministic hadamard of size <= 0"):
        plan_hadamard((4, 8), torch.bfloat16, -4)
    with pytest.raises(ValueError, match=r"Cannot construct deterministic hadamard of size != 2\^n"):
        plan_hadamard((4, 12), torch.bfloat16, 12)
    with pytest.raises(ValueError, match="64 must divide 96"):
        plan_hadamard((4, 96), torch.bfloat16, 64)
    with pytest.raises(ValueError, match="64 must divide 100"):
        plan_hadamard((100, 64), torch.bfloat16, 64, 0, torch.float64)


@pytest.mark.parametrize("kwargs", [
    dict(shape=(4, 64), dtype=torch.bfloat16, size=64, precision=torch.bfloat16),
    dict(shape=(4, 64), dtype=torch.float16, size=64, precision=torch.float16),
    dict(shape=(4, 64), dtype=torch.float64, size=64),
    dict(shape=(4, 64), dtype=torch.int8, size=64),
    dict(shape=(4, 64), dtype=torch.bfloat16, size=64, device_type="cpu"),
    dict(shape=(4, 64), dtype=torch.bfloat16, size=64, device_type="meta"),
    dict(shape=(4, 64), dtype=torch.bfloat16, size=64, contiguous=False),
    dict(shape=(2, 32768), dtype=torch.bfloat16, size=32768),
    dict(shape=(2, 32768), dtype=torch.bfloat16, size=32768, precision=torch.float64),
    dict(shape=(2, 64, 8), dtype=torch.bfloat16, size=64, dim=1),  # neither the first nor the last dimension
])
def test_plan_declines(kwargs):
    from compressed_tensors_amd.codec import plan_hadamard

    with pytest.raises(NotImplementedError):
        plan_hadamard(**kwargs)


# ---- the configuration surface ---------------------------------------------------------------------------------------------------
def test_config_round_trip_and_defaults():
    import compressed_tensors_amd as cta

    args = cta.TransformArgs(targets="Linear", location="input", ignore="lm_head")
    assert args.targets == ["Linear"] and args.ignore == ["lm_head"] and args.inverse is False and args.is_online()
    assert not cta.TransformArgs(targets=["x"], location=cta.TransformLocation.WEIGHT_OUTPUT).is_online()
    assert cta.TransformLocation("k_cache").is_online() and not cta.TransformLocation("weight_input").is_online()
    scheme = cta.TransformScheme(type="hadamard", apply=[args], head_dim=64, precision=torch.float64)
    assert (scheme.randomize, scheme.requires_grad) == (False, False)
    assert cta.TransformScheme(type="hadamard").precision is torch.float32 and cta.TransformScheme(type="hadamard").apply == []
    cfg = cta.TransformConfig(config_groups={"r1": scheme, "r2": cta.TransformScheme(type="hadamard")})
    d = cfg.to_dict()
    assert d["config_groups"]["r1"]["precision"] == "torch.float64" and d == cfg.model_dump()
    assert json.loads(json.dumps(d)) == d  # plain JSON
    assert cta.TransformConfig.from_dict(d) == cfg and cta.TransformConfig.from_dict(d).to_dict() == d
    with pytest.raises(ValueError):
        cta.TransformArgs.from_dict({"targets": ["a"], "location": "input", "bogus": 1})
    with pytest.raises(ValueError):
        cta.TransformArgs(targets=["a"], location="nowhere")


def test_from_dict_of_upstreams_own_dump():
    import compressed_tensors_amd as cta

    cfg = cta.TransformConfig.from_dict(UPSTREAM_DUMP)
    assert cfg.to_dict() == UPSTREAM_DUMP
    assert cfg == cta.TransformConfig.from_dict(C.MODEL_CONFIG)
    v = cfg.config_groups["v"]
    assert v.head_dim == 64 and v.precision is torch.float32 and [a.location for a in v.apply] == ["input", "weight_input"] and v.apply[1].inverse


@pytest.mark.skipif(not ref_import.available(), reason="upstream reference sources not present on this machine")
def test_upstreams_pydantic_objects_are_accepted():
    ref_import.import_reference()
    try:
        from compressed_tensors.transform import TransformConfig as UpConfig
    except ImportError as e:
        pytest.skip(f"upstream's transform package does not import here: {e}")
    import compressed_tensors_amd as cta

    up = UpConfig.model_validate(C.MODEL_CONFIG)
    assert cta.TransformConfig.coerce(up).to_dict() == up.model_dump() == UPSTREAM_DUMP


# ---- apply_transform_config ------------------------------------------------------------------------------------------------------
def _meta_model():
    with torch.device("meta"):
        return torch.nn.Sequential(torch.nn.Linear(64, 128, dtype=torch.bfloat16), torch.nn.Linear(128, 32, bias=False, dtype=torch.bfloat16))


def test_apply_on_a_meta_model_registers_hooks_without_touching_data():
    import compressed_tensors_amd as cta

    m = _meta_model()
    cfg = cta.TransformConfig({"r": cta.TransformScheme("hadamard", [cta.TransformArgs("re:1", "input"), cta.TransformArgs("Linear", "output", ignore="1")],
                                                      head_dim=32)})
    cta.apply_transform_config(m, cfg)
    assert m.transform_config is cfg
    t_in, t_out = m[1].r_input, m[0].r_output
    assert isinstance(t_in, cta.HadamardTransform) and (t_in.size, t_in.dim, t_in.precision) == (32, -1, torch.float32)
    assert isinstance(t_out, cta.HadamardTransform) and t_out.size == 32
    assert not hasattr(m[1], "r_output") and not hasattr(m[0], "r_input")  # targets / ignore
    assert len(m[1]._forward_pre_hooks) == 1 and len(m[0]._forward_hooks) == 1 and not m[0]._forward_pre_hooks
    assert not list(t_in.parameters()) and not list(t_in.buffers())  # no n x n weight
    assert all(p.is_meta for p in m.parameters())


def test_get_transform_size_and_dims():
    from compressed_tensors_amd.transform import get_transform_size, transform_dim

    lin, emb = torch.nn.Linear(64, 128, device="meta"), torch.nn.Embedding(512, 64, device="meta")
    assert [get_transform_size(lin, loc) for loc in ("input", "weight_input", "weight_output", "output")] == [64, 64, 128, 128]
    assert [get_transform_size(emb, loc) for loc in ("weight_input", "weight_output")] == [512, 64]
    assert get_transform_size(lin, "weight_output", 32) == 32 and get_transform_size(torch.nn.ReLU(), "output", 16) == 16
    with pytest.raises(ValueError, match="48 must divide 128"):
        get_transform_size(lin, "weight_output", 48)
    with pytest.raises(NotImplementedError):
        get_transform_size(torch.nn.ReLU(), "output")
    assert [transform_dim(loc, torch.nn.Linear) for loc in ("input", "output", "weight_input", "weight_output")] == [-1, -1, -1, 0]
    assert [transform_dim(loc, torch.nn.Embedding) for loc in ("weight_input", "weight_output")] == [0, -1]
    for r in dict(C.case_list()).values():  # the cases module restates the same mapping
        assert transform_dim(r["location"], getattr(torch.nn, r["module"])) == C.dim_of(r)


@pytest.mark.parametrize("scheme_kwargs,field", [
    (dict(type="random-hadamard"), "type"), (dict(type="matrix-multiply"), "type"), (dict(type="hadamard", randomize=True), "randomize"),
    (dict(type="hadamard", requires_grad=True), "requires_grad"),
])
def test_apply_rejects_unsupported_scheme_fields(scheme_kwargs, field):
    import compressed_tensors_amd as cta

    m = _meta_model()
    cfg = cta.TransformConfig({"ok": cta.TransformScheme("hadamard", [cta.TransformArgs("Linear", "input")]),
                               "bad": cta.TransformScheme(apply=[cta.TransformArgs("Linear", "input")], **scheme_kwargs)})
    with pytest.raises(NotImplementedError, match=field):
        cta.apply_transform_config(m, cfg)
    assert not hasattr(m, "transform_config") and not m[0]._forward_pre_hooks  # checked before anything is changed


@pytest.mark.parametrize("location", ["q_attn", "k_cache"])
def test_apply_rejects_attention_locations(location):
    import compressed_tensors_amd as cta

    cfg = cta.TransformConfig({"r": cta.TransformScheme("hadamard", [cta.TransformArgs("Linear", location)])})
    with pytest.raises(NotImplementedError, match="location"):
        cta.apply_transform_config(_meta_model(), cfg)


def test_there_is_no_cpu_fallback():
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import codec

    x = torch.ones(4, 64, dtype=torch.bfloat16)
    # without a GPU: the package's usual RuntimeError; with one, a CPU tensor is declined (install() hands it to the reference)
    expect = (NotImplementedError, "GPU tensors") if torch.cuda.is_available() else (RuntimeError, "no CPU fallback")
    with pytest.raises(expect[0], match=expect[1]):
        codec.hadamard_transform(x, 64)
    m = torch.nn.Sequential(torch.nn.Linear(64, 64, dtype=torch.bfloat16))
    cfg = cta.TransformConfig({"r": cta.TransformScheme("hadamard", [cta.TransformArgs("Linear", "weight_input")])})
    with pytest.raises(expect[0], match=expect[1]):
        cta.apply_transform_config(m, cfg)
    with pytest.raises(ValueError, match="must divide"):  # upstream's errors come first, GPU or not
        codec.hadamard_transform(x, 128)


def test_model_compressor_writes_upstreams_transform_config(tmp_path):
    import compressed_tensors_amd as cta

    m = _meta_model()
    online_only = {"config_groups": {"v": dict(C.MODEL_CONFIG["config_groups"]["v"], apply=C.MODEL_CONFIG["config_groups"]["v"]["apply"][:1])}}
    cta.apply_transform_config(m, cta.TransformConfig.from_dict(online_only))  # a meta model: only the hook is registered
    m.transform_config = cta.TransformConfig.from_dict(C.MODEL_CONFIG)  # the full config of the fixture, as a GPU run attaches it
    cta.ModelCompressor.from_pretrained_model(m).update_config(str(tmp_path))
    with open(tmp_path / "config.json") as f:
        written = json.load(f)
    assert written["quantization_config"]["transform_config"] == UPSTREAM_DUMP


def test_model_compressor_carries_the_attached_config(tmp_path):
    import compressed_tensors_amd as cta

    m = _meta_model()
    cfg = cta.TransformConfig({"r": cta.TransformScheme("hadamard", [cta.TransformArgs("Linear", "input")], head_dim=32)})
    cta.apply_transform_config(m, cfg)
    comp = cta.ModelCompressor.from_pretrained_model(m)
    assert comp.transform_config is cfg
    comp.update_config(str(tmp_path))
    with open(tmp_path / "config.json") as f:
        assert json.load(f)["quantization_config"]["transform_config"] == cfg.to_dict()


# ---- install(patch_transforms=True) against the live reference ------------------------------------------------------------------
@pytest.mark.skipif(not ref_import.available(), reason="upstream reference sources not present on this machine")
def test_patch_transforms_tags_only_the_sylvester_factory_and_uninstall_restores():
    ref_import.import_reference()
    try:
        import compressed_tensors.transform.factory.hadamard as up_h
        from compressed_tensors.transform import TransformArgs, TransformFactory, TransformScheme
    except ImportError as e:
        pytest.skip(f"upstream's transform package does not import here: {e}")
    import compressed_tensors_amd.install as ct_amd

    orig_create, orig_forward = up_h.HadamardFactory.create_transform, up_h.HadamardTransform.forward
    lin = torch.nn.Linear(64, 64, dtype=torch.bfloat16)
    args = TransformArgs(targets=["Linear"], location="input")
    ct_amd.install(patch_transforms=True)
    try:
        ct_amd.install(patch_transforms=True)  # idempotent
        assert up_h.HadamardFactory.create_transform is not orig_create and up_h.HadamardTransform.forward is not orig_forward
        plain = TransformFactory.from_scheme(TransformScheme(type="hadamard"), name="a").create_transform(lin, args)
        assert getattr(plain, "_ct_sylvester", False) is True
        permuted = TransformFactory.from_scheme(TransformScheme(type="hadamard", randomize=True), name="b", seed=0).create_transform(lin, args)
        assert permuted.perm is not None  # tagged or not, a permutation keeps it upstream's
        if os.path.exists(os.path.join(os.path.dirname(up_h.__file__), "..", "utils", "hadamards.safetensors")):
            rnd = TransformFactory.from_scheme(TransformScheme(type="random-hadamard"), name="c", seed=0).create_transform(lin, args)
            assert type(rnd) is up_h.HadamardTransform and not getattr(rnd, "_ct_sylvester", False)
        # a CPU value runs the original: upstream's own result
        x = C.synth(dict(gen="ints", dtype="bf16", shape=[3, 64], salt=5))
        assert torch.equal(plain(x), orig_forward(plain, x)) and torch.equal(plain(x), C.butterfly(x, 64))
    finally:
        ct_amd.uninstall()
    assert up_h.HadamardFactory.create_transform is orig_create and up_h.HadamardTransform.forward is orig_forward
