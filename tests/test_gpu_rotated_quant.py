"""The fused rotation + dynamic QDQ launch (csrc/ct_rotated.hip) on the MI355X: against the reference's outputs on every fixture
case (tests/golden/rotated*, tools/gen_golden_rotated.py), launch counts, bit-identity with the two existing launches it replaces,
scales only, no host synchronisation, graph capture, and modules under transform.fuse_input_quantization."""
import collections
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hadamard_cases as H  # noqa: E402
import _rotated_cases as C  # noqa: E402
import ref_import  # noqa: E402

D = C.D
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "rotated_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
DEV = torch.device("cuda:0")
PARTS = ("rotated", "out", "scale", "zp")


def _args(preset):
    from compressed_tensors_amd.quantization import QuantizationArgs

    return QuantizationArgs(**C.PRESETS[preset])


def _gs(preset, name="gs"):
    return D.global_scale_of(name).to(DEV) if preset == "nvfp4" and name and name != "nogs" else None


@pytest.fixture(autouse=True)
def every_form_enabled(request, monkeypatch):
    """The kernels are tested in every form they compute.  Which forms the plan dispatches as shipped (dynamic.MEASURED_FASTER:
    those measured faster than the two launches) is test_as_shipped_dispatch_follows_the_measurements."""
    from compressed_tensors_amd.quantization import dynamic

    if not request.node.name.startswith("test_as_shipped"):
        monkeypatch.setattr(dynamic, "MEASURED_FASTER", dynamic.ALL_FORMS)


@pytest.fixture()
def counted():
    from compressed_tensors_amd import _lib

    counts = collections.Counter()
    orig = _lib.call

    def call(name, *a):
        counts[name] += 1
        return orig(name, *a)

    _lib.call = call
    import compressed_tensors_amd.codec as codec_mod

    saved = codec_mod.call
    codec_mod.call = call
    try:
        yield counts
    finally:
        _lib.call = orig
        codec_mod.call = saved


@pytest.fixture(scope="module")
def golden_tensors():
    from safetensors.torch import load_file

    return load_file(os.path.join(GOLDEN, "rotated.safetensors"))


# ---- 1. every fixture case against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_matches_the_reference(key, counted, golden_tensors):
    from compressed_tensors_amd.quantization.dynamic import plan_rotated_dynamic, rotated_fake_quantize

    entry = MANIFEST[key]
    r = entry["recipe"]
    x = C.synth(r)
    assert C.sha(x) == entry["x_sha256"], "the recipe no longer synthesises the reference's input"
    gs = _gs(r["preset"], r["gs"])
    args = _args(r["preset"])
    plan = plan_rotated_dynamic(x.shape, x.dtype, r["size"], args, gs)
    out, scale, zp, rotated = rotated_fake_quantize(x.to(DEV), r["size"], args, gs, return_qparams=True, return_rotated=True)
    torch.cuda.synchronize()
    got = dict(rotated=rotated, out=out, scale=scale, zp=zp)
    for name in PARTS:
        t = got[name]
        assert str(t.dtype).replace("torch.", "") == entry[name]["dtype"], (name, t.dtype)
        assert list(t.shape) == entry[name]["shape"], (name, t.shape)
        if entry["stored"]:
            ref = golden_tensors[f"{key}.{name}"]
            bad = (C.by_value(t).view(torch.uint8) != C.by_value(ref).view(torch.uint8)).nonzero()
            assert bad.numel() == 0, f"{name} differs from the stored reference, first at byte {bad[0].tolist()}"
        assert C.sha(t) == entry[name]["sha256"], f"{name} differs from the reference"
    if plan.fused:
        assert dict(counted) == {"ct_hadamard_dynamic_qdq": 1}, counted
    else:
        assert sum(counted.values()) == 2 and counted["ct_hadamard_rows"] == 1, counted


@pytest.mark.parametrize("key", ["fp8_group128.bf16.2x4x256.n128", "fp8_token.bf16.1x9x14336.n128", "fp8_token.bf16.1x8x1024.n1024",
                                 "nvfp4.bf16.1x8x1024.n1024.nogs", "fp8_token.bf16.1x9x4096.n1024"])
def test_as_shipped_dispatch_follows_the_measurements(key, counted):
    """as shipped: one call for a form in MEASURED_FASTER, the two existing calls for every other — the reference's results either way"""
    from compressed_tensors_amd.quantization import dynamic

    entry = MANIFEST[key]
    r = entry["recipe"]
    args = _args(r["preset"])
    plan = dynamic.plan_rotated_dynamic(r["shape"], C.DTYPES[r["dtype"]], r["size"], args, None)
    assert plan.fused == (plan.form is not None and dynamic._measure_key(plan.form, r["size"]) in dynamic.MEASURED_FASTER)
    out, scale, zp, rotated = dynamic.rotated_fake_quantize(C.synth(r).to(DEV), r["size"], args, None, return_qparams=True, return_rotated=True)
    torch.cuda.synchronize()
    for name, t in (("rotated", rotated), ("out", out), ("scale", scale), ("zp", zp)):
        assert C.sha(t) == entry[name]["sha256"], name
    assert dict(counted) == ({"ct_hadamard_dynamic_qdq": 1} if plan.fused else {"ct_hadamard_rows": 1, "ct_dynamic_qdq": 1}), counted


# ---- 2. kernel launches, counted by the profiler -------------------------------------------------------------------------------------
def _launches_of(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and any(s in e.name for s in ("rot_", "had_", "dyn_"))]


@pytest.mark.parametrize("preset,shape,n,form,expect", [
    ("fp8_group128", (1, 32, 4096), 128, "in_wave", 1), ("nvfp4", (1, 32, 4096), 64, "in_wave", 1), ("fp8_token", (2, 16, 512), 512, "in_wave", 1),
    ("mxfp4", (1, 32, 4096), 4096, "block", 1), ("fp8_group128", (1, 8, 8192), 8192, "block", 1),
    ("fp8_group128", (1, 8, 16384), 16384, None, 2), ("fp8_token", (1, 8, 16384), 16384, None, 2),  # measured slower in one launch: declined
    ("fp8_token", (2, 16, 4096), 4096, "block_row", 1), ("int8_token", (1, 16, 1024), 1024, "block_row", 1),
    ("fp8_token", (1, 16, 14336), 128, "head_row", 1), ("int8_token", (1, 16, 14336), 512, "head_row", 1),
    ("fp8_token", (1, 16, 4096), 1024, None, 2), ("fp8_token", (64, 4096), 128, None, 3), ("fp8_tensor", (1, 64, 4096), 4096, None, 3),
])
def test_launch_counts(preset, shape, n, form, expect, counted):
    from compressed_tensors_amd.quantization.dynamic import plan_rotated_dynamic, rotated_fake_quantize

    x = torch.randn(shape, dtype=D.BF16, device=DEV)
    gs = _gs(preset)
    plan = plan_rotated_dynamic(shape, D.BF16, n, _args(preset), gs)
    assert plan.form == form and plan.launches() == expect
    kernels = _launches_of(lambda: rotated_fake_quantize(x, n, _args(preset), gs))
    assert len(kernels) == expect, kernels
    if form is not None:
        assert "rot_" in kernels[0] and set(counted) == {"ct_hadamard_dynamic_qdq"}


# ---- 3. fused == the two launches it replaces, bit for bit ---------------------------------------------------------------------------
GROUP_KINDS = ["fp8_group128", "nvfp4", "nvfp4_nogs", "mxfp4", "mxfp8", "int4_group32_asym"]
TOKEN_KINDS = ["fp8_token", "int8_token", "int8_token_asym", "int4_token_asym"]
IDENTITY_SHAPES = [
    # (form, shape, n, kinds)
    ("in_wave", (3, 5, 256), 64, GROUP_KINDS + TOKEN_KINDS),  # 480 units: does not fill a workgroup
    ("in_wave", (1, 7, 128), 2, GROUP_KINDS + TOKEN_KINDS),  # n < 8: the butterfly stays inside a unit
    ("in_wave", (2, 9, 512), 512, GROUP_KINDS + TOKEN_KINDS),
    ("in_wave", (2, 33, 256), 32, GROUP_KINDS),  # n between the group sizes
    ("block", (1, 3, 1024), 1024, GROUP_KINDS),
    ("block", (2, 3, 4096), 2048, GROUP_KINDS),
    ("block", (1, 5, 8192), 8192, GROUP_KINDS),
    ("block_row", (1, 3, 1024), 1024, TOKEN_KINDS),
    ("block_row", (3, 1, 2048), 2048, TOKEN_KINDS),
    ("block_row", (1, 5, 4096), 4096, TOKEN_KINDS),
    ("block_row", (1, 3, 8192), 8192, TOKEN_KINDS),
    ("head_row", (1, 5, 1536), 128, TOKEN_KINDS),
    ("head_row", (1, 3, 14336), 512, TOKEN_KINDS),
    ("head_row", (2, 2, 11008), 64, TOKEN_KINDS),
    ("head_row", (1, 2, 32768), 8, TOKEN_KINDS),
    ("head_row", (2, 3, 192), 64, TOKEN_KINDS),
]


def _identity_params():
    for form, shape, n, kinds in IDENTITY_SHAPES:
        for kind in kinds:
            for dt in D.DTYPES:
                yield pytest.param(form, shape, n, kind, dt, id=f"{form}-{'x'.join(map(str, shape))}-n{n}-{kind}-{dt}")


def _inputs(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    for s in (0.02, 1.0, 30.0):
        yield f"randn*{s}", (torch.randn(shape, generator=g, dtype=torch.float32) * s).to(dtype)
    yield "synth", D.synth(tuple(shape), dtype, seed % 13)  # every magnitude class, +-0, subnormals, +-inf, NaN


def _both(x, n, preset, gs, want_fused=True):
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.quantization.dynamic import dynamic_fake_quantize, plan_rotated_dynamic, rotated_fake_quantize

    args = _args(preset)
    assert plan_rotated_dynamic(x.shape, x.dtype, n, args, gs).fused == want_fused
    fused = rotated_fake_quantize(x, n, args, gs, return_qparams=True, return_rotated=True)
    rot = codec.hadamard_transform(x, n)
    comp = dynamic_fake_quantize(rot, args, gs, return_qparams=True) + (rot,)
    torch.cuda.synchronize()
    return fused, comp


def _assert_same_bits(fused, comp, what):
    for name, a, b in zip(("out", "scale", "zp", "rotated"), fused, comp):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        assert D.canonical_bytes(a) == D.canonical_bytes(b), f"{what}: {name} differs from the two-launch composition"


@pytest.mark.parametrize("form,shape,n,kind,dt", list(_identity_params()))
def test_fused_equals_the_composition(form, shape, n, kind, dt):
    from compressed_tensors_amd.quantization.dynamic import plan_rotated_dynamic

    preset = "nvfp4" if kind == "nvfp4_nogs" else kind
    gs = _gs(preset) if kind != "nvfp4_nogs" else None
    assert plan_rotated_dynamic(shape, D.DTYPES[dt], n, _args(preset), gs).form == form
    for what, x in _inputs(shape, D.DTYPES[dt], seed=n + len(kind)):
        fused, comp = _both(x.to(DEV), n, preset, gs)
        _assert_same_bits(fused, comp, what)


@pytest.mark.parametrize("preset,n", [("fp8_group128", 128), ("nvfp4", 128), ("fp8_token", 128), ("int8_token", 512), ("fp8_token", 8192), ("mxfp4", 8192)])
def test_fused_equals_the_composition_on_a_large_activation(preset, n):
    x = torch.randn((1, 2048, 8192), generator=torch.Generator().manual_seed(n), dtype=torch.float32).to(D.BF16).to(DEV)
    fused, comp = _both(x, n, preset, _gs(preset))
    _assert_same_bits(fused, comp, "randn")


def test_a_declined_shape_is_the_composition():
    x = torch.randn((1, 9, 4096), generator=torch.Generator().manual_seed(1), dtype=torch.float32).to(D.BF16).to(DEV)
    fused, comp = _both(x, 1024, "fp8_token", None, want_fused=False)
    _assert_same_bits(fused, comp, "randn")


def test_the_library_declines_what_the_plan_declines():
    from compressed_tensors_amd import codec

    kw = dict(kind="fp8", num_bits=8, symmetric=True, scale_shape=(1,), scale_dtype=None, zp_dtype=None)
    for shape, n, L in (((9, 4096), 128, 9 * 4096), ((1, 9, 4096), 1024, 4096), ((1, 2, 65536), 128, 65536), ((2, 4, 516), 4, 516),
                        ((1, 2, 16384), 16384, 16384), ((1, 2, 16384), 16384, 128)):
        with pytest.raises(NotImplementedError):
            codec.hadamard_dynamic_qdq(torch.zeros(shape, dtype=D.BF16, device=DEV), n, seg_len=L, **kw)
    with pytest.raises(NotImplementedError):  # 16-byte alignment, as hadamard_transform
        codec.hadamard_dynamic_qdq(torch.zeros(8 * 64 + 8, dtype=D.BF16, device=DEV)[4:-4].reshape(8, 64), 64, seg_len=64, **kw)
    torch.cuda.synchronize()


# ---- 4. scales only ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,shape,n", [("fp8_group128", (2, 9, 512), 64), ("nvfp4", (1, 3, 4096), 4096), ("int8_token_asym", (1, 5, 2048), 2048),
                                            ("fp8_token", (1, 5, 1536), 128)])
def test_scales_only(preset, shape, n):
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.quantization.dynamic import plan_rotated_dynamic

    x = D.synth(shape, D.BF16, 5).to(DEV)
    gs = _gs(preset)
    dp = plan_rotated_dynamic(shape, D.BF16, n, _args(preset), gs).dynamic
    kw = dict(kind=dp.kind, seg_len=dp.seg_len, num_bits=dp.num_bits, symmetric=dp.symmetric, global_scale=gs, scale_shape=dp.scale_shape,
              scale_dtype=dp.scale_dtype, zp_dtype=dp.zp_dtype)
    out, scale, zp, rotated = codec.hadamard_dynamic_qdq(x, n, want_out=False, **kw)
    out2, scale2, zp2, rotated2 = codec.hadamard_dynamic_qdq(x, n, want_out=True, want_rotated=True, **kw)
    torch.cuda.synchronize()
    assert out is None and rotated is None and out2 is not None
    assert D.canonical_bytes(scale) == D.canonical_bytes(scale2) and D.canonical_bytes(zp) == D.canonical_bytes(zp2)
    assert D.canonical_bytes(rotated2) == D.canonical_bytes(codec.hadamard_transform(x, n))


# ---- 5. no host synchronisation, graph capture ---------------------------------------------------------------------------------------
CAPTURED = [("fp8_group128", (2, 16, 4096), 128), ("nvfp4", (1, 8, 4096), 4096), ("fp8_token", (2, 8, 4096), 4096), ("int8_token", (1, 16, 14336), 128)]


def test_no_host_synchronisation():
    from compressed_tensors_amd.quantization.dynamic import rotated_fake_quantize

    for preset, shape, n in CAPTURED:
        x = torch.randn(shape, dtype=D.BF16, device=DEV)
        args, gs = _args(preset), _gs(preset)
        rotated_fake_quantize(x, n, args, gs)  # warm: the first call loads the library
        torch.cuda.set_sync_debug_mode("error")
        try:
            rotated_fake_quantize(x, n, args, gs, return_qparams=True, return_rotated=True)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_the_entry_is_graph_capturable():
    """the entry allocates nothing and never synchronises: captured once, replayed on changing inputs"""
    from compressed_tensors_amd import _lib, codec
    from compressed_tensors_amd.quantization.dynamic import dynamic_fake_quantize, plan_rotated_dynamic

    lib = _lib.load()
    jobs = []
    for preset, shape, n in CAPTURED:
        gs = _gs(preset)
        dp = plan_rotated_dynamic(shape, D.BF16, n, _args(preset), gs).dynamic
        x = torch.zeros(shape, dtype=D.BF16, device=DEV)
        jobs.append(dict(preset=preset, n=n, gs=gs, dp=dp, x=x, out=torch.empty_like(x), rot=torch.empty_like(x),
                         scale=torch.empty(dp.scale_shape, dtype=dp.scale_dtype, device=DEV), zp=torch.empty(dp.scale_shape, dtype=dp.zp_dtype, device=DEV)))

    def launches(stream):
        for j in jobs:
            dp = j["dp"]
            rc = lib.ct_hadamard_dynamic_qdq(j["x"].data_ptr(), _lib.BF16, j["x"].numel(), j["n"], dp.seg_len, codec.DYNAMIC_KINDS[dp.kind], dp.num_bits,
                                            int(dp.symmetric), None if j["gs"] is None else j["gs"].data_ptr(), j["rot"].data_ptr(), j["out"].data_ptr(),
                                            j["scale"].data_ptr(), j["zp"].data_ptr(), codec.DT[dp.zp_dtype], stream)
            assert rc == 0, (rc, _lib.last_error())

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        launches(_lib.stream_on(DEV, side.cuda_stream))  # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches(_lib.stream_on(DEV, torch.cuda.current_stream(DEV).cuda_stream))
    for rep in range(3):
        for j in jobs:
            j["x"].copy_(D.synth(tuple(j["x"].shape), D.BF16, rep + 1).to(DEV))
            for name in ("out", "rot"):
                j[name].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for j in jobs:
            rot = codec.hadamard_transform(j["x"], j["n"])
            eager = dynamic_fake_quantize(rot, _args(j["preset"]), j["gs"], return_qparams=True) + (rot,)
            _assert_same_bits((j["out"], j["scale"], j["zp"], j["rot"]), eager, f"replay {rep} of {j['preset']}")


# ---- 6. modules ----------------------------------------------------------------------------------------------------------------------
def _quantized_forward(module, x):
    """shaped like upstream's quantized_forward (quantization/lifecycle/forward.py:244-289), the input side"""
    from compressed_tensors_amd.quantization.dynamic import forward_quantize

    scheme = getattr(module, "quantization_scheme", None)
    if getattr(module, "quantization_enabled", True) and scheme is not None and getattr(module, "quantization_status", None) is not None \
            and scheme.input_activations is not None:
        x = forward_quantize(module, x, "input", scheme.input_activations)
    return torch.nn.functional.linear(x, module.weight, module.bias)


def _model(preset, fuse):
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import transform
    from compressed_tensors_amd.quantization import QuantizationScheme

    m = H.model().to(DEV)
    cta.apply_transform_config(m, cta.TransformConfig.from_dict(H.MODEL_CONFIG))
    lin = m[1]  # the input rotation (head_dim 64) sits on the second Linear
    if preset is not None:
        lin.quantization_scheme = QuantizationScheme(targets=["Linear"], input_activations=_args(preset))
        lin.quantization_status = "frozen"
        if preset == "nvfp4":
            lin.input_global_scale = torch.tensor([37.5], device=DEV)
    lin.forward = lambda x: _quantized_forward(lin, x)
    names = transform.fuse_input_quantization(m) if fuse else []
    return m, names


@pytest.mark.parametrize("preset", ["fp8_token", "int8_token", "nvfp4", "mxfp4", "int8_token_asym"])
def test_modules_under_fuse_input_quantization(preset):
    x = torch.randn(2, 8, 64, generator=torch.Generator().manual_seed(3), dtype=torch.float32).to(D.BF16).to(DEV)
    plain, none = _model(preset, fuse=False)
    fused, names = _model(preset, fuse=True)
    assert none == [] and names == ["1"]
    want, got = plain(x), fused(x)
    assert want.dtype == got.dtype and torch.equal(want.view(torch.int16), got.view(torch.int16))
    assert [k.split("_kernel")[0].split("::")[-1].split(" ")[-1] for k in _launches_of(lambda: plain(x))] == ["had_group", "dyn_group"]
    one = _launches_of(lambda: fused(x))
    assert len(one) == 1 and "rot_group_kernel" in one[0], one
    # a 2-D input of the same module: token on 2-D is the tensor form, which the plan declines — the hook rotates only (the
    # group kinds do not look at the token dimension and fuse as before)
    x2 = x.reshape(16, 64)
    assert torch.equal(plain(x2).view(torch.int16), fused(x2).view(torch.int16))
    assert len(_launches_of(lambda: fused(x2))) == (len(_launches_of(lambda: plain(x2))) if "token" in preset else 1)
    # quantization_enabled = False: nothing is quantized, the rotation stays
    bare, _ = _model(None, fuse=False)
    fused[1].quantization_enabled = False
    assert torch.equal(fused(x).view(torch.int16), bare(x).view(torch.int16))
    assert [("had_" in k) for k in _launches_of(lambda: fused(x))] == [True]


@pytest.mark.skipif(not ref_import.available(), reason="no reference on this machine")
@pytest.mark.parametrize("preset", ["fp8_token", "nvfp4"])
def test_modules_under_upstreams_quantized_forward(preset):
    """upstream's own set_forward_quantized under install(patch_forward=True): its forward_quantize reaches the wrapper, which
    consults the hand-off before anything else"""
    ref_import.import_reference()
    from compressed_tensors.quantization import QuantizationArgs as UpArgs
    from compressed_tensors.quantization import QuantizationScheme as UpScheme
    from compressed_tensors.quantization import QuantizationStatus
    from compressed_tensors.quantization.lifecycle.forward import set_forward_quantized

    import compressed_tensors_amd as cta
    import compressed_tensors_amd.install as ct_amd
    from compressed_tensors_amd import _lib, transform

    def build(fuse):
        m = H.model().to(DEV)
        cta.apply_transform_config(m, cta.TransformConfig.from_dict(H.MODEL_CONFIG))
        lin = m[1]
        lin.quantization_scheme = UpScheme(targets=["Linear"], input_activations=UpArgs(**C.PRESETS[preset]))
        lin.quantization_status = QuantizationStatus.FROZEN
        if preset == "nvfp4":
            lin.register_buffer("input_global_scale", torch.tensor([37.5], device=DEV))
        set_forward_quantized(lin)
        return m, (transform.fuse_input_quantization(m) if fuse else [])

    x = torch.randn(2, 8, 64, generator=torch.Generator().manual_seed(4), dtype=torch.float32).to(D.BF16).to(DEV)
    counts = collections.Counter()
    lib = _lib.load()
    saved = {n: getattr(lib, n) for n in ("ct_dynamic_qdq", "ct_dynamic_qdq_tensor", "ct_hadamard_rows", "ct_hadamard_dynamic_qdq")}
    for n in saved:
        def counting(*a, _o=saved[n], _n=n):
            counts[_n] += 1
            return _o(*a)
        setattr(lib, n, counting)
    ct_amd.install(patch_forward=True)
    try:
        plain, _ = build(False)
        fused, names = build(True)
        counts.clear()  # apply_transform_config rotated the weights
        want = plain(x)
        two = dict(counts)
        counts.clear()
        got = fused(x)
        one = dict(counts)
    finally:
        ct_amd.uninstall()
        for n, f in saved.items():
            setattr(lib, n, f)
    assert names == ["1"]
    assert two == {"ct_hadamard_rows": 1, "ct_dynamic_qdq": 1} and one == {"ct_hadamard_dynamic_qdq": 1}, (two, one)
    assert torch.equal(want.view(torch.int16), got.view(torch.int16))
