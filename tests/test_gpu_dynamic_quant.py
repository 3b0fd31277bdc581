"""The fused dynamic activation QDQ (csrc/ct_dynamic.hip) on the MI355X: against the reference's outputs on every fixture case
(tests/golden/dynamic*, tools/gen_golden_dynamic.py) — the QDQ, the scales-only entry, and the same inputs at a base address
that is not 16-byte aligned — launch counts, no host synchronisation, an exhaustive bf16 / fp16 sweep against an eager
restatement, and quantized Linear modules under install(patch_forward=True)."""
import collections
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dynamic_cases as C  # noqa: E402
import ref_import  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "dynamic_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
DEV = torch.device("cuda:0")
TORCH_DT = {"bfloat16": C.BF16, "float16": C.F16, "float32": C.F32, "int8": torch.int8, "uint8": torch.uint8, "float8_e4m3fn": C.F8}


def _args(preset):
    from compressed_tensors_amd.quantization import QuantizationArgs

    return QuantizationArgs(**C.PRESETS[preset])


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


_GOLDEN, _BIG_INPUTS = {}, {}


def _golden_tensors():
    from safetensors.torch import load_file

    if not _GOLDEN:
        _GOLDEN.update(load_file(os.path.join(GOLDEN, "dynamic.safetensors")))
    return _GOLDEN


def _input(key):
    """the recipe's input; the few inputs of millions of elements are synthesised once for the tests that share them"""
    r = MANIFEST[key]["recipe"]
    if torch.Size(r["shape"]).numel() < 1 << 20:
        return C.make_input(r)
    if key not in _BIG_INPUTS:
        _BIG_INPUTS[key] = C.make_input(r)
    return _BIG_INPUTS[key]


def _assert_matches(key, got):
    """every tensor of `got` (name -> result) has the dtype, the shape and the values of the reference's: by sha256, and byte for
    byte where the fixture keeps the tensor"""
    entry = MANIFEST[key]
    for name, t in got.items():
        assert str(t.dtype).replace("torch.", "") == entry[name]["dtype"], (name, t.dtype)
        assert list(t.shape) == entry[name]["shape"], (name, t.shape)
        assert C.sha(t) == entry[name]["sha256"], f"{name} differs from the reference"
        if entry["stored"]:
            ref = _golden_tensors()[f"{key}.{name}"]
            assert C.canonical_bytes(t.view(torch.uint8) if t.dtype == C.F8 else t) == C.canonical_bytes(ref), f"{name} differs from the stored reference"


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_dynamic_qdq_matches_the_reference(key, counted):
    from compressed_tensors_amd.quantization.dynamic import dynamic_fake_quantize

    entry = MANIFEST[key]
    r = entry["recipe"]
    x = _input(key)
    assert C.sha(x) == entry["x_sha256"], "the recipe no longer synthesises the reference's input"
    gs = C.global_scale_of(r["gs"]) if r["gs"] else None
    out, scale, zp = dynamic_fake_quantize(x.to(DEV), _args(r["preset"]), gs.to(DEV) if gs is not None else None, return_qparams=True)
    torch.cuda.synchronize()
    for name, t in (("out", out), ("scale", scale), ("zp", zp)):
        assert str(t.dtype).replace("torch.", "") == entry[name]["dtype"], (name, t.dtype)
        assert list(t.shape) == entry[name]["shape"], (name, t.shape)
        assert C.sha(t) == entry[name]["sha256"], f"{name} differs from the reference"
    if entry["stored"]:
        g = _golden_tensors()
        for name, t in (("out", out), ("scale", scale), ("zp", zp)):
            ref = g[f"{key}.{name}"]
            if t.dtype == C.F8:
                t = t.view(torch.uint8)
            assert C.canonical_bytes(t) == C.canonical_bytes(ref), f"{name} differs from the stored reference"
    assert sum(counted.values()) == 1, counted  # one C-ABI entry per call (the tensor form launches twice inside it)


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_scales_only_entry_matches_the_reference(key, counted):
    """compute_dynamic_scales_and_zp (out == nullptr in every kernel): the reference's scale and zero point, and nothing else launched"""
    from compressed_tensors_amd.quantization.dynamic import compute_dynamic_scales_and_zp

    r = MANIFEST[key]["recipe"]
    gs = C.global_scale_of(r["gs"]) if r["gs"] else None
    scale, zp = compute_dynamic_scales_and_zp(_input(key).to(DEV), _args(r["preset"]), global_scale=gs.to(DEV) if gs is not None else None)
    torch.cuda.synchronize()
    _assert_matches(key, dict(scale=scale, zp=zp))
    assert sum(counted.values()) == 1, counted


# a contiguous input one element into its buffer: no 16-byte alignment, so every load and store takes its scalar form, and groups
# (with and without the NVFP4 global scale) go to the one-workgroup-per-segment kernel; the tensor form and the twice-read rows too
MISALIGNED = [
    "fp8_group128.bf16.2x4x256", "nvfp4.bf16.2x4x256.gs", "nvfp4.bf16.2x4x256.nogs", "mxfp4.bf16.2x4x256", "fp8_token.bf16.2x4x256",
    "int8_token_asym.bf16.2x4x256", "int4_group32_asym.bf16.2x2x4x128", "nvfp4.f32.2x4x256.gs", "fp8_group128.f16.1x9x4096",
    "fp8_tensor.bf16.8x256.finite", "int8_tensor_asym.f32.33x1001.finite.first", "int8_token_asym.f16.1x3x32776.finite",
]


@pytest.mark.parametrize("key", MISALIGNED)
def test_misaligned_contiguous_input(key, counted, monkeypatch):
    from compressed_tensors_amd.quantization.dynamic import compute_dynamic_scales_and_zp, dynamic_fake_quantize

    entry = MANIFEST[key]
    r = entry["recipe"]
    x = _input(key)
    pad = 16 // x.element_size()
    buf = torch.full((x.numel() + 2 * pad,), 3.0, dtype=x.dtype, device=DEV)  # a fresh allocation: 16-byte aligned
    view = buf[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    before = buf.clone()
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 != 0 and view.is_contiguous()
    gs = C.global_scale_of(r["gs"]) if r["gs"] else None  # "nogs" is None too
    gs = gs.to(DEV) if gs is not None else None
    # the output the codec allocates for this input sits one element into a buffer of its own, so a store outside it shows
    out_buf = torch.full_like(buf, 3.0)
    empty_like, handed = torch.empty_like, []

    def guarded_empty_like(t, *a, **kw):
        if t is not view:
            return empty_like(t, *a, **kw)
        handed.append(out_buf[1:1 + x.numel()].view(x.shape))
        return handed[-1]

    monkeypatch.setattr(torch, "empty_like", guarded_empty_like)
    out, scale, zp = dynamic_fake_quantize(view, _args(r["preset"]), gs, return_qparams=True)
    monkeypatch.undo()
    only_scale, only_zp = compute_dynamic_scales_and_zp(view, _args(r["preset"]), global_scale=gs)
    torch.cuda.synchronize()
    assert len(handed) == 1 and out.data_ptr() == handed[0].data_ptr() and out.data_ptr() % 16 != 0
    _assert_matches(key, dict(out=out, scale=scale, zp=zp))
    _assert_matches(key, dict(scale=only_scale, zp=only_zp))
    assert sum(counted.values()) == 2, counted
    assert torch.equal(buf.view(torch.uint8), before.view(torch.uint8)), "the input's buffer was written to"
    assert bool((out_buf[:1] == 3).all()) and bool((out_buf[1 + x.numel():] == 3).all()), "a store outside the output"


def _launches_of(fn):
    """kernel launches of one call, counted by the profiler (the tensor form is one entry that launches twice)"""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "dyn_" in e.name]


@pytest.mark.parametrize("preset,shape,expect", [
    ("fp8_token", (2, 64, 4096), 1), ("int8_token", (1, 16, 14336), 1), ("fp8_group128", (1, 32, 4096), 1),
    ("nvfp4", (1, 32, 4096), 1), ("mxfp4", (1, 32, 4096), 1), ("fp8_tensor", (1, 64, 4096), 2), ("fp8_token", (64, 4096), 2),
])
def test_launch_counts(preset, shape, expect, counted):
    from compressed_tensors_amd.quantization.dynamic import dynamic_fake_quantize

    x = torch.randn(shape, dtype=C.BF16, device=DEV)
    gs = torch.tensor([37.5], device=DEV) if preset == "nvfp4" else None
    dynamic_fake_quantize(x, _args(preset), gs)
    assert sum(counted.values()) == 1
    kernels = _launches_of(lambda: dynamic_fake_quantize(x, _args(preset), gs))
    assert len(kernels) == expect, kernels


def test_no_host_synchronisation():
    from compressed_tensors_amd.quantization.dynamic import compute_dynamic_scales_and_zp, dynamic_fake_quantize

    x = torch.randn(2, 16, 4096, dtype=C.BF16, device=DEV)
    gs = torch.tensor([37.5], device=DEV)
    for preset in ("fp8_token", "nvfp4", "mxfp4", "fp8_tensor"):
        args = _args(preset)
        g = gs if preset == "nvfp4" else None
        dynamic_fake_quantize(x, args, g)  # warm: the first call loads the library
        torch.cuda.set_sync_debug_mode("error")
        try:
            dynamic_fake_quantize(x, args, g)
            compute_dynamic_scales_and_zp(x, args, global_scale=g)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


# ---- exhaustive sweep: every bf16 / fp16 bit pattern as one element of a row with fixed companions -----------------------------
def _eager(x, args, gs):
    """the reference's arithmetic restated in eager torch (helpers.py:50-195, forward_helpers.py:180-215), on the same device"""
    from compressed_tensors_amd.quantization.dynamic import plan_dynamic

    plan = plan_dynamic(x.shape, x.dtype, args, gs)
    st = args.strategy.value
    v = x.unflatten(-1, (-1, args.group_size)) if st in ("group", "tensor_group") else x
    mn, mx = (v.amin(-1), v.amax(-1)) if st in ("group", "tensor_group") else (v.amin(-1, keepdim=True), v.amax(-1, keepdim=True))
    mn, mx = torch.min(mn, torch.zeros_like(mn)), torch.max(mx, torch.zeros_like(mx))
    amax = torch.max(mn.abs(), mx.abs())
    if plan.kind == "int":
        scale = amax / (float(2 ** args.num_bits - 1) / 2)
        eps = torch.finfo(x.dtype).eps
    elif plan.kind == "fp8":
        scale = amax / 448.0
        eps = torch.finfo(x.dtype).eps
    elif plan.kind == "nvfp4":
        scale = amax / 6.0
        if gs is not None:
            scale = gs * scale
        scale = torch.clamp(scale, -448, 448).to(C.F8).to(scale.dtype)
        eps = 0.125
    else:  # mx
        bits = amax.view(torch.int16).to(torch.int32) if x.dtype != C.F32 else amax.view(torch.int32)
        mant, expo = (7, 8) if x.dtype == C.BF16 else (10, 5)
        p2 = ((bits + (1 << (mant - 2))) & (((1 << (expo + 1)) - 1) << mant)).to(torch.int16).view(x.dtype)
        e = 127 + torch.floor(torch.log2(p2)) - (2 if plan.kind == "mxfp4" else 8)
        # a NaN group: the reference's CPU min / max hand round_to_power_2 an all-ones NaN, whose masked sum is +0 -> code 0
        e = torch.where(torch.isnan(amax), torch.zeros_like(e), e)
        e = torch.round(torch.clamp(e, 0, 255)).to(torch.uint8)
        scale = (2.0 ** (e.to(torch.int32) - 127).to(torch.float)).to(x.dtype)
        eps = 1
    scale = torch.where(scale == 0, torch.tensor(eps, dtype=scale.dtype, device=x.device), scale)
    qmin, qmax = {"int": (-(2 ** args.num_bits) / 2, 2 ** args.num_bits / 2 - 1), "fp8": (-448.0, 448.0), "mxfp8": (-448.0, 448.0)}.get(plan.kind, (-6.0, 6.0))
    s = scale / gs if gs is not None else scale
    s_b = s.unsqueeze(-1) if st in ("group", "tensor_group") else s
    scaled = v / s_b
    scaled += torch.zeros((), dtype=x.dtype, device=x.device)
    q = torch.clamp(scaled, qmin, qmax)
    if plan.kind == "int":
        q = torch.round(q)
    elif plan.kind in ("fp8", "mxfp8"):
        q = q.to(C.F8).to(scaled.dtype)
    else:
        from compressed_tensors_amd.codec import cast_to_fp4

        q = cast_to_fp4(q)
    out = (q.to(s_b.dtype) - 0) * s_b
    return out.flatten(-2).to(x.dtype) if st in ("group", "tensor_group") else out


@pytest.mark.parametrize("dtype", [C.BF16, C.F16])
@pytest.mark.parametrize("preset", ["fp8_token", "int8_token", "nvfp4", "mxfp4"])
def test_exhaustive_bit_patterns(dtype, preset):
    from compressed_tensors_amd.quantization.dynamic import dynamic_fake_quantize

    row = 32 if preset == "mxfp4" else (16 if preset == "nvfp4" else 64)
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    comp = (torch.arange(row - 1, dtype=torch.float32) - row / 2) / 8
    x = torch.cat([pats[:, None], comp.to(dtype)[None, :].expand(65536, row - 1)], dim=1).reshape(1, 65536, row).contiguous().to(DEV)
    gs = torch.tensor([37.5], device=DEV) if preset == "nvfp4" else None
    args = _args(preset)
    out = dynamic_fake_quantize(x, args, gs)
    ref = _eager(x, args, gs)
    assert out.dtype == ref.dtype == dtype
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(out), nan)
    assert torch.equal(out[~nan].view(torch.int16), ref[~nan].view(torch.int16))


# ---- modules under install(patch_forward=True) --------------------------------------------------------------------------------
MODULE_PRESETS = ["FP8_DYNAMIC", "W4AFP8", "W8A8", "FP8_BLOCK", "NVFP4", "MXFP4", "MXFP8"]  # W8A8: INT8_W8A8


@pytest.mark.skipif(not ref_import.available(), reason="no reference on this machine")
@pytest.mark.parametrize("preset", MODULE_PRESETS)
def test_modules_under_patch_forward(preset):
    ref_import.import_reference()
    from compressed_tensors.quantization import QuantizationStatus, preset_name_to_scheme
    from compressed_tensors.quantization.lifecycle.initialize import initialize_module_for_quantization

    import compressed_tensors_amd.install as ct_amd
    from compressed_tensors_amd import _lib

    try:
        scheme = preset_name_to_scheme(preset, ["Linear"])
    except (KeyError, ValueError) as e:
        pytest.skip(f"preset {preset} not in this reference: {e}")
    torch.manual_seed(0)
    stack = torch.nn.Sequential(*[torch.nn.Linear(256, 256, bias=False, dtype=C.BF16) for _ in range(3)]).to(DEV)
    for lin in stack:
        initialize_module_for_quantization(lin, scheme)
        with torch.no_grad():
            if hasattr(lin, "weight_scale"):
                lin.weight_scale.fill_(0.01) if lin.weight_scale.dtype.is_floating_point else lin.weight_scale.fill_(120)
            if hasattr(lin, "input_global_scale"):
                lin.input_global_scale.fill_(37.5)
            if hasattr(lin, "weight_global_scale"):
                lin.weight_global_scale.fill_(1000.0)
        lin.quantization_status = QuantizationStatus.FROZEN
    x = torch.randn(2, 8, 256, dtype=C.BF16, device=DEV)
    want = stack(x)
    counts = collections.Counter()
    lib = _lib.load()
    saved = {n: getattr(lib, n) for n in ("ct_dynamic_qdq", "ct_dynamic_qdq_tensor")}
    for n in saved:
        def counted(*a, _o=saved[n], _n=n):
            counts[_n] += 1
            return _o(*a)
        setattr(lib, n, counted)
    ct_amd.install(patch_forward=True)
    try:
        got = stack(x)
    finally:
        ct_amd.uninstall()
        for n, f in saved.items():
            setattr(lib, n, f)
    assert got.dtype == want.dtype and torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert sum(counts.values()) >= 3, counts  # one per Linear's input
