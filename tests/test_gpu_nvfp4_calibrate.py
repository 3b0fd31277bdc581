"""The calibrated half of NVFP4 activations on the device: MinMaxObserver.get_global_scale (kind 2 of ct_attn_observe) against the fixtures the
reference's test observer wrote (tools/gen_golden_nvfp4_calib.py), and modeling.calibrate_global_scales end to end.  Everything is bit-exact.
Every test here needs an MI355X:  python -m pytest tests -m gpu"""
import json
import os

import pytest
import torch

import _nvfp4_calib_cases as C
import oracle as O
from _golden import GOLDEN_DIR

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
with open(os.path.join(GOLDEN_DIR, "nvfp4_calib_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
RECIPES = {k: v["recipe"] for k, v in MANIFEST.items()}
_GOLDEN = {}


def golden(key):
    if not _GOLDEN:
        from safetensors.torch import load_file

        _GOLDEN.update(load_file(os.path.join(GOLDEN_DIR, "nvfp4_calib.safetensors")))
    return _GOLDEN[f"{key}.global_scale"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cta():
    import compressed_tensors_amd as m
    from compressed_tensors_amd import _lib

    _lib.load()  # fail loudly if the HIP extension is missing
    return m


def preset_args(cta, **kw):
    """the input arguments of upstream's NVFP4 preset"""
    return cta.QuantizationArgs(**dict(dict(num_bits=4, type="float", symmetric=True, strategy="tensor_group", group_size=16, dynamic="local",
                                            observer="static_minmax", scale_dtype=torch.float8_e4m3fn,
                                            zp_dtype=torch.float8_e4m3fn), **kw))


def on_device(x, dev):
    """x on the GPU in the same storage layout (its storage moved as a whole, the view rebuilt)"""
    base = torch.empty(x.untyped_storage().nbytes() // x.element_size(), dtype=x.dtype)
    base.set_(x.untyped_storage(), 0, base.shape)
    return base.to(dev).as_strided(x.shape, x.stride(), x.storage_offset())


def same_f32(a, b):
    return a.dtype == b.dtype == F32 and a.shape == b.shape and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def test_manifest_matches_the_case_list():
    cases = C.case_list()
    assert [k for k, _ in cases] == sorted(MANIFEST, key=[k for k, _ in cases].index) and len(cases) == len(MANIFEST)
    for key, recipe in cases:
        assert MANIFEST[key]["recipe"] == recipe, key
    plain = [r for r in RECIPES.values() if "shape" in r]
    assert {tuple(r["shape"]) for r in plain} >= {(1, 1, 16), (2, 3, 64), (1, 257, 96), (4, 4100, 32), (2, 8, 64, 20)}
    assert {(r["layout"], r["dtype"]) for r in plain} == {(layout, d) for layout in ("contiguous", "slice", "transposed") for d in ("bf16", "f16", "f32")}
    assert {(r["special"], r["dtype"]) for r in plain if r["special"]} == {(s, d) for s in C.SPECIALS for d in ("bf16", "f16", "f32")}


@pytest.mark.parametrize("key", sorted(k for k, r in RECIPES.items() if "shape" in r))
def test_get_global_scale_equals_the_reference_observer(cta, dev, key, monkeypatch):
    """one ct_attn_observe on the view as it is — a slice and a transposed view are read in place —, the reference's float32 (1,) result"""
    from compressed_tensors_amd import codec

    r = RECIPES[key]
    x = C.build(r, RECIPES)
    assert C.sha(x) == MANIFEST[key]["x_sha256"] and list(x.stride()) == MANIFEST[key]["x_strides"]
    xd = on_device(x, dev)
    assert xd.stride() == x.stride() and (r["layout"] == "contiguous") == xd.is_contiguous()
    seen, real = [], codec.call
    monkeypatch.setattr(codec, "call", lambda name, *a: seen.append((name, a)) or real(name, *a))
    monkeypatch.setattr(torch.Tensor, "contiguous", lambda self, *a, **k: pytest.fail("copied a view the kernel can index"))
    observer = cta.quantization.MinMaxObserver("input", preset_args(cta), None)
    got = observer.get_global_scale(xd)
    monkeypatch.undo()
    assert [name for name, _ in seen] == ["ct_attn_observe"] and seen[0][1][2] == 2  # kind 2
    assert seen[0][1][0][0].x == xd.data_ptr()  # the descriptor names the view's own memory
    assert got.is_cuda and same_f32(got, golden(key)), (key, got, golden(key))
    if x.dtype != F32 and not r["special"]:
        assert same_f32(got, O.generate_gparam(x.contiguous().reshape(1, -1)))


@pytest.mark.parametrize("name", ["bf16", "f16", "f32"])
def test_static_accumulates_and_memoryless_does_not(cta, dev, name):
    b0, b1 = (C.build(RECIPES[f"batch{i}.{name}"], RECIPES).to(dev) for i in (0, 1))
    static = cta.quantization.MinMaxObserver("input", preset_args(cta), None)
    assert same_f32(static.get_global_scale(b0), golden(f"batch0.{name}"))
    assert same_f32(static.get_global_scale(b1), golden(f"concat.{name}"))  # the extremes of both batches
    assert not same_f32(golden(f"concat.{name}"), golden(f"batch1.{name}"))
    static.reset()
    assert same_f32(static.get_global_scale(b1), golden(f"batch1.{name}"))
    memoryless = cta.quantization.MinMaxObserver("input", preset_args(cta, observer="memoryless_minmax"), None)
    memoryless.get_global_scale(b0)
    assert same_f32(memoryless.get_global_scale(b1), golden(f"batch1.{name}"))  # the last batch's own
    # forward stays refused for these arguments
    with pytest.raises(NotImplementedError, match="dynamic arguments are not observed"):
        static(b0)


def test_the_parameter_is_written_in_place(cta, dev):
    x = C.build(RECIPES["contiguous.bf16.2x3x64"], RECIPES).to(dev)
    p = torch.nn.Parameter(torch.full((1,), -7.0, device=dev), requires_grad=False)
    ptr = p.data_ptr()
    observer = cta.quantization.MinMaxObserver("input", preset_args(cta), None)
    out = observer.get_global_scale(x, p)
    assert out is p and p.data_ptr() == ptr and same_f32(p.data, golden("contiguous.bf16.2x3x64"))
    with pytest.raises(ValueError, match="global_scale must be a contiguous torch.float32 tensor of shape \\(1,\\)"):
        observer.get_global_scale(x, torch.empty(1, dtype=BF16, device=dev))
    # the C entry holds its own line: a global scale is float32 and has no zero point
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    d = (_lib.AttnObserveTensor * 1)()
    state = cta.codec.attn_observe_state(1, dev)
    d[0].x, d[0].state, d[0].scale, d[0].B, d[0].H, d[0].S, d[0].D, d[0].per_head = x.data_ptr(), state.data_ptr(), p.data_ptr(), 1, 2, 3, 64, 0
    d[0].x_stride[:] = (0, 192, 64)
    assert lib.ct_attn_observe(d, 1, 2, 0, 1, _lib.BF16, _lib.BF16, _lib.I8, 0, _lib.stream_on(dev)) != 0
    assert "float32" in _lib.last_error()
    assert lib.ct_attn_observe(d, 1, 3, 0, 1, _lib.BF16, _lib.F32, _lib.I8, 0, _lib.stream_on(dev)) != 0 and "kind must be" in _lib.last_error()
    torch.cuda.synchronize()
    assert same_f32(p.data, golden("contiguous.bf16.2x3x64"))  # nothing was launched


def test_calibrate_global_scales_end_to_end(cta, dev):
    """a two-Linear bf16 MLP under the NVFP4 preset, two calibration batches, then forward_quantize of a third under the calibrated scale"""
    from compressed_tensors_amd import modeling
    from compressed_tensors_amd.quantization import dynamic

    torch.manual_seed(7)
    model = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.GELU(), torch.nn.Linear(64, 64)).to(dev).to(BF16)
    act = preset_args(cta)
    weights = cta.QuantizationArgs(num_bits=4, type="float", symmetric=True, strategy="tensor_group", group_size=16, scale_dtype=torch.float8_e4m3fn,
                                   zp_dtype=torch.float8_e4m3fn)
    for m in (model[0], model[2]):
        m.quantization_scheme = cta.QuantizationScheme(targets=["Linear"], weights=weights, input_activations=act)
    before = {k: (list(m._parameters), list(m._modules), len(m._forward_pre_hooks), len(m._forward_hooks)) for k, m in enumerate(model)}
    captured = {0: [], 2: []}
    taps = [model[k].register_forward_pre_hook(lambda mod, args, k=k: captured[k].append(args[0].detach().clone())) for k in (0, 2)]
    g = torch.Generator().manual_seed(3)
    batches = [(torch.randn(2, 5, 64, generator=g) * s).to(BF16).to(dev) for s in (4.0, 0.5)]
    with modeling.calibrate_global_scales(model):
        params = {k: model[k].input_global_scale for k in (0, 2)}
        ptrs = {k: p.data_ptr() for k, p in params.items()}
        for b in batches:
            model(b)
    for t in taps:
        t.remove()
    for k in (0, 2):
        p = model[k].input_global_scale
        assert p is params[k] and p.data_ptr() == ptrs[k] and p.dtype == F32 and p.shape == (1,) and not p.requires_grad
        union = torch.cat(captured[k], dim=0).reshape(1, -1)
        assert same_f32(p.data, O.generate_gparam(union.cpu())), (k, p)
    assert float(model[0].input_global_scale) != float(model[2].input_global_scale)
    for k, m in enumerate(model):  # nothing is left on the modules but the parameter
        params_before, modules, pre, post = before[k]
        assert list(m._modules) == modules and len(m._forward_pre_hooks) == pre and len(m._forward_hooks) == post
        assert [n for n in m._parameters if n not in params_before] == (["input_global_scale"] if k in (0, 2) else [])
    third = (torch.randn(3, 4, 64, generator=g) * 2.0).to(BF16).to(dev)
    got = dynamic.forward_quantize(model[0], third, "input", act)
    want = dynamic.dynamic_fake_quantize(third, act, model[0].input_global_scale.data.clone())
    assert got.dtype == BF16 and torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert not torch.equal(want.view(torch.int16), dynamic.dynamic_fake_quantize(third, act, torch.ones(1, device=dev)).view(torch.int16))
