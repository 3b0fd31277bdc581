"""Host side of the dynamic activation QDQ (quantization/dynamic.py, install(patch_forward=True)): the dispatch rule, the scale
and zero-point shapes and dtypes the host plans against the reference's (tests/golden/dynamic_manifest.json), and the rebinding of
the reference's forward_quantize / compute_dynamic_scales_and_zp.  No GPU needed."""
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

from compressed_tensors_amd.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors_amd.quantization.dynamic import plan_dynamic  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "dynamic_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]


def test_public_names():
    import compressed_tensors_amd.quantization as q

    assert callable(q.compute_dynamic_scales_and_zp) and callable(q.forward_quantize)
    assert QuantizationArgs(num_bits=4, type="float", strategy="tensor_group", group_size=16, dynamic="local").dynamic == "local"


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_planned_shapes_and_dtypes_match_the_reference(key):
    entry = MANIFEST[key]
    r = entry["recipe"]
    plan = plan_dynamic(tuple(r["shape"]), C.DTYPES[r["dtype"]], QuantizationArgs(**C.PRESETS[r["preset"]]),
                        C.global_scale_of(r["gs"]) if r["gs"] else None)
    assert list(plan.scale_shape) == entry["scale"]["shape"] == entry["zp"]["shape"]
    assert str(plan.scale_dtype).replace("torch.", "") == entry["scale"]["dtype"]
    assert str(plan.zp_dtype).replace("torch.", "") == entry["zp"]["dtype"]
    assert entry["out"]["dtype"] == r["dtype"].replace("bf16", "bfloat16").replace("f16", "float16").replace("f32", "float32")
    assert plan.segs * plan.seg_len == torch.Size(r["shape"]).numel()
    token_2d = C.PRESETS[r["preset"]]["strategy"] == "token" and len(r["shape"]) <= 2
    assert plan.tensor_form == (token_2d or C.PRESETS[r["preset"]]["strategy"] == "tensor")


def test_manifest_matches_the_case_list():
    cases = dict(C.case_list())
    assert set(MANIFEST) == set(cases)
    for key, recipe in cases.items():
        assert MANIFEST[key]["recipe"] == recipe and MANIFEST[key]["stored"] == C.stored(recipe), key


def test_finite_whole_tensor_fixtures_are_meaningful():
    """A condition on the fixtures: where the whole tensor is one segment, synth's NaN row makes the reference's scale and output
    all NaN, which pins NaN propagation and nothing else.  Every preset with such a form also has cases marked `finite`, and in
    those the reference's output has no NaN and takes many values (`out_nan`, `out_distinct`: tools/gen_golden_dynamic.py), so a
    wrong scale, zero point, qmin or qmax changes the bytes that tests/test_gpu_dynamic_quant.py compares."""
    finite = {}
    for key, entry in MANIFEST.items():
        r = entry["recipe"]
        if not C.tensor_form(r):
            continue
        finite.setdefault(r["preset"], [])
        if r.get("finite"):
            numel = torch.Size(r["shape"]).numel()
            assert entry["out_nan"] == 0, key
            assert entry["out_distinct"] >= min(numel // 2, 2 ** (C.PRESETS[r["preset"]]["num_bits"] - 2)), (key, entry["out_distinct"])
            finite[r["preset"]].append(key)
        else:
            assert entry["out_nan"] == torch.Size(r["shape"]).numel(), key  # the all-NaN cases stay what they are
    with_tensor_form = {p for p, a in C.PRESETS.items() if a["strategy"] in ("tensor", "token")}
    assert set(finite) == with_tensor_form
    assert all(finite[p] for p in with_tensor_form), {p for p in with_tensor_form if not finite[p]}


def test_make_input_recipes():
    """entries without the optional keys synthesise what they always did; `finite` drops the edge rows; `plant` decides the extremes"""
    base = dict(preset="int8_tensor_asym", dtype="bf16", shape=[33, 1001], salt=4, gs=None)
    assert C.sha(C.make_input(base)) == C.sha(C.synth((33, 1001), C.BF16, 4))
    x = C.make_input(dict(base, finite=True))
    assert x.shape == (33, 1001) and x.is_contiguous() and C.sha(x) == C.sha(C.synth((41, 1001), C.BF16, 4)[8:])
    assert bool(torch.isfinite(x).all()) and float(x.abs().max()) <= 128 < C.PLANT_OTHER < C.PLANT_MAX < torch.finfo(torch.float16).max
    n = x.numel()
    for plant, at in (("first", 0), ("last", n - 1), ("middle", n // 2 + 3)):
        for salt, sign in ((4, 1.0), (5, -1.0)):
            y = C.make_input(dict(base, salt=salt, finite=True, plant=plant)).reshape(-1)
            other = (at + C.PLANT_APART) % n
            assert float(y[at]) == sign * C.PLANT_MAX and float(y[other]) == -sign * C.PLANT_OTHER
            assert float(y.max()) == max(float(y[at]), float(y[other])) and float(y.min()) == min(float(y[at]), float(y[other]))
            assert (at // 8 // 256) % 3 != (other // 8 // 256) % 3  # 33033 elements: three partials, 256 units of 8 apart
            rest = torch.ones(n, dtype=torch.bool)
            rest[[at, other]] = False
            assert torch.equal(y[rest], C.make_input(dict(base, salt=salt, finite=True)).reshape(-1)[rest])
            z = C.make_input(dict(base, preset="fp8_tensor", salt=salt, finite=True, plant=plant)).reshape(-1)  # symmetric: one extreme
            assert float(z[at]) == sign * C.PLANT_MAX and float(z.abs().max()) == C.PLANT_MAX and int((z.abs() > 128).sum()) == 1


def _args(**kw):
    return QuantizationArgs(**{"num_bits": 8, "type": "float", "strategy": "token", "symmetric": True, "dynamic": True, **kw})


@pytest.mark.parametrize("kw,shape,dtype,gs,err", [
    (dict(), (2, 3, 64), torch.bfloat16, None, None),
    (dict(type="int"), (2, 64), torch.float16, None, None),
    (dict(type="int", symmetric=False, num_bits=3), (4, 2, 2, 16), torch.float32, None, None),
    (dict(strategy="channel"), (2, 3, 64), torch.bfloat16, None, ValueError),  # the reference raises for dynamic channel
    (dict(strategy="block", block_structure=[128, 128]), (2, 3, 64), torch.bfloat16, None, ValueError),
    (dict(symmetric=False), (2, 3, 64), torch.bfloat16, None, NotImplementedError),  # FP8 asymmetric: no kernel
    (dict(), (2, 3, 64), torch.float64, None, NotImplementedError),
    (dict(), (2, 3, 0), torch.bfloat16, None, NotImplementedError),
    (dict(strategy="group", group_size=128), (2, 3, 192), torch.bfloat16, None, NotImplementedError),  # H % gs: the reference raises
    (dict(type="int", scale_dtype=torch.float16), (2, 3, 64), torch.bfloat16, None, NotImplementedError),
    (dict(), (2, 3, 64), torch.bfloat16, torch.ones(1), NotImplementedError),  # a global scale outside NVFP4
    (dict(num_bits=4, strategy="tensor_group", group_size=16, scale_dtype=torch.float8_e4m3fn), (2, 3, 64), torch.bfloat16, torch.ones(1), None),
    (dict(num_bits=4, strategy="group", group_size=32, scale_dtype=torch.uint8, zp_dtype=torch.uint8), (3, 64), torch.float16, None, None),
    (dict(num_bits=4, strategy="group", group_size=16), (3, 64), torch.bfloat16, None, NotImplementedError),  # FP4 without a scale dtype
])
def test_dispatch_rule(kw, shape, dtype, gs, err):
    if err is None:
        plan = plan_dynamic(shape, dtype, _args(**kw), gs)
        assert plan.launches() in (1, 2)
    else:
        with pytest.raises(err):
            plan_dynamic(shape, dtype, _args(**kw), gs)


def test_launch_plan():
    assert plan_dynamic((2, 16, 4096), torch.bfloat16, _args(), None).launches() == 1
    assert plan_dynamic((64, 4096), torch.bfloat16, _args(), None).launches() == 2  # 2-D token: the whole tensor
    assert plan_dynamic((2, 16, 4096), torch.bfloat16, _args(strategy="tensor"), None).launches() == 2
    assert plan_dynamic((4, 16), torch.bfloat16, _args(strategy="tensor"), None).launches() == 1


def test_forward_quantize_control_flow():
    """returns before any kernel: a compressed weight, an empty value; group activations under an initialised g_idx are refused"""
    from compressed_tensors_amd.quantization import forward_quantize

    m = torch.nn.Linear(4, 4)
    m.quantization_status = "compressed"
    w = torch.randn(4, 4)
    assert forward_quantize(m, w, "weight", _args()) is w
    m.quantization_status = "frozen"
    e = torch.empty(0, 4)
    assert forward_quantize(m, e, "input", _args()) is e
    m.weight_g_idx = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        forward_quantize(m, torch.randn(2, 32), "input", _args(strategy="group", group_size=16))


needs_ref = pytest.mark.skipif(not ref_import.available(), reason="no reference on this machine")


@needs_ref
def test_patch_forward_rebinds_and_uninstall_restores():
    ref_import.import_reference()
    import compressed_tensors.quantization.lifecycle.forward as up_forward
    import compressed_tensors.quantization.utils as up_utils
    import compressed_tensors.quantization.utils.helpers as up_helpers

    import compressed_tensors_amd.install as ct_amd

    fq, cd = up_forward.forward_quantize, up_helpers.compute_dynamic_scales_and_zp
    assert not hasattr(fq, "_ct_original")
    ct_amd.install(patch_forward=True)
    try:
        assert up_forward.forward_quantize._ct_original is fq
        assert up_forward.compute_dynamic_scales_and_zp._ct_original is cd
        assert up_helpers.compute_dynamic_scales_and_zp._ct_original is cd
        assert up_utils.compute_dynamic_scales_and_zp._ct_original is cd
        wrapped = up_forward.forward_quantize
        ct_amd.install(patch_forward=True)  # again: the same wrappers, nothing recorded twice
        assert up_forward.forward_quantize is wrapped
        # CPU activations go to the original
        from compressed_tensors.quantization import QuantizationArgs as UpArgs

        args = UpArgs(num_bits=8, type="float", strategy="token", symmetric=True, dynamic=True)
        x = torch.randn(2, 3, 64, dtype=torch.bfloat16)
        s, z = up_forward.compute_dynamic_scales_and_zp(value=x, args=args, module=None)
        s0, z0 = cd(value=x, args=args, module=None)
        assert torch.equal(s, s0) and torch.equal(z.view(torch.uint8), z0.view(torch.uint8))
    finally:
        ct_amd.uninstall()
    assert up_forward.forward_quantize is fq
    assert up_forward.compute_dynamic_scales_and_zp is cd and up_helpers.compute_dynamic_scales_and_zp is cd


@needs_ref
@pytest.mark.parametrize("kw", [dict(), dict(patch_functions=True)])
def test_other_install_modes_leave_forward_quantize_alone(kw):
    ref_import.import_reference()
    import compressed_tensors.quantization.lifecycle.forward as up_forward
    import compressed_tensors.quantization.utils.helpers as up_helpers

    import compressed_tensors_amd.install as ct_amd

    fq, cd = up_forward.forward_quantize, up_helpers.compute_dynamic_scales_and_zp
    ct_amd.install(**kw)
    try:
        assert up_forward.forward_quantize is fq and up_helpers.compute_dynamic_scales_and_zp is cd
    finally:
        ct_amd.uninstall()


@needs_ref
def test_patch_functions_after_patch_forward_still_patches():
    """the two keywords keep separate tables: one installed first does not stop the other"""
    ref_import.import_reference()
    import compressed_tensors.quantization.lifecycle.forward as up_forward

    import compressed_tensors_amd.install as ct_amd

    fake = up_forward.fake_quantize
    ct_amd.install(patch_forward=True)
    try:
        ct_amd.install(patch_functions=True)
        assert up_forward.fake_quantize._ct_original is fake
        assert hasattr(up_forward.forward_quantize, "_ct_original")
    finally:
        ct_amd.uninstall()
    assert up_forward.fake_quantize is fake
