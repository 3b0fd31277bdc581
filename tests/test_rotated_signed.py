"""Host side of the signed power-of-two Hadamard rotation fused into the dynamic QDQ launch (quantization/dynamic.py:
plan_rotated_dynamic(signed=True); csrc/ct_rotated_signed.hip): the exported entry and the plan table from shapes alone.  No GPU."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dynamic_cases as D  # noqa: E402

from compressed_tensors_amd import _lib, codec  # noqa: E402
from compressed_tensors_amd.quantization import QuantizationArgs, dynamic  # noqa: E402

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _plan(preset, shape, n, dtype=BF16, **kw):
    gs = torch.tensor([37.5]) if preset == "nvfp4" else None
    return dynamic.plan_rotated_dynamic(shape, dtype, n, QuantizationArgs(**(preset if isinstance(preset, dict) else D.PRESETS[preset])), gs, **kw)


def test_the_entry_is_declared_prototyped_and_exported():
    argtypes, restype = _lib._PROTOTYPES["ct_hadamard_signed_dynamic_qdq"]
    assert "ct_hadamard_signed_dynamic_qdq" in _lib.EXPORTED_SYMBOLS and len(argtypes) == 16 and restype is _lib._PROTOTYPES["ct_dynamic_qdq"][1]
    with open(os.path.join(ROOT, "include", "ct_hip.h")) as f:
        assert "int ct_hadamard_signed_dynamic_qdq(const void* x, int xdt, int64_t numel, int64_t n, const int8_t* signs, int64_t seg_len" in f.read()
    assert callable(codec.hadamard_signed_dynamic_qdq) and "hadamard_signed_dynamic_qdq" in codec.__all__
    assert dynamic.ROTATED_SIGNED_MEASURED_FASTER <= dynamic.ALL_FORMS


@pytest.mark.parametrize("preset,shape,n,dtype,want", [  # want: the key of a served shape, or a piece of the named refusal
    ("mxfp4", (1, 5, 1024), 64, BF16, "in_wave"), ("nvfp4", (1, 5, 1024), 64, F16, "in_wave"), ("fp8_group128", (5, 256), 128, BF16, "in_wave"),
    ("fp8_token", (1, 5, 384), 128, BF16, "head_row"), ("int8_token_asym", (2, 3, 32768), 8, F16, "head_row"),
    ("fp8_group128", (1, 5, 1024), 1024, BF16, "block_1024"), ("mxfp8", (1, 5, 8192), 4096, F16, "block_4096"),
    ("fp8_token", (1, 5, 1024), 1024, BF16, "block_row_1024"), ("int8_token_asym", (1, 5, 2048), 2048, BF16, "block_row_2048"),
    ("fp8_token", (1, 5, 8192), 8192, F16, "block_row_8192"),
    ("fp8_token", (1, 5, 192), 96, BF16, "96 is not a power of two"),  # a ValueError: the composition has no such rotation either
    ("fp8_token", (1, 5, 16384), 16384, BF16, "exceeds the fused maximum 8192"),
    ("fp8_token", (1, 5, 1024), 1024, F32, "float32 activations"),
    ("fp8_tensor", (1, 5, 1024), 1024, BF16, "tensor form"), ("fp8_token", (5, 1024), 1024, BF16, "tensor form"),
    ("fp8_token", (1, 5, 24), 4, BF16, "blocks of 4 elements are not whole 16-byte units"),
    (dict(D.PRESETS["fp8_group128"], group_size=24), (1, 5, 48), 16, BF16, "segments of 24 elements are not whole 16-byte units of whole blocks of 16"),
    ("fp8_token", (1, 5, 65536), 128, BF16, "rows of 65536 elements exceed the staged form (32768)"),
    ("fp8_token", (1, 5, 4096), 1024, BF16, "a segment of 4096 elements over workgroup-sized blocks of 1024"),
])
def test_signed_plan_table(preset, shape, n, dtype, want, monkeypatch):
    if "power of two" in want:
        with pytest.raises(ValueError, match=want):
            _plan(preset, shape, n, dtype, signed=True)
        return
    shipped = _plan(preset, shape, n, dtype, signed=True)  # as shipped nothing is measured: the key speaks for the shape, the empty set declines it
    assert not shipped.fused and shipped.form is None and shipped.launches() == 1 + shipped.dynamic.launches()
    assert type(shipped.hadamard) is codec.HadamardKPlan and shipped.hadamard.form == "butterfly"
    monkeypatch.setattr(dynamic, "ROTATED_SIGNED_MEASURED_FASTER", dynamic.ALL_FORMS)
    plan = _plan(preset, shape, n, dtype, signed=True)
    if want in dynamic.ALL_FORMS:
        assert plan.fused and plan.key == shipped.key == want and plan.reason is None and plan.launches() == 1
        assert "ROTATED_SIGNED_MEASURED_FASTER" in shipped.reason
    else:
        assert not plan.fused and plan.form is None and plan.key is shipped.key is None and want in plan.reason == shipped.reason


@pytest.mark.parametrize("preset,shape,n,form", [("fp8_token", (1, 5, 4096), 4096, "block_row"), ("fp8_group128", (1, 5, 1024), 1024, "block"),
                                                 ("fp8_token", (1, 5, 384), 128, "head_row"), ("mxfp4", (1, 5, 1024), 64, None)])
def test_without_signs_the_plan_is_the_one_before(preset, shape, n, form, monkeypatch):
    """signed=False is the default and the unsigned rule: plan_hadamard's plan, MEASURED_FASTER (in_wave is not in it), untouched by the signed set"""
    monkeypatch.setattr(dynamic, "ROTATED_SIGNED_MEASURED_FASTER", dynamic.ALL_FORMS)
    plan, explicit = _plan(preset, shape, n), _plan(preset, shape, n, signed=False)
    assert type(plan.hadamard) is codec.HadamardPlan and plan.hadamard == explicit.hadamard == codec.plan_hadamard(shape, BF16, n)
    assert (plan.fused, plan.form, plan.key, plan.reason) == (explicit.fused, explicit.form, explicit.key, explicit.reason)
    assert plan.form == form and plan.fused == (form is not None) and (plan.key in dynamic.MEASURED_FASTER) == plan.fused
