"""Host side of the random-hadamard rotation fused into the dynamic QDQ launch (quantization/dynamic.py: plan_rotated_k_dynamic;
csrc/ct_rotated_k.hip): the plan table from shapes alone, the exported entry, and the dispatch set against its profile.  No GPU."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dynamic_cases as D  # noqa: E402

from compressed_tensors_amd import _lib, codec, transform  # noqa: E402
from compressed_tensors_amd.quantization import QuantizationArgs, dynamic  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32


def _plan(preset, shape, n, k, dtype=BF16):
    gs = torch.tensor([37.5]) if preset == "nvfp4" else None
    return dynamic.plan_rotated_k_dynamic(shape, dtype, n, k, QuantizationArgs(**D.PRESETS[preset]), gs)


@pytest.mark.parametrize("preset,shape,n,k,dtype,want,launches", [  # want: the key of a served shape, or a piece of the reason
    ("fp8_token", (1, 3, 4480), 4480, 140, BF16, "mfma_row_tt1", 1), ("int8_token", (1, 9, 11008), 11008, 172, torch.float16, "mfma_row_tt2", 1),
    ("fp8_token", (1, 9, 28672), 28672, 224, BF16, "mfma_row_tt4", 1), ("int8_token_asym", (1, 9, 18944), 18944, 148, BF16, "mfma_row_tt4", 1),
    ("fp8_group128", (9, 4480), 4480, 140, BF16, "mfma_group_tt1", 1), ("mxfp4", (1, 5, 1376), 1376, 172, BF16, "mfma_group_tt1", 1),
    ("nvfp4", (1, 5, 2368), 2368, 148, BF16, "mfma_group_tt1", 1), ("mxfp8", (2, 2, 2 * 11008), 11008, 172, BF16, "mfma_group_tt2", 1),
    ("fp8_group128", (1, 9, 14336), 14336, 224, torch.float16, "mfma_group_tt2", 1), ("nvfp4", (1, 9, 28672), 28672, 224, BF16, "mfma_group_tt4", 1),
    ("fp8_group128", (1, 2, 8 * 1376), 1376, 172, BF16, "a segment of 128 elements over rotation blocks of 1376", 2),  # 128 divides the row, not the block
    ("fp8_token", (1, 5, 1376), 1376, 172, BF16, "shares its workgroup with 3 more blocks", 2),  # G > 1
    ("fp8_token", (1, 3, 4096), 4096, 1, BF16, "k == 1", 2), ("fp8_token", (1, 3, 4480), 4480, 140, F32, "float32 activations", 3),
    ("fp8_token", (1, 3, 3072), 3072, 12, BF16, "runs of 256 elements", 3), ("nvfp4", (3, 560), 560, 140, BF16, "runs of 4 elements", 3),  # the vector form
    ("fp8_token", (2, 3, 2 * 4480), 4480, 140, BF16, "2 rotation blocks", 2),
    ("fp8_tensor", (1, 9, 4480), 4480, 140, BF16, "tensor form", 3), ("fp8_token", (9, 4480), 4480, 140, BF16, "tensor form", 3),
])
def test_plan_table(preset, shape, n, k, dtype, want, launches, monkeypatch):
    shipped = _plan(preset, shape, n, k, dtype)  # as shipped: the key speaks for the shape, the set decides
    assert shipped.fused == (shipped.key in dynamic.ROTATED_K_MEASURED_FASTER) and (shipped.reason is None) == shipped.fused
    monkeypatch.setattr(dynamic, "ROTATED_K_MEASURED_FASTER", dynamic.ROTATED_K_ALL_FORMS)
    plan = _plan(preset, shape, n, k, dtype)
    if want in dynamic.ROTATED_K_ALL_FORMS:
        assert plan.fused and plan.key == shipped.key == want and plan.form == want.rsplit("_", 1)[0] and plan.reason is None and plan.hadamard.form == "mfma"
    else:
        assert not plan.fused and plan.form is None and plan.key is None and want in plan.reason, plan.reason
    assert plan.launches() == launches and plan.dynamic.segs * plan.dynamic.seg_len == torch.Size(shape).numel()


def test_the_entry_is_exported():
    argtypes, restype = _lib._PROTOTYPES["ct_hadamard_k_dynamic_qdq"]
    assert "ct_hadamard_k_dynamic_qdq" in _lib.EXPORTED_SYMBOLS and len(argtypes) == 18 and restype is _lib._PROTOTYPES["ct_dynamic_qdq"][1]
    with open(os.path.join(ROOT, "include", "ct_hip.h")) as f:
        assert "int ct_hadamard_k_dynamic_qdq(const void* x, int xdt, int64_t numel, int64_t n, int64_t k, const int8_t* had_k" in f.read()
    assert callable(codec.hadamard_k_dynamic_qdq) and callable(dynamic.random_rotated_fake_quantize) and callable(transform.fuse_random_input_quantization)


def test_as_shipped_every_dispatched_key_is_measured_faster():
    """the set holds only keys whose every verdict of profiles/rotated_k_bench.jsonl says "faster"; an empty set needs no profile"""
    assert dynamic.ROTATED_K_MEASURED_FASTER <= dynamic.ROTATED_K_ALL_FORMS
    if dynamic.ROTATED_K_MEASURED_FASTER:
        with open(os.path.join(ROOT, "profiles", "rotated_k_bench.jsonl")) as f:
            verdicts = [v for v in map(json.loads, f) if "verdict" in v]
        for key in dynamic.ROTATED_K_MEASURED_FASTER:
            rows = [v for v in verdicts if v["key"] == key]
            assert rows and all(v["faster"] for v in rows), (key, rows)
