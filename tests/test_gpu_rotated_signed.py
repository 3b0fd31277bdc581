"""The signed power-of-two Hadamard rotation fused into the dynamic QDQ launch (csrc/ct_rotated_signed.hip) on the MI355X:
bit-identity with the two launches it replaces, a float64 reference on exact inputs, the FP8 bound of tests/test_gpu_rotated_k.py."""
import collections
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dynamic_cases as D  # noqa: E402
import _random_hadamard_cases as C  # noqa: E402

from compressed_tensors_amd import codec  # noqa: E402
from compressed_tensors_amd.quantization import QuantizationArgs, dynamic  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# One item per form, its cases (n, columns, kind, rows, signs, dtypes) inside it (the GPU suite keeps its item count down): the smallest
# shape at which the form can go wrong, 5 rows each so that the last workgroup is ragged, bf16 and fp16
BOTH = ("bf16", "f16")
FORMS = {
    "in_wave": [(64, 1024, "mxfp4", 5, "seeded", BOTH), (64, 1024, "nvfp4", 5, "seeded", BOTH)],  # two tiles of 512 units, the second one ragged
    "head_row": [(128, 384, "fp8_token", 5, "seeded", BOTH)],  # three blocks per staged token row
    "block": [(1024, 1024, "fp8_group128", 5, "seeded", BOTH)],  # in-wave groups inside a workgroup-sized block
    "block_row": [(1024, 1024, "fp8_token", 5, "seeded", BOTH), (1024, 1024, "int8_token_asym", 5, "seeded", BOTH),
                  (8192, 8192, "fp8_token", 5, "seeded", BOTH),  # the most units per thread, four waves
                  (4096, 4096, "fp8_token", 5, "minus", ("bf16",))],  # every sign -1, two waves
    # more rows than the capped grid has workgroups: later rounds reuse the signs in registers, the LDS exchange and the reduction area
    "later_rounds": [(64, 1024, "mxfp4", 4100, "seeded", ("bf16",)), (128, 384, "fp8_token", 4100, "seeded", ("bf16",)),
                     (1024, 1024, "fp8_group128", 4100, "seeded", ("bf16",)), (4096, 4096, "fp8_token", 2050, "seeded", ("bf16",))],
}


def _signs(n, mode):
    if mode == "minus":
        return torch.full((n,), -1, dtype=torch.int8, device=DEV)
    return (torch.randint(0, 2, (n,), generator=torch.Generator().manual_seed(n), dtype=torch.int8) * 2 - 1).to(DEV)


def _reference_rotation(x, n, signs):
    """(x.double() * s) @ H_n / sqrt(n) with H_n = H_(n / m) (x) H_m as two small float64 products.  The divisor is float32(sqrt n),
    the value the rotation divides by, and the quotient passes through float32, the type the rotation computes in, on its way to
    the one rounding to x's dtype: for the integer inputs of this file every sum is exact in both types, so this IS the result."""
    m = min(n, 1024)
    v = (x.double().reshape(-1, n) * signs.double()).reshape(-1, n // m, m)
    y = torch.einsum("pa,rab,bq->rpq", C.sylvester(n // m), v, C.sylvester(m)).reshape(x.shape)
    return (y / torch.tensor(n, dtype=C.F64).sqrt().to(C.F32).to(C.F64)).to(C.F32).to(x.dtype)


@pytest.mark.parametrize("form", FORMS)
def test_signed_fusion(form, monkeypatch):
    """1. out, scale, zero point and rotated are the composition's bytes, from exactly one launch of the new entry;  2. on integers
    |x| <= 128 (n * 128 < 2^24: every butterfly sum is exact in float32) the rotated tensor equals the float64 reference;  3. for the
    FP8 kinds `out` is within the bound tests/test_gpu_rotated_k.py derives (one E4M3 step at the element's magnitude plus the scale's
    roundings: tol = s (step + 3 u (|q| + step))) of the float64 QDQ of that rotated tensor.  Fails without the feature."""
    counts, orig = collections.Counter(), codec.call
    monkeypatch.setattr(codec, "call", lambda name, *a: counts.update([name]) or orig(name, *a))
    for n, cols, kind, rows, mode, dts in FORMS[form]:
        for dt in dts:
            _check(n, cols, kind, dt, rows, mode, counts)


def _check(n, cols, kind, dt, rows, mode, counts):
    dtype, signs, what = D.DTYPES[dt], _signs(n, mode), f"n = {n}, {kind}, {dt}, {rows} rows, {mode} signs"
    args, gs = QuantizationArgs(**D.PRESETS[kind]), (D.global_scale_of("gs").to(DEV) if kind == "nvfp4" else None)
    inputs = [torch.randn((1, rows, cols), generator=torch.Generator().manual_seed(n + rows), dtype=torch.float32).to(dtype)]
    if rows == 5:
        inputs.append(C.synth(dict(gen="ints", dtype=dt, shape=[1, rows, cols], salt=n % 89)))
    for x in inputs:
        counts.clear()
        fused = dynamic.rotated_fake_quantize(x.to(DEV), n, args, gs, signs=signs, fused=True, return_qparams=True, return_rotated=True)
        assert dict(counts) == {"ct_hadamard_signed_dynamic_qdq": 1}, (what, counts)
        comp = dynamic.rotated_fake_quantize(x.to(DEV), n, args, gs, signs=signs, fused=False, return_qparams=True, return_rotated=True)
        for name, a, b in zip(("out", "scale", "zp", "rotated"), fused, comp):
            assert a.dtype == b.dtype and a.shape == b.shape and D.canonical_bytes(a) == D.canonical_bytes(b), f"{what}: {name} differs from the composition"
    if rows != 5:
        return  # the later rounds of the grid: the identity above is their check
    want_rot = _reference_rotation(x, n, signs.cpu())
    assert torch.equal(fused[3].cpu(), want_rot), what
    if kind.startswith("fp8"):
        u, L = C.ULP[dtype], dynamic.plan_rotated_dynamic(x.shape, dtype, n, args, signed=True).dynamic.seg_len
        seg = want_rot.to(C.F64).reshape(-1, L)
        s = seg.abs().amax(-1, keepdim=True) / 448.0
        t = seg / s
        q = t.to(torch.float32).clamp(-448, 448).to(torch.float8_e4m3fn).to(C.F64)
        step = torch.exp2(torch.floor(torch.log2((t.abs() * (1 + 4 * u)).clamp(2.0 ** -6, 448.0))) - 3)
        err = (fused[0].cpu().to(C.F64).reshape(-1, L) - q * s).abs()
        assert bool((err <= s * (step + 3 * u * (q.abs() + step))).all()), what


def test_a_size_that_is_not_a_power_of_two_is_refused():
    x = torch.zeros((1, 5, 192), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="96 is not a power of two"):
        dynamic.rotated_fake_quantize(x, 96, QuantizationArgs(**D.PRESETS["fp8_token"]), signs=_signs(96, "seeded"), fused=True)
