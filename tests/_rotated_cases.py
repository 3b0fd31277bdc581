"""The case matrix of the fused rotation + dynamic QDQ fixtures (tools/gen_golden_rotated.py writes them, tests/test_rotated_quant.py
and tests/test_gpu_rotated_quant.py read them): an online Hadamard rotation of size n along the last dimension, then the dynamic
QDQ of a preset of tests/_dynamic_cases.py.  A case is fully described by its recipe.

Inputs are chosen so that the reference's GEMM and any butterfly agree in every element, which makes the reference a bit-exact
target: integers in [-128, 128] from the integer hash of tests/_hadamard_cases.py, times a per-row power of two
2^((7 * row + salt) % 9 - 4).  Every partial sum is then an integer multiple of a power of two below 2^24, exact in float32 in
any order.  The first rows are edge rows: all zeros, one non-zero (every |r| of its block equal: ties), a -0.0, one +inf, one NaN,
a constant row (one non-zero per block after the rotation).

Everything is compared BY VALUE: zeros are rewritten to +0.0 and NaNs canonicalised before hashing.  A GEMM turns a -0.0 result
into +0.0 where a butterfly does not, and the FP8 / FP4 QDQ carries that sign to its output, so the sign of a zero is a property
of the BLAS, not of the transform.

A known difference of ct_dynamic_qdq (csrc/ct_dynamic.h, dyn_qparams), not of this work: the MX scale of a group that holds a NaN.
The reference's round_to_power_2 adds to the BITS of the group's amax, and the NaN pattern its CPU min / max hand back depends on
which SIMD lanes held the NaN, not on any value: the reference run by tools/gen_golden_rotated.py gives 2^-127 for a group that is
all NaN or ends in one NaN (the layout tests/_dynamic_cases.py pins, and the kernels' rule) and +inf for a group whose second half
is NaN.  NaN payloads are not modelled.  Behind a rotation with n < 32 a NaN spreads over half an MX group, so
the MX cases with n = 8 and 16 keep every row but that one: their NaN row is a second +inf row (`nan_row: false` in the recipe).
MX behind small rotations with NaNs is covered by the bit-identity with the two existing launches (tests/test_gpu_rotated_quant.py).

Where the whole tensor is one segment (the tensor strategy, token on a 2-D input) the +inf and NaN rows make the one scale and
the whole output NaN.  Those cases have a twin with `finite: true` in the recipe: the two rows hold +128 and -128 in place of
+inf and NaN, so the twin's scale is a number and its output takes many values."""
import hashlib
import math

import torch

import _dynamic_cases as D
import _hadamard_cases as H

F32, BF16, F16, F8 = D.F32, D.BF16, D.F16, D.F8
DTYPES = D.DTYPES
PRESETS = D.PRESETS
EDGE_ROWS = 6
MAX_FIXTURE_BYTES = 512 * 1024  # rotated.safetensors + rotated_manifest.json together


def synth(recipe) -> torch.Tensor:
    shape, dtype, salt = tuple(recipe["shape"]), DTYPES[recipe["dtype"]], recipe["salt"]
    numel, cols = math.prod(shape), shape[-1]
    ints = (H._hash(numel, salt) % 257 - 128).to(torch.float64)
    row = torch.arange(numel, dtype=torch.int64) // cols
    x = (ints * torch.pow(2.0, ((row * 7 + salt) % 9 - 4).to(torch.float64))).to(dtype).reshape(shape)
    flat = x.reshape(-1, cols)
    k = torch.arange(cols)
    base = ints[:cols].to(torch.float32)
    finite = recipe.get("finite", False)
    edge = [
        torch.zeros(cols),
        torch.where(k == cols // 3, torch.tensor(64.0), torch.tensor(0.0)),  # one non-zero
        torch.where(k == 0, torch.tensor(-0.0), base),  # a -0.0 among ordinary values
        torch.where(k == cols // 2, torch.tensor(128.0 if finite else float("inf")), base),
        torch.where(k == cols - 1, torch.tensor(-128.0 if finite else float("nan") if recipe.get("nan_row", True) else float("inf")), base),
        torch.full((cols,), 3.0),  # constant
    ]
    assert len(edge) == EDGE_ROWS
    for r, e in enumerate(edge[: flat.shape[0]]):
        flat[r] = e.to(dtype)
    return x


def case_list():
    """[(key, recipe)]: recipe = preset, dtype, shape, size (the rotation block n), salt, gs (NVFP4 global-scale name or None), nan_row,
    and `finite: true` for the twins without a +inf or NaN row"""
    out = []
    dts = list(DTYPES)

    def add(preset, dt, shape, size, gs=None, finite=False):
        group = PRESETS[preset].get("group_size")
        if group and shape[-1] % group:
            return
        if preset == "nvfp4" and gs is None:
            gs = "nogs"
        key = f"{preset}.{dt}.{'x'.join(map(str, shape))}.n{size}" + (f".{gs}" if gs else "") + (".finite" if finite else "")
        if key in dict(out):
            return
        out.append((key, dict(preset=preset, dtype=dt, shape=list(shape), size=size, salt=len(out) % 11 + 1, gs=gs,
                              nan_row=not (preset in ("mxfp4", "mxfp8") and size < 32),  # a half-NaN MX group: module docstring
                              **({"finite": True} if finite else {}))))

    kinds = ["fp8_token", "int8_token", "fp8_group128", "nvfp4", "mxfp4", "mxfp8", "int8_token_asym", "int4_group32_asym"]
    # n <= 512 with in-wave segments (groups, short token rows); every kind, bf16 always and a second dtype in rotation
    small = [(8, (2, 4, 64)), (16, (2, 4, 64)), (32, (1, 8, 128)), (64, (2, 4, 128)), (128, (2, 4, 256)), (256, (1, 8, 256)), (512, (1, 8, 512))]
    for i, (n, shape) in enumerate(small):
        for j, p in enumerate(kinds):
            for dt in sorted({"bf16", dts[(i + j) % 3]}):
                add(p, dt, shape, n)
                if p == "nvfp4":
                    add(p, dt, shape, n, "gs")
    add("nvfp4", "bf16", (2, 4, 128), 64, "gsbig")
    for p in ("fp8_token", "nvfp4", "int8_token_asym"):  # 4-D: the token row is dims >= 2
        add(p, "bf16", (2, 2, 4, 64), 64, "gs" if p == "nvfp4" else None)
        add(p, "f16", (1, 3, 3, 128), 32, "gs" if p == "nvfp4" else None)
    # n = 1024 .. 8192: one workgroup per block; groups are reduced in the wave, a token row of n elements across the waves
    for i, n in enumerate((1024, 2048, 4096, 8192)):
        for j, p in enumerate(kinds):
            add(p, dts[(i + j) % 3], (1, 9, n), n, "gs" if p == "nvfp4" else None)
    for p in ("fp8_token", "fp8_group128", "nvfp4", "int8_token"):
        add(p, "bf16", (1, 8, 1024), 1024)
    add("fp8_group128", "bf16", (9, 8192), 8192)  # 2-D: groups do not need a token dimension
    add("mxfp4", "f16", (3, 2, 2, 2048), 1024)  # two blocks per row, 4-D
    # a token row of head-dim blocks (row lengths that are not powers of two)
    for n in (128, 512):
        for j, p in enumerate(("fp8_token", "int8_token", "int8_token_asym")):
            add(p, ("bf16", "f16")[j % 2], (1, 9, 14336), n)
        add("fp8_group128", "bf16", (1, 9, 14336), n)
    add("fp8_token", "bf16", (2, 4, 1024), 128)
    add("int8_token", "bf16", (1, 8, 1024), 64)
    add("fp8_token", "f32", (2, 4, 1536), 512)
    add("int8_token_asym", "f16", (1, 7, 11008), 64)
    add("fp8_token", "bf16", (1, 2, 32768), 256)  # the longest staged row
    add("fp8_token", "bf16", (2, 4, 192), 64)  # a short row that is not 8 * 2^k
    # declined shapes: two or three launches, the same results
    add("fp8_token", "bf16", (9, 4096), 128)  # token on a 2-D input: one segment, the tensor form
    add("fp8_tensor", "bf16", (1, 9, 1024), 64)
    add("fp8_token", "bf16", (1, 9, 4096), 1024)  # a token row of several workgroup-sized blocks
    add("int8_token", "f16", (1, 9, 2048), 1024)
    add("fp8_token", "bf16", (1, 2, 65536), 128)  # a row longer than the staged form
    # the tensor form on finite values: the two cases above whose one scale is NaN, without their +inf and NaN rows
    add("fp8_token", "bf16", (9, 4096), 128, finite=True)
    add("fp8_tensor", "bf16", (1, 9, 1024), 64, finite=True)
    return out


# what plan_rotated_dynamic must say for the declined cases above (every other case fuses)
DECLINED = {
    "fp8_token.bf16.9x4096.n128": 3,
    "fp8_tensor.bf16.1x9x1024.n64": 3,
    "fp8_token.bf16.1x9x4096.n1024": 2,
    "int8_token.f16.1x9x2048.n1024": 2,
    "fp8_token.bf16.1x2x65536.n128": 2,
    "fp8_token.bf16.9x4096.n128.finite": 3,
    "fp8_tensor.bf16.1x9x1024.n64.finite": 3,
}


def stored(recipe) -> bool:
    """the small bfloat16 cases keep the reference's tensors; every case keeps its recipe and the sha256 of input and outputs"""
    return recipe["dtype"] == "bf16" and math.prod(recipe["shape"]) <= 2048


def by_value(t: torch.Tensor) -> torch.Tensor:
    """every zero rewritten to +0.0 and every NaN to one canonical NaN (float8 as its bytes)"""
    t = t.detach().cpu().contiguous()
    if t.dtype in (F32, F16, BF16):
        t = torch.where(t == 0, torch.zeros_like(t), t)
        t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t)
    elif t.dtype == F8:
        t = t.view(torch.uint8)
    if t.dtype == torch.uint8:  # float8 bytes (a uint8 zero point is all zeros: untouched)
        t = torch.where(t == 0x80, torch.zeros_like(t), t)
        t = torch.where((t & 0x7F) == 0x7F, torch.full_like(t, 0x7F), t)
    return t


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(by_value(t).view(torch.uint8).numpy().tobytes()).hexdigest()


def equal_by_value(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = by_value(a), by_value(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
