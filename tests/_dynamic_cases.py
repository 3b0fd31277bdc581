"""The case matrix of the dynamic activation QDQ fixtures (tools/gen_golden_dynamic.py writes them, tests/test_gpu_dynamic_quant.py
and tests/test_dynamic_quant.py read them).  Inputs are synthesised from integer formulas, so a case is fully described by its
recipe.  Every case keeps the sha256 of its input and of the reference's outputs; the small bfloat16 cases also keep the
reference's outputs themselves (to show where a mismatch is)."""
import hashlib

import torch

F32, BF16, F16, F8 = torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn
DTYPES = {"bf16": BF16, "f16": F16, "f32": F32}

# the activation arguments of the presets (quantization/quant_scheme.py), plus asymmetric INT and the tensor strategy
PRESETS = {
    "fp8_token": dict(num_bits=8, type="float", strategy="token", symmetric=True, dynamic=True),  # FP8_DYNAMIC, W4AFP8
    "int8_token": dict(num_bits=8, type="int", strategy="token", symmetric=True, dynamic=True),  # INT8_W8A8
    "fp8_group128": dict(num_bits=8, type="float", strategy="group", group_size=128, symmetric=True, dynamic=True),  # FP8_BLOCK
    "nvfp4": dict(num_bits=4, type="float", strategy="tensor_group", group_size=16, symmetric=True, dynamic="local",
                  scale_dtype=F8, zp_dtype=F8),  # NVFP4
    "mxfp4": dict(num_bits=4, type="float", strategy="group", group_size=32, symmetric=True, dynamic=True, scale_dtype=torch.uint8,
                  zp_dtype=torch.uint8),
    "mxfp8": dict(num_bits=8, type="float", strategy="group", group_size=32, symmetric=True, dynamic=True, scale_dtype=torch.uint8,
                  zp_dtype=torch.uint8),
    "fp8_tensor": dict(num_bits=8, type="float", strategy="tensor", symmetric=True, dynamic=True),
    "int8_tensor_asym": dict(num_bits=8, type="int", strategy="tensor", symmetric=False, dynamic=True),
    "int4_group32_asym": dict(num_bits=4, type="int", strategy="group", group_size=32, symmetric=False, dynamic=True),
    **{f"int{b}_token_asym": dict(num_bits=b, type="int", strategy="token", symmetric=False, dynamic=True) for b in range(2, 9)},
}
# NVFP4 runs with these global scales: none, a plain one, and one that pushes global_scale * scale past the e4m3 range
NVFP4_GLOBAL = {"nogs": None, "gs": 37.5, "gsbig": 30000.0}


def global_scale_of(name):
    v = NVFP4_GLOBAL[name]
    return None if v is None else torch.tensor([v], dtype=F32)


def synth(shape, dtype, salt):
    """values of every magnitude class from an integer hash of the flat index; the first rows of the last dim are edge rows"""
    n = 1
    for d in shape:
        n *= d
    i = torch.arange(n, dtype=torch.int64)
    h = ((i * 2654435761 + salt * 40503) ^ (i >> 7) * 97) & 0xFFFFFFFF
    mant = ((h & 0xFFFF) - 32768).to(torch.float64) / 4096.0  # [-8, 8)
    row = i // shape[-1]
    expo = ((row * 7 + salt) % 9 - 4).to(torch.float64)  # rows in 2^-4 .. 2^4
    x = (mant * torch.pow(2.0, expo)).to(dtype).reshape(shape)
    flat = x.reshape(-1, shape[-1])
    cols = shape[-1]
    fi = torch.finfo(dtype)
    edge = [
        torch.zeros(cols),  # all zeros: the eps scale
        torch.tensor([(-0.0 if k % 2 else 0.0) for k in range(cols)]),  # +-0
        torch.full((cols,), fi.smallest_normal / 4).to(dtype).float() * torch.tensor([(-1.0) ** k for k in range(cols)]),  # subnormal maxima
        torch.where(torch.arange(cols) == cols // 2, torch.tensor(float("inf")), mant[:cols].float()),  # +inf
        torch.where(torch.arange(cols) == 1, torch.tensor(float("-inf")), mant[:cols].float()),  # -inf
        torch.where(torch.arange(cols) == cols - 1, torch.tensor(float("nan")), mant[:cols].float()),  # NaN
        # amax 448 -> FP8 scale 1: the other values sit on FP8 / E2M1 rounding midpoints
        torch.tensor([448.0 if k == 0 else (1.0 + 1 / 16 + (k % 8) / 8) * (2.0 ** (k % 5 - 2)) * (-1) ** k for k in range(cols)]),
        torch.tensor([fi.max if k == 0 else fi.tiny * (k + 1) for k in range(cols)]),  # E8M0 clamp extremes (largest / tiniest)
    ]
    for r, e in enumerate(edge[: flat.shape[0]]):
        flat[r] = e.to(dtype)
    # one canonical NaN: the reference's MX scale of a NaN group depends on the NaN's payload (round_to_power_2 adds to the bits),
    # which the kernels do not model (NaN payload and sign are not compared)
    return x.masked_fill_(torch.isnan(x), float("nan"))


def case_list():
    """[(key, recipe)]: recipe = preset, dtype, shape, salt, gs (NVFP4 global-scale name or None)"""
    out = []

    def add(preset, dt, shape, salt, gs=None):
        key = f"{preset}.{dt}.{'x'.join(map(str, shape))}" + (f".{gs}" if gs else "")
        out.append((key, dict(preset=preset, dtype=dt, shape=list(shape), salt=salt, gs=gs)))

    shapes = [(8, 256), (2, 4, 256), (2, 2, 4, 128)]  # 2-D (token: the whole tensor), 3-D, 4-D
    for p in PRESETS:
        for dt in DTYPES:
            for s_i, shape in enumerate(shapes):
                if p == "nvfp4":
                    for g in NVFP4_GLOBAL:
                        add(p, dt, shape, 3 * s_i + 1, g)
                else:
                    add(p, dt, shape, 3 * s_i + 2)
    # row lengths 16 ... 32768 (bf16 and fp16, the presets' strategies)
    for p in ("fp8_token", "int8_token", "int8_token_asym", "fp8_group128", "nvfp4", "mxfp4"):
        for L in (16, 48, 4096, 18432, 28672, 32768):
            if p in ("fp8_group128",) and L % 128:
                continue
            if p in ("nvfp4", "mxfp4") and L % 32:
                continue
            for dt in ("bf16", "f16"):
                add(p, dt, (1, 9, L), L % 97, "gs" if p == "nvfp4" else None)
    return out


def stored(recipe) -> bool:
    """the small bfloat16 cases keep the reference's outputs; every case keeps its recipe and the sha256 of input and outputs"""
    n = 1
    for d in recipe["shape"]:
        n *= d
    return n <= 4096 and recipe["dtype"] == "bf16"


def canonical_bytes(t: torch.Tensor) -> bytes:
    """raw bytes with every NaN rewritten to one canonical NaN (NaN payload and sign are not compared)"""
    t = t.detach().cpu().contiguous()
    if t.dtype in (F32, F16, BF16):
        t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t)
    if t.dtype == F8:
        t = t.view(torch.uint8)
        t = torch.where((t & 0x7F) == 0x7F, torch.full_like(t, 0x7F), t)
    return t.view(torch.uint8).numpy().tobytes()


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(canonical_bytes(t)).hexdigest()
