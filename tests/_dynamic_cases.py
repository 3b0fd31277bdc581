"""The case matrix of the dynamic activation QDQ fixtures (tools/gen_golden_dynamic.py writes them, tests/test_gpu_dynamic_quant.py
and tests/test_dynamic_quant.py read them).  Inputs are synthesised from integer formulas, so a case is fully described by its
recipe (`make_input`).  Every case keeps the sha256 of its input and of the reference's outputs; the small bfloat16 cases also keep
the reference's outputs themselves (to show where a mismatch is).

`synth` writes its edge rows (zeros, +-0, subnormals, +-inf, NaN, 448, the dtype's maximum) into the first rows of every input.
Rows are independent under a per-row or per-group scale, but where the whole tensor is ONE segment (the tensor strategy, token
on a 1-D / 2-D input) the NaN row makes scale and output all NaN: those cases pin NaN propagation and nothing else.  The
recipes marked `finite` have no edge rows, so the one scale is a finite number and the output takes many values; `plant` puts
the extremes that decide it at a chosen flat index."""
import hashlib
import math

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


PLANT_MAX, PLANT_OTHER = 200.0, 152.0  # exact in every dtype, above every body value (|mant| <= 8 times at most 2^4)
PLANT_APART = 8 * 256  # elements one workgroup of dyn_partial_kernel reads per step: the next workgroup's partial
PLANT_AT = {"first": lambda n: 0, "last": lambda n: n - 1, "middle": lambda n: n // 2 + 3}


def make_input(recipe):
    """The input of a recipe: synth(shape, dtype, salt), changed by the optional keys
      finite: true                   the body formula only: eight extra leading rows take synth's edge rows and are dropped, so no
                                     value is non-finite and none is the dtype's maximum
      plant: first | last | middle   (finite recipes) the element of largest magnitude, +-PLANT_MAX, at flat index 0, numel - 1
                                     (inside a ragged tail unit) or numel // 2 + 3; an asymmetric preset gets the other extreme,
                                     -+PLANT_OTHER, PLANT_APART elements further on (cyclically): in another partial of the tensor form"""
    shape, dtype, salt = tuple(recipe["shape"]), DTYPES[recipe["dtype"]], recipe["salt"]
    if not recipe.get("finite"):
        assert not recipe.get("plant")
        return synth(shape, dtype, salt)
    cols = shape[-1]
    x = synth((math.prod(shape) // cols + 8, cols), dtype, salt)[8:].clone().reshape(shape)
    if recipe.get("plant"):
        flat = x.reshape(-1)
        n = flat.numel()
        at = PLANT_AT[recipe["plant"]](n)
        sign = -1.0 if salt % 2 else 1.0
        flat[at] = PLANT_MAX * sign
        if not PRESETS[recipe["preset"]]["symmetric"]:
            flat[(at + PLANT_APART) % n] = -PLANT_OTHER * sign
    return x


def tensor_form(recipe) -> bool:
    """the whole tensor is one segment: the tensor strategy, and token on a 1-D / 2-D input"""
    st = PRESETS[recipe["preset"]]["strategy"]
    return st == "tensor" or (st == "token" and len(recipe["shape"]) <= 2)


def case_list():
    """[(key, recipe)]: recipe = preset, dtype, shape, salt, gs (NVFP4 global-scale name or None), and make_input's optional keys"""
    out = []

    def add(preset, dt, shape, salt, gs=None, **extra):
        key = f"{preset}.{dt}.{'x'.join(map(str, shape))}" + (f".{gs}" if gs else "")
        key += "".join(f".{k if v is True else v}" for k, v in extra.items())
        assert key not in dict(out), key
        out.append((key, dict(preset=preset, dtype=dt, shape=list(shape), salt=salt, gs=gs, **extra)))

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

    # ---- finite inputs: the whole tensor as one segment, with a scale that is a number -------------------------------------------------
    dts = list(DTYPES)
    whole_presets = ("fp8_tensor", "int8_tensor_asym", "fp8_token", "int8_token", "int8_token_asym")

    def whole(p, shape):  # token is the whole tensor only on a 2-D input: the same elements, the same last dimension
        return shape if PRESETS[p]["strategy"] == "tensor" else (math.prod(shape[:-1]), shape[-1])

    # one launch (ct_dynamic_qdq, <= 512 elements): 15 a ragged segment, 64 and 512 in-wave segments of 8 and 64 lanes;
    # the tensor entry: one partial (2048; 513: numel % 8 = 1), three partials (36864; 33033: numel % 8 = 1)
    shapes = [(1, 3, 5), (4, 16), (2, 4, 64), (8, 256), (3, 171), (9, 4096), (33, 1001)]
    for i, p in enumerate(whole_presets):
        for j, shape in enumerate(shapes):
            add(p, dts[(i + j) % 3], whole(p, shape), 11 + j, finite=True)
        for j, plant in enumerate(PLANT_AT):
            add(p, dts[(i + j + 1) % 3], (33, 1001), 21 + j, finite=True, plant=plant)
    # above both caps of the tensor entry (CT_DYNAMIC_PARTS = 1024 partials of 256 x 8 units, kCUs * 8 = 2048 workgroups of 256 x 4
    # units: 16 777 216 elements each), numel % 8 = 7
    big = (4099, 4101)
    add("fp8_tensor", "bf16", big, 41, finite=True, plant="last")
    add("fp8_tensor", "f16", big, 42, finite=True, plant="middle")
    add("int8_tensor_asym", "f16", big, 43, finite=True, plant="last")
    add("int8_token", "f32", big, 44, finite=True, plant="middle")
    # the tensor strategy does not look at the dimensions
    for p in ("fp8_tensor", "int8_tensor_asym"):
        for dt in DTYPES:
            for s_i, shape in enumerate([(2, 4, 256), (2, 2, 4, 128)]):
                add(p, dt, shape, 51 + s_i, finite=True)
    # the other widths' qmin / qmax in the tensor form
    for b in range(2, 8):
        add(f"int{b}_token_asym", dts[b % 3], (8, 256), 60 + b, finite=True)

    # ---- token rows: ragged lengths (the scalar loads and stores; edge rows kept: rows are independent), segments of one and of
    # eight lanes, and the rows past the staged form (32768 elements) that are read twice ------------------------------------------------
    row_presets = ("fp8_token", "int8_token", "int8_token_asym")
    for j, L in enumerate((7, 8, 64, 100, 4100, 32776, 32772)):
        for i, p in enumerate(row_presets):
            if L % 8:
                add(p, dts[(i + j) % 3], (2, 5, L), 71 + j)
            else:
                add(p, dts[(i + j) % 3], (1, 3, L), 71 + j, finite=True)
    for j, L in enumerate((7, 100, 4100, 32772)):
        add("int4_token_asym", dts[(2 + j) % 3], (2, 5, L), 81 + j)
    add("int8_token_asym", "f16", (1, 3, 65536), 91, finite=True)
    add("fp8_token", "f32", (1, 3, 65536), 92, finite=True)
    # more than 2^20 segments: the grid-stride loop of dyn_seg_kernel, in its vector and in its scalar form
    add("fp8_token", "bf16", (1025, 1024, 24), 93, finite=True)
    add("int8_token_asym", "f16", (1025, 1024, 7), 94)
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
