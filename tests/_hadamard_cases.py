"""The case matrix of the Hadamard rotation fixtures (tools/gen_golden_hadamard.py writes them, tests/test_hadamard.py and
tests/test_gpu_hadamard.py read them).  A case is fully described by its recipe: inputs are synthesised from integer formulas
(tiers A and C "grid") or from a seeded CPU generator (tier B, tier C "randn"), and every case keeps the sha256 of its input.

  tier A  online, float32: integer-valued inputs (|k| <= 128).  Every partial sum is an integer below 2^24, so every summation
          order is exact and the reference's GEMM result is the one result: compared in every element, by value.
  tier B  online, float32: seeded randn * s.  No reference output is kept: GEMM and butterfly differ in the last bit of the
          float32 sum, so the check is the derived bound `bound()` against a float64 butterfly (the generator asserts that the
          reference meets it on the same inputs).
  tier C  offline, float64 (what upstream uses for every fused location): grid weights k * 2^-14 and randn * 0.02 weights in
          bf16 / fp16.  Sums of 16-bit floats of ordinary exponent spread are exact in float64: compared in every element.

Floats are compared BY VALUE: a row of -0.0 comes out of a GEMM as +0.0 and out of a butterfly as -0.0 in element 0 — the sign of
a zero result is a property of the BLAS, not of the transform.  `sha()` therefore rewrites every zero to +0.0 before hashing."""
import hashlib
import math

import torch

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
DTYPES = {"bf16": BF16, "f16": F16, "f32": F32}
SIZES = [2 ** k for k in range(1, 14)]  # 2 ... 8192
ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24}  # one output rounding
FLOOR = {BF16: 0.0, F16: 2.0 ** -25, F32: 0.0}  # the fp16 subnormal floor


def _hash(numel, salt):
    i = torch.arange(numel, dtype=torch.int64)
    return ((i * 2654435761 + salt * 40503) ^ ((i >> 7) * 97)) & 0xFFFFFFFF


def synth(recipe) -> torch.Tensor:
    shape, dtype = tuple(recipe["shape"]), DTYPES[recipe["dtype"]]
    numel = math.prod(shape)
    if recipe["gen"] == "ints":  # integers in [-128, 128]
        v = (_hash(numel, recipe["salt"]) % 257 - 128).to(F64)
    elif recipe["gen"] == "grid":  # k * 2^-14, |k| <= 4096
        v = (_hash(numel, recipe["salt"]) % 8193 - 4096).to(F64) * 2.0 ** -14
    else:  # "randn": seeded, scaled
        v = torch.randn(numel, generator=torch.Generator().manual_seed(recipe["salt"]), dtype=F32) * recipe["scale"]
    return v.to(dtype).reshape(shape)


def dim_of(recipe) -> int:
    """apply_transform_weight's dimension (transform/utils/matrix.py:97-121): dim 0 for Linear weight_output and Embedding
    weight_input, the last one for everything else"""
    return 0 if (recipe["module"], recipe["location"]) in (("Linear", "weight_output"), ("Embedding", "weight_input")) else -1


def precision_of(recipe) -> torch.dtype:
    return F64 if recipe["location"] in ("weight_input", "weight_output") else F32


def butterfly(x, n, dim=-1, acc=F32, cast=True):
    """FWHT over blocks of n along dim, accumulated in `acc`, ONE division by sqrt(n) in acc, cast to x's dtype"""
    v = x.to(acc).movedim(dim, -1)
    shape = v.shape
    h = 1
    while h < n:
        v = v.reshape(-1, n // (2 * h), 2, h)
        v = torch.stack((v[:, :, 0] + v[:, :, 1], v[:, :, 0] - v[:, :, 1]), dim=2)
        h *= 2
    v = (v.reshape(shape) / torch.tensor(n, dtype=F64).sqrt().to(acc)).movedim(-1, dim)
    return v.to(x.dtype) if cast else v


def bound(x, n, dim=-1):
    """tier B: (exact, tolerance) per element.  exact = float64 butterfly; tolerance = E + u * (|exact| + E) + f with
    E = (log2 n + 2) * 2^-23 * sum|x_i| / sqrt(n): twice the first-order pairwise-summation bound log2 n * 2^-24 * sum|x_i|
    plus the division; u one rounding to the output dtype; f the fp16 subnormal floor.  Derived, not measured."""
    exact = butterfly(x, n, dim, F64, cast=False)
    sums = butterfly(x.abs(), 1, dim, F64, cast=False).movedim(dim, -1)
    shape = sums.shape
    sums = sums.reshape(-1, n).sum(-1, keepdim=True).expand(-1, n).reshape(shape).movedim(-1, dim)
    E = (math.log2(n) + 2) * 2.0 ** -23 * sums / math.sqrt(n)
    return exact, E + ULP[x.dtype] * (exact.abs() + E) + FLOOR[x.dtype]


def case_list():
    """[(key, recipe)]: recipe = tier, gen, dtype, shape, size, location, module, inverse, salt, scale"""
    out = []

    def add(tier, gen, dt, shape, size, location="input", module="Linear", inverse=False, salt=0, scale=None, tag=""):
        key = f"{tier}.{gen}{tag}.{dt}.{'x'.join(map(str, shape))}.n{size}.{module}.{location}" + (".inv" if inverse else "")
        assert key not in dict(out), key
        out.append((key, dict(tier=tier, gen=gen, dtype=dt, shape=list(shape), size=size, location=location, module=module,
                              inverse=inverse, salt=salt, scale=scale)))

    # tiers A and B: every power of two 2 ... 8192, three dtypes, 2-D with row counts that do not fill a workgroup, 3-D, head_dim blocks
    for i, n in enumerate(SIZES):
        for j, dt in enumerate(DTYPES):
            rows = (1, 3, 65)[(i + j) % 3]
            add("A", "ints", dt, (rows, n), n, salt=i + 1)
            add("A", "ints", dt, (2, 3, n), n, location="output", salt=i + 2)
            s = (0.02, 1.0, 30.0)[(i + j) % 3]
            add("B", "randn", dt, (rows, n), n, salt=100 + 3 * i + j, scale=s, tag=f"{s:g}")
    for n in (64, 128):
        for cols, rows in ((4096, 3), (8192, 65)):
            for dt in DTYPES:
                add("A", "ints", dt, (rows, cols), n, salt=n + cols)
                add("B", "randn", dt, (rows, cols), n, salt=200 + n + cols, scale=1.0, tag="1")
    for n in (256, 8192):  # every scale at a small and at the largest size
        for s in (0.02, 1.0, 30.0):
            for dt in DTYPES:
                add("B", "randn", dt, (2, 2, n), n, location="output", salt=300 + n, scale=s, tag=f"{s:g}")
    # tier C: every fused location of Linear and Embedding, inverse both ways, with / without head_dim (64), bf16 / fp16, both weight kinds
    for gen, scale in (("grid", None), ("randn", 0.02)):
        for dt in ("bf16", "f16"):
            for module in ("Linear", "Embedding"):
                for location in ("weight_input", "weight_output"):
                    for inverse in (False, True):
                        for size in (None, 64):
                            shape = (128, 256)
                            r = dict(module=module, location=location)
                            n = size or shape[dim_of(r)]
                            add("C", gen, dt, shape, n, location, module, inverse, salt=7 + len(out), scale=scale)
            add("C", gen, dt, (512, 1), 512, "weight_output", "Linear", salt=11 + len(out), scale=scale, tag="bias")  # bias.unsqueeze(-1)
            add("C", gen, dt, (512, 1), 128, "weight_output", "Linear", salt=13 + len(out), scale=scale, tag="bias")
    for location in ("weight_input", "weight_output"):  # by sha256 only
        add("C", "randn", "bf16", (1024, 2048), 2048 if location == "weight_input" else 1024, location, salt=40, scale=0.02)
        add("C", "grid", "f16", (1000, 2048), 2048 if location == "weight_input" else 8, location, salt=41)
        add("C", "randn", "bf16", (4096, 4096), 4096, location, salt=42, scale=0.02)
        add("C", "randn", "bf16", (8192, 520), 8192 if location == "weight_output" else 8, location, salt=43, scale=0.02)
    return out


def stored(recipe) -> bool:
    """the small cases keep the reference's output itself; every case of tiers A and C keeps its sha256"""
    return recipe["tier"] != "B" and math.prod(recipe["shape"]) <= 512


def sha(t: torch.Tensor) -> str:
    """sha256 of the raw bytes with every zero rewritten to +0.0 (x + 0.0 turns -0.0 into +0.0 and changes nothing else):
    equal hashes <=> equal by value in every element, for NaN-free tensors"""
    t = t.detach().cpu().contiguous().reshape(-1) + 0.0
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


# the two-layer model of the apply_transform_config tests: weight_output on the first Linear (with its bias), input + inverse
# weight_input on the second
MODEL_CONFIG = {
    "config_groups": {
        "u": {"type": "hadamard", "apply": [{"targets": ["0"], "location": "weight_output", "inverse": False, "ignore": []}],
              "randomize": False, "requires_grad": False, "head_dim": None, "precision": "torch.float32"},
        "v": {"type": "hadamard", "apply": [{"targets": ["1"], "location": "input", "inverse": False, "ignore": []},
                                            {"targets": ["1"], "location": "weight_input", "inverse": True, "ignore": []}],
              "randomize": False, "requires_grad": False, "head_dim": 64, "precision": "torch.float32"},
    }
}


def model(dtype=BF16):
    """Linear(64 -> 128, bias) then Linear(128 -> 32): grid weights from the integer hash"""
    m = torch.nn.Sequential(torch.nn.Linear(64, 128, bias=True, dtype=dtype), torch.nn.Linear(128, 32, bias=False, dtype=dtype))
    dt = {v: k for k, v in DTYPES.items()}[dtype]
    with torch.no_grad():
        m[0].weight.copy_(synth(dict(gen="grid", dtype=dt, shape=[128, 64], salt=51)))
        m[0].bias.copy_(synth(dict(gen="grid", dtype=dt, shape=[128], salt=52)))
        m[1].weight.copy_(synth(dict(gen="grid", dtype=dt, shape=[32, 128], salt=53)))
    return m.requires_grad_(False)
