"""The case matrix of the random-hadamard fixtures (tools/gen_golden_random_hadamard.py writes them, tests/test_random_hadamard.py
and tests/test_gpu_random_hadamard.py read them).  The tiers are those of tests/_hadamard_cases.py:

  tier A  online, float32: integers |x| <= 128.  n * 128 < 2^24 up to n = 28672, so every summation order is exact — the matrix
          cores' included — and the reference's GEMM result is the one result: compared in every element, by value.
  tier B  online, float32: seeded randn * s, against the derived bound `bound()` around a float64 evaluation.
  tier C  offline, float64: grid (k * 2^-14) and randn * 0.02 weights in bf16 / fp16: compared in every element.

The weight of size n is upstream's `random_hadamard_matrix(n, ..., gen=Generator().manual_seed(n))`.  The fixtures keep its
factors (tests/golden/random_hadamard.safetensors: `had_k.<n>` int8 K x K — absent when K == 1 — and `signs.<n>` int8) and, for
n <= 96, the weight itself; `weight_from_factors` rebuilds any other one."""
import math

import torch
from _hadamard_cases import BF16, DTYPES, F16, F32, F64, FLOOR, ULP, sha, synth  # noqa: F401  (re-exported for the tests)

# n: (K, M).  K a multiple of 32: 224, 160, 192; K a multiple of 4 only: 172, 148, 140; M = 8 ... 128; K == 1 with signs
SIZES = {
    1792: (224, 8), 14336: (224, 64), 28672: (224, 128), 2560: (160, 16), 5120: (160, 32), 3072: (192, 16),
    1376: (172, 8), 11008: (172, 64), 2368: (148, 16), 18944: (148, 128), 4480: (140, 32),
    40: (40, 1), 96: (96, 1),
    64: (1, 64), 128: (1, 128), 4096: (1, 4096), 8192: (1, 8192),
}
FULL_WEIGHT_MAX = 96
REAL = (11008, 14336, 18944, 28672)  # the MLP sizes of the issue: a few rows each


def sylvester(m, dtype=F64):
    i = torch.arange(m)
    bits, parity = i[:, None] & i[None, :], torch.zeros(m, m, dtype=torch.int64)
    while bool(bits.any()):
        parity ^= bits & 1
        bits = bits >> 1
    return (1 - 2 * parity).to(dtype)


def weight_from_factors(n, had_k, signs, dtype=F32):
    """signs[:, None] * kron(had_k, H_M).T"""
    k = 1 if had_k is None else had_k.shape[0]
    hk = torch.ones(1, 1, dtype=dtype) if had_k is None else had_k.to(dtype)
    return signs.to(dtype)[:, None] * torch.kron(hk, sylvester(n // k, dtype)).t()


def structured(x, n, had_k, signs, transposed=False, dim=-1, acc=F64, cast=True):
    """value @ W / sqrt(n) (W.T when transposed) along dim, evaluated from the factors in `acc`: signs, a butterfly over M, the
    K x K mix, ONE division by fl(sqrt n) in acc"""
    k = 1 if had_k is None else had_k.shape[0]
    m = n // k
    v = x.to(acc).movedim(dim, -1)
    shape = v.shape
    v = v.reshape(-1, k, m)
    s = signs.to(acc).reshape(k, m)
    if not transposed:
        v = v * s
    h = 1
    while h < m:
        v = v.reshape(-1, k, m // (2 * h), 2, h)
        v = torch.stack((v[:, :, :, 0] + v[:, :, :, 1], v[:, :, :, 0] - v[:, :, :, 1]), dim=3)
        h *= 2
    v = v.reshape(-1, k, m)
    if had_k is not None:
        hk = had_k.to(acc)
        v = torch.einsum("pk,bkt->bpt", hk.t() if transposed else hk, v)
    if transposed:
        v = v * s
    v = (v.reshape(shape) / torch.tensor(n, dtype=F64).sqrt().to(acc)).movedim(-1, dim)
    return v.to(x.dtype) if cast else v


def bound(x, n, had_k, signs, transposed=False, dim=-1):
    """tier B: (exact, tolerance) per element.  exact = the float64 evaluation; tolerance = E + u * (|exact| + E) + f with
    E = (K + log2 M + 2) * 2^-23 * sum|x_i| / sqrt(n): twice the first-order bound of a K-term recursive sum followed by log2 M
    pairwise levels, plus the division; u one rounding to the output dtype; f the fp16 subnormal floor.  Derived, not measured."""
    k = 1 if had_k is None else had_k.shape[0]
    exact = structured(x, n, had_k, signs, transposed, dim, F64, cast=False)
    sums = x.to(F64).abs().movedim(dim, -1)
    shape = sums.shape
    sums = sums.reshape(-1, n).sum(-1, keepdim=True).expand(-1, n).reshape(shape).movedim(-1, dim)
    E = (k + math.log2(n // k) + 2) * 2.0 ** -23 * sums / math.sqrt(n)
    return exact, E + ULP[x.dtype] * (exact.abs() + E) + FLOOR[x.dtype]


def dim_of(recipe) -> int:
    return 0 if (recipe["module"], recipe["location"]) in (("Linear", "weight_output"), ("Embedding", "weight_input")) else -1


def transposed_of(recipe) -> bool:
    """value @ W.T for Linear / Embedding weight_input, value @ W otherwise; `inverse` selects the other one"""
    return (recipe["location"] == "weight_input") != bool(recipe["inverse"])


def precision_of(recipe) -> torch.dtype:
    return F64 if recipe["location"] in ("weight_input", "weight_output") else F32


def case_list():
    """[(key, recipe)]: recipe = tier, gen, dtype, shape, size, location, module, inverse, salt, scale.  An online case with
    inverse=True is the transposed form on an activation."""
    out = []

    def add(tier, gen, dt, shape, size, location="input", module="Linear", inverse=False, salt=0, scale=None, tag=""):
        key = f"{tier}.{gen}{tag}.{dt}.{'x'.join(map(str, shape))}.n{size}.{module}.{location}" + (".inv" if inverse else "")
        assert key not in dict(out), key
        out.append((key, dict(tier=tier, gen=gen, dtype=dt, shape=list(shape), size=size, location=location, module=module,
                              inverse=inverse, salt=salt, scale=scale)))

    # tiers A and B: every size, plain and transposed, three dtypes; the real sizes with 3 rows, the others with row counts that
    # do not fill a group of blocks, and a 3-D activation
    for i, n in enumerate(SIZES):
        for j, dt in enumerate(DTYPES):
            rows = 3 if n in REAL else (1, 5, 67)[(i + j) % 3] if n <= 4096 else (2, 3, 9)[(i + j) % 3]
            for inverse in (False, True):
                add("A", "ints", dt, (rows, n), n, inverse=inverse, salt=i + 1)
                s = (0.02, 1.0, 30.0)[(i + j) % 3]
                add("B", "randn", dt, (rows, n), n, inverse=inverse, salt=100 + 3 * i + j, scale=s, tag=f"{s:g}")
            if n <= 5120:
                add("A", "ints", dt, (2, 3, 2 * n), n, location="output", salt=i + 2)  # head_dim blocks: two blocks per row
    # tier C: every fused location of Linear and Embedding, inverse both ways, bf16 / fp16, both weight kinds, at a size of each
    # form of the mix: 1376 (K = 172, pads), 1792 (K = 224), 96 (M = 1), 128 (K == 1)
    for gen, scale in (("grid", None), ("randn", 0.02)):
        for dt in ("bf16", "f16"):
            for module in ("Linear", "Embedding"):
                for location in ("weight_input", "weight_output"):
                    for inverse in (False, True):
                        for n in (1376, 96, 128) if gen == "grid" else (1792,):
                            other = 24
                            shape = (n, other) if dim_of(dict(module=module, location=location)) == 0 else (other, n)
                            add("C", gen, dt, shape, n, location, module, inverse, salt=7 + len(out), scale=scale)
            add("C", gen, dt, (1376, 1), 1376, "weight_output", "Linear", salt=11 + len(out), scale=scale, tag="bias")  # bias.unsqueeze(-1)
    for location in ("weight_input", "weight_output"):  # a real size at the weight's twin of the online rotation
        add("C", "randn", "bf16", (16, 14336) if location == "weight_input" else (14336, 16), 14336, location, salt=40, scale=0.02)
        add("C", "grid", "f16", (8, 8192) if location == "weight_input" else (8192, 8), 8192, location, salt=41)
    return out


def stored(recipe) -> bool:
    """the small cases keep the reference's output itself; every case of tiers A and C keeps its sha256"""
    return recipe["tier"] != "B" and math.prod(recipe["shape"]) <= 512


# the model of the apply_transform_config tests: weight_output (with the bias) on the first Linear in one group; the online
# rotation in front of the second Linear and its inverse folded into that weight in two more (upstream keeps ONE weight per group
# and size, at the precision of its first use: a group that mixed an online and a fused location of one size would run the fused
# one in float32 upstream, in float64 here)
MODEL_SIZE = 1376
MODEL_CONFIG = {
    "config_groups": {
        "u": {"type": "random-hadamard", "apply": [{"targets": ["0"], "location": "weight_output", "inverse": False, "ignore": []}],
              "randomize": False, "requires_grad": False, "head_dim": None, "precision": "torch.float32"},
        "v": {"type": "random-hadamard", "apply": [{"targets": ["1"], "location": "input", "inverse": False, "ignore": []}],
              "randomize": False, "requires_grad": False, "head_dim": None, "precision": "torch.float32"},
        "w": {"type": "random-hadamard", "apply": [{"targets": ["1"], "location": "weight_input", "inverse": True, "ignore": []}],
              "randomize": False, "requires_grad": False, "head_dim": None, "precision": "torch.float32"},
    }
}


def model(dtype=BF16):
    """Linear(16 -> 1376, bias) then Linear(1376 -> 8): grid weights from the integer hash"""
    n = MODEL_SIZE
    m = torch.nn.Sequential(torch.nn.Linear(16, n, bias=True, dtype=dtype), torch.nn.Linear(n, 8, bias=False, dtype=dtype))
    dt = {v: k for k, v in DTYPES.items()}[dtype]
    with torch.no_grad():
        m[0].weight.copy_(synth(dict(gen="grid", dtype=dt, shape=[n, 16], salt=61)))
        m[0].bias.copy_(synth(dict(gen="grid", dtype=dt, shape=[n], salt=62)))
        m[1].weight.copy_(synth(dict(gen="grid", dtype=dt, shape=[8, n], salt=63)))
    return m.requires_grad_(False)
