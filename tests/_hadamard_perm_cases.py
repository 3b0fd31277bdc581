"""The case matrix of the permuted-rotation fixtures (`TransformScheme.randomize=True`; tools/gen_golden_hadamard_perm.py writes
them, tests/test_hadamard_perm.py and tests/test_gpu_hadamard_perm.py read them).  The tiers are those of tests/_hadamard_cases.py:

  tier A  online, float32: integers |x| <= 128 — every summation order is exact, the reference's GEMM result is the one result
  tier C  offline, float64: grid (k * 2^-14) and randn * 0.02 weights in bf16 / fp16

Both compared in every element, by value.  Random inputs have no reference output: the GPU tests compare the one launch with the
composition bit for bit, and both with `bound()` around the float64 evaluation of the gathered input.

The reference is upstream's own factory: `TransformFactory.from_scheme(scheme(randomize=True), name=..., seed=S)`, one factory per
(type, size), which draws `perm = torch.randperm(n, generator=factory.generator)` at the first transform of that size — for
`random-hadamard` right after the weight, from the same generator.  S = PERM_SEED + n for the `hadamard` type and S = n for
`random-hadamard`, so that the weight is the one tests/golden/random_hadamard.safetensors already holds the factors of.  The
fixtures keep every drawn permutation (`perm.<type>.<n>`, int16) and the reference's output of the small cases.

The identity: with q = argsort(p) and G_i(v)[j] = v[i[j]],  T_{W[p][:, p]}(x) = G_p(T_W(G_q(x)))  for every location and inverse."""
import math

import torch
from _hadamard_cases import BF16, DTYPES, F16, F32, F64, bound, butterfly, sha, synth  # noqa: F401  (re-exported for the tests)
from _random_hadamard_cases import SIZES, structured  # noqa: F401

PERM_SEED = 1000
GROUP_SIZES = (2, 4, 8, 16, 64, 128, 512)  # hadp_group_kernel
BLOCK_SIZES = (1024, 2048, 4096, 8192, 16384)  # hadp_block_kernel
RANDOM_K1 = (64, 128, 4096, 8192)  # random-hadamard with K == 1: the signs ride in the permuted launch
RANDOM_K = (96, 1792)  # K > 1: the composition
MODEL_SEED = 7


def seed_of(kind, n) -> int:
    return PERM_SEED + n if kind == "hadamard" else n


def gather(x, index, n, dim=-1):
    """G_index over every block of n along dim"""
    d = dim % x.dim()
    return x.unflatten(d, (-1, n)).index_select(d + 1, index).flatten(d, d + 1)


def inverse_of(p):
    q = torch.empty_like(p)
    q[p] = torch.arange(p.numel(), dtype=p.dtype)
    return q


def dim_of(recipe) -> int:
    return 0 if (recipe["module"], recipe["location"]) in (("Linear", "weight_output"), ("Embedding", "weight_input")) else -1


def transposed_of(recipe) -> bool:
    return (recipe["location"] == "weight_input") != bool(recipe["inverse"])


def precision_of(recipe) -> torch.dtype:
    return F64 if recipe["location"] in ("weight_input", "weight_output") else F32


def restated(recipe, x, p, had_k=None, signs=None, cast=True):
    """G_p(T_W(G_q(x))) from this repository's restatements of T_W: `butterfly` for the hadamard type, `structured` for
    random-hadamard, in the accumulator of the location"""
    n, dim, acc = recipe["size"], dim_of(recipe), precision_of(recipe)
    g = gather(x, inverse_of(p), n, dim)
    if recipe["type"] == "hadamard":
        z = butterfly(g, n, dim, acc, cast)
    else:
        z = structured(g, n, had_k, signs, transposed_of(recipe), dim, acc, cast)
    return gather(z, p, n, dim)


def case_list():
    """[(key, recipe)]: recipe = type, tier, gen, dtype, shape, size, location, module, inverse, salt, scale"""
    out = []

    def add(kind, tier, gen, dt, shape, size, location="input", module="Linear", inverse=False, salt=0, scale=None, tag=""):
        key = f"{kind}.{tier}.{gen}{tag}.{dt}.{'x'.join(map(str, shape))}.n{size}.{module}.{location}" + (".inv" if inverse else "")
        assert key not in dict(out), key
        out.append((key, dict(type=kind, tier=tier, gen=gen, dtype=dt, shape=list(shape), size=size, location=location, module=module,
                              inverse=inverse, salt=salt, scale=scale)))

    H = "hadamard"
    # tier A: every size of both kernels in every dtype, row counts 1 / 3 / 65 (a few at the largest sizes)
    for i, n in enumerate(GROUP_SIZES + BLOCK_SIZES):
        for j, dt in enumerate(DTYPES):
            rows = (1, 3, 65)[(i + j) % 3] if n <= 4096 else (1, 3, 5)[(i + j) % 3]
            add(H, "A", "ints", dt, (rows, n), n, salt=i + 1)
    add(H, "A", "ints", "bf16", (3, 2), 2, salt=31)  # a partial last unit: 6 and 20 elements
    add(H, "A", "ints", "f32", (5, 4), 4, salt=32)
    for dt in DTYPES:  # head-dim blocks: the same permutation in every block of a row
        add(H, "A", "ints", dt, (3, 4096), 64, salt=33)
        add(H, "A", "ints", dt, (65, 1024), 128, salt=34)
    for n in (64, 1024):
        add(H, "A", "ints", "bf16", (2, 3, n), n, location="output", salt=35)
    # tier C: the column form (ragged transpose tiles, head_dim), the bias column, the row form with inverse both ways
    for gen, scale in (("grid", None), ("randn", 0.02)):
        for dt in ("bf16", "f16"):
            add(H, "C", gen, dt, (128, 256), 128, "weight_output", salt=41, scale=scale)
            add(H, "C", gen, dt, (256, 24), 64, "weight_output", salt=42, scale=scale)
            add(H, "C", gen, dt, (512, 1), 512, "weight_output", salt=43, scale=scale, tag="bias")
            add(H, "C", gen, dt, (512, 1), 128, "weight_output", salt=44, scale=scale, tag="bias")
            for inverse in (False, True):
                add(H, "C", gen, dt, (24, 256), 256, "weight_input", inverse=inverse, salt=45, scale=scale)
            add(H, "C", gen, dt, (256, 24), 256, "weight_input", "Embedding", salt=46, scale=scale)
    for i, n in enumerate(BLOCK_SIZES):  # float64 accumulation in the block kernel (16384: the composition); by sha256
        add(H, "C", "grid", ("bf16", "f16")[i % 2], (3, n), n, "weight_input", salt=50 + i)
    add(H, "C", "randn", "bf16", (2048, 40), 2048, "weight_output", salt=56, scale=0.02)
    # random-hadamard: K == 1 (signs in the permuted launch), plain and transposed; K > 1 (the composition)
    R = "random-hadamard"
    for i, n in enumerate(RANDOM_K1 + RANDOM_K):
        for j, dt in enumerate(DTYPES):
            for inverse in (False, True):
                add(R, "A", "ints", dt, ((1, 3, 5)[(i + j) % 3], n), n, inverse=inverse, salt=60 + i)
    for dt in ("bf16", "f16"):
        for inverse in (False, True):
            add(R, "C", "grid", dt, (24, 128), 128, "weight_input", inverse=inverse, salt=70)
            add(R, "C", "grid", dt, (128, 24), 128, "weight_output", inverse=inverse, salt=71)
            add(R, "C", "grid", dt, (4, 96), 96, "weight_input", inverse=inverse, salt=72)
    return out


def stored(recipe) -> bool:
    """the small cases keep the reference's output itself; every case keeps its sha256"""
    return math.prod(recipe["shape"]) <= 512


# the two-layer model of tests/_hadamard_cases.py::model() under its MODEL_CONFIG with randomize=True in both groups
def model_config():
    from _hadamard_cases import MODEL_CONFIG

    cfg = {"config_groups": {k: dict(v, randomize=True) for k, v in MODEL_CONFIG["config_groups"].items()}}
    return cfg
