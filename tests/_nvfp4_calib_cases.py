"""The case matrix of the calibrated NVFP4 global-scale fixtures (tools/gen_golden_nvfp4_calib.py writes them,
tests/test_gpu_nvfp4_calibrate.py reads them).  An input is an integer formula placed in a storage layout, so a case is fully described by
its recipe; every case keeps the sha256 of its input and the reference observer's `get_global_scale` result itself (four bytes)."""
import hashlib

import torch

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = {"bf16": BF16, "f16": F16, "f32": F32}
# (1, 1, 16): one lane of one row; (1, 257, 96): rows that are no multiple of a workgroup's; (4, 4100, 32): the row loop under the capped grid;
# (2, 8, 64, 20): rows that are no whole 8-element units — the element form
SHAPES = {"contiguous": [(1, 1, 16), (2, 3, 64), (1, 257, 96), (4, 4100, 32), (2, 8, 64, 20)],
          "slice": [(2, 5, 64)],        # [..., :64] of rows of 72: the last dimension contiguous, the rows apart
          "transposed": [(2, 8, 5, 64)]}  # (B, S, H, D).transpose(1, 2): what an attention module sees
SPECIALS = ("zero", "negative", "nan", "inf")
SPECIAL_SHAPE = (2, 3, 64)


def values(shape, dtype, seed: int, amp: float):
    """integers in [-32760, 32760] by a multiplicative hash, over 4096: exact in float32, then rounded once to `dtype`"""
    n = 1
    for d in shape:
        n *= d
    i = torch.arange(n, dtype=torch.int64)
    v = ((i + 17 * seed) * 2654435761 % 65521 - 32760).to(torch.float32) * (amp / 4096.0)
    return v.to(dtype).reshape(shape)


def make(recipe):
    """the observed tensor of a recipe, in its layout (a view where the layout is one)"""
    shape, dtype = tuple(recipe["shape"]), DTYPES[recipe["dtype"]]
    x = values(shape, dtype, recipe["seed"], recipe["amp"])
    special = recipe.get("special")
    if special is None:  # the extreme is ONE element, somewhere in the middle: a row the walk skips changes the result
        x.view(-1)[x.numel() * 5 // 7] = recipe["amp"] * (-16.0 if recipe["seed"] % 2 else 16.0)
    if special == "zero":
        x = torch.zeros(shape, dtype=dtype)
    elif special == "negative":
        x = -x.abs() - 0.25
    elif special == "nan":
        x.view(-1)[x.numel() // 2] = float("nan")
    elif special == "inf":
        x.view(-1)[x.numel() - 3] = float("inf")
    layout = recipe["layout"]
    if layout == "slice":
        wide = torch.full(shape[:-1] + (shape[-1] + 8,), 1e4, dtype=dtype)  # what lies between the rows would win every maximum
        wide[..., : shape[-1]] = x
        return wide[..., : shape[-1]]
    if layout == "transposed":
        return x.transpose(1, 2).contiguous().transpose(1, 2)
    return x


def key_of(r):
    tail = f".{r['special']}" if r.get("special") else ""
    return ".".join([r["layout"], r["dtype"], "x".join(str(d) for d in r["shape"])]) + tail


def case_list():
    """[(key, recipe)], deterministic: every shape of every layout and every special value in every dtype, and per dtype the two batches of
    the accumulation test (`batch0` holds the larger values, so the running result differs from the last batch's own) with their concatenation"""
    out = []
    for name in DTYPES:
        seed = 1
        for layout, shapes in SHAPES.items():
            for shape in shapes:
                out.append(dict(layout=layout, dtype=name, shape=list(shape), seed=seed, special=None, amp=0.25 + 0.5 * seed))
                seed += 1
        for special in SPECIALS:
            out.append(dict(layout="contiguous", dtype=name, shape=list(SPECIAL_SHAPE), seed=seed, special=special, amp=1.0))
            seed += 1
    cases = [(key_of(r), r) for r in out]
    for name in DTYPES:
        for part, amp in (("batch0", 3.0), ("batch1", 0.5)):
            r = dict(layout="contiguous", dtype=name, shape=[2, 7, 96], seed=40 + len(part) + int(amp), special=None, amp=amp)
            cases.append((f"{part}.{name}", r))
        cases.append((f"concat.{name}", dict(concat=[f"batch0.{name}", f"batch1.{name}"], dtype=name)))
    return cases


def build(recipe, recipes):
    """the tensor of a recipe; a `concat` recipe is its parts along the first dimension"""
    if "concat" in recipe:
        return torch.cat([make(recipes[k]) for k in recipe["concat"]], dim=0)
    return make(recipe)


def sha(x):
    return hashlib.sha256(x.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
