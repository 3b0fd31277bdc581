"""The case matrix of the group-wise 8-bit round-to-nearest fixture (tools/gen_golden_group8_rtn.py writes it, tests/test_group8_rtn.py and
tests/test_gpu_group8_rtn.py read it).  A case is (shape, group, dtype, special); its input is an integer formula of its recipe.  The fixture holds
every input `x` and, per kind, the reference's `scale`, `zero_point` and codes `q` (MXFP8: also the E8M0 bytes `e8m0`; INT: also the 8-bit
pack-quantized words `packed`)."""
import hashlib

import torch

BF16, F16, F32, F8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
DTYPES = {"bf16": BF16, "f16": F16, "f32": F32}
# kind -> the QuantizationArgs of the weights besides strategy and group_size
KINDS = {"mxfp8": dict(num_bits=8, type="float", symmetric=True, scale_dtype=torch.uint8, zp_dtype=torch.uint8),
         "fp8": dict(num_bits=8, type="float", symmetric=True),
         "int8": dict(num_bits=8, type="int", symmetric=True),
         "int8_zp": dict(num_bits=8, type="int", symmetric=False)}
GROUP_MAX = 1024  # the largest group the plan admits: 64 lanes of 16 elements

# what the one-pass kernel's plan takes.  One group alone; 3 rows of 3 groups with planted ones; one full workgroup of either lane width (256 lanes of
# 16 or 32 elements) plus one group: a partial last workgroup whose dead lanes sit in the reduction; groups of 64 and 256 (4 and 16 lanes: the
# row_half_mirror / row_mirror steps); the largest group on two rows (64 lanes: both wave shuffles); planted maxima; rows of extreme values
FAST = [((1, 32), 32, None), ((1, 128), 128, None), ((3, 96), 32, "planted"), ((3, 384), 128, "planted"), ((1, 8224), 32, None), ((1, 8320), 128, None),
        ((4, 512), 64, None), ((4, 512), 256, None), ((2, GROUP_MAX), GROUP_MAX, None), ((2, 256), 32, "maxima"), ((2, 256), 128, "maxima"),
        ((3, 128), 32, "extremes"), ((3, 128), 128, "extremes")]
# what it refuses: float32 weights, a group that is no 32 * 2^k, the first group size above the plan's maximum
FALLBACK = [((4, 64), 32, "f32"), ((2, 96), 48, "bf16"), ((2, 96), 48, "f16"), ((1, 2 * GROUP_MAX), 2 * GROUP_MAX, "bf16"), ((1, 2 * GROUP_MAX), 2 * GROUP_MAX, "f16")]


def key_of(shape, group, dtype: str, special=None) -> str:
    return f"{shape[0]}x{shape[1]}.g{group}.{dtype}" + (f".{special}" if special else "")


def case_list():
    """[(key, recipe)] — recipe = dict(shape, group, dtype, special, fast, salt).  Deterministic."""
    out = []
    for shape, group, special in FAST:
        for dtype in ("bf16", "f16"):
            out.append((key_of(shape, group, dtype, special), dict(shape=list(shape), group=group, dtype=dtype, special=special, fast=True)))
    for shape, group, dtype in FALLBACK:
        out.append((key_of(shape, group, dtype), dict(shape=list(shape), group=group, dtype=dtype, special=None, fast=False)))
    for i, (_, r) in enumerate(out):
        r["salt"] = i % 7 + 1
    return out


def kinds_of(r):
    """the kinds a case is recorded under: MXFP8 for groups of 32 only"""
    return [k for k in KINDS if k != "mxfp8" or r["group"] == 32]


def make_weight(r) -> torch.Tensor:
    """the case's weight on the CPU: a multiplicative hash of the element index mapped to [-7.8, 7.8] in steps of 2^-8, under a per-group magnitude
    of 2^-6 .. 2^3 that differs between neighbouring groups and signs that make some groups one-sided"""
    rows, cols = r["shape"]
    g = r["group"]
    dt = DTYPES[r["dtype"]]
    i = torch.arange(rows * cols, dtype=torch.int64).reshape(rows, cols)
    h = ((i + 977 * r["salt"]) * 2654435761) % 4294967296
    v = ((h >> 7) % 4001 - 2000).to(torch.float32) / 256.0
    grp = torch.arange(rows)[:, None] * 5 + (torch.arange(cols)[None, :] // g) * 3 + r["salt"]
    v = v * torch.pow(2.0, (grp % 10 - 6).to(torch.float32))
    v = torch.where(grp % 4 == 1, v.abs() + 0.001, v)    # an all-positive group: zero joins the range
    v = torch.where(grp % 4 == 3, -v.abs() - 0.001, v)   # an all-negative one
    x = v.to(dt)
    special = r["special"]
    if special == "planted":
        x[0, g:2 * g] = 0                      # an all-zero group: scale = the dtype's eps (MX: 1)
        x[1, :g] = torch.where(torch.arange(g) % 2 == 0, -2.0 ** -24, 2.0 ** -24).to(dt)  # tiny values of both signs under one large value
        x[1, 3] = 4.0
        x[1, g + 4] = -0.0                     # a -0.0 quotient: + the (all-zero) zero point = +0.0
        x[2, :g] = (x[2, :g].float() * 0.01).to(dt)
        x[2, 5] = 448.0 * 0.0078125            # exactly the format's maximum times the FP8 scale of this group: the code is 448
        x[2, g:2 * g] = (x[2, g:2 * g].float().clamp(-0.9, 0.9)).to(dt)
        x[2, g + 7] = -127.0 * 0.0078125       # exactly -(INT8 maximum) times the symmetric scale
    elif special == "maxima":
        x = (x.float() * 0.01).to(dt)
        x[0, 0] = 3.0                          # the first element of a group
        x[0, 2 * g - 1] = -5.0                 # the last element of a group
        x[rows - 1, cols - 1] = 7.0            # the last element of the tensor
    elif special == "extremes":
        fi = torch.finfo(dt)
        sign = torch.where(torch.arange(cols) % 3 == 0, -1.0, 1.0)
        x[0] = (sign * fi.max).to(dt)                        # +- the largest finite value
        x[1] = (sign * fi.tiny).to(dt)                       # +- the smallest normal
        x[2] = (sign.double() * fi.tiny / 4).to(dt)          # a subnormal
    return x.contiguous()


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def oracle_outputs(O, x: torch.Tensor, group: int, kind: str) -> dict:
    """what the fixture records, from the pinned oracle's composition: its group-wise calculate_qparams, then its group quantize — FLOAT with the
    all-zero zero point of a calibrated scheme present — then (MXFP8) its E8M0 encoding, (INT) its 8-bit pack_to_int32"""
    if kind in ("fp8", "mxfp8"):
        scale = O.calculate_qparams_float(x, kind=kind, group_size=group)
        q = O.quantize(x, scale, torch.zeros(scale.shape, dtype=F8), num_bits=8, strategy="group", group_size=group, dtype=F8, qtype="float")
        out = dict(scale=scale, q=q)  # (a FLOAT scheme's zero point is all zeros: not recorded)
        if kind == "mxfp8":
            out["e8m0"] = O.e8m0_encode(scale)
        return out
    scale, zp = O.calculate_qparams_minmax(x, num_bits=8, group_size=group, symmetric=KINDS[kind]["symmetric"])
    q = O.quantize(x, scale, zp, num_bits=8, strategy="group", group_size=group, dtype=torch.int8)
    return dict(scale=scale, zero_point=zp, q=q, packed=O.pack_to_int32(q, 8))


def bits(t: torch.Tensor) -> torch.Tensor:
    if t.dtype.itemsize == 1:
        return t.view(torch.uint8)
    return t.view(torch.int16) if t.dtype in (BF16, F16) else t.view(torch.int32) if t.dtype == F32 else t
