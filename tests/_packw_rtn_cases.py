"""The case matrix of the pack-quantized W2-W7 round-to-nearest fixture (tools/gen_golden_packw_rtn.py writes it, tests/test_packw_rtn.py and
tests/test_gpu_packw_rtn.py read it).  A case is (shape, group, dtype, special); its input is an integer formula of its recipe.  The fixture holds
every input `x` and, per (num_bits, symmetric), the reference's `scale`, `zero_point`, the packed words `packed` = pack_to_int32(quantize(x), bits)
and, for an asymmetric scheme, the stored zero points `zp_packed` = pack_to_int32(zero_point, bits, packed_dim=0)."""
import hashlib

import torch

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = {"bf16": BF16, "f16": F16, "f32": F32}
BITS = (2, 3, 5, 6, 7)
GROUP_MAX = 2048  # the largest group the plan admits: 64 lanes of 32 elements

# what the one-pass kernel's plan takes (group None: channel-wise, group = cols).  One lane alone; 3 rows of 3 groups with planted ones (per width:
# the planted codes depend on it); one full workgroup of 256 lanes plus one group — a partial last workgroup whose dead lanes sit in the reduction —
# at one and at four lanes per group; groups of 64 and 256 (the 2-lane and 8-lane DPP steps); the largest group on two rows (64 lanes: the whole
# wave); a channel-wise case; planted maxima; rows of extreme values
FAST = [((1, 32), 32, None), ((3, 96), 32, "planted"), ((3, 384), 128, "planted"), ((1, 8224), 32, None), ((1, 8320), 128, None),
        ((4, 512), 64, None), ((4, 512), 256, None), ((2, GROUP_MAX), GROUP_MAX, None), ((3, 256), None, None), ((2, 256), 32, "maxima"),
        ((2, 256), 128, "maxima"), ((3, 128), 32, "extremes"), ((3, 128), 128, "extremes")]
# what it refuses: float32 weights, a group that is no 32 * 2^k, the first group size above the plan's maximum, a row that is no whole 32-element
# pack groups (channel-wise: pack_to_int32 pads the last word)
FALLBACK = [((4, 64), 32, "f32"), ((2, 96), 48, "bf16"), ((2, 96), 48, "f16"), ((1, 2 * GROUP_MAX), 2 * GROUP_MAX, "bf16"),
            ((1, 2 * GROUP_MAX), 2 * GROUP_MAX, "f16"), ((2, 40), None, "bf16"), ((2, 40), None, "f16")]


def key_of(shape, group, dtype: str, special=None, bits=None) -> str:
    return f"{shape[0]}x{shape[1]}.g{group or 'ch'}.{dtype}" + (f".{special}" if special else "") + (f".b{bits}" if bits else "")


def case_list():
    """[(key, recipe)] — recipe = dict(shape, group, dtype, special, fast, salt, bits).  `bits`: the widths the case is recorded under (a planted case
    is built for one width).  Deterministic."""
    out = []
    for shape, group, special in FAST:
        for dtype in ("bf16", "f16"):
            for b in (BITS if special == "planted" else (None,)):
                out.append((key_of(shape, group, dtype, special, b),
                            dict(shape=list(shape), group=group, dtype=dtype, special=special, fast=True, bits=[b] if b else list(BITS))))
    for shape, group, dtype in FALLBACK:
        out.append((key_of(shape, group, dtype), dict(shape=list(shape), group=group, dtype=dtype, special=None, fast=False, bits=list(BITS))))
    for i, (_, r) in enumerate(out):
        r["salt"] = i % 7 + 1
    return out


def make_weight(r) -> torch.Tensor:
    """the case's weight on the CPU: a multiplicative hash of the element index mapped to [-7.8, 7.8] in steps of 2^-8, under a per-group magnitude
    of 2^-6 .. 2^3 that differs between neighbouring groups and signs that make some groups one-sided (as tests/_group8_rtn_cases.make_weight)"""
    rows, cols = r["shape"]
    g = r["group"] or cols
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
        b = r["bits"][0]
        qmax, s = float(2 ** (b - 1) - 1), 2.0 ** -7
        x[0, :g] = x[0, :g].abs()              # an all-positive group
        x[0, g:2 * g] = 0                      # an all-zero group: scale = the dtype's eps
        x[0, 2 * g:] = -x[0, 2 * g:].abs()     # an all-negative group
        x[1, :g] = torch.where(torch.arange(g) % 2 == 0, -2.0 ** -24, 2.0 ** -24).to(dt)  # tiny values of both signs under one large value
        x[1, 3] = 4.0
        x[1, g + 4] = -0.0                     # a -0.0 quotient
        # symmetric: amax = (2^b - 1) 2^-8 makes the scale exactly 2^-7; +-qmax * scale are then exactly the codes +-qmax
        x[2, :g] = (x[2, :g].float().clamp(-0.4, 0.4) * s).to(dt)
        x[2, 2] = (2 ** b - 1) * 2.0 ** -8
        x[2, 5] = qmax * s
        x[2, 9] = -qmax * s
        # asymmetric: min = qmin * 2^-7 and max = qmax * 2^-7 make the scale exactly 2^-7 and the zero point 0: both ends sit exactly on their codes
        x[2, g:2 * g] = (x[2, g:2 * g].float().clamp(-0.4, 0.4) * s).to(dt)
        x[2, g + 7] = -(qmax + 1.0) * s
        x[2, g + 11] = qmax * s
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


def tag(bits: int, symmetric: bool) -> str:
    return f"w{bits}" + ("" if symmetric else "a")


def oracle_outputs(O, x: torch.Tensor, group, bits: int, symmetric: bool) -> dict:
    """what the fixture records, from the pinned oracle's composition: its group-wise (group None: row-wise) calculate_qparams, its quantize, its
    pack_to_int32 along the columns and, for an asymmetric scheme, along the rows of the zero points"""
    scale, zp = O.calculate_qparams_minmax(x, num_bits=bits, group_size=group, symmetric=symmetric)
    q = O.quantize(x, scale, zp, num_bits=bits, strategy="group" if group else "channel", group_size=group, dtype=torch.int8)
    out = dict(scale=scale, zero_point=zp, packed=O.pack_to_int32(q, bits))
    if not symmetric:
        out["zp_packed"] = O.pack_to_int32(zp, bits, packed_dim=0)
    return out


def bits_of(t: torch.Tensor) -> torch.Tensor:
    """a view whose torch.equal is raw-bit equality"""
    if t.dtype.itemsize == 1:
        return t.view(torch.uint8)
    return t.view(torch.int16) if t.dtype in (BF16, F16) else t.view(torch.int32) if t.dtype == F32 else t
