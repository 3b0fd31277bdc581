"""The case matrix of the channel-wise 8-bit round-to-nearest fixture (tools/gen_golden_channel8_rtn.py writes it, tests/test_channel8_rtn.py and
tests/test_gpu_channel8_rtn.py read it).  A case is (shape, dtype, special); its input is an integer formula of its recipe.  Per stored case and kind
the fixture holds the reference's `scale`, `zero_point` (INT) and codes `q`; the input `x` itself only for cases of at most 4096 elements — the
manifest keeps every input's sha256 and `make_weight` regenerates it."""
import hashlib

import torch

BF16, F16, F32, F8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
DTYPES = {"bf16": BF16, "f16": F16, "f32": F32}
# kind -> the QuantizationArgs of the weights besides the strategy
KINDS = {"fp8": dict(num_bits=8, type="float", symmetric=True),
         "int8": dict(num_bits=8, type="int", symmetric=True),
         "int8_zp": dict(num_bits=8, type="int", symmetric=False)}
MAX_COLS = 65536  # the plan's maximum (CT_RTN_CHANNEL8_MAX_COLS)
X_STORED_MAX = 4096  # inputs above this many elements are regenerated, not stored

# what the one-pass kernel's plan takes, the smallest shape at which each path can still go wrong:
#   (1, 8)      one unit, 63 idle lanes
#   (5, 512)    wave form, one load per lane; 5 rows: a partial last workgroup of four waves.  Rows: all zero / one-sided positive / planted / +- the
#               largest finite value / +- the smallest normal
#   (2, 1032)   wave form, a ragged third load.  Rows: a subnormal / a -0.0 among ordinary values
#   (2, 2048)   the last wave-form width of a symmetric scheme.  Rows: one-sided positive / ordinary
#   (2, 2056)   the first workgroup-form width (unit 257).  Rows: all zero / planted
#   (1, 4104), (1, 8200)   the first widths of the 4- and 8-unit instantiations
#   (1, 8192)   the asymmetric wave form's last width
#   (1, 16384)  the last row that lives in registers (not stored: against the oracle and the composition only)
#   (1, 16392)  the first long row, one unit beyond
#   (1, 29568)  a real down_proj row whose unit count (3696) is no multiple of 256
#   (1, 65536)  the plan's maximum (not stored)
# every long row carries its maximum in its LAST unit and its minimum in its FIRST
FAST = [((1, 8), None), ((5, 512), "rows5"), ((2, 1032), "rows2a"), ((2, 2048), "rows2b"), ((2, 2056), "rows2c"), ((1, 4104), None), ((1, 8200), None),
        ((1, 8192), None), ((1, 16384), None), ((1, 16392), "long"), ((1, 29568), "long"), ((1, MAX_COLS), "long")]
NOT_STORED = {(1, 16384), (1, MAX_COLS), (1, MAX_COLS + 8)}
# what it refuses: float32 weights, cols % 8 != 0, one unit above the maximum
FALLBACK = [((4, 64), "f32"), ((2, 100), "bf16"), ((2, 100), "f16"), ((1, MAX_COLS + 8), "bf16"), ((1, MAX_COLS + 8), "f16")]


def key_of(shape, dtype: str) -> str:
    return f"{shape[0]}x{shape[1]}.{dtype}"


def case_list():
    """[(key, recipe)] — recipe = dict(shape, dtype, special, fast, stored, salt).  Deterministic."""
    out = []
    for shape, special in FAST:
        for dtype in ("bf16", "f16"):
            out.append((key_of(shape, dtype), dict(shape=list(shape), dtype=dtype, special=special, fast=True, stored=tuple(shape) not in NOT_STORED)))
    for shape, dtype in FALLBACK:
        out.append((key_of(shape, dtype), dict(shape=list(shape), dtype=dtype, special="long" if shape[1] > 16384 else None, fast=False,
                                               stored=tuple(shape) not in NOT_STORED)))
    for i, (_, r) in enumerate(out):
        r["salt"] = i % 7 + 1
    return out


def x_stored(r) -> bool:
    return r["stored"] and r["shape"][0] * r["shape"][1] <= X_STORED_MAX


def planted_row(x, row, dt):
    """small values under +-3.5 = the FP8 maximum times the scale 2^-7 (the codes +-448; INT8: the row's extreme is the code +-127), and a -0.0"""
    x[row] = (x[row].float().clamp(-0.9, 0.9)).to(dt)
    x[row, 5] = 3.5
    x[row, 7] = -3.5
    x[row, 9] = -0.0


def make_weight(r) -> torch.Tensor:
    """the case's weight on the CPU: a multiplicative hash of the element index mapped to [-7.8, 7.8] in steps of 2^-8, under a per-row magnitude
    of 2^-6 .. 2^3"""
    rows, cols = r["shape"]
    dt = DTYPES[r["dtype"]]
    i = torch.arange(rows * cols, dtype=torch.int64).reshape(rows, cols)
    h = ((i + 977 * r["salt"]) * 2654435761) % 4294967296
    v = ((h >> 7) % 4001 - 2000).to(torch.float32) / 256.0
    mag = torch.arange(rows)[:, None] * 5 + r["salt"]
    x = (v * torch.pow(2.0, (mag % 10 - 6).to(torch.float32))).to(dt)
    fi = torch.finfo(dt)
    sign = torch.where(torch.arange(cols) % 3 == 0, -1.0, 1.0)
    special = r["special"]
    if special == "rows5":
        x[0] = 0                                             # an all-zero row: scale = the dtype's eps
        x[1] = (x[1].float().abs() + 0.001).to(dt)           # one-sided positive: the asymmetric zero point at the range's end
        planted_row(x, 2, dt)
        x[3] = (sign * fi.max).to(dt)                        # +- the largest finite value
        x[4] = (sign * fi.tiny).to(dt)                       # +- the smallest normal
    elif special == "rows2a":
        x[0] = (sign.double() * fi.tiny / 4).to(dt)          # a subnormal
        x[1, 1031] = -0.0                                    # in the ragged third load
    elif special == "rows2b":
        x[0] = (x[0].float().abs() + 0.001).to(dt)
    elif special == "rows2c":
        x[0] = 0
        planted_row(x, 1, dt)
        x[1, 2055] = 3.5                                     # the row's maximum again, in unit 257
    elif special == "long":
        x = (x.float().clamp(-100.0, 100.0)).to(dt)
        x[0, cols - 1] = 300.0                               # the row's maximum in its LAST unit
        x[0, 0] = -200.0                                     # its minimum in its FIRST
    return x.contiguous()


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def oracle_outputs(O, x: torch.Tensor, kind: str) -> dict:
    """what the fixture records, from the pinned oracle's composition: its per-row calculate_qparams, then its channel quantize — FLOAT with the
    all-zero zero point of a calibrated scheme present"""
    if kind == "fp8":
        scale = O.calculate_qparams_float(x, kind="fp8")
        q = O.quantize(x, scale, torch.zeros(scale.shape, dtype=F8), num_bits=8, strategy="channel", dtype=F8, qtype="float")
        return dict(scale=scale, q=q)  # (a FLOAT scheme's zero point is all zeros: not recorded)
    scale, zp = O.calculate_qparams_minmax(x, num_bits=8, symmetric=KINDS[kind]["symmetric"])
    q = O.quantize(x, scale, zp, num_bits=8, strategy="channel", dtype=torch.int8)
    return dict(scale=scale, zero_point=zp, q=q)


def bits(t: torch.Tensor) -> torch.Tensor:
    if t.dtype.itemsize == 1:
        return t.view(torch.uint8)
    return t.view(torch.int16) if t.dtype in (BF16, F16) else t.view(torch.int32) if t.dtype == F32 else t
