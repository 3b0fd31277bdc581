"""The case matrix of the compress-side scale fixture (tools/gen_golden_compress_scales.py writes it, tests/test_compress_scales.py and
tests/test_gpu_compress_scales.py read it): what `quantize_and_pack`, `quantize_tensor`, `fake_quantize_tensor` and the compressors' `compress`
are handed by a checkpoint or a calibrator — weights, GIVEN scales and zero points — over the whole domain of the scales.  The scale side is the
sibling module's (tests/_decompress_scale_cases.py: `sweep16`, `sweep32`, `edge`, the salts, the `cross` pairing), imported, not copied.

Everything is a pure integer function of a GLOBAL index:
  group gi, position j   as in the sibling module
  scale    `sweep16`, `cross`, `sweep32`: the sibling's.  `guard`: the patterns one ulp below, at and one ulp above each end point of the range
           guard that DESIGN section 2 names for the scale's dtype (bf16 2^-64, 2^64; fp16 2^-14, 2^15; fp32 2^-100, 2^100), both signs: 12
           patterns, group gi holds pattern (gi * 5 + 3) mod 12 — any 12 consecutive groups hold all of them, so both sides of every end point
           meet inside every wave.
  weights  built from the group's OWN scale, so that a group says something under any scale:  x_j = rnd_X(fl32(t_j - z) * fl32(s)), z the
           group's zero point (0 without one), with the targets
               t_j = ((77 j + h(gi)) mod 2 (2^bits + 4)) / 2 - (2^(bits-1) + 2)
           every half-integer from two below the lowest code to two above the highest: every tie and every clamp edge (77 is prime to the
           modulus, so any run of that many positions holds every target; at 7 bits, modulus 264 = 8 * 3 * 11, the step is 79).  The bit pattern of x_j is then moved by -1 / 0 / +1 per position
           ((5 j + (h >> 7)) mod 3 - 1: one ulp off the tie, either way), and the last five positions of every group hold +0, -0, +inf, -inf
           and NaN.  Under a non-finite or zero scale the products are themselves 0, inf or NaN: they stay, they are inputs like any other.
  float8   (`qtype` fp8) the targets are the 256 float8_e4m3fn values, the midpoints between neighbouring finite ones, +-480 (beyond the
           clamp) and +-1e-3 (below half the smallest subnormal), taken by (77 (j + G (gi div 17)) + h(gi mod 17)) mod 512: 77 is odd, so
           any 512 consecutive positions hold every one, and the groups 17 apart — in a cross those of one edge scale — continue each other.
  fp32 cross  the sibling's 17 edge scales restated for fp32 (`edge32`), under the same pairing with the zero points.
  FP4      (`qtype` fp4; `fp4_case_list`) NVFP4: groups of 16 whose scale is a float8 value — all 256 bytes, byte (77 gi + 5) mod 256 — held in
           the weight's dtype, under ONE global scale per case, chosen so that s_eff = fl32(scale / global) lies inside the kernel's guard
           [2^-20, 2^10] for every finite positive byte, exactly at either end for one byte, one fp32 ulp outside either end, or outside for
           all.  MXFP4: groups of 32 under every positive power of two the dtype holds, subnormal ones included.  Targets: the sixteen E2M1
           values, the midpoints between neighbours, and +-7, +-8 (beyond the clamp at 6): 34, taken by (77 j + h) mod 34.
  zero points  the sibling's: hashed per group over the width's own range (`ib`, `i4`), every int8 (`i8`), float8 bytes (`f8`) or all-zero
           float8 (`f8z`); the cross takes them from the pair.
Scales and zero points are written as bit patterns, never through a Python float; the weights are one fp32 product and one rounding."""
import functools
import hashlib
import json
import os

import torch

import _decompress_scale_cases as D
from _decompress_scale_cases import BF16, F8, F16, F32, canonical, sha  # noqa: F401

DTYPES = D.DTYPES
GOLDEN = D.GOLDEN
SWEEP = D.SWEEP
WHOLE_MAX = 40 * 1024  # a `cross` output of at most this many bytes is kept whole in compress_scales.safetensors

# the end points of the range guards ("proven shortcuts"), as exponents of two
GUARD_ENDS = {"bf16": (-64, 64), "f16": (-14, 15), "f32": (-100, 100)}
_FMT = {"bf16": (8, 7), "f16": (5, 10), "f32": (8, 23)}


def guard_bits(dtype: str) -> list:
    """the 12 guard patterns: for each end point 2^e the pattern below, at and above it, then the same with the sign bit"""
    ebits, m = _FMT[dtype]
    bias = (1 << (ebits - 1)) - 1
    pos = []
    for e in GUARD_ENDS[dtype]:
        at = (e + bias) << m
        assert 0 < e + bias < (1 << ebits) - 1
        pos += [at - 1, at, at + 1]
    sign = 1 << (ebits + m)
    return pos + [p | sign for p in pos]


def guard_inside(dtype: str) -> list:
    """for each guard pattern: is it inside the guard's range (the end points are)"""
    lo = [False, True, True]
    hi = [True, True, False]
    return (lo + hi) * 2


def edge_bits(dtype: str) -> list:
    """the 17 edge scales as bit patterns: the sibling's for the 16-bit dtypes, and the same construction for fp32 — +-0, +- smallest and
    largest subnormal, +- smallest normal, +-1, +- largest finite, +-inf, the quiet NaN, the NaN of smallest payload, all ones"""
    if dtype != "f32":
        return D.edge(dtype)
    inf, one = 0x7F800000, 0x3F800000
    out = []
    for p in (0, 1, 0x7FFFFF, 0x800000, one, inf - 1, inf):
        out += [p, p | 0x80000000]
    return out + [inf | 0x400000, inf | 1, 0xFFFFFFFF]


def _case(key, bits, shape, group, sdt, scales="sweep16", zp=None, qtype="int", ops=("pack",), **extra):
    r = dict(bits=bits, shape=list(shape), group=group, sdt=sdt, xdt=sdt, scales=scales, zp=zp, qtype=qtype, ops=list(ops), row0=0, sweeps=0, g_idx=None, attn=None, gs=None)
    r.update(extra)
    return key, r


def case_list():
    """[(key, recipe)] — recipe = dict(bits, qtype, shape, group (None: channel-wise), sdt, xdt, scales, zp, g_idx, ops, row0, sweeps, attn (the
    (B, H, S, D) a q / k / v state has: `shape` is its (H, S * D) view, the attn_head strategy the channel strategy on it)); `ops` are
    the reference operations recorded for the case: `q` quantize to int8, `pack` the pack-quantized words of that, `q32` quantize to int32,
    `qx` quantize to the float dtype the reference picks, `fq` fake_quantize, `f8` quantize to float8_e4m3fn, `fq8` fake_quantize of FLOAT 8 bit"""
    out = []
    for dt in ("bf16", "f16"):
        # ---- W4: lean (g128, channel-wise rows), flat (g32, g64), activation ordering
        for zp in (None, "ib"):
            z = zp or "sym"
            out.append(_case(f"w4.g128.{z}.{dt}", 4, (512, 16384), 128, dt, zp=zp, ops=("pack", "fq")))
            out.append(_case(f"w4.guard.g128.{z}.{dt}", 4, (8, 16384), 128, dt, scales="guard", zp=zp, ops=("pack", "fq")))
            out.append(_case(f"w4.g32.{z}.{dt}", 4, (128, 16384), 32, dt, zp=zp))
            out.append(_case(f"w4.g64.{z}.{dt}", 4, (256, 16384), 64, dt, zp=zp))
            out.append(_case(f"w4.g16.{z}.{dt}", 4, (64, 16384), 16, dt, zp=zp))  # a scale per two units: no four units share one
            out.append(_case(f"w4.chan32.{z}.{dt}", 4, (65536, 32), None, dt, zp=zp))
            out.append(_case(f"w4.chan20.{z}.{dt}", 4, (65536, 20), None, dt, zp=zp, ops=("pack", "q32", "qx")))
        out.append(_case(f"w4.gidx128.ib.{dt}", 4, (512, 16384), 128, dt, zp="ib", g_idx=3))
        out.append(_case(f"w4.gidx512.sym.{dt}", 4, (128, 65536), 128, dt, g_idx=5))
        out.append(_case(f"w4.cross.g128.sym.{dt}", 4, (8, 4608), 128, dt, scales="cross", ops=("pack", "fq")))
        out.append(_case(f"w4.cross.g128.i4.{dt}", 4, (8, 4608), 128, dt, scales="cross", zp="i4"))
        out.append(_case(f"w4.cross.g128.i8.{dt}", 4, (128, 4352), 128, dt, scales="cross", zp="i8", ops=("pack", "fq")))
        out.append(_case(f"w4.cross.g32.i8.{dt}", 4, (32, 4352), 32, dt, scales="cross", zp="i8"))
        out.append(_case(f"w4.cross.gidx.i8.{dt}", 4, (128, 4352), 128, dt, scales="cross", zp="i8", g_idx=9))
        out.append(_case(f"w4.cross.chan20.i8.{dt}", 4, (4352, 20), None, dt, scales="cross", zp="i8", ops=("pack", "qx")))
        # ---- the other widths
        out.append(_case(f"w1.chan32.sym.{dt}", 1, (65536, 32), None, dt))
        out.append(_case(f"w1.chan20.sym.{dt}", 1, (65536, 20), None, dt))
        for b in (2, 3, 5, 6, 7):
            out.append(_case(f"w{b}.g128.sym.{dt}", b, (512, 16384), 128, dt))
            out.append(_case(f"w{b}.g64.ib.{dt}", b, (256, 16384), 64, dt, zp="ib"))
            out.append(_case(f"w{b}.cross.g128.ib.{dt}", b, (1 << b, 17 * 128), 128, dt, scales="cross", zp="ib"))
        out.append(_case(f"w3.guard.g128.ib.{dt}", 3, (8, 16384), 128, dt, scales="guard", zp="ib"))
        # ---- 8 bit: int8 codes, the packed words, fake quantize
        for zp in (None, "i8"):
            z = zp or "sym"
            out.append(_case(f"q8.chan256.{z}.{dt}", 8, (65536, 256), None, dt, zp=zp, ops=("q", "pack")))
            out.append(_case(f"q8.g128.{z}.{dt}", 8, (512, 16384), 128, dt, zp=zp, ops=("q", "pack", "fq")))
        out.append(_case(f"q8.g16.i8.{dt}", 8, (64, 16384), 16, dt, zp="i8", ops=("q", "pack")))   # shared: a scale per two units
        out.append(_case(f"q8.g8.i8.{dt}", 8, (32, 16384), 8, dt, zp="i8", ops=("q", "pack")))     # not shared: a scale per unit
        out.append(_case(f"q6.g128.ib.{dt}", 6, (512, 16384), 128, dt, zp="ib", ops=("q",)))
        out.append(_case(f"q8.guard.g128.i8.{dt}", 8, (8, 16384), 128, dt, scales="guard", zp="i8", ops=("q", "pack", "fq")))
        out.append(_case(f"q8.chan20.i8.{dt}", 8, (65536, 20), None, dt, zp="i8", ops=("pack", "q", "qx")))
        out.append(_case(f"q8.cross.g256.sym.{dt}", 8, (8, 4352), 256, dt, scales="cross", ops=("q", "pack", "fq")))
        out.append(_case(f"q8.cross.g256.i8.{dt}", 8, (256, 4352), 256, dt, scales="cross", zp="i8", ops=("q", "pack", "fq")))
        # ---- float8 codes
        for zp in (None, "f8z", "f8"):
            z = zp or "sym"
            out.append(_case(f"f8.g128.{z}.{dt}", 8, (512, 16384), 128, dt, zp=zp, qtype="fp8", ops=("f8", "fq8")))
        out.append(_case(f"f8.chan256.sym.{dt}", 8, (65536, 256), None, dt, qtype="fp8", ops=("f8",)))
        out.append(_case(f"f8.guard.g128.f8.{dt}", 8, (8, 16384), 128, dt, scales="guard", zp="f8", qtype="fp8", ops=("f8", "fq8")))
        out.append(_case(f"f8.cross.g256.sym.{dt}", 8, (8, 4352), 256, dt, scales="cross", qtype="fp8", ops=("f8", "fq8")))
        out.append(_case(f"f8.cross.g256.f8.{dt}", 8, (256, 4352), 256, dt, scales="cross", zp="f8", qtype="fp8", ops=("f8", "fq8")))
        # ---- static q / k / v QDQ: a head per row of (H, S * D) — 17 heads, one edge scale each; 272 heads: each under every zero point -8 .. 7
        out.append(_case(f"attn.int8.sym.{dt}", 8, (17, 64 * 128), None, dt, scales="cross", ops=("q", "fq"), attn=[1, 17, 64, 128]))
        out.append(_case(f"attn.fp8.sym.{dt}", 8, (17, 64 * 128), None, dt, scales="cross", qtype="fp8", ops=("f8", "fq8"), attn=[1, 17, 64, 128]))
        out.append(_case(f"attn.int8.i4.{dt}", 8, (272, 4 * 128), None, dt, scales="cross", zp="i4", ops=("q", "fq"), attn=[1, 272, 4, 128]))
    # ---- fp32 scales: fp32 arithmetic, whatever the weights are
    for zp in (None, "i8"):
        z = zp or "sym"
        for xdt in ("bf16", "f32"):
            out.append(_case(f"w4.f32.g128.{z}.x{xdt}", 4, (64, 4096), 128, "f32", scales="sweep32", zp=zp, xdt=xdt))
        out.append(_case(f"q8.f32.g256.{z}", 8, (64, 8192), 256, "f32", scales="sweep32", zp=zp, ops=("q", "pack", "fq")))
        out.append(_case(f"q8.f32.guard.{z}", 8, (8, 8192), 256, "f32", scales="guard", zp=zp, ops=("q", "pack", "fq")))
        out.append(_case(f"w4.f32.guard.{z}", 4, (8, 4096), 128, "f32", scales="guard", zp=zp))
    out.append(_case("q8.f32.cross.g256.sym", 8, (8, 4352), 256, "f32", scales="cross", ops=("q", "pack", "fq")))
    out.append(_case("q8.f32.cross.g256.i8", 8, (256, 4352), 256, "f32", scales="cross", zp="i8", ops=("q", "pack", "fq")))
    out.append(_case("w4.f32.cross.g128.i8.xbf16", 4, (128, 4352), 128, "f32", scales="cross", zp="i8", xdt="bf16"))
    out.append(_case("f8.f32.cross.g256.f8", 8, (256, 4352), 256, "f32", scales="cross", zp="f8", qtype="fp8", ops=("f8",)))
    for zp in (None, "f8"):
        out.append(_case(f"f8.f32.g256.{zp or 'sym'}", 8, (64, 8192), 256, "f32", scales="sweep32", zp=zp, qtype="fp8", ops=("f8",)))
    return out + fp4_case_list()


# ---- FP4 with given scales ------------------------------------------------------------------------------------------------------------------------
FP4_GUARD = (-20, 10)  # ct_fp4.hip's refined reciprocal serves s_eff in [2^-20, 2^10]
# global scales as fp32 bit patterns.  The finite positive float8 values run from 2^-9 (byte 0x01) to 448 (0x7E); 256 is byte 0x78.
FP4_GLOBALS = {
    "one": 0x3F800000,      # 1: every finite positive byte inside
    "odd": 0x43A6AAAB,      # 1000 / 3: inside, and no power of two
    "lo": 0x45000000,       # 2^11: byte 0x01 gives s_eff = 2^-20, the lower end point itself
    "lo_out": 0x45000001,   # 2^11 (1 + 2^-23), the next global scale up: byte 0x01 falls just below 2^-20 (two fp32 places)
    "lo2": 0x45800000,      # 2^12: byte 0x01 outside (2^-21), byte 0x02 at the end point
    "hi": 0x3E800000,       # 2^-2: byte 0x78 gives 2^10, the upper end point itself; 288 .. 448 outside
    "hi_in": 0x3E800001,    # 2^-2 (1 + 2^-23), the next global scale up: byte 0x78 just below 2^10 (two fp32 places)
    "hi_out": 0x3E7FFFFF,   # 2^-2 (1 - 2^-24): byte 0x78 one ulp above 2^10
    "far_lo": 0x53800000,   # 2^40: every byte far below the guard
    "far_hi": 0x30800000,   # 2^-30: every byte far above it
}
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
_FP4_POS = sorted(set(_E2M1) | {(a + b) / 2 for a, b in zip(_E2M1, _E2M1[1:])} | {7.0, 8.0})
FP4_TARGETS = tuple(_FP4_POS) + tuple(-v for v in _FP4_POS)  # 34: +0 and -0 among them


def pow2_bits(dtype: str) -> list:
    """every positive power of two of a 16-bit dtype as a bit pattern, the subnormal ones first"""
    e, m = _FMT[dtype]
    return [1 << k for k in range(m)] + [k << m for k in range(1, (1 << e) - 1)]


def fp4_case_list():
    out = []
    for dt in ("bf16", "f16"):
        for name, bits in FP4_GLOBALS.items():
            out.append(_case(f"fp4.nv.{name}.{dt}", 4, (64, 1024), 16, dt, scales="f8bytes", qtype="fp4", ops=("fp4", "fp4s"), gs=bits))
        out.append(_case(f"fp4.mx.{dt}", 4, (128, 2048), 32, dt, scales="pow2", qtype="fp4", ops=("fp4", "fp4s")))
    return out


def global_scale(r):
    """float32 (1,) or None"""
    return None if r["gs"] is None else torch.tensor([r["gs"]], dtype=torch.int64).to(torch.int32).view(F32)


def effective_scale(r, s: torch.Tensor) -> torch.Tensor:
    """float32: what the weights are divided by — the scale, or for NVFP4 fl32(scale / global scale)"""
    return s.float() if r["gs"] is None else s.float() / global_scale(r)


def fp4_format(r) -> str:
    return "nvfp4-pack-quantized" if r["group"] == 16 else "mxfp4-pack-quantized"


def is_sweep16(r) -> bool:
    return r["scales"] == "sweep16"


def _drec(r):
    """the recipe as the sibling module reads it"""
    zp = {"f8z": None}.get(r["zp"], r["zp"])
    sdt = "bf16" if r["scales"] == "cross" and r["sdt"] == "f32" else r["sdt"]  # (the pairing only counts the edge scales: 17 in every dtype)
    return dict(r, zp=zp, sdt=sdt, ctype="int", cgroup=None, e8m0=False, scales="sweep16" if r["scales"] == "guard" else r["scales"])


layout = D.layout


def group_index(r):
    return D.group_index(_drec(r))


def scale_bits(r) -> torch.Tensor:
    """int64 (rows, groups per row): the scale's bit pattern"""
    if r["scales"] == "cross" and r["sdt"] == "f32":
        e = torch.tensor(edge_bits("f32"), dtype=torch.int64)
        return e[D._cross_pair(_drec(r), group_index(r)) % len(e)]
    if r["scales"] == "f8bytes":  # the float8 value of byte (77 gi + 5) mod 256, held exactly in the 16-bit dtype
        by = (group_index(r) * 77 + 5) % 256
        return by.to(torch.uint8).view(F8).to(DTYPES[r["sdt"]]).view(torch.int16).to(torch.int64) & 0xFFFF
    if r["scales"] == "pow2":
        p = torch.tensor(pow2_bits(r["sdt"]), dtype=torch.int64)
        return p[(group_index(r) * 77 + 5) % len(p)]
    if r["scales"] != "guard":
        return D.scale_bits(_drec(r))
    gi = group_index(r)
    return torch.tensor(guard_bits(r["sdt"]), dtype=torch.int64)[(gi * 5 + 3) % 12]


def _as_float(bits: torch.Tensor, dtype: str) -> torch.Tensor:
    if dtype == "f32":
        return (bits - ((bits >> 31) << 32)).to(torch.int32).view(F32)
    return D._as16(bits, dtype)


def scale(r) -> torch.Tensor:
    return _as_float(scale_bits(r), r["sdt"])


def zero_point(r):
    """int8 (float8 for `f8`, `f8z`) of the scale's shape, or None"""
    if r["zp"] == "f8z":
        rows, _, _, G = layout(r)
        return torch.zeros((rows, G), dtype=torch.int8).view(F8)
    return D.zero_point(_drec(r))


def g_idx(r):
    return D.g_idx(_drec(r))


F8_TARGETS = 512  # a power of two: the odd step 77 reaches every one of them in any run of 512 positions


@functools.lru_cache(maxsize=None)
def f8_targets() -> torch.Tensor:
    """float32 (512,): the 256 float8 values (its two NaNs and both zeros among them), the 252 midpoints between neighbouring finite ones, +-480
    (beyond the clamp at 448) and +-1e-3 (below half the smallest subnormal: where the sign of an underflowed zero is decided)"""
    vals = torch.arange(256, dtype=torch.int64).to(torch.uint8).view(F8).float()
    finite = torch.sort(torch.unique(vals[~torch.isnan(vals)])).values  # 253 values, one zero
    mid = (finite[1:] + finite[:-1]) / 2
    t = torch.cat([vals, mid, torch.tensor([480.0, -480.0, 1e-3, -1e-3])])
    assert t.numel() == F8_TARGETS
    return t


def _step(m: int) -> int:
    """77, or 79 where 77 shares a factor with the modulus (7 bits: 264 = 8 * 3 * 11, under which 77 j takes 24 values only)"""
    import math

    return 77 if math.gcd(77, m) == 1 else 79


def target_index(r, gi, j) -> torch.Tensor:
    """int64: which float8 / FP4 target position (gi, j) holds"""
    h = ((gi * 2654435761) >> 15) & 0xFFFF
    if r["qtype"] == "fp8":
        # the groups gi, gi + 17, gi + 34, ... (in a cross: the groups of ONE edge scale) walk on through the table where the one before stopped,
        # so two groups of 256 hold all 512 targets between them
        g = r["group"] or r["shape"][1]
        return (77 * (j + g * (gi // 17)) + ((((gi % 17) * 2654435761) >> 15) & 0xFFFF)) % F8_TARGETS
    n = len(FP4_TARGETS)
    return (_step(n) * j + h) % n


def targets(r, gi, j) -> torch.Tensor:
    """float32, exact: the quotient position (gi, j) aims at, before the zero point"""
    h = ((gi * 2654435761) >> 15) & 0xFFFF
    if r["qtype"] == "fp8":
        return f8_targets()[target_index(r, gi, j)]
    if r["qtype"] == "fp4":
        return torch.tensor(FP4_TARGETS, dtype=torch.float32)[target_index(r, gi, j)]
    bits = r["bits"]
    m = 2 * ((1 << bits) + 4)
    return ((_step(m) * j + h) % m).float() / 2 - ((1 << (bits - 1)) + 2)


def weights(r, s=None, z=None) -> torch.Tensor:
    rows, cols, g, G = layout(r)
    s = scale(r) if s is None else s
    z = zero_point(r) if z is None else z
    col = D._perm(_drec(r))[None, :]
    cg = (col // g).expand(rows, cols)
    gi = (torch.arange(rows, dtype=torch.int64)[:, None] + r["row0"]) * G + cg
    j = (col % g).expand(rows, cols)
    t = targets(r, gi, j)
    if z is not None:
        t = t - torch.gather(z.float(), 1, cg)  # exact in fp32: half-integers below 2^9
    x = (t * torch.gather(effective_scale(r, s), 1, cg)).to(DTYPES[r["xdt"]])  # one fp32 product, one rounding to X
    h = ((gi * 2654435761) >> 15) & 0xFFFF
    bump = (5 * j + (h >> 7)) % 3 - 1
    if r["xdt"] == "f32":
        raw = x.view(torch.int32)
        raw += bump.to(torch.int32)  # wraps
        special = torch.tensor([0, -0x80000000, 0x7F800000, 0x7F800000 - 0x80000000, 0x7FC00000], dtype=torch.int64).to(torch.int32)
    else:
        raw = x.view(torch.int16)
        raw += bump.to(torch.int16)  # wraps
        e, m = _FMT[r["xdt"]]
        inf = ((1 << e) - 1) << m
        special = torch.tensor([0, -0x8000, inf, inf - 0x8000, inf | (1 << (m - 1))], dtype=torch.int64).to(torch.int16)
    tail = j - (g - 5)
    raw.copy_(torch.where(tail >= 0, special[tail.clamp(min=0)], raw))
    return x


def inputs(r) -> dict:
    s, z = scale(r), zero_point(r)
    return dict(x=weights(r, s, z), scale=s, zero_point=z, g_idx=g_idx(r))


def input_sha(t: dict) -> str:
    h = hashlib.sha256()
    for name in ("x", "scale", "zero_point", "g_idx"):
        if t[name] is not None:
            h.update(sha(t[name].view(torch.uint8) if t[name].dtype == F8 else t[name]).encode())
    return h.hexdigest()


def kw_of(r) -> dict:
    return dict(num_bits=r["bits"], strategy="group", group_size=r["group"]) if r["group"] else dict(num_bits=r["bits"], strategy="channel")


def oracle_outputs(O, r, t=None, ops=None) -> dict:
    """op -> the pinned oracle's answer (see `case_list` for the ops)"""
    t = t or inputs(r)
    kw = dict(kw_of(r), g_idx=t["g_idx"])
    x, s, z = t["x"], t["scale"], t["zero_point"]
    out = {}
    for op in ops or r["ops"]:
        if op in ("q", "pack"):
            if "q" not in out:
                out["q"] = O.quantize(x, s, z, dtype=torch.int8, **kw)
            if op == "pack":
                out["pack"] = O.pack_to_int32(out["q"], r["bits"]).contiguous()
        elif op == "q32":
            out[op] = O.quantize(x, s, z, dtype=torch.int32, **kw)
        elif op == "qx":
            out[op] = O.quantize(x, s, z, **kw)
        elif op == "fq":
            out[op] = O.fake_quantize(x, s, z, **kw)
        elif op in ("fp4", "fp4s"):
            if "fp4" not in out:
                c = O.fp4_compress(x, s, global_scale(r), fmt=fp4_format(r))
                out["fp4"], out["fp4s"] = c["weight_packed"], c["weight_scale"]
        elif op == "f8":
            out[op] = O.quantize(x, s, z, dtype=F8, qtype="float", **kw)
        elif op == "fq8":
            out[op] = O.fake_quantize(x, s, z, qtype="float", **kw)
        else:
            raise KeyError(op)
    return {op: out[op] for op in ops or r["ops"]}


# ---- what the manifest keeps -------------------------------------------------------------------------------------------------------------------
def code_stats(r, t, q: torch.Tensor) -> dict:
    """of the int8 codes of an integer case: the code histogram, the groups per number of distinct codes, and the share of elements whose
    quotient is NaN (a NaN weight, a NaN scale, 0 / 0, inf / inf) — the only elements a platform-defined answer could touch"""
    rows, cols, g, G = layout(r)
    bits = r["bits"]
    col_group = t["g_idx"].to(torch.int64) if t["g_idx"] is not None else torch.arange(cols) // g
    u = q.to(torch.int64) + (1 << (bits - 1))
    hist = torch.bincount(u.reshape(-1), minlength=1 << bits)
    seen = torch.zeros((rows, G, 1 << bits), dtype=torch.bool)
    seen[torch.arange(rows)[:, None].expand(rows, cols), col_group[None, :].expand(rows, cols), u] = True
    distinct = torch.bincount(seen.sum(dim=2).reshape(-1), minlength=(1 << bits) + 1)
    return dict(histogram=hist.tolist(), groups_by_distinct_codes={str(i): int(n) for i, n in enumerate(distinct.tolist()) if n})


def nan_quotient(r, t) -> torch.Tensor:
    """bool (rows, cols): the elements whose quotient x / s is NaN (a NaN weight, a NaN scale, 0 / 0, inf / inf)"""
    s = effective_scale(r, t["scale"])
    quot = t["x"].float() / s[:, (t["g_idx"].to(torch.int64) if t["g_idx"] is not None else torch.arange(r["shape"][1]) // layout(r)[2])]
    return torch.isnan(quot)


MASKED_OPS = ("q32", "fp4")


def masked(r, t, op: str, out: torch.Tensor) -> torch.Tensor:
    """THE mask of this fixture, and the only one: the cast of a NaN to int32 is platform-defined — x86's conversion gives INT_MIN (whose low
    byte, the int8 answer, is the 0 every platform agrees on), the GPU's saturating conversion and the oracle 0 — so an int32-typed `quantize`
    is not compared where the quotient is NaN: those elements are set to 0 on every side before the comparison.  Every other op passes through.
    FP4 codes have no NaN either: a NaN quotient has the magnitude 0 and the sign bit of a NaN — x86 divisions make it negative, the GPU
    positive — so bit 3 of exactly those nibbles is cleared on every side."""
    if op not in MASKED_OPS:
        return out
    nanq = nan_quotient(r, t).to(out.device)
    if op == "fp4":  # element 2 i in the low nibble of byte i
        keep = ~((nanq[:, 0::2].to(torch.uint8) << 3) | (nanq[:, 1::2].to(torch.uint8) << 7))
        return out & keep
    return out.masked_fill(nanq, 0)


def scale_stats(r, t) -> dict:
    s = t["scale"].float()
    quot = nan_quotient(r, t).to(torch.float32)
    return dict(nan_scales=int(torch.isnan(s).sum()), inf_scales=int(torch.isinf(s).sum()), groups=s.numel(),
                nan_quotients=int(quot.sum()), numel=quot.numel(),
                masked={op: int(nan_quotient(r, t).sum()) for op in r["ops"] if op in MASKED_OPS})


def record(out: torch.Tensor) -> dict:
    f = out.float()
    return dict(dtype=str(out.dtype).replace("torch.", ""), shape=list(out.shape), sha256=sha(canonical(out)),
                nans=int(torch.isnan(f).sum()), infs=int(torch.isinf(f).sum()), zeros=int((f == 0).sum()))


def stored_whole(r, op: str, out: torch.Tensor) -> bool:
    return r["scales"] == "cross" and out.numel() * out.element_size() <= WHOLE_MAX


@functools.lru_cache(maxsize=None)
def load_fixture():
    """(tensors of the `cross` outputs kept whole, keyed `case/op`; manifest)"""
    from safetensors.torch import load_file

    with open(os.path.join(GOLDEN, "compress_scales_manifest.json")) as f:
        manifest = json.load(f)
    return load_file(os.path.join(GOLDEN, "compress_scales.safetensors")), manifest


def fixture_mismatch(key: str, op: str, got: torch.Tensor) -> str:
    """"" if `got` is what the fixture records for the case's op: dtype, shape, canonical sha256, the NaN / inf / zero counts, and the canonical
    bits of the whole tensor where the fixture holds it"""
    tensors, manifest = load_fixture()
    want, mine = manifest["cases"][key]["out"][op], record(got.cpu())
    bad = [k for k in want if k != "whole" and want[k] != mine[k]]
    if not bad and want["whole"]:
        kept = tensors[f"{key}/{op}"]
        if not torch.equal(canonical(kept.view(got.dtype) if kept.dtype != got.dtype else kept), canonical(got.cpu())):
            bad.append("whole")
    return ", ".join(f"{k}: {mine.get(k)} != {want.get(k)}" for k in bad)
