"""The case matrix of the decompress-side scale fixture (tools/gen_golden_decompress_scales.py writes it, tests/test_decompress_scales.py and
tests/test_gpu_decompress_scales.py read it): what `decompress`, `dequantize_tensor` and `unpack_and_dequantize` are handed by a checkpoint — codes,
STORED scales and zero points — over the whole domain of the scales: +-0, subnormals, +-inf, every NaN, negative scales, products that overflow or
land in the subnormal range.

Everything is a pure integer function of a GLOBAL index, so a case that is a row window of a taller tensor (`row0`) holds exactly that tensor's rows:
  group gi = (row0 + row) * groups_per_row + group_in_row   element position j = column % code_group
  scale    `sweep16`: copy k = gi // 65536 of the sweep, pattern (p * 40503 + SALTS[k]) mod 65536 with p = gi mod 65536 — every 16-bit pattern exactly
           once per copy, and because 40503 is odd and large neighbouring groups, lanes and DPP rows hold unrelated patterns: a NaN's neighbours are
           ordinary numbers, and a kernel that picks the wrong entry of a wave's run gives different bits.
           `cross`: pair pi = gi mod (len(edge) * zero points): edge scale pi % len(edge) under zero point pi // len(edge) — with every code in every
           group that is every (edge scale, zero point, code) triple.  `sweeps` = n: n copies of the sweep first, the cross behind them.
           `sweep32` (fp32 scales): every exponent x mantissas {0, 1, 0x400000, 0x7FFFFF} x both signs, 2048 patterns, permuted by p * 1229 + 7.
  codes    ((j * 77 + (j >> bits) * 3 + h(gi)) mod 2^bits) - 2^(bits - 1): 77 is odd, so every aligned run of 2^bits positions holds every code;
           float8 codes are the same bytes, 0x7F, 0xFF (its NaNs) and 0x80 (-0) among them.
  zero points  hashed per group over the int8 range (`i8`), -8 .. 7 (`i4`: what a packed int4 zero point can hold), the width's own range (`ib`) or
           all 256 float8 bytes (`f8`); the cross takes them from the pair.
Scales and zero points are written as bit patterns, never through a Python float."""
import functools
import json
import math
import os

import torch

from _nonfinite_rtn_cases import BF16, F8, F16, F32, canonical, sha  # noqa: F401  (canonical / sha: the sibling case modules' own)

DTYPES = {"bf16": BF16, "f16": F16, "f32": F32}
SALTS = (12345, 40961, 7, 29989, 51111)  # one per copy of the sweep
SWEEP = 65536
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WHOLE_MAX = 80 * 1024  # a `cross` output of at most this many bytes is kept whole in decompress_scales.safetensors

# (exponent bits, mantissa bits)
_FMT = {"bf16": (8, 7), "f16": (5, 10)}


def edge(dtype: str) -> list:
    """the edge scales as 16-bit patterns: +-0, +- smallest and largest subnormal, +- smallest normal, +-1, +- largest finite, +-inf, the quiet NaN,
    the NaN of smallest payload, all ones"""
    e, m = _FMT[dtype]
    mant = (1 << m) - 1
    inf = ((1 << e) - 1) << m
    one = ((1 << (e - 1)) - 1) << m
    pos = [0, 1, mant, 1 << m, one, inf - 1, inf]  # 0, smallest and largest subnormal, smallest normal, 1, largest finite, inf
    out = []
    for p in pos:
        out += [p, p | 0x8000]
    return out + [inf | (1 << (m - 1)), inf | 1, 0xFFFF]


def sweep16_bits(copy: int = 0) -> torch.Tensor:
    """int64 (65536,): place in copy `copy` of the sweep -> 16-bit pattern; each pattern exactly once"""
    return (torch.arange(SWEEP, dtype=torch.int64) * 40503 + SALTS[copy]) % SWEEP


def _as16(bits: torch.Tensor, dtype: str) -> torch.Tensor:
    return (bits - ((bits >> 15) << 16)).to(torch.int16).view(DTYPES[dtype])


def sweep16(dtype: str, copy: int = 0) -> torch.Tensor:
    """(65536,) of `dtype`: every 16-bit pattern as a scale, in the sweep's order"""
    return _as16(sweep16_bits(copy), dtype)


def sweep32() -> torch.Tensor:
    """float32 (2048,): every exponent x mantissas {0, 1, 0x400000, 0x7FFFFF} x both signs"""
    b = sweep32_bits()
    return (b - ((b >> 31) << 32)).to(torch.int32).view(F32)


def sweep32_bits() -> torch.Tensor:
    """int64 (2048,): pattern number -> fp32 bits"""
    p = torch.arange(2048, dtype=torch.int64)
    mant = torch.tensor([0, 1, 0x400000, 0x7FFFFF], dtype=torch.int64)[p & 3]
    return ((p >> 10) << 31) | (((p >> 2) & 255) << 23) | mant


def _case(key, bits, shape, group, sdt, scales="sweep16", zp=None, ctype="int", **extra):
    r = dict(bits=bits, shape=list(shape), group=group, sdt=sdt, scales=scales, zp=zp, ctype=ctype, row0=0, sweeps=0, cgroup=None, g_idx=None, e8m0=False)
    r.update(extra)
    return key, r


def case_list():
    """[(key, recipe)] — recipe = dict(bits, ctype, shape, row0, group (None: channel-wise), cgroup, sdt, scales, sweeps, zp, g_idx, e8m0)"""
    out = []
    for dt in ("bf16", "f16"):
        # ---- W4
        for zp in (None, "i8", "i4"):
            out.append(_case(f"w4.g128.{zp or 'sym'}.{dt}", 4, (512, 16384), 128, dt, zp=zp))
        for zp in (None, "i8"):
            out.append(_case(f"w4.g128x2.{zp or 'sym'}.{dt}", 4, (1024, 16384), 128, dt, zp=zp))  # two copies of the sweep
            out.append(_case(f"w4.g128c.{zp or 'sym'}.{dt}", 4, (576, 16384), 128, dt, zp=zp, sweeps=1))  # the sweep, the cross in the last 64 rows
            # the last 512 rows of (2112, 16384): copy 3 of the sweep from row 1600, the cross in rows 2048 .. 2111
            out.append(_case(f"w4.g128.tail.{zp or 'sym'}.{dt}", 4, (512, 16384), 128, dt, zp=zp, row0=1600, sweeps=4))
            out.append(_case(f"w4.chan20.{zp or 'sym'}.{dt}", 4, (65536, 20), None, dt, zp=zp))
        out.append(_case(f"w4.g256.i8.{dt}", 4, (256, 65536), 256, dt, zp="i8"))
        out.append(_case(f"w4.g32.i8.{dt}", 4, (128, 16384), 32, dt, zp="i8"))
        out.append(_case(f"w4.g64.i8.{dt}", 4, (256, 16384), 64, dt, zp="i8"))
        out.append(_case(f"w4.gidx128.i8.{dt}", 4, (512, 16384), 128, dt, zp="i8", g_idx=3))
        out.append(_case(f"w4.gidx512.sym.{dt}", 4, (128, 65536), 128, dt, g_idx=5))
        out.append(_case(f"w4.cross.g128.sym.{dt}", 4, (8, 4608), 128, dt, scales="cross"))
        out.append(_case(f"w4.cross.g128.i4.{dt}", 4, (8, 4608), 128, dt, scales="cross", zp="i4"))
        out.append(_case(f"w4.cross.g128.i8.{dt}", 4, (128, 4352), 128, dt, scales="cross", zp="i8"))
        out.append(_case(f"w4.cross.g256.i8.{dt}", 4, (256, 4352), 256, dt, scales="cross", zp="i8"))
        out.append(_case(f"w4.cross.g32.i8.{dt}", 4, (32, 4352), 32, dt, scales="cross", zp="i8"))
        out.append(_case(f"w4.cross.g64.i8.{dt}", 4, (64, 4352), 64, dt, scales="cross", zp="i8"))
        out.append(_case(f"w4.cross.gidx.i8.{dt}", 4, (128, 4352), 128, dt, scales="cross", zp="i8", g_idx=9))
        out.append(_case(f"w4.cross.chan20.i8.{dt}", 4, (4352, 20), None, dt, scales="cross", zp="i8"))
        out.append(_case(f"w1.chan32.sym.{dt}", 1, (65536, 32), None, dt))
        out.append(_case(f"w1.chan20.sym.{dt}", 1, (65536, 20), None, dt))
        # ---- the other widths
        for b in (2, 3, 5, 6, 7):
            out.append(_case(f"w{b}.g128.sym.{dt}", b, (512, 16384), 128, dt))
            out.append(_case(f"w{b}.g64.sym.{dt}", b, (256, 16384), 64, dt))
            out.append(_case(f"w{b}.cross.g128.ib.{dt}", b, (1 << b, 17 * 128), 128, dt, scales="cross", zp="ib"))
        # ---- 8-bit: int8 codes (as bytes, or packed four to a word), float8 codes
        for zp in (None, "i8"):
            out.append(_case(f"q8.chan256.{zp or 'sym'}.{dt}", 8, (65536, 256), None, dt, zp=zp))
            out.append(_case(f"q8.g128.{zp or 'sym'}.{dt}", 8, (512, 16384), 128, dt, zp=zp, cgroup=256))
            out.append(_case(f"q8.g256.{zp or 'sym'}.{dt}", 8, (512, 32768), 256, dt, zp=zp))
        # the sweep, the cross in the last 4352 rows
        out.append(_case(f"q8.chan256c.i8.{dt}", 8, (65536 + 4352, 256), None, dt, zp="i8", sweeps=1))
        out.append(_case(f"f8.chan256c.f8.{dt}", 8, (65536 + 4352, 256), None, dt, zp="f8", ctype="fp8", sweeps=1))
        out.append(_case(f"q8.chan20.i8.{dt}", 8, (65536, 20), None, dt, zp="i8"))
        out.append(_case(f"q8.chan12.i8.{dt}", 8, (65536, 12), None, dt, zp="i8"))
        out.append(_case(f"q8.cross.g256.sym.{dt}", 8, (8, 4352), 256, dt, scales="cross"))
        out.append(_case(f"q8.cross.g256.i8.{dt}", 8, (256, 4352), 256, dt, scales="cross", zp="i8"))
        out.append(_case(f"q8.cross.chan12.i8.{dt}", 8, (4352, 12), None, dt, scales="cross", zp="i8"))
        for zp in (None, "f8"):
            out.append(_case(f"f8.chan256.{zp or 'sym'}.{dt}", 8, (65536, 256), None, dt, zp=zp, ctype="fp8"))
            out.append(_case(f"f8.g128.{zp or 'sym'}.{dt}", 8, (512, 16384), 128, dt, zp=zp, ctype="fp8", cgroup=256))
        out.append(_case(f"f8.cross.g256.sym.{dt}", 8, (8, 4352), 256, dt, scales="cross", ctype="fp8"))
        out.append(_case(f"f8.cross.g256.f8.{dt}", 8, (256, 4352), 256, dt, scales="cross", zp="f8", ctype="fp8"))
    # ---- fp32 scales, fp32 output
    for zp in (None, "i8"):
        out.append(_case(f"w4.f32.g128.{zp or 'sym'}", 4, (64, 4096), 128, "f32", scales="sweep32", zp=zp))
        out.append(_case(f"q8.f32.g256.{zp or 'sym'}", 8, (64, 8192), 256, "f32", scales="sweep32", zp=zp))
    for zp in (None, "f8"):
        out.append(_case(f"f8.f32.g256.{zp or 'sym'}", 8, (64, 8192), 256, "f32", scales="sweep32", zp=zp, ctype="fp8"))
    # ---- MXFP8: all 256 E8M0 bytes (one per row; 255 is NaN, 0 is 2^-127, a bfloat16 subnormal) x all 256 float8 codes
    out.append(_case("mxfp8.e8m0", 8, (256, 8192), 32, "bf16", scales="e8m0", ctype="fp8", cgroup=256, e8m0=True))
    return out


def is_sweep16(r) -> bool:
    return r["scales"] == "sweep16" and r["row0"] == 0


def _zp_range(r):
    if r["zp"] is None:
        return None
    if r["zp"] in ("i8", "f8"):
        return -128, 256
    if r["zp"] == "i4":
        return -8, 16
    return -(1 << (r["bits"] - 1)), 1 << r["bits"]


def layout(r):
    """(rows, cols, group, groups per row)"""
    rows, cols = r["shape"]
    g = r["group"] or cols
    return rows, cols, g, cols // g


def group_index(r) -> torch.Tensor:
    rows, cols, g, G = layout(r)
    return (torch.arange(rows, dtype=torch.int64)[:, None] + r["row0"]) * G + torch.arange(G, dtype=torch.int64)[None, :]


def _cross_pair(r, gi):
    """pair number, or -1 where the group belongs to a copy of the sweep"""
    if r["scales"] != "cross" and not r["sweeps"]:
        return torch.full_like(gi, -1)
    n = len(edge(r["sdt"])) * (_zp_range(r)[1] if r["zp"] else 1)
    if r["scales"] == "cross":
        return gi % n
    return torch.where(gi >= r["sweeps"] * SWEEP, (gi - r["sweeps"] * SWEEP) % n, torch.full_like(gi, -1))


def scale_bits(r) -> torch.Tensor:
    """int64 (rows, groups per row): the scale's bit pattern"""
    gi = group_index(r)
    if r["scales"] == "sweep32":
        return sweep32_bits()[(gi % 2048 * 1229 + 7) % 2048]
    if r["scales"] == "e8m0":
        return ((gi // layout(r)[3]) * 77 + 5) % 256  # constant per row
    salt = torch.tensor(SALTS, dtype=torch.int64)[(gi // SWEEP).clamp(max=len(SALTS) - 1)]
    bits = ((gi % SWEEP) * 40503 + salt) % SWEEP
    pair = _cross_pair(r, gi)
    e = torch.tensor(edge(r["sdt"]), dtype=torch.int64)
    return torch.where(pair >= 0, e[pair.clamp(min=0) % len(e)], bits)


def scale(r) -> torch.Tensor:
    b = scale_bits(r)
    if r["scales"] == "e8m0":
        return b.to(torch.uint8)
    if r["sdt"] == "f32":
        return (b - ((b >> 31) << 32)).to(torch.int32).view(F32)
    return _as16(b, r["sdt"])


def zero_point(r):
    """int8 (float8 for `f8`) of the scale's shape, or None"""
    if r["zp"] is None:
        return None
    lo, n = _zp_range(r)
    gi = group_index(r)
    z = ((gi * 2246822519 + 374761393) >> 13) % n
    if r["scales"] == "cross" or r["sweeps"]:
        pair = _cross_pair(r, gi)
        z = torch.where(pair >= 0, pair.clamp(min=0) // len(edge(r["sdt"])), z)
    z = (z + lo).to(torch.int8)
    return z.view(F8) if r["zp"] == "f8" else z


def codes(r) -> torch.Tensor:
    """int8 (rows, cols) in the width's range, or float8 of the same bytes"""
    rows, cols, g, G = layout(r)
    bits = r["bits"]
    cg = r["cgroup"] or g
    col = _perm(r)[None, :]  # (activation ordering: a column's place in ITS group)
    ci = (torch.arange(rows, dtype=torch.int64)[:, None] + r["row0"]) * (cols // cg) + col // cg  # the code group's global number
    j = col % cg
    h = ((ci * 2654435761) >> 15) & 255
    q = ((j * 77 + (j >> bits) * 3 + h) % (1 << bits) - (1 << (bits - 1))).to(torch.int8)
    return q.view(F8) if r["ctype"] == "fp8" else q


def _perm(r) -> torch.Tensor:
    """int64 (cols,): a column's place in the group order — the identity without activation ordering, else the multiplicative permutation
    (c * 2654435761 + salt) mod cols (the multiplier is a prime that divides no width used here)"""
    cols = r["shape"][1]
    c = torch.arange(cols, dtype=torch.int64)
    if r["g_idx"] is None:
        return c
    assert math.gcd(2654435761, cols) == 1
    return (c * 2654435761 + r["g_idx"]) % cols


def g_idx(r):
    """int32 (cols,) or None: a balanced activation ordering — column c belongs to group _perm(c) // group"""
    return None if r["g_idx"] is None else (_perm(r) // layout(r)[2]).to(torch.int32)


def inputs(r) -> dict:
    return dict(q=codes(r), scale=scale(r), zero_point=zero_point(r), g_idx=g_idx(r))


def input_sha(t: dict) -> str:
    import hashlib

    h = hashlib.sha256()
    for name in ("q", "scale", "zero_point", "g_idx"):
        if t[name] is not None:
            h.update(sha(t[name].view(torch.uint8) if t[name].dtype == F8 else t[name]).encode())
    return h.hexdigest()


def oracle_output(O, r, t=None) -> torch.Tensor:
    """the pinned oracle's `dequantize` of the case (MXFP8: under its decoded exponents)"""
    t = t or inputs(r)
    s = O.e8m0_decode(t["scale"]) if r["e8m0"] else t["scale"]
    if r["group"] is None:
        return O.dequantize(t["q"], s, t["zero_point"], strategy="channel")
    return O.dequantize(t["q"], s, t["zero_point"], strategy="group", group_size=r["group"], g_idx=t["g_idx"])


def counts(t: torch.Tensor) -> dict:
    f = t.float()
    return dict(nans=int(torch.isnan(f).sum()), infs=int(torch.isinf(f).sum()),
                subnormals=int(((f != 0) & (f.abs() < torch.finfo(t.dtype).tiny)).sum()), numel=t.numel())


def record(out: torch.Tensor) -> dict:
    """what the manifest keeps of an output"""
    return dict(dtype=str(out.dtype).replace("torch.", ""), shape=list(out.shape), sha256=sha(canonical(out)), **counts(out))


def stored_whole(key: str, r, out: torch.Tensor) -> bool:
    return r["scales"] == "cross" and out.numel() * out.element_size() <= WHOLE_MAX


@functools.lru_cache(maxsize=None)
def load_fixture():
    """(tensors of the `cross` outputs kept whole, manifest)"""
    from safetensors.torch import load_file

    with open(os.path.join(GOLDEN, "decompress_scales_manifest.json")) as f:
        manifest = json.load(f)
    return load_file(os.path.join(GOLDEN, "decompress_scales.safetensors")), manifest


def fixture_mismatch(key: str, got: torch.Tensor) -> str:
    """"" if `got` is what the fixture records for the case: dtype, shape, canonical sha256 and the NaN / inf / subnormal counts, and the canonical
    bits of the whole tensor where the fixture holds it"""
    tensors, manifest = load_fixture()
    want, mine = manifest["cases"][key]["out"], record(got.cpu())
    bad = [k for k in want if k != "whole" and want[k] != mine[k]]
    if not bad and want["whole"] and not torch.equal(canonical(tensors[key]), canonical(got.cpu())):
        bad.append("whole")
    return ", ".join(f"{k}: {mine.get(k)} != {want.get(k)}" for k in bad)
