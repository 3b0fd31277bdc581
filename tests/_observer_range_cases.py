"""The case matrix of the observer-range fixture (tools/gen_golden_observer_ranges.py writes it, tests/test_observer_ranges.py and
tests/test_gpu_observer_ranges.py read it): what the kernels that COMPUTE a scale and a zero point from the weight — `minmax_qparams`,
`minmax_qparams_float`, `generate_gparam` and the observer halves of the one-pass RTN kernels — are handed, over the whole domain of a group's
extremes: subnormal ranges, ranges whose scale overflows the dtype, `mx - mn` overflowing in fp16, all-zero groups (0 / 0 in the zero point),
one-sided groups, +-inf, every NaN.  The pattern side is the sibling modules' (`sweep16`, `sweep16_bits`, `sweep32`, `edge`, `_as16`, `canonical`,
`sha`; the fp32 edges of `_compress_scale_cases`), imported, not copied.

A group's result depends only on its minimum, its maximum and whether it holds a NaN, so a case plants an EXTREME and a PARTNER in every group and
fills the rest below them.  Everything is a pure integer function of a GLOBAL index, written as a bit pattern:
  group gi = row * groups_per_row + group_in_row (a block case: block row * blocks per row + block), position j within the group of `glen`
  elements (a ragged last group is shorter)
  extreme  `sweep16`: pattern sweep16_bits(0)[gi] — every 16-bit pattern once.  `exp16`: every exponent x significand {0, 1, half, all ones} x
           sign (2048 bf16 patterns, 256 f16), permuted by p * 1229 + 7.  `sweep32`: the sibling's 2048 fp32 patterns under the same
           permutation.  At position (77 gi + salt) mod glen (`last`: the group's last position).
  partner  the opposite sign, magnitude finite edge (5 gi + 3) mod 6 of {0, smallest subnormal, largest subnormal, smallest normal, 1, largest
           finite}, glen / 2 + 5 positions further: in another 16-byte unit — another lane of the per-unit kernels — in every group of 32 or
           more elements (of 16: in 3 groups of 8).
  fill     (`graded`) position j of sign s — s from a hash of (gi, j) — holds magnitude (mag_s * ((37 j + h(gi)) mod 256)) >> 8, mag_s the
           magnitude bits of the planted value of that sign (the largest finite pattern where that is NaN or inf): never above it.
  `cross`  all 289 ordered pairs of the 17 edge patterns: extreme edge[gi mod 17], partner edge[gi div 17 mod 17], (`copy` fill) every other
           position a copy of the extreme (of the partner where the extreme is a NaN): one-sided groups, all-zero groups, inf with -inf, NaN
           with inf, negative NaN.
  `ties`   INT, asymmetric: for each width b, each k < 2^b and e in {-7, 0, 6}: mn = -(2 k + 1) 2^e, mx = (2 (2^b - 1) - (2 k + 1)) 2^e, which
           puts mn / scale at or next to a half-integer; whatever rounding to the dtype makes of them is the input (`copy` fill).
So a group's min and max are exactly its two planted values, up to the sign of a zero; tests/test_observer_ranges.py asserts it."""
import functools
import json
import os

import torch

import _compress_scale_cases as C
import _decompress_scale_cases as D
from _decompress_scale_cases import BF16, F8, F16, F32, _as16, canonical, edge, sha, sweep16, sweep16_bits, sweep32  # noqa: F401

DTYPES = D.DTYPES
GOLDEN = D.GOLDEN
SWEEP = D.SWEEP
_FMT = {"bf16": (8, 7), "f16": (5, 10), "f32": (8, 23)}
# NVFP4 global scales as fp32 bit patterns (`gen`: generate_gparam of the case's finite part, computed)
NV_GLOBALS = {"one": 0x3F800000, "lo": 0x3A800000, "mid": 0x44600000, "hi": 0x45800000, "gen": None}  # 1, 2^-10, 896, 2^12
TIE_EXPONENTS = (-7, 0, 6)
CHUNK = 1 << 21  # elements built at a time


def fmt(dt):
    """(sign bit, inf pattern, pattern of 1, mantissa bits)"""
    e, m = _FMT[dt]
    return 1 << (e + m), ((1 << e) - 1) << m, ((1 << (e - 1)) - 1) << m, m


def finite_edges(dt) -> list:
    """0, smallest subnormal, largest subnormal, smallest normal, 1, largest finite — as magnitude bits"""
    _, inf, one, m = fmt(dt)
    return [0, 1, (1 << m) - 1, 1 << m, one, inf - 1]


def edge_bits(dt) -> list:
    return C.edge_bits(dt)


def as_float(bits: torch.Tensor, dt: str) -> torch.Tensor:
    return C._as_float(bits, dt) if dt == "f32" else _as16(bits, dt)


def exp16_bits(dt) -> torch.Tensor:
    """int64: every exponent x significand {0, 1, half, all ones} x sign of a 16-bit dtype, permuted"""
    e, m = _FMT[dt]
    n = 1 << (e + 3)
    p = torch.arange(n, dtype=torch.int64)
    sig = torch.tensor([0, 1, 1 << (m - 1), (1 << m) - 1], dtype=torch.int64)[p & 3]
    bits = ((p >> (e + 2)) << 15) | (((p >> 2) & ((1 << e) - 1)) << m) | sig
    return bits[(p * 1229 + 7) % n]


def sweep32_perm() -> torch.Tensor:
    p = torch.arange(2048, dtype=torch.int64)
    return D.sweep32_bits()[(p * 1229 + 7) % 2048]


def tie_pairs(dt) -> tuple:
    """(mn bits, mx bits), int64 (1530,): the `ties` groups, widths 1 .. 8 one after the other"""
    mn, mx = [], []
    for b in range(1, 9):
        for k in range(1 << b):
            for e in TIE_EXPONENTS:
                mn.append(-(2 * k + 1) * 2.0 ** e)
                mx.append((2 * ((1 << b) - 1) - (2 * k + 1)) * 2.0 ** e)
    out = []
    for v in (mn, mx):
        t = torch.tensor(v, dtype=torch.float64).to(DTYPES[dt])
        out.append(t.view(torch.int16).to(torch.int64) & 0xFFFF)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pattern(pat: str, dt: str) -> tuple:
    """(extreme bits, partner bits or None) int64 (n,): group gi holds entry gi mod n; a partner of None is the finite edge of the other sign"""
    if pat == "sweep16":
        return sweep16_bits(0), None
    if pat == "exp16":
        return exp16_bits(dt), None
    if pat == "sweep32":
        return sweep32_perm(), None
    if pat == "cross":
        e = torch.tensor(edge_bits(dt), dtype=torch.int64)
        gi = torch.arange(len(e) ** 2)
        return e[gi % len(e)], e[gi // len(e)]
    if pat == "ties":
        return tie_pairs(dt)
    raise KeyError(pat)


def _case(key, dt, pat, shape, group, ops, **extra):
    r = dict(dt=dt, pat=pat, shape=list(shape), group=group, ops=list(ops), salt=11, last=False, block=None, built=None, fill="copy" if pat in ("cross", "ties") else "graded")
    r.update(extra)
    return key, r


def int_ops(widths, syms="sa") -> list:
    return [f"i{b}{s}" for b in widths for s in syms]


ALL = range(1, 9)
# rows a wave reduces in trips of 512 units (eight 16-byte loads per lane) and a tail of four or eight loads: 96 a 4-load tail of one live load, 1992 one
# whose last load is live, 2056 an 8-load tail of five live loads, 4000 one whose last load is live, 4096 one trip and no tail, 5632 a trip and a short
# tail, 6496 a trip and a long tail
CHANNEL_WIDTHS = (96, 1992, 2056, 4000, 4096, 5632, 6496)
NV_OPS = [f"nv.{n}" for n in NV_GLOBALS]


def case_list():
    """[(key, recipe)] — recipe = dict(dt, pat, shape, group (None: the row), block ([bh, bw]: the groups are the blocks), fill, salt, last, ops);
    an op is `i<bits><s|a>` (INT, symmetric / asymmetric), `fp8`, `mxfp4`, `mxfp8` or `nv.<global scale>`"""
    out = []
    for dt in ("bf16", "f16"):
        n = len(pattern("exp16", dt)[0])  # 2048 / 256
        er = 64 if dt == "bf16" else 8    # rows of an exp16 case of 32 groups per row
        out.append(_case(f"s16.g32.{dt}", dt, "sweep16", (512, 4096), 32, int_ops(ALL) + ["fp8", "mxfp4", "mxfp8"]))
        out.append(_case(f"s16.g8.{dt}", dt, "sweep16", (512, 1024), 8, int_ops((4, 8)), salt=3))
        out.append(_case(f"s16.g16.{dt}", dt, "sweep16", (512, 2048), 16, int_ops((4, 8)) + NV_OPS, salt=5))
        out.append(_case(f"s16.g128.{dt}", dt, "sweep16", (512, 16384), 128, int_ops(range(2, 9)) + ["fp8"], salt=7))
        out.append(_case(f"s16.chan20.{dt}", dt, "sweep16", (65536, 20), None, int_ops((4, 8)), salt=9))
        out.append(_case(f"s16.blk4x16.{dt}", dt, "sweep16", (4096, 1024), None, int_ops((8,)) + ["fp8"], block=[4, 16], salt=13))
        out.append(_case(f"e16.g512.{dt}", dt, "exp16", (er, 32 * 512), 512, int_ops((4, 8), "s")))
        out.append(_case(f"e16.row.g32.{dt}", dt, "exp16", (1, (n + 1) * 32), 32, int_ops((4, 8), "s")))
        out.append(_case(f"e16.g2048.{dt}", dt, "exp16", (er, 32 * 2048), 2048, int_ops((4, 8))))
        out.append(_case(f"e16.g1024.{dt}", dt, "exp16", (er, 32 * 1024), 1024, int_ops((4, 8), "s")))
        for cols in CHANNEL_WIDTHS:
            out.append(_case(f"e16.chan{cols}.{dt}", dt, "exp16", (n, cols), None, int_ops((4, 8)) + ["fp8"], salt=cols % 89))
        # the `tensor` strategy: the exp16 tensor of groups of 32 (`built`), observed as ONE row
        out.append(_case(f"e16.tensor.{dt}", dt, "exp16", (1, n * 32), None, int_ops((4, 8)), built=dict(shape=[er, 32 * 32], group=32)))
        out.append(_case(f"e16.blk128.{dt}", dt, "exp16", (er * 128, 32 * 128), None, int_ops((8,)) + ["fp8"], block=[128, 128]))
        out.append(_case(f"ties.g32.{dt}", dt, "ties", (90, 17 * 32), 32, int_ops(ALL, "a")))
        out.append(_case(f"c16.g16.{dt}", dt, "cross", (17, 34 * 16), 16, NV_OPS))
        out.append(_case(f"c16.g32.{dt}", dt, "cross", (17, 17 * 32), 32, int_ops(range(2, 9)) + ["fp8", "mxfp4", "mxfp8"]))
        out.append(_case(f"c16.g128.{dt}", dt, "cross", (17, 17 * 128), 128, int_ops(range(2, 9)) + ["fp8"]))
        out.append(_case(f"c16.g48.{dt}", dt, "cross", (97, 100), 48, int_ops((4, 8))))
        out.append(_case(f"c16.g20.{dt}", dt, "cross", (58, 100), 20, int_ops((4, 8))))
        out.append(_case(f"c16.blk16x64.{dt}", dt, "cross", (17 * 16, 17 * 64), None, int_ops((8,)) + ["fp8"], block=[16, 64]))
    f32 = ["fp8", "mxfp4", "mxfp8"]
    out.append(_case("s32.g32", "f32", "sweep32", (64, 1024), 32, int_ops((4, 8)) + f32))
    out.append(_case("s32.g128", "f32", "sweep32", (64, 4096), 128, int_ops((4, 8))))
    out.append(_case("s32.g8", "f32", "sweep32", (64, 256), 8, int_ops((4, 8))))
    out.append(_case("s32.chan96", "f32", "sweep32", (2048, 96), None, int_ops((4, 8))))
    out.append(_case("c32.g32", "f32", "cross", (17, 17 * 32), 32, int_ops((4, 8)) + f32))
    out.append(_case("c32.g128", "f32", "cross", (17, 17 * 128), 128, int_ops((4, 8))))
    out.append(_case("c32.g8", "f32", "cross", (17, 17 * 8), 8, int_ops((4, 8))))
    out.append(_case("c32.chan5632", "f32", "cross", (289, 5632), None, int_ops((4, 8))))
    return out


def gparam_shapes():
    return ((4, 64), (3, 20))


def gparam_case(dt: str, shape) -> dict:
    """the `generate_gparam` inputs: one tensor of `shape` per exp16 pattern and per edge, the extreme its LAST element — built as one group each"""
    n = len(pattern("exp16", dt)[0]) + len(edge_bits(dt))
    return dict(dt=dt, pat="gparam", shape=[n, shape[0] * shape[1]], group=None, ops=[], salt=11, last=True, block=None, built=None, fill="graded")


@functools.lru_cache(maxsize=None)
def _gparam_pattern(dt):
    return torch.cat([pattern("exp16", dt)[0], torch.tensor(edge_bits(dt), dtype=torch.int64)]), None


def is_sweep16(r) -> bool:
    return r["pat"] == "sweep16"


def layout(r):
    """(group rows, group cols, group, groups per row) of the matrix whose rows hold the groups one after the other: the weight itself, or for a
    block case the blocks as rows"""
    rows, cols = r["shape"]
    if r["block"]:
        bh, bw = r["block"]
        return (rows // bh) * (cols // bw), bh * bw, bh * bw, 1
    g = r["group"] or cols
    return rows, cols, g, -(-cols // g)


def planted_bits(r) -> tuple:
    """(extreme, partner) int64 (group rows, groups per row): the two planted bit patterns of every group"""
    rows, cols, g, G = layout(r)
    ext, par = _gparam_pattern(r["dt"]) if r["pat"] == "gparam" else pattern(r["pat"], r["dt"])
    gi = torch.arange(rows, dtype=torch.int64)[:, None] * G + torch.arange(G, dtype=torch.int64)[None, :]
    E = ext[gi % len(ext)]
    if par is not None:
        return E, par[gi % len(ext)]
    sign = fmt(r["dt"])[0]
    mag = torch.tensor(finite_edges(r["dt"]), dtype=torch.int64)[(5 * gi + 3) % 6]
    return E, mag | (sign - (E & sign))  # the opposite sign


def planted(r) -> tuple:
    E, P = planted_bits(r)
    return as_float(E, r["dt"]), as_float(P, r["dt"])


def positions(r) -> tuple:
    """(extreme's, partner's position, group length) int64 (group rows, groups per row)"""
    rows, cols, g, G = layout(r)
    gi = torch.arange(rows, dtype=torch.int64)[:, None] * G + torch.arange(G, dtype=torch.int64)[None, :]
    glen = torch.minimum(torch.tensor(g), cols - torch.arange(G, dtype=torch.int64) * g)[None, :].expand(rows, G)
    pe = glen - 1 if r["last"] else (77 * gi + r["salt"]) % glen
    pp = (pe + glen // 2 + 5) % glen
    assert bool((pe != pp).all())
    return pe, pp, glen


def _rows(r, lo: int, hi: int, E, P, pe, pp) -> torch.Tensor:
    """int64 (hi - lo, group cols): the bit patterns of group rows lo .. hi"""
    rows, cols, g, G = layout(r)
    sign, inf, _, _ = fmt(r["dt"])
    col = torch.arange(cols, dtype=torch.int64)
    cg, j = col // g, (col % g)[None, :]
    E, P, pe, pp = (t[lo:hi][:, cg] for t in (E, P, pe, pp))
    if r["fill"] == "copy":
        fill = torch.where((E & (sign - 1)) > inf, P, E)
    else:
        gi = (torch.arange(lo, hi, dtype=torch.int64)[:, None] * G + cg[None, :])
        h = ((gi * 2654435761) >> 15) & 0xFFFF
        s = (((j * 40503 + h * 31) >> 4) & 1) * sign
        mag = torch.where((E & sign) == s, E, P) & (sign - 1)  # the planted value of that sign (the partner's is the other one)
        mag = torch.clamp(mag, max=inf - 1)
        fill = ((mag * ((37 * j + h) & 255)) >> 8) | s
    return torch.where(j == pe, E, torch.where(j == pp, P, fill))


def group_matrix_bits(r) -> torch.Tensor:
    rows, cols, g, G = layout(r)
    E, P = planted_bits(r)
    pe, pp, _ = positions(r)
    step = max(1, CHUNK // cols)
    store = torch.int32 if r["dt"] == "f32" else torch.int16
    wrap = 32 if r["dt"] == "f32" else 16
    out = torch.empty((rows, cols), dtype=store)
    for lo in range(0, rows, step):
        b = _rows(r, lo, min(rows, lo + step), E, P, pe, pp)
        out[lo:lo + step] = (b - ((b >> (wrap - 1)) << wrap)).to(store)
    return out


def from_groups(r, m: torch.Tensor) -> torch.Tensor:
    """the weight of a case from its group matrix (a block case: the blocks laid out as blocks)"""
    if not r["block"]:
        return m
    (R, Cc), (bh, bw) = r["shape"], r["block"]
    return m.reshape(R // bh, Cc // bw, bh, bw).permute(0, 2, 1, 3).reshape(R, Cc).contiguous()


def to_groups(r, x: torch.Tensor) -> torch.Tensor:
    """the groups of a case's weight as rows (a block case: `_block_rows` restated for whole blocks)"""
    if not r["block"]:
        return x
    (R, Cc), (bh, bw) = r["shape"], r["block"]
    return x.reshape(R // bh, bh, Cc // bw, bw).permute(0, 2, 1, 3).reshape(-1, bh * bw).contiguous()


def grid(r) -> tuple:
    """the shape of a case's scale table"""
    if r["block"]:
        return (r["shape"][0] // r["block"][0], r["shape"][1] // r["block"][1])
    return (layout(r)[0], layout(r)[3])


def built(r) -> dict:
    """the recipe a case's weight is built from: its own, unless the case observes a tensor built of smaller groups under another shape"""
    return dict(r, **r["built"], built=None) if r.get("built") else r


def weight(r) -> torch.Tensor:
    b = built(r)
    return from_groups(b, group_matrix_bits(b).view(DTYPES[r["dt"]])).reshape(r["shape"])


def group_minmax(r, x: torch.Tensor) -> tuple:
    """torch.aminmax of every group, (group rows, groups per row) each — what a min-max observer hands `calculate_qparams`"""
    m = to_groups(r, x)
    rows, cols, g, G = layout(r)
    if cols % g == 0:
        return torch.aminmax(m.unflatten(-1, (G, g)), dim=-1)
    mm = [torch.aminmax(m[:, c:c + g], dim=-1) for c in range(0, cols, g)]
    return torch.stack([a for a, _ in mm], dim=1), torch.stack([b for _, b in mm], dim=1)


def nan_groups(r, x: torch.Tensor) -> torch.Tensor:
    """bool, of the scale table's shape: the groups that hold a NaN"""
    return torch.isnan(group_minmax(r, x)[0]).reshape(grid(r))


def finite_part(x: torch.Tensor) -> torch.Tensor:
    return torch.where(torch.isfinite(x), x, torch.zeros_like(x))


def parse_op(op: str) -> dict:
    if op[0] == "i":
        return dict(kind="int", bits=int(op[1]), symmetric=op[2] == "s")
    if op.startswith("nv."):
        return dict(kind="nvfp4", gs=op[3:])
    return dict(kind=op)


def global_scale(O, r, x, op):
    """float32 (1,): the global scale of an `nv.*` op"""
    name = parse_op(op)["gs"]
    if NV_GLOBALS[name] is None:
        return O.generate_gparam(finite_part(x))
    return torch.tensor([NV_GLOBALS[name]], dtype=torch.int64).to(torch.int32).view(F32)


def oracle_output(O, r, x, op) -> tuple:
    """(scale, zero point or None) of the pinned oracle, of the scale table's shape"""
    p = parse_op(op)
    m = to_groups(r, x)
    g = None if r["block"] else r["group"]
    if p["kind"] == "int":
        s, z = O.calculate_qparams_minmax(m, num_bits=p["bits"], group_size=g, symmetric=p["symmetric"])
        return s.reshape(grid(r)), z.reshape(grid(r))
    gs = global_scale(O, r, x, op) if p["kind"] == "nvfp4" else None
    return O.calculate_qparams_float(m, kind=p["kind"], group_size=g, global_scale=gs).reshape(grid(r)), None


# ---- what the manifest keeps -------------------------------------------------------------------------------------------------------------------
MASKED_OPS = ("mxfp4", "mxfp8")


def masked(r, x, op: str, scale: torch.Tensor) -> torch.Tensor:
    """THE mask of this fixture, and the only one: the MX scale of a group that holds a NaN rests on the reference's cast of a NaN to uint8, which
    its vector and scalar loops evaluate differently (inf in a small tensor, 2^-127 or 1 in a large one; the project pins inf) — those scales are
    set to 0 on every side before the comparison WITH THE REFERENCE'S RECORD.  Kernel and oracle are compared whole."""
    if op not in MASKED_OPS:
        return scale
    return scale.masked_fill(nan_groups(r, x).to(scale.device), 0)


def eps_of(dt: str) -> float:
    return torch.finfo(DTYPES[dt]).eps


def record(r, op, scale: torch.Tensor, zp) -> dict:
    f = scale.float()
    out = dict(dtype=str(scale.dtype).replace("torch.", ""), shape=list(scale.shape), sha256=sha(canonical(scale)), nans=int(torch.isnan(f).sum()),
               infs=int(torch.isinf(f).sum()), zeros=int((f == 0).sum()))
    if op[0] == "i":
        out["eps"] = int((f == eps_of(r["dt"])).sum())
        out["zp_sha256"] = sha(zp)
        out["zps"] = int(torch.unique(zp).numel())
    return out


def stored_whole(r) -> bool:
    return r["pat"] == "cross"


@functools.lru_cache(maxsize=None)
def load_fixture():
    """(tensors of the `cross` outputs kept whole, keyed `case/op/scale` and `case/op/zp`; manifest)"""
    from safetensors.torch import load_file

    with open(os.path.join(GOLDEN, "observer_ranges_manifest.json")) as f:
        manifest = json.load(f)
    return load_file(os.path.join(GOLDEN, "observer_ranges.safetensors")), manifest


def fixture_mismatch(key: str, op: str, r, x, scale: torch.Tensor, zp) -> str:
    """"" if (scale, zero point) is what the fixture records for the case's op: dtype, shape, canonical sha256, the NaN / inf / zero / eps counts,
    the zero points' sha256, and the canonical bits of the whole tensors where the fixture holds them (`cross`)"""
    tensors, manifest = load_fixture()
    scale = masked(r, x, op, scale.cpu())
    zp = None if zp is None else zp.cpu()
    want, mine = manifest["cases"][key]["out"][op], record(r, op, scale, zp)
    bad = [k for k in want if k != "whole" and want[k] != mine[k]]
    if not bad and want["whole"]:
        if not torch.equal(canonical(tensors[f"{key}/{op}/scale"]), canonical(scale)):
            bad.append("whole")
        if zp is not None and not torch.equal(tensors[f"{key}/{op}/zp"], zp):
            bad.append("whole zp")
    return ", ".join(f"{k}: {mine.get(k)} != {want.get(k)}" for k in bad)


def gparam_mismatch(dt: str, shape, got: torch.Tensor) -> str:
    want = load_fixture()[1]["gparam"][f"{dt}.{shape[0]}x{shape[1]}"]
    mine = gparam_record(got.cpu())
    return ", ".join(f"{k}: {mine[k]} != {want[k]}" for k in mine if want[k] != mine[k])


def gparam_record(gs: torch.Tensor) -> dict:
    return dict(dtype=str(gs.dtype).replace("torch.", ""), shape=list(gs.shape), sha256=sha(canonical(gs)), ones=int((gs == 1).sum()))
