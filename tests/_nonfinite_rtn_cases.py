"""The case matrix of the non-finite round-to-nearest fixture (tools/gen_golden_nonfinite_rtn.py writes it, tests/test_nonfinite_rtn.py and
tests/test_gpu_nonfinite_rtn.py read it): NaN and +-inf weights through every one-pass dense-checkpoint quantizer.  A case is one weight: an
integer-synthesised finite base (the formula of tests/_packw_rtn_cases.make_weight) with `plant` writing BIT PATTERNS into chosen regions — a
region is a group, a row or a block, i.e. what one scale is computed over.  One weight carries many plants, one per row (or per block), every
planted group of a row of three has an untouched neighbour on each side, and every weight of more than one row has an untouched last row.

Where a plant sits, from the kernels' own lane arithmetic (csrc/ct_quant.hip, ct_quant_wb.hip, ct_fp4.hip):
  pack (ct_rtn_quant_pack_w4 / _wb)   a lane owns 32 consecutive elements, a group of g is g / 32 adjacent lanes reduced by DPP (quad_perm xor 1, xor 2,
                                      row_half_mirror, row_mirror) and, beyond 16 lanes, ds_bpermute xor 16 and xor 32.
      a  g32   (n, 96)     1 lane, no reduction: positions 0 and 31
      b  g128  (n, 384)    4 lanes, two quad_perm steps: positions 0 (lane 0), 33 (lane 1), 127 (lane 3)
      c  g2048 (n, 2048)   64 lanes, all four DPP steps and both shuffles: positions 0 (lane 0), 1023 (lane 31), 2047 (lane 63)
      d  channel (n, 256)  8 lanes, up to row_half_mirror: positions 0 (lane 0), 100 (lane 3), 255 (lane 7)
      e  g32   (1, 8224)   257 lanes: one full workgroup of 256 and a second with ONE live lane, whose 255 dead lanes carry the identity — the plant
                           sits in that last group; a second one in group 128 (wave 2, lane 0 of the full workgroup)
  channel8 (ct_rtn_quant_channel8)    a unit is 8 elements.  Wave form: unit u is load u / 64 of lane u % 64.  Row and long form: unit u is load u / 256 of
                                      thread u % 256; four waves combine through LDS; the long form streams units >= 2048 in trips of 4 x 256.
      wave   (n, 256)      32 live lanes of 64: positions 0 (lane 0), 129 (lane 16: beyond the DPP row), 255 (lane 31, the last live one)
      (n, 2048) / (n, 2056)  symmetric: the last wave-form width (unit 255 = lane 63) / the first row-form width (unit 256 = thread 0, load 1)
      (n, 8192) / (n, 8200)  asymmetric: the last wave-form width (unit 1023 = lane 63, load 15) / the first row-form width (unit 1024)
      row    (n, 16384)    position 16383 = unit 2047 = thread 255 = the last lane of wave 3, load 7: it crosses the LDS combine; 5000 = wave 1
      long   (n, 16392), (n, 24584)   position 100 (registers), 16384 (the first streamed unit), cols - 1 (the very last unit: at 24584 that is unit
                           3072, alone in the SECOND trip of the streamed loop)
  block8 (ct_rtn_quant_block8)        a workgroup per block, unit u of the block's row-major order is load u / 256 of thread u % 256.
      [128, 128] at (130, 256)   block (0, 0) at its last row and column (unit 2047 = thread 255, load 7), and the ragged block (1, 1) — two live rows,
                           32 live units — at its last live element
      [4, 16] at (8, 64)   8 units, 248 dead threads; planted blocks on a checkerboard
      [16, 1024] at (16, 2048)   2048 units: 8 full loads; block 0 or block 1 is planted, the other is clean
  group8 (ct_rtn_quant_group8)        a lane owns 16 elements, a group of g is g / 16 lanes: positions 0, 15 (the last of lane 0), g - 16 (the first of
                                      the last lane), g - 1 at g = 32 (2 lanes), 128 (8 lanes), 1024 (64 lanes: both shuffles)
  fp4 (ct_rtn_mxfp4_quant_pack, ct_rtn_nvfp4_quant_pack)   a lane owns one group of 32 = two NVFP4 groups of 16: positions 0, 15, 16, 31; and
                           (2, 8224) whose only plant is the last element: NVFP4's tensor-wide amax (ct_generate_gparam; the table's atomic key)."""
import hashlib

import torch

BF16, F16, F32, F8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
DTYPES = {"bf16": BF16, "f16": F16}
# the 16-bit patterns.  nan_min is the NaN with the smallest payload: the key just above +inf; nan_ones is all ones
PATTERNS = {"bf16": dict(nan=0x7FC0, neg_nan=0xFFC0, nan_min=0x7F81, nan_ones=0xFFFF, inf=0x7F80, neg_inf=0xFF80),
            "f16": dict(nan=0x7E00, neg_nan=0xFE00, nan_min=0x7C01, nan_ones=0xFFFF, inf=0x7C00, neg_inf=0xFC00)}
# plant -> [(pattern, which)]: which = 0 the plant's position, 1 its partner position (half a region further: another lane), "all" the whole region
PLANTS = {"nan": [("nan", 0)], "neg_nan": [("neg_nan", 0)], "nan_min": [("nan_min", 0)], "nan_ones": [("nan_ones", 0)], "inf": [("inf", 0)],
          "neg_inf": [("neg_inf", 0)], "both_inf": [("inf", 0), ("neg_inf", 1)], "nan_inf": [("nan", 0), ("inf", 1)], "all_nan": [("nan", "all")],
          "all_inf": [("inf", "all")]}
HOLDS_NAN = {"nan", "neg_nan", "nan_min", "nan_ones", "nan_inf", "all_nan"}
# the order the block slots take them in: even entries go to a weight's first slot, odd ones to its second, so both see a NaN and an infinity
BLOCK_ORDER = ("nan", "neg_inf", "inf", "nan_min", "neg_nan", "nan_ones", "both_inf", "nan_inf", "all_nan", "all_inf")
PACK_BITS = (2, 3, 4, 5, 6, 7)
PACK_KINDS = [f"w{b}{a}" for b in PACK_BITS for a in ("", "a")]  # "w3": 3 bits symmetric, "w3a": asymmetric
KINDS8 = {"fp8": dict(num_bits=8, type="float", symmetric=True), "int8": dict(num_bits=8, type="int", symmetric=True),
          "int8_zp": dict(num_bits=8, type="int", symmetric=False)}
MX_KINDS = ("mxfp8", "mxfp4")
EXPLICIT_GLOBAL_SCALE = 64.0  # the twin of the NVFP4 last-element weight: a finite global scale given by the caller
WHOLE_MAX = 4096  # a recorded tensor of more bytes is kept as canonical sha256 + NaN count in the manifest


def _combos(positions):
    """(plant, position) per planted row: NaN and inf of either sign at EVERY position, the other point plants at the first, the two whole-region ones"""
    out = [(p, pos) for pos in positions for p in ("nan", "neg_nan", "inf", "neg_inf")]
    out += [(p, positions[i % len(positions)]) for i, p in enumerate(("nan_min", "nan_ones", "both_inf", "nan_inf"))]
    return out + [("all_nan", 0), ("all_inf", 0)]


def _row_plants(positions, start, length):
    """one planted region [start, start + length) per row, rows 0 .. n - 1; row n stays clean"""
    return [dict(plant=p, region=[i, i + 1, start, start + length], at=[0, pos], partner=[0, (pos + length // 2) % length])
            for i, (p, pos) in enumerate(_combos(positions))]


def _grouped(family, form, g, positions, **extra):
    """(n, 3 g): the middle group of every row but the last is planted"""
    plants = _row_plants(positions, g, g)
    return dict(family=family, form=form, shape=[len(plants) + 1, 3 * g], group=g, plants=plants, **extra)


def _rowwise(family, form, cols, positions, group=None):
    plants = _row_plants(positions, 0, cols)
    return dict(family=family, form=form, shape=[len(plants) + 1, cols], group=group, plants=plants)


def _block_cases():
    out = []
    # [128, 128] at (130, 256): slot 0 = the full block (0, 0) at its last row and column, slot 1 = the ragged block (1, 1) at its last live element
    for v in range(5):
        a, b = BLOCK_ORDER[2 * v], BLOCK_ORDER[2 * v + 1]
        plants = [dict(plant=a, region=[0, 128, 0, 128], at=[127, 127], partner=[63, 63]),
                  dict(plant=b, region=[128, 130, 128, 256], at=[1, 127], partner=[0, 63])]
        out.append(dict(family="block8", form=f"b128x128.v{v}", shape=[130, 256], block=[128, 128], plants=plants))
    # [4, 16] at (8, 64): blocks (0, 0), (0, 2), (1, 1), (1, 3)
    slots = [((0, 0), (3, 15)), ((0, 2), (0, 0)), ((1, 1), (2, 8)), ((1, 3), (1, 7))]
    for v in range(3):
        plants = []
        for ((br, bc), (i, j)), p in zip(slots, BLOCK_ORDER[4 * v:4 * v + 4]):
            plants.append(dict(plant=p, region=[4 * br, 4 * br + 4, 16 * bc, 16 * bc + 16], at=[i, j], partner=[(i + 2) % 4, (j + 8) % 16]))
        out.append(dict(family="block8", form=f"b4x16.v{v}", shape=[8, 64], block=[4, 16], plants=plants))
    # [16, 1024] at (16, 2048): one of the two blocks
    spots = [(15, 1023), (0, 0), (7, 512)]
    for v, p in enumerate(BLOCK_ORDER):
        c0, (i, j) = 1024 * (v % 2), spots[v % 3]
        plants = [dict(plant=p, region=[0, 16, c0, c0 + 1024], at=[i, j], partner=[(i + 8) % 16, (j + 512) % 1024])]
        out.append(dict(family="block8", form=f"b16x1024.v{v}", shape=[16, 2048], block=[16, 1024], plants=plants))
    return out


def _forms():
    out = [_grouped("pack", "a", 32, (0, 31)), _grouped("pack", "b", 128, (0, 33, 127)), _rowwise("pack", "c", 2048, (0, 1023, 2047), group=2048),
           _rowwise("pack", "d", 256, (0, 100, 255)),
           dict(family="pack", form="e", shape=[1, 8224], group=32, plants=[
               dict(plant="nan", region=[0, 1, 8192, 8224], at=[0, 7], partner=[0, 23]),
               dict(plant="neg_inf", region=[0, 1, 4096, 4128], at=[0, 31], partner=[0, 15])])]
    out += [_rowwise("channel8", "wave", 256, (0, 129, 255)), _rowwise("channel8", "sym_wave_last", 2048, (0, 1000, 2047)),
            _rowwise("channel8", "sym_row_first", 2056, (0, 1029, 2055)), _rowwise("channel8", "asym_wave_last", 8192, (0, 4099, 8191)),
            _rowwise("channel8", "asym_row_first", 8200, (0, 4099, 8199)), _rowwise("channel8", "row", 16384, (0, 5000, 16383)),
            _rowwise("channel8", "long1", 16392, (100, 16384, 16391)), _rowwise("channel8", "long2", 16384 + 4 * 256 * 8 + 8, (100, 16384, 24583))]
    out += _block_cases()
    out += [_grouped("group8", f"g{g}", g, (0, 15, g - 16, g - 1)) for g in (32, 128, 1024)]
    out.append(_grouped("fp4", "g32", 32, (0, 15, 16, 31), global_scale=None))
    out.append(dict(family="fp4", form="clean", shape=[3, 96], group=32, plants=[], global_scale=None))
    for p in ("nan", "inf"):
        for gs in (None, EXPLICIT_GLOBAL_SCALE):
            out.append(dict(family="fp4", form=f"last_{p}" + ("_gs" if gs else ""), shape=[2, 8224], group=32, global_scale=gs,
                            plants=[dict(plant=p, region=[1, 2, 8192, 8224], at=[0, 31], partner=[0, 15])]))
    return out


def case_list():
    """[(key, recipe)] — recipe = dict(family, form, shape, dtype, group | block, plants, salt[, global_scale]).  Deterministic."""
    out = []
    for i, form in enumerate(_forms()):
        for dtype in ("bf16", "f16"):
            out.append((f"{form['family']}.{form['form']}.{dtype}", dict(form, dtype=dtype, salt=i % 7 + 1)))
    return out


def kinds_of(r):
    """the kinds a case is recorded under"""
    if r["family"] == "pack":
        return list(PACK_KINDS)
    if r["family"] in ("channel8", "block8"):
        return list(KINDS8)
    if r["family"] == "group8":
        return (["mxfp8"] if r["group"] == 32 else []) + list(KINDS8)
    return ["nvfp4"] if r["form"].startswith("last_") else ["mxfp4", "nvfp4"]


def make_weight(r) -> torch.Tensor:
    """the case's finite base on the CPU: a multiplicative hash of the element index mapped to [-7.8, 7.8] in steps of 2^-8, under a per-region
    magnitude of 2^-6 .. 2^3 that differs between neighbouring regions and signs that make some regions one-sided (tests/_packw_rtn_cases.make_weight)"""
    rows, cols = r["shape"]
    bh, g = r["block"] if r["family"] == "block8" else (1, r["group"] or cols)
    i = torch.arange(rows * cols, dtype=torch.int64).reshape(rows, cols)
    h = ((i + 977 * r["salt"]) * 2654435761) % 4294967296
    v = ((h >> 7) % 4001 - 2000).to(torch.float32) / 256.0
    grp = (torch.arange(rows)[:, None] // bh) * 5 + (torch.arange(cols)[None, :] // g) * 3 + r["salt"]
    v = v * torch.pow(2.0, (grp % 10 - 6).to(torch.float32))
    v = torch.where(grp % 4 == 1, v.abs() + 0.001, v)    # an all-positive region: zero joins the range
    v = torch.where(grp % 4 == 3, -v.abs() - 0.001, v)   # an all-negative one
    return v.to(DTYPES[r["dtype"]]).contiguous()


def _signed(pattern: int) -> int:
    return pattern - 65536 if pattern >= 32768 else pattern


def plant(x: torch.Tensor, r, value=None) -> torch.Tensor:
    """a copy of `x` with the recipe's plants written as 16-bit patterns (never through a Python float: a NaN's payload and sign would not survive);
    `value`: write this finite value in their place instead — the weight the isolation tests compare with"""
    out = x.clone()
    raw = out.view(torch.int16)
    pats = PATTERNS[r["dtype"]]
    fill = int(torch.tensor([value], dtype=x.dtype).view(torch.int16)) if value is not None else None
    for p in r["plants"]:
        r0, r1, c0, c1 = p["region"]
        for name, which in PLANTS[p["plant"]]:
            bits = fill if value is not None else _signed(pats[name])
            if which == "all":
                raw[r0:r1, c0:c1] = bits
            else:
                dr, dc = p["at"] if which == 0 else p["partner"]
                raw[r0 + dr, c0 + dc] = bits
    return out


def planted_mask(r) -> torch.Tensor:
    """bool (rows, cols): the elements of every planted region (the whole group / row / block, not only the plant itself)"""
    m = torch.zeros(r["shape"], dtype=torch.bool)
    for p in r["plants"]:
        r0, r1, c0, c1 = p["region"]
        m[r0:r1, c0:c1] = True
    return m


def region_grid(r, kind=None):
    """(region height, region width) of one scale of this case under this kind"""
    rows, cols = r["shape"]
    if r["family"] == "block8":
        return tuple(r["block"])
    if r["family"] == "fp4":
        return (1, 16 if kind == "nvfp4" else 32)
    return (1, r["group"] or cols)


def planted_regions(r, kind=None) -> torch.Tensor:
    """bool, the shape of the kind's scale: the regions that hold any element of a planted region"""
    h, w = region_grid(r, kind)
    m = planted_mask(r)
    rows, cols = m.shape
    rb = -(-rows // h)
    p = torch.zeros((rb * h, cols), dtype=torch.bool)
    p[:rows] = m
    return p.reshape(rb, h, cols // w, w).any(dim=3).any(dim=1)


def weight(r) -> torch.Tensor:
    return plant(make_weight(r), r)


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.reshape(-1).contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def canonical(t: torch.Tensor) -> torch.Tensor:
    """the raw bits of `t` with every NaN rewritten to ONE NaN: NaN payload and sign are not compared.  float8_e4m3fn: 0x7F and
    0xFF are its two NaNs.  Integer tensors pass through."""
    t = t.contiguous()
    if t.dtype == F8:
        b = t.view(torch.uint8)
        return torch.where((b & 0x7F) == 0x7F, torch.full_like(b, 0x7F), b)
    if t.dtype in (BF16, F16):
        b = t.view(torch.int16)
        return torch.where(torch.isnan(t), torch.full_like(b, 0x7FC0 if t.dtype == BF16 else 0x7E00), b)
    if t.dtype == F32:
        b = t.view(torch.int32)
        return torch.where(torch.isnan(t), torch.full_like(b, 0x7FC00000), b)
    return t


def nan_count(t: torch.Tensor) -> int:
    return int(torch.isnan(t.float()).sum()) if t.dtype.is_floating_point else 0


def fp4_sign_mask(O, x: torch.Tensor, r, kind: str) -> torch.Tensor:
    """uint8, the shape of the packed FP4 bytes: 0x08 / 0x80 where the low / high nibble's element has a NaN quotient x / scale (a NaN element,
    a NaN scale, inf / inf).  E2M1 has no NaN: cast_to_fp4 gives such an element the magnitude 0, and pack_fp4_to_uint8 copies torch.signbit of the
    NaN into the nibble's sign bit — the sign of a NaN, which an x86 division makes negative and the GPU positive.  NaN sign is not compared
    (DESIGN section 2), so `comparable` clears exactly these bits; the three magnitude bits of the same nibbles stay compared."""
    if kind == "mxfp4":
        s = O.calculate_qparams_float(x, kind="mxfp4", group_size=32)
        t = x / s.repeat_interleave(32, dim=-1)
    else:
        gs = O.generate_gparam(x) if r["global_scale"] is None else torch.tensor([r["global_scale"]], dtype=F32)
        s = O.calculate_qparams_float(x, kind="nvfp4", group_size=16, global_scale=gs)
        t = x.float() / (s.float() / gs.float()).repeat_interleave(16, dim=-1)
    nan = torch.isnan(t).to(torch.uint8)
    return (nan[:, 0::2] << 3) | (nan[:, 1::2] << 7)


_LISTED_WIDTH = {("mxfp8", "scale"): 1, ("mxfp8", "e8m0"): 1, ("mxfp8", "q"): 32, ("mxfp4", "scale"): 1, ("mxfp4", "e8m0"): 1, ("mxfp4", "packed"): 16}


def comparable(outs: dict, kind: str, sign_mask=None, listed=()) -> dict:
    """{name: what is compared of it}: `canonical` of every output, the packed FP4 bytes without the sign bits of `sign_mask`, and the entries of
    the `listed` (row, group) pairs of an MX kind — scale, exponent byte and the codes of those groups — blanked"""
    out = {}
    for name, t in outs.items():
        c = canonical(t.cpu()).clone()
        if sign_mask is not None and name == "packed":
            c = c & ~sign_mask
        w = _LISTED_WIDTH.get((kind, name))
        for row, g in listed if w else ():
            c[row, w * g:w * g + w] = 0
        out[name] = c
    return out


def load_fixture():
    """(tensors, manifest) of tests/golden/nonfinite_rtn.*: the float8 results, stored as bytes, are float8 again"""
    import json
    import os

    from safetensors.torch import load_file

    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "nonfinite_rtn_manifest.json")) as f:
        manifest = json.load(f)
    tensors = load_file(os.path.join(golden, "nonfinite_rtn.safetensors"))
    for key, entry in manifest["cases"].items():
        for name, m in entry["out"].items():
            if m["whole"] and m["dtype"] == "float8_e4m3fn":
                tensors[f"{key}.{name}"] = tensors[f"{key}.{name}"].view(F8)
    return tensors, manifest


def listed_groups(manifest, key: str, kind: str) -> list:
    """the (row, group) pairs of this case and kind on the manifest's list of MX groups where the reference is not the weight path's rule"""
    return [(row, g) for k, kd, row, g in manifest["mx_exceptions"] if k == key and kd == kind]


def fixture_mismatches(fixture, key: str, kind: str, got: dict, sign_mask=None) -> list:
    """the names of `got` (an entry's or the oracle's outputs, raw) that are not what the fixture records for this case and kind, outside the
    listed MX groups: dtype, shape and the compared bits — of the whole tensor where the fixture holds it, else their sha256 and the NaN count"""
    tensors, manifest = fixture
    listed = listed_groups(manifest, key, kind)
    mine = comparable(got, kind, sign_mask, listed)
    bad = []
    for name, c in mine.items():
        m = manifest["cases"][key]["out"][f"{kind}.{name}"]
        ok = str(got[name].dtype).replace("torch.", "") == m["dtype"] and list(got[name].shape) == m["shape"]
        if ok and m["whole"]:
            ok = torch.equal(c, comparable({name: tensors[f"{key}.{kind}.{name}"]}, kind, sign_mask, listed)[name])
        elif ok:
            ok = not listed and sha(c) == m["sha256"] and nan_count(got[name].cpu()) == m["nans"]
        if not ok:
            bad.append(name)
    return bad


def pack_kind(kind: str):
    """"w3a" -> (3, False)"""
    return int(kind[1]), not kind.endswith("a")


def oracle_outputs(O, x: torch.Tensor, r, kind: str) -> dict:
    """what the fixture records, from the pinned oracle, composed exactly as the sibling case modules compose it (tests/_packw_rtn_cases,
    _channel8_rtn_cases, _block_rtn_cases, _group8_rtn_cases); FP4: calculate_qparams_float under generate_gparam, fp4_compress, e8m0_encode"""
    family, group = r["family"], r.get("group")
    if family == "pack":
        bits, symmetric = pack_kind(kind)
        scale, zp = O.calculate_qparams_minmax(x, num_bits=bits, group_size=group, symmetric=symmetric)
        q = O.quantize(x, scale, zp, num_bits=bits, strategy="group" if group else "channel", group_size=group, dtype=torch.int8)
        out = dict(scale=scale, zero_point=zp, packed=O.pack_to_int32(q, bits))
        if not symmetric:
            out["zp_packed"] = O.pack_to_int32(zp, bits, packed_dim=0)
        return out
    if family == "channel8":
        if kind == "fp8":
            scale = O.calculate_qparams_float(x, kind="fp8")
            return dict(scale=scale, q=O.quantize(x, scale, torch.zeros(scale.shape, dtype=F8), num_bits=8, strategy="channel", dtype=F8, qtype="float"))
        scale, zp = O.calculate_qparams_minmax(x, num_bits=8, symmetric=KINDS8[kind]["symmetric"])
        return dict(scale=scale, zero_point=zp, q=O.quantize(x, scale, zp, num_bits=8, strategy="channel", dtype=torch.int8))
    if family == "block8":
        import _block_rtn_cases as B

        scale, zp, q = B.oracle_triple(O, x, r["block"], kind)
        return dict(scale=scale, zero_point=zp, q=q)
    if family == "group8":
        if kind in ("fp8", "mxfp8"):
            scale = O.calculate_qparams_float(x, kind=kind, group_size=group)
            q = O.quantize(x, scale, torch.zeros(scale.shape, dtype=F8), num_bits=8, strategy="group", group_size=group, dtype=F8, qtype="float")
            out = dict(scale=scale, q=q)
            if kind == "mxfp8":
                out["e8m0"] = O.e8m0_encode(scale)
            return out
        scale, zp = O.calculate_qparams_minmax(x, num_bits=8, group_size=group, symmetric=KINDS8[kind]["symmetric"])
        q = O.quantize(x, scale, zp, num_bits=8, strategy="group", group_size=group, dtype=torch.int8)
        return dict(scale=scale, zero_point=zp, q=q, packed=O.pack_to_int32(q, 8))
    if kind == "mxfp4":
        scale = O.calculate_qparams_float(x, kind="mxfp4", group_size=32)
        c = O.fp4_compress(x, scale, fmt="mxfp4-pack-quantized")
        return dict(scale=scale, packed=c["weight_packed"], e8m0=c["weight_scale"])
    gs = O.generate_gparam(x) if r["global_scale"] is None else torch.tensor([r["global_scale"]], dtype=F32)
    scale = O.calculate_qparams_float(x, kind="nvfp4", group_size=16, global_scale=gs)
    c = O.fp4_compress(x, scale, gs, fmt="nvfp4-pack-quantized")
    return dict(scale=scale, packed=c["weight_packed"], scale_f8=c["weight_scale"], global_scale=gs)
