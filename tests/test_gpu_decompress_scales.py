"""Every decompress kernel over the whole domain of STORED scales (tests/_decompress_scale_cases.py): every 16-bit pattern as a scale (`sweep16`,
bfloat16 and float16), the edge scales crossed with every zero point and every code (`cross`), the fp32 exponent sweep and all 256 E8M0 bytes,
through each form of `unpack_and_dequantize`, `unpack_and_dequantize_with_zp`, `dequantize_tensor`, the table launches and the compressors'
`decompress`.  A result is compared bit for bit (`eq` of test_oracle_golden: NaN == NaN, -0.0 != +0.0) with the pinned oracle on the CPU and, as
canonical sha256 and NaN / inf / subnormal counts, with what the reference recorded (tests/golden/decompress_scales_manifest.json).  Every test
asserts the precondition of the dispatch rule it relies on (ct_unpack_dequant, dequantize_impl, decomp_unroll, decomp_unroll_grouped,
launch_wb_unpack_dequant in csrc), so a later change of a rule cannot silently move its case to another kernel.
Every test here needs an MI355X:  python -m pytest tests -m gpu"""
import functools

import pytest
import torch
from test_oracle_golden import eq

import _decompress_scale_cases as C
import oracle as O

pytestmark = pytest.mark.gpu

CASES = dict(C.case_list())
DTS = ("bf16", "f16")
ROUND = 256 * 8 * 256  # the chip's lanes in one residency round: 256 CUs x 8 workgroups x 256 lanes (decomp_unroll's round_lanes)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cta():
    import compressed_tensors_amd as m
    from compressed_tensors_amd import _lib

    _lib.load()  # fail loudly if the HIP extension is missing
    return m


@functools.lru_cache(maxsize=3)
def cpu_side(key):
    """(inputs, the oracle's output) of a case on the CPU; never written to"""
    r = CASES[key]
    t = C.inputs(r)
    if r["ctype"] == "int":
        t["packed"] = O.pack_to_int32(t["q"], r["bits"]).contiguous()
    return t, C.oracle_output(O, r, t)


def on(dev, t, *names):
    return [None if t[n] is None else t[n].to(dev) for n in names]


def check(key, got):
    want = cpu_side(key)[1]
    got = got.cpu()
    assert eq(got, want), (key, int((C.canonical(got) != C.canonical(want)).sum()) if got.shape == want.shape else got.shape)
    assert C.fixture_mismatch(key, got) == ""


def units_of(r):
    return r["shape"][0] * r["shape"][1] // 8


def kw_of(r):
    return dict(num_bits=r["bits"], strategy="group", group_size=r["group"]) if r["group"] else dict(num_bits=r["bits"], strategy="channel")


def unpack(cta, dev, key, **kw):
    r = CASES[key]
    t = cpu_side(key)[0]
    packed, scale, zp, g_idx = on(dev, t, "packed", "scale", "zero_point", "g_idx")
    return cta.codec.unpack_and_dequantize(packed, tuple(r["shape"]), scale, zp, g_idx=g_idx, **kw_of(r), **kw)


def takes_w4_lean(r):
    """w4_eligible: int4, 16-bit scales, cols % 8 == 0, group % 8 == 0, no activation ordering"""
    return r["bits"] == 4 and r["sdt"] in DTS and r["g_idx"] is None and r["shape"][1] % 8 == 0 and (r["group"] or r["shape"][1]) % 8 == 0


def w4_form(r):
    """the template ct_unpack_dequant picks for a lean W4 tensor with contiguous, allocator-aligned tables: (units per lane, scale loader)"""
    u, g = units_of(r), r["group"] or r["shape"][1]
    unroll = 4 if 2 * ROUND < u <= 4 * ROUND else 2
    upg_shift = (g // 8).bit_length() - 1
    zp8 = r["zp"] is not None
    if upg_shift == 4 and u % 64 == 0 and u > 8 * ROUND:
        return unroll, "scalar"
    if zp8 and upg_shift >= 4 and u % 16 == 0:
        return unroll, "rowlead"
    return unroll, "perlane"


# ---- W4 -------------------------------------------------------------------------------------------------------------------------------------
W4_FORMS = {
    "1_perlane_sym_u2": ("w4.g128.sym", (2, "perlane")),
    "1_perlane_sym_u2_cross": ("w4.cross.g128.sym", (2, "perlane")),
    "2_u4_sym": ("w4.g128x2.sym", (4, "perlane")),
    "2_u4_asym": ("w4.g128x2.i8", (4, "rowlead")),
    "2_u4_sym_cross": ("w4.g128c.sym", (4, "perlane")),
    "2_u4_asym_cross": ("w4.g128c.i8", (4, "rowlead")),
    "3_rowlead_g128": ("w4.g128.i8", (2, "rowlead")),
    "3_rowlead_g128_cross": ("w4.cross.g128.i8", (2, "rowlead")),
    "3_rowlead_g256": ("w4.g256.i8", (4, "rowlead")),
    "3_rowlead_g256_cross": ("w4.cross.g256.i8", (2, "rowlead")),
    "4_perlane_asym_g32": ("w4.g32.i8", (2, "perlane")),
    "4_perlane_asym_g32_cross": ("w4.cross.g32.i8", (2, "perlane")),
    "4_perlane_asym_g64": ("w4.g64.i8", (2, "perlane")),
    "4_perlane_asym_g64_cross": ("w4.cross.g64.i8", (2, "perlane")),
}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", list(W4_FORMS))
def test_w4_lean_forms(cta, dev, form, dt):
    key, want_form = W4_FORMS[form]
    key = f"{key}.{dt}"
    r = CASES[key]
    assert takes_w4_lean(r) and w4_form(r) == want_form
    if r["zp"]:
        assert cpu_side(key)[0]["zero_point"].dtype is torch.int8  # the row-leader form reads int8 zero points only
    check(key, unpack(cta, dev, key))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("zp", ["sym", "i8"])
def test_w4_form_5_scalar_scale_loads(cta, dev, zp, dt):
    """(2112, 16384): more than eight residency rounds.  The whole result against the same tensor decompressed in 512-row blocks (forms 1 and 3,
    checked against the oracle above), its first and last 512 rows against the oracle directly; the last 64 rows hold the cross."""
    head, tail = f"w4.g128.{zp}.{dt}", f"w4.g128.tail.{zp}.{dt}"
    big = dict(CASES[head], shape=[2112, 16384], sweeps=4)
    assert takes_w4_lean(big) and w4_form(big) == (2, "scalar") and w4_form(CASES[head])[1] == ("rowlead" if zp == "i8" else "perlane")
    assert CASES[tail]["row0"] + CASES[tail]["shape"][0] == 2112 and CASES[tail]["sweeps"] == 4
    t = C.inputs(big)
    packed = O.pack_to_int32(t["q"], 4).contiguous().to(dev)
    scale, z = on(dev, t, "scale", "zero_point")
    assert scale.data_ptr() % 8 == 0 and (z is None or z.data_ptr() % 4 == 0)
    kw = dict(num_bits=4, strategy="group", group_size=128)
    got = cta.codec.unpack_and_dequantize(packed, (2112, 16384), scale, z, **kw)
    for r0 in range(0, 2112, 512):
        r1 = min(2112, r0 + 512)
        blk = cta.codec.unpack_and_dequantize(packed[r0:r1].contiguous(), (r1 - r0, 16384), scale[r0:r1].contiguous(), None if z is None else z[r0:r1].contiguous(), **kw)
        assert eq(got[r0:r1], blk), r0
    check(head, got[:512])
    check(tail, got[1600:])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key", ["w4.g128.i4", "w4.cross.g128.i4"])
@pytest.mark.parametrize("want_zero_point", [True, False])
def test_w4_form_6_packed_zero_points(cta, dev, want_zero_point, key, dt):
    key = f"{key}.{dt}"
    r = CASES[key]
    t = cpu_side(key)[0]
    assert r["group"] == 128 and cta.codec.w4_packed_zp_readable(r["shape"][1], r["group"])
    packed, scale = on(dev, t, "packed", "scale")
    zpp = O.pack_to_int32(t["zero_point"], 4, packed_dim=0).contiguous().to(dev)
    got = cta.codec.unpack_and_dequantize_with_zp(packed, tuple(r["shape"]), scale, zpp, num_bits=4, want_zero_point=want_zero_point)
    assert got is not None, "not the layout ct_unpack_dequant_w4_zp takes"
    check(key, got[0])
    assert (got[1] is None) if not want_zero_point else torch.equal(got[1].cpu(), t["zero_point"])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("table", ["int8_zp", "packed_zp", "sym"])
def test_w4_form_7_table_launch(cta, dev, table, dt):
    """two items of different row counts in one ct_unpack_dequant_batch launch"""
    keys = {"int8_zp": ("w4.g128.i8", "w4.cross.g128.i8"), "packed_zp": ("w4.g128.i4", "w4.cross.g128.i4"), "sym": ("w4.g128.sym", "w4.cross.g128.sym")}[table]
    keys = [f"{k}.{dt}" for k in keys]
    assert CASES[keys[0]]["shape"][0] != CASES[keys[1]]["shape"][0]
    items = []
    for key in keys:
        r, t = CASES[key], cpu_side(key)[0]
        packed, scale, zp = on(dev, t, "packed", "scale", "zero_point")
        items.append((r, packed, scale, zp, t))
    if table == "packed_zp":
        scheme = cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(num_bits=4, group_size=128, symmetric=False, strategy="group"))
        sds = []
        for r, packed, scale, zp, t in items:
            assert cta.codec.w4_packed_zp_readable(r["shape"][1], 128)
            sds.append({"weight_packed": packed, "weight_scale": scale, "weight_shape": torch.tensor(r["shape"]),
                        "weight_zero_point": O.pack_to_int32(t["zero_point"], 4, packed_dim=0).contiguous().to(dev)})
        pre = cta.PackedQuantizationCompressor._batch_decompress(sds, [scheme] * 2)
        assert all(w is not None for w, _ in pre), "the table did not take the items"
        outs = cta.PackedQuantizationCompressor.decompress_many(sds, scheme)
        for key, (r, _, _, _, t), out in zip(keys, items, outs):
            assert torch.equal(out["weight_zero_point"].cpu(), t["zero_point"])
            check(key, out["weight"])
        return
    for r, packed, scale, zp, t in items:
        assert cta.codec.w4_batch_eligible(r["shape"], scale.dtype, scale, zp, num_bits=4, strategy="group", group_size=128, device=packed.device)
        assert packed.data_ptr() % 16 == 0
    outs = cta.codec.unpack_and_dequantize_many([(p, r["shape"], s, z) for r, p, s, z, _ in items], num_bits=4, strategy="group", group_size=128)
    for key, out in zip(keys, outs):
        check(key, out)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key,tables", [("w4.gidx128.i8", (1, 128)), ("w4.gidx512.sym", (257, 512)), ("w4.cross.gidx.i8", (1, 128))])
def test_w4_form_8_activation_ordering(cta, dev, key, tables, dt):
    key = f"{key}.{dt}"
    r = CASES[key]
    G = r["shape"][1] // r["group"]
    assert r["g_idx"] is not None and tables[0] <= G <= tables[1] and r["shape"][1] % 8 == 0  # w4_gidx_ok, and the LDS table launch_w4_gidx sizes
    g = cpu_side(key)[0]["g_idx"]
    assert g.dtype is torch.int32 and torch.equal(torch.bincount(g.to(torch.int64)), torch.full((G,), r["group"]))  # balanced
    check(key, unpack(cta, dev, key))


@pytest.mark.parametrize("zp", ["sym", "i8"])
def test_w4_form_9_fp32_scales(cta, dev, zp):
    key = f"w4.f32.g128.{zp}"
    r = CASES[key]
    assert r["sdt"] == "f32" and r["shape"][1] % 8 == 0 and r["group"] % 8 == 0 and r["g_idx"] is None  # w4_unpack_dequant_f32_kernel's branch
    got = unpack(cta, dev, key)
    assert got.dtype is torch.float32
    check(key, got)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key", ["w4.chan20.sym", "w4.chan20.i8", "w4.cross.chan20.i8", "q8.chan20.i8", "w1.chan20.sym"])
def test_form_10_any_layout_kernels(cta, dev, key, dt):
    key = f"{key}.{dt}"
    r = CASES[key]
    assert r["shape"][1] % 8 != 0 and not takes_w4_lean(r)  # no lean kernel takes a row that is no multiple of 8 (nor of 32) columns
    check(key, unpack(cta, dev, key))


# ---- the other widths ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["g128.sym", "cross.g128.ib"])
@pytest.mark.parametrize("bits", [2, 3, 5, 6, 7])
def test_other_widths(cta, dev, bits, kind, dt):
    """wb_unpack_dequant_kernel; groups of 128 with units % 64 == 0 take its scalar-load form (launch_wb_unpack_dequant)"""
    key = f"w{bits}.{kind}.{dt}"
    r = CASES[key]
    assert r["shape"][1] % 32 == 0 and r["group"] == 128 and units_of(r) % 64 == 0 and r["g_idx"] is None  # wb_layout_ok, the scalar form
    check(key, unpack(cta, dev, key))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key", ["w1.chan32.sym", "w2.g64.sym", "w3.g64.sym", "w5.g64.sym", "w6.g64.sym", "w7.g64.sym"])
def test_other_widths_per_lane_scales(cta, dev, key, dt):
    """wb_unpack_dequant_kernel's per-lane scale loads: a scale per 8 units (groups of 64) or 4 (1 bit, channel-wise rows of 32 columns), not 16"""
    key = f"{key}.{dt}"
    r = CASES[key]
    assert r["shape"][1] % 32 == 0 and (r["group"] or r["shape"][1]) % 32 == 0 and (r["group"] or r["shape"][1]) // 8 != 16 and r["g_idx"] is None
    check(key, unpack(cta, dev, key))


# ---- 8-bit -------------------------------------------------------------------------------------------------------------------------------------
def q8_lean(r):
    """the flat 8-bit kernels' layout: 16-bit scales, cols % 8 == 0, group % 8 == 0 (packed words: cols % 32 == 0)"""
    return r["bits"] == 8 and r["sdt"] in DTS and r["shape"][1] % 32 == 0 and (r["group"] or r["shape"][1]) % 8 == 0 and r["g_idx"] is None


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key", ["q8.chan256.sym", "q8.chan256.i8", "q8.g256.sym", "q8.g256.i8", "q8.cross.g256.sym", "q8.cross.g256.i8"])
def test_packed_8_bit(cta, dev, key, dt):
    """q8_dequant_kernel<..., 128>: the codes packed four to a word"""
    key = f"{key}.{dt}"
    r = CASES[key]
    assert q8_lean(r)
    assert (4 if 2 * ROUND < units_of(r) <= 4 * ROUND else 2) == {"chan256": 4, "g256": 4, "cross": 2}[key.split(".")[1]]  # decomp_unroll_grouped
    check(key, unpack(cta, dev, key))


def dequant_units_per_lane(r):
    """decomp_unroll"""
    u = units_of(r)
    if r["group"] is not None or u <= 2 * ROUND or u >= 8 * ROUND or (r["zp"] and u > 6 * ROUND):
        return 2
    return 8


Q8_KEYS = {"chan256.sym": 8, "chan256.zp": 8, "chan256c.zp": 8, "g128.sym": 2, "g128.zp": 2, "cross.g256.sym": 2, "cross.g256.zp": 2}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", list(Q8_KEYS))
@pytest.mark.parametrize("codes", ["q8", "f8"])
def test_dequantize_tensor_8_bit_codes(cta, dev, codes, kind, dt):
    """q8_dequant_kernel<..., 0> (int8 codes, int8 zero points) and f8_dequant_kernel (float8 codes, float8 zero points)"""
    key = f"{codes}.{kind.replace('zp', 'i8' if codes == 'q8' else 'f8')}.{dt}"
    r = CASES[key]
    assert q8_lean(r) and dequant_units_per_lane(r) == Q8_KEYS[kind]
    q, scale, zp = on(dev, cpu_side(key)[0], "q", "scale", "zero_point")
    assert q.dtype is (torch.int8 if codes == "q8" else torch.float8_e4m3fn) and q.data_ptr() % 8 == 0
    check(key, cta.codec.dequantize_tensor(q, scale, zp))


@pytest.mark.parametrize("entry,key", [("dequantize_tensor", "q8.f32.g256.sym"), ("dequantize_tensor", "q8.f32.g256.i8"), ("dequantize_tensor", "f8.f32.g256.sym"),
                                       ("dequantize_tensor", "f8.f32.g256.f8"), ("packed", "q8.f32.g256.sym"), ("packed", "q8.f32.g256.i8")])
def test_fp32_scales_8_bit(cta, dev, entry, key):
    """f32_quads_kernel: fp32 scales to fp32 output, int8 / float8 codes and the packed 8-bit words"""
    r = CASES[key]
    assert r["sdt"] == "f32" and r["shape"][1] % 8 == 0 and r["group"] % 8 == 0  # f32_quads_ok
    if entry == "packed":
        got = unpack(cta, dev, key)
    else:
        q, scale, zp = on(dev, cpu_side(key)[0], "q", "scale", "zero_point")
        got = cta.codec.dequantize_tensor(q, scale, zp)
    assert got.dtype is torch.float32
    check(key, got)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("qdt", [torch.int8, torch.int32], ids=["int8", "int32"])
@pytest.mark.parametrize("key", ["q8.chan12.i8", "q8.cross.chan12.i8"])
def test_generic_dequant_units_kernel(cta, dev, key, qdt, dt):
    key = f"{key}.{dt}"
    r = CASES[key]
    assert r["shape"][1] % 8 != 0 or qdt is torch.int32  # neither flat kernel takes these: dequantize_impl falls to dequant_units_kernel
    q, scale, zp = on(dev, cpu_side(key)[0], "q", "scale", "zero_point")
    check(key, cta.codec.dequantize_tensor(q.to(qdt), scale, zp))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("codes", ["q8", "f8"])
def test_8_bit_tables(cta, dev, codes, dt):
    """q8_dequant_batch_kernel through IntQuantizationCompressor / FloatQuantizationCompressor.decompress_many: two state dicts each way —
    without and with zero points (float8 ones for the float codes)"""
    from compressed_tensors_amd.compressors.naive_quantized.base import FloatQuantizationCompressor, IntQuantizationCompressor

    comp = IntQuantizationCompressor if codes == "q8" else FloatQuantizationCompressor
    z = "i8" if codes == "q8" else "f8"
    args = cta.QuantizationArgs(num_bits=8, type="int" if codes == "q8" else "float", strategy="group", group_size=128)
    scheme = cta.QuantizationScheme(targets=["Linear"], weights=args, input_activations=cta.QuantizationArgs(num_bits=8))
    for keys in ((f"{codes}.g128.sym.{dt}", f"{codes}.cross.g256.sym.{dt}"), (f"{codes}.g128.{z}.{dt}", f"{codes}.cross.g256.{z}.{dt}")):
        sds = []
        for key in keys:
            q, scale, zp = on(dev, cpu_side(key)[0], "q", "scale", "zero_point")
            sds.append({"weight": q, "weight_scale": scale, **({} if zp is None else {"weight_zero_point": zp})})
        assert all(w is not None for w in comp._batch_decompress(sds)), "the table did not take the items"
        for key, out in zip(keys, comp.decompress_many(sds, scheme)):
            check(key, out["weight"])


# ---- class level -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_packed_compressor_decompress(cta, dev, dt):
    """a pack-quantized state dict whose weight_scale is the sweep, its zero points in stored form"""
    key = f"w4.g128.i4.{dt}"
    r, t = CASES[key], cpu_side(key)[0]
    scheme = cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(num_bits=4, group_size=128, symmetric=False, strategy="group"))
    packed, scale = on(dev, t, "packed", "scale")
    sd = {"weight_packed": packed, "weight_scale": scale, "weight_shape": torch.tensor(r["shape"]),
          "weight_zero_point": O.pack_to_int32(t["zero_point"], 4, packed_dim=0).contiguous().to(dev)}
    out = cta.PackedQuantizationCompressor.decompress(sd, scheme)
    assert torch.equal(out["weight_zero_point"].cpu(), t["zero_point"])
    check(key, out["weight"])


def test_mxfp8_compressor_decompress(cta, dev):
    """all 256 E8M0 bytes (255: NaN; 0: 2^-127, a bfloat16 subnormal) x all 256 float8 codes"""
    from compressed_tensors_amd.compressors.mxfp8 import MXFP8QuantizationCompressor

    key = "mxfp8.e8m0"
    q, scale = on(dev, cpu_side(key)[0], "q", "scale")
    assert scale.dtype is torch.uint8 and q.dtype is torch.float8_e4m3fn
    args = cta.QuantizationArgs(num_bits=8, type="float", strategy="group", group_size=32, scale_dtype=torch.uint8, zp_dtype=torch.uint8)
    out = MXFP8QuantizationCompressor.decompress({"weight": q, "weight_scale": scale}, cta.QuantizationScheme(targets=["Linear"], weights=args))
    assert out["weight"].dtype is torch.bfloat16
    check(key, out["weight"])
