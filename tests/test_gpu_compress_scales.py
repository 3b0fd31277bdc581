"""Every compress kernel over the whole domain of GIVEN scales (tests/_compress_scale_cases.py): every 16-bit pattern as a scale (`sweep16`,
bfloat16 and float16), the edge scales crossed with every zero point (`cross`), the fp32 exponent sweep, and the patterns at and one ulp either
side of every range guard's end points (`guard`), under weights built from each group's own scale so that every tie and clamp edge of the width
occurs in it — through each form of `quantize_and_pack`, `quantize_and_pack_with_zp`, `quantize_tensor`, `fake_quantize_tensor`, the table
launches and the compressors' `compress`.  A result is compared bit for bit (`eq` of test_oracle_golden: NaN == NaN, -0.0 != +0.0; float8 codes:
`eq_f8`, a NaN code is a NaN code) with the pinned oracle on the CPU and, as canonical sha256 and NaN / inf / zero counts, with what the reference
recorded (tests/golden/compress_scales_manifest.json).  The one property not compared is the int32 cast of a NaN (`_compress_scale_cases.masked`).
Every test asserts the precondition of the dispatch rule it relies on (ct_quant_pack, quantize_impl, fake_quantize_impl, w4_compress_variant,
wb_layout_ok in csrc), so a later change of a rule cannot silently move its case to another kernel.
Every test here needs an MI355X:  python -m pytest tests -m gpu"""
import ctypes
import functools

import pytest
import torch
from test_oracle_golden import eq, eq_f8

import _compress_scale_cases as C
import oracle as O

pytestmark = pytest.mark.gpu

CASES = dict(C.case_list())
DTS = ("bf16", "f16")
ROUND = 256 * 8 * 256  # the chip's lanes in one residency round (kW4RoundLanes of ct_w4_variant.h)


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


@pytest.fixture(scope="module")
def diag_lib():
    """the diagnostics build of the library (-DCT_DIAG): the only one that reads CT_W4_COMPRESS (tests/test_w4_compress_lds.py)"""
    from compressed_tensors_amd import _lib

    _lib.load()
    lib = ctypes.CDLL(_lib.DIAG_LIB_PATH)
    for name, (argtypes, restype) in _lib._PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    return lib


@functools.lru_cache(maxsize=3)
def cpu_side(key):
    """(inputs, the oracle's outputs per op) of a case on the CPU; never written to"""
    r = CASES[key]
    t = C.inputs(r)
    return t, C.oracle_outputs(O, r, t)


def on(dev, t, *names):
    return [None if t[n] is None else t[n].to(dev) for n in names]


def check(key, op, got):
    r = CASES[key]
    t, outs = cpu_side(key)
    want = outs[op]
    got = C.masked(r, t, op, got.cpu())
    want = C.masked(r, t, op, want)
    same = eq_f8(got, want) if want.dtype is C.F8 else eq(got, want)
    assert got.dtype is want.dtype and same, (key, op, int((C.canonical(got) != C.canonical(want)).sum()) if got.shape == want.shape else got.shape)
    assert C.fixture_mismatch(key, op, got) == "", (key, op)


def run(cta, dev, key, op, zp_dtype=None):
    """the product's entry point for a recorded op of a case"""
    r = CASES[key]
    x, s, z, g = on(dev, cpu_side(key)[0], "x", "scale", "zero_point", "g_idx")
    if zp_dtype is not None:
        z = z.to(zp_dtype)
    kw = dict(C.kw_of(r), g_idx=g)
    c = cta.codec
    if op == "pack":
        return c.quantize_and_pack(x, s, z, **kw)
    if op in ("q", "q32", "qx"):
        return c.quantize_tensor(x, s, z, dtype={"q": torch.int8, "q32": torch.int32, "qx": None}[op], **kw)
    if op == "fq":
        return c.fake_quantize_tensor(x, s, z, **kw)
    if op == "f8":
        return c.quantize_tensor(x, s, z, dtype=C.F8, qtype="float", **kw)
    if op == "fq8":
        return c.fake_quantize_tensor(x, s, z, qtype="float", **kw)
    raise KeyError(op)


def lanes32(r):
    return r["shape"][0] * r["shape"][1] // 32


def w4_eligible(r):
    """w4_eligible && cols % 32 == 0: int4, 16-bit weights and scales of one dtype, no activation ordering, unit-aligned groups"""
    g = r["group"] or r["shape"][1]
    return r["bits"] == 4 and r["sdt"] in DTS and r["xdt"] == r["sdt"] and r["g_idx"] is None and r["shape"][1] % 32 == 0 and g % 8 == 0


def w4_lean(r, zp_dtype=torch.int8):
    """ct_quant_pack's lean branch: four consecutive units share a scale (group % 32 == 0 or the whole row), a flat scale table, units per group
    a power of two >= 4, int8 or no zero points"""
    g = r["group"] or r["shape"][1]
    upg = g // 8
    return w4_eligible(r) and g % 32 == 0 and upg & (upg - 1) == 0 and upg >= 4 and (r["zp"] is None or zp_dtype is torch.int8)


def w4_variant(r, forced=None):
    """w4_compress_variant for a 16-byte aligned input"""
    lds_ok = lanes32(r) >= 64
    if forced in (None, "auto"):
        return "lds" if lds_ok and lanes32(r) >= 4 * ROUND else "plain"
    return "lds" if forced == "lds" and lds_ok else "plain"


# ---- W4 -------------------------------------------------------------------------------------------------------------------------------------
W4_LEAN = ["w4.g128.sym", "w4.g128.ib", "w4.guard.g128.sym", "w4.guard.g128.ib", "w4.cross.g128.sym", "w4.cross.g128.i8", "w4.cross.g128.i4",
           "w4.g32.sym", "w4.g32.ib", "w4.cross.g32.i8", "w4.g64.sym", "w4.g64.ib", "w4.chan32.sym", "w4.chan32.ib"]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key", W4_LEAN)
def test_w4_lean_plain_loads(cta, dev, key, dt):
    """w4_quant_pack_lean_kernel: a lane's 32 weights under the scale of group lane >> gshift — four lanes per group at 128, two at 64, one at 32
    and channel-wise rows of 32"""
    key = f"{key}.{dt}"
    r = CASES[key]
    assert w4_lean(r) and w4_variant(r) == "plain"
    x, s, z = on(dev, cpu_side(key)[0], "x", "scale", "zero_point")
    assert x.data_ptr() % 16 == 0 and (z is None or z.dtype is torch.int8)
    check(key, "pack", run(cta, dev, key, "pack"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key", ["w4.g128.sym", "w4.g128.ib", "w4.guard.g128.sym", "w4.guard.g128.ib", "w4.cross.g128.sym", "w4.cross.g128.i8", "w4.g32.ib"])
def test_w4_lean_lds_dma(diag_lib, dev, monkeypatch, key, dt):
    """w4_quant_pack_lds_kernel, forced through the diagnostics library: equal to the plain form and to the oracle"""
    from compressed_tensors_amd import _lib, codec

    key = f"{key}.{dt}"
    r = CASES[key]
    assert w4_lean(r) and w4_variant(r, "lds") == "lds" and w4_variant(r, "plain") == "plain"
    monkeypatch.setattr(_lib, "_lib", diag_lib)
    x, s, z = on(dev, cpu_side(key)[0], "x", "scale", "zero_point")
    assert x.data_ptr() % 16 == 0
    got = {}
    for variant in ("plain", "lds"):
        monkeypatch.setenv("CT_W4_COMPRESS", variant)
        got[variant] = codec.quantize_and_pack(x, s, z, **C.kw_of(r))
    assert torch.equal(got["plain"], got["lds"])
    check(key, "pack", got["lds"])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key,zp_dtype,shared", [("w4.g16.sym", None, False), ("w4.g16.ib", None, False), ("w4.g128.ib", torch.int32, True),
                                                 ("w4.cross.g128.i8", torch.int32, True), ("w4.guard.g128.ib", torch.int32, True)])
def test_w4_flat(cta, dev, key, zp_dtype, shared, dt):
    """w4_quant_pack_kernel<..., shared / not>: groups of 16 (no four units share a scale), and int32 zero points, which leave the lean branch"""
    key = f"{key}.{dt}"
    r = CASES[key]
    g = r["group"]
    assert w4_eligible(r) and not w4_lean(r, zp_dtype or torch.int8) and (g % 32 == 0) is shared
    check(key, "pack", run(cta, dev, key, "pack", zp_dtype=zp_dtype))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key", ["w4.g128.ib", "w4.cross.g128.i4"])
def test_w4_stored_zero_points(cta, dev, key, dt):
    """w4_quant_pack_one_kernel through ct_quant_pack_w4_zp: the packed words and the stored form of the zero points (-8 .. 7) from one launch"""
    key = f"{key}.{dt}"
    r = CASES[key]
    t = cpu_side(key)[0]
    x, s, z = on(dev, t, "x", "scale", "zero_point")
    assert r["group"] % 32 == 0 and r["shape"][1] % 32 == 0 and z.dtype is torch.int8 and int(z.min()) >= -8 and int(z.max()) <= 7
    got = cta.codec.quantize_and_pack_with_zp(x, s, z, **C.kw_of(r))
    assert got is not None, "not the layout ct_quant_pack_w4_zp takes"
    check(key, "pack", got[0])
    assert torch.equal(got[1].cpu(), O.pack_to_int32(t["zero_point"], 4, packed_dim=0).contiguous())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("table", ["sym", "int8_zp", "stored_zp"])
def test_w4_tables(cta, dev, table, dt):
    """w4_quant_pack_batch_kernel: two items of different heights in one launch"""
    keys = {"sym": ("w4.g128.sym", "w4.cross.g128.sym"), "int8_zp": ("w4.g128.ib", "w4.cross.g128.i8"), "stored_zp": ("w4.g128.ib", "w4.cross.g128.i4")}[table]
    keys = [f"{k}.{dt}" for k in keys]
    assert CASES[keys[0]]["shape"][0] != CASES[keys[1]]["shape"][0]
    items = [on(dev, cpu_side(k)[0], "x", "scale", "zero_point") for k in keys]
    kw = dict(num_bits=4, strategy="group", group_size=128)
    for k, (x, s, z) in zip(keys, items):
        assert cta.codec.w4_batch_eligible(x.shape, x.dtype, s, z, device=x.device, **kw) and x.is_contiguous() and x.data_ptr() % 16 == 0
    if table == "stored_zp":
        outs = []
        for x, s, z in items:
            outs.append((torch.empty((x.shape[0], x.shape[1] // 8), dtype=torch.int32, device=dev),
                         torch.empty(((x.shape[0] * 4 + 31) // 32, s.shape[1]), dtype=torch.int32, device=dev)))
        entries = [(x, s, z, o[0], x.shape[0], x.shape[1], 128, o[1]) for (x, s, z), o in zip(items, outs)]
        cta.codec.W4Batch(entries, "compress", items[0][0].dtype).launch()
        torch.cuda.synchronize()
        for k, o in zip(keys, outs):
            check(k, "pack", o[0])
            assert torch.equal(o[1].cpu(), O.pack_to_int32(cpu_side(k)[0]["zero_point"], 4, packed_dim=0).contiguous())
        return
    for k, out in zip(keys, cta.codec.quantize_and_pack_many(items, **kw)):
        check(k, "pack", out)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key,tables", [("w4.gidx128.ib", (1, 128)), ("w4.gidx512.sym", (257, 512)), ("w4.cross.gidx.i8", (1, 128))])
def test_w4_activation_ordering(cta, dev, key, tables, dt):
    """w4_gidx_rows_kernel: the row's reciprocals staged in LDS (0 = divide), 128 and 512 groups per row"""
    key = f"{key}.{dt}"
    r = CASES[key]
    G = r["shape"][1] // r["group"]
    assert r["g_idx"] is not None and tables[0] <= G <= tables[1] and r["shape"][1] % 8 == 0 and r["xdt"] == r["sdt"]  # w4_gidx_ok, launch_w4_gidx's tables
    g = cpu_side(key)[0]["g_idx"]
    assert g.dtype is torch.int32 and torch.equal(torch.bincount(g.to(torch.int64)), torch.full((G,), r["group"]))  # balanced
    check(key, "pack", run(cta, dev, key, "pack"))


@pytest.mark.parametrize("key", [f"w4.f32.{k}.{z}{x}" for z in ("sym", "i8") for k, x in (("g128", ".xbf16"), ("g128", ".xf32"), ("guard", ""))]
                         + ["w4.f32.cross.g128.i8.xbf16"])
def test_w4_fp32_result(cta, dev, key):
    """w4_quant_pack_f32_kernel: bfloat16 / fp32 weights under fp32 scales — fp32 arithmetic, f32_fast_rcp and the divide near a half-integer"""
    r = CASES[key]
    assert r["bits"] == 4 and r["sdt"] == "f32" and r["shape"][1] % 8 == 0 and r["group"] % 8 == 0 and r["g_idx"] is None
    assert torch.result_type(cpu_side(key)[0]["x"], cpu_side(key)[0]["scale"]) is torch.float32
    check(key, "pack", run(cta, dev, key, "pack"))


# ---- fp32 weights -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["q", "pack", "fq"])
@pytest.mark.parametrize("key", ["q8.f32.g256.sym", "q8.f32.g256.i8", "q8.f32.guard.sym", "q8.f32.guard.i8", "q8.f32.cross.g256.sym", "q8.f32.cross.g256.i8"])
def test_fp32_8_bit(cta, dev, key, op):
    """f32_quant_units_kernel (`quantize_tensor` to int8) and f32_quads_kernel (the packed 8-bit words, `fake_quantize_tensor`)"""
    r = CASES[key]
    assert r["xdt"] == "f32" and r["sdt"] == "f32" and r["shape"][1] % 8 == 0 and r["group"] % 8 == 0 and r["g_idx"] is None  # f32_quads_ok
    got = run(cta, dev, key, op)
    assert got.data_ptr() % 16 == 0
    check(key, op, got)


@pytest.mark.parametrize("key", ["f8.f32.g256.sym", "f8.f32.g256.f8", "f8.f32.cross.g256.f8"])
def test_fp32_to_float8(cta, dev, key):
    """f32_quant_units_kernel<..., true>: float8 codes from fp32 weights"""
    r = CASES[key]
    assert r["xdt"] == "f32" and r["sdt"] == "f32" and r["shape"][1] % 8 == 0 and r["group"] % 8 == 0
    check(key, "f8", run(cta, dev, key, "f8"))


# ---- the other widths ---------------------------------------------------------------------------------------------------------------------------
def wb_ok(r, s=None, z=None):
    """wb_layout_ok: widths 1-3, 5-7, 16-bit weights and scales of one dtype, int8 or no zero points, cols % 32 == 0, group % 32 == 0 and a divisor
    of the row, a flat scale table of (rows, cols / group) (`s`, `z`: the tensors handed in, where the caller has them)"""
    rows, cols = r["shape"]
    g = r["group"] or cols
    if s is not None and not (tuple(s.shape) == (rows, cols // g) and s.is_contiguous() and (z is None or (z.dtype is torch.int8 and z.shape == s.shape))):
        return False
    return (r["bits"] in (1, 2, 3, 5, 6, 7) and r["sdt"] in DTS and r["xdt"] == r["sdt"] and r["g_idx"] is None and cols % 32 == 0 and g % 32 == 0
            and cols % g == 0 and r["zp"] in (None, "ib", "i8", "i4") and rows * (cols // 32) < 1 << 38)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["g128.sym", "g64.ib", "cross.g128.ib"])
@pytest.mark.parametrize("bits", [2, 3, 5, 6, 7])
def test_other_widths(cta, dev, bits, kind, dt):
    """wb_quant_pack_lean_kernel: four lanes per group (128) and two (64)"""
    key = f"w{bits}.{kind}.{dt}"
    assert wb_ok(CASES[key], *on(dev, cpu_side(key)[0], "scale", "zero_point"))
    check(key, "pack", run(cta, dev, key, "pack"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key", ["w1.chan32.sym", "w3.guard.g128.ib"])
def test_other_widths_one_bit_and_guard(cta, dev, key, dt):
    key = f"{key}.{dt}"
    assert wb_ok(CASES[key], *on(dev, cpu_side(key)[0], "scale", "zero_point"))
    check(key, "pack", run(cta, dev, key, "pack"))


# ---- any layout -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key,op", [("w4.chan20.sym", "pack"), ("w4.chan20.ib", "pack"), ("w4.cross.chan20.i8", "pack"), ("q8.chan20.i8", "pack"),
                                    ("w1.chan20.sym", "pack"), ("w4.chan20.sym", "q32"), ("w4.chan20.ib", "q32"), ("w4.chan20.sym", "qx"),
                                    ("w4.chan20.ib", "qx"), ("w4.cross.chan20.i8", "qx"), ("q8.chan20.i8", "q"), ("q8.chan20.i8", "qx")])
def test_any_layout_kernels(cta, dev, key, op, dt):
    """quant_pack_g32_lo / _hi (the packed words) and quant_units_kernel (codes as int8, int32 and in the float dtype the reference picks: there the
    sign of a zero left by `+ zero_point` after an underflow is compared): rows of 20 columns, which no lean kernel takes"""
    key = f"{key}.{dt}"
    r = CASES[key]
    assert r["shape"][1] % 8 != 0 and not w4_eligible(r) and not wb_ok(r) and not q8_lean(r)
    got = run(cta, dev, key, op)
    if op == "qx":
        assert got.dtype is C.DTYPES[dt]
    check(key, op, got)


# ---- 8 bit ------------------------------------------------------------------------------------------------------------------------------------------
def q8_lean(r):
    """q8_eligible: 16-bit weights and scales of one dtype, cols % 16 == 0, unit-aligned groups (the packed words: cols % 32 == 0)"""
    g = r["group"] or r["shape"][1]
    return r["sdt"] in DTS and r["xdt"] == r["sdt"] and r["g_idx"] is None and r["shape"][1] % 32 == 0 and g % 8 == 0


Q8 = [("q8.chan256.sym", True), ("q8.chan256.i8", True), ("q8.g128.sym", True), ("q8.g128.i8", True), ("q8.g16.i8", True), ("q8.g8.i8", False),
      ("q8.guard.g128.i8", True), ("q8.cross.g256.sym", True), ("q8.cross.g256.i8", True)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", ["q", "pack"])
@pytest.mark.parametrize("key,shared", Q8)
def test_8_bit_codes_and_packed_words(cta, dev, key, shared, op, dt):
    """q8_quant_kernel<..., shared / not, 0> (int8 codes) and <..., 128> (the packed words: four (code + 128) bytes)"""
    key = f"{key}.{dt}"
    r = CASES[key]
    g = r["group"] or r["shape"][1]
    assert r["bits"] == 8 and q8_lean(r) and (g % 16 == 0) is shared
    check(key, op, run(cta, dev, key, op))


@pytest.mark.parametrize("dt", DTS)
def test_6_bit_codes(cta, dev, dt):
    """q8_quant_kernel with the clamp of another width: int8 codes of a 6-bit scheme"""
    key = f"q6.g128.ib.{dt}"
    assert CASES[key]["bits"] == 6 and q8_lean(CASES[key])
    check(key, "q", run(cta, dev, key, "q"))


F8 = ["f8.g128.sym", "f8.g128.f8z", "f8.g128.f8", "f8.chan256.sym", "f8.guard.g128.f8", "f8.cross.g256.sym", "f8.cross.g256.f8"]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key", F8)
def test_float8_codes(cta, dev, key, dt):
    """f8_quant_kernel: all 256 float8 values and the midpoints between neighbours as targets; zero points absent, all-zero float8, float8 bytes"""
    key = f"{key}.{dt}"
    r = CASES[key]
    assert r["qtype"] == "fp8" and q8_lean(r)
    z = cpu_side(key)[0]["zero_point"]
    assert z is None or z.dtype is C.F8
    got = run(cta, dev, key, "f8")
    assert got.dtype is C.F8
    check(key, "f8", got)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("codes", ["q8", "f8"])
def test_8_bit_tables(cta, dev, codes, dt):
    """q8_quant_batch_kernel through IntQuantizationCompressor / FloatQuantizationCompressor: two state dicts per launch — without and with zero
    points (float8 ones for the float codes)"""
    from compressed_tensors_amd.compressors.naive_quantized.base import FloatQuantizationCompressor, IntQuantizationCompressor

    comp = IntQuantizationCompressor if codes == "q8" else FloatQuantizationCompressor
    op = "q" if codes == "q8" else "f8"
    z = "i8" if codes == "q8" else "f8"
    for sym, keys in ((True, (f"{codes}.g128.sym.{dt}", f"{codes}.cross.g256.sym.{dt}")), (False, (f"{codes}.g128.{z}.{dt}", f"{codes}.cross.g256.{z}.{dt}"))):
        sds, schemes = [], []
        for key in keys:
            r = CASES[key]
            x, s, zp = on(dev, cpu_side(key)[0], "x", "scale", "zero_point")
            sds.append({"weight": x, "weight_scale": s, **({} if zp is None else {"weight_zero_point": zp})})
            args = cta.QuantizationArgs(num_bits=8, type="int" if codes == "q8" else "float", strategy="group", group_size=r["group"],
                                        symmetric=sym or codes == "f8")
            schemes.append(cta.QuantizationScheme(targets=["Linear"], weights=args))
        outs = comp._batch_compress(sds, schemes)
        assert all(w is not None for w in outs), "the table did not take the items"
        torch.cuda.synchronize()
        for key, out in zip(keys, outs):
            check(key, op, out)
        for key, sd, scheme in zip(keys, sds, schemes):  # and the class's own entry, one state dict at a time
            check(key, op, comp.compress(sd, scheme)["weight"])


# ---- fake quantize -----------------------------------------------------------------------------------------------------------------------------------
FQ_LEAN = ["w4.g128.sym", "w4.g128.ib", "w4.guard.g128.sym", "w4.guard.g128.ib", "w4.cross.g128.sym", "w4.cross.g128.i8", "q8.g128.sym", "q8.g128.i8",
           "q8.guard.g128.i8", "q8.cross.g256.sym", "q8.cross.g256.i8"]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key", FQ_LEAN)
def test_fake_quantize_lean(cta, dev, key, dt):
    """fq16_lean_kernel: int 4 and 8 bit, int8 or no zero points; every output value bitwise, signed zeros included"""
    key = f"{key}.{dt}"
    r = CASES[key]
    g = r["group"]
    assert r["qtype"] == "int" and r["sdt"] in DTS and r["shape"][1] % 8 == 0 and (g // 8) & (g // 8 - 1) == 0 and r["g_idx"] is None
    check(key, "fq", run(cta, dev, key, "fq"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key,op,zp_dtype", [("w4.g128.ib", "fq", torch.int32), ("q8.g128.i8", "fq", torch.int32), ("w4.cross.g128.i8", "fq", torch.int32),
                                             ("f8.g128.sym", "fq8", None), ("f8.g128.f8z", "fq8", None), ("f8.g128.f8", "fq8", None),
                                             ("f8.guard.g128.f8", "fq8", None), ("f8.cross.g256.sym", "fq8", None), ("f8.cross.g256.f8", "fq8", None)])
def test_fake_quantize_flat(cta, dev, key, op, zp_dtype, dt):
    """fq16_kernel: what the lean form does not take — int32 zero points, and the float8 kind"""
    key = f"{key}.{dt}"
    r = CASES[key]
    assert r["sdt"] in DTS and r["shape"][1] % 8 == 0 and r["group"] % 8 == 0 and r["g_idx"] is None
    assert (r["qtype"] == "fp8") or zp_dtype is torch.int32  # fkind != 0, or zdt != CT_I8
    check(key, op, run(cta, dev, key, op, zp_dtype=zp_dtype))


# ---- FP4 with given scales ------------------------------------------------------------------------------------------------------------------------------
FP4_KEYS = [f"fp4.nv.{name}" for name in C.FP4_GLOBALS] + ["fp4.mx"]


def fp4_lean(r, x, s):
    """the lean form of ct_fp4_quant_pack / _stored: 2-D 16-bit weights, whole groups per row, every lane owns four whole units, the scale table
    flat and of a float dtype (MXFP4: a 16-bit one), a global scale exactly for NVFP4"""
    rows, cols = r["shape"]
    return (x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16) and cols % r["group"] == 0 and (rows * cols) % 32 == 0 and x.is_contiguous()
            and tuple(s.shape) == (rows, cols // r["group"]) and s.is_contiguous() and x.data_ptr() % 16 == 0 and s.data_ptr() % 8 == 0
            and s.dtype is x.dtype and (r["gs"] is not None) == (r["group"] == 16))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("entry", ["pack", "stored"])
@pytest.mark.parametrize("key", FP4_KEYS)
def test_fp4_given_scales(cta, dev, key, entry, dt):
    """ct_fp4_quant_pack and ct_fp4_quant_pack_stored: NVFP4 under all 256 float8 scale bytes times a global scale that puts s_eff inside, at either
    end of, next to and far outside the guard [2^-20, 2^10] of the refined reciprocal; MXFP4 under every power of two (the multiply by the
    reciprocal serves 2^-100 .. 2^100).  The sign bit of a code whose quotient is NaN is not compared"""
    key = f"{key}.{dt}"
    r = CASES[key]
    x, s = on(dev, cpu_side(key)[0], "x", "scale")
    gs = None if r["gs"] is None else C.global_scale(r).to(dev)
    assert fp4_lean(r, x, s)
    if entry == "pack":
        check(key, "fp4", cta.codec.fp4_quantize_and_pack(x, s, gs, group_size=r["group"]))
        return
    got = cta.codec.fp4_quantize_and_pack_stored(x, s, gs, group_size=r["group"], scale_dtype=C.F8 if r["group"] == 16 else torch.uint8)
    assert got is not None, "not the layout ct_fp4_quant_pack_stored takes"
    check(key, "fp4", got[0])
    check(key, "fp4s", got[1])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fmt", ["nv", "mx"])
def test_fp4_tables(cta, dev, fmt, dt):
    """ct_fp4_quant_pack_batch: every NVFP4 case of the dtype in ONE launch, each item under its own global scale; the MXFP4 case next to its
    first 64 rows as a second item"""
    c = cta.codec
    keys = [f"{k}.{dt}" for k in FP4_KEYS if k.split(".")[1] == fmt]
    group = 16 if fmt == "nv" else 32
    items = []
    for key in keys:
        r = CASES[key]
        x, s = on(dev, cpu_side(key)[0], "x", "scale")
        gs = None if r["gs"] is None else C.global_scale(r).to(dev)
        assert fp4_lean(r, x, s) and r["group"] == group
        items.append((key, x, s, gs, None))
    if fmt == "mx":
        key, x, s, _, _ = items[0]
        items.append((key, x[:64].contiguous(), s[:64].contiguous(), None, 64))
    assert len(items) >= 2
    IW = c._ITEM_WORDS
    packed = [torch.empty((x.shape[0], x.shape[1] // 2), dtype=torch.uint8, device=dev) for _, x, _, _, _ in items]
    stored = [torch.empty(tuple(s.shape), dtype=C.F8 if group == 16 else torch.uint8, device=dev) for _, _, s, _, _ in items]
    flat = []
    for (_, x, s, gs, _), p_, st in zip(items, packed, stored):
        flat += [x.data_ptr(), s.data_ptr(), 0 if gs is None else gs.data_ptr(), p_.data_ptr(), x.shape[0], x.shape[1], group, 0, 0, 0, st.data_ptr()] + [0] * (IW - 11)
    c.launch_fp4_words(torch.tensor(flat, dtype=torch.int64), len(items), "compress", dev, group, items[0][1].dtype, items[0][2].dtype)
    torch.cuda.synchronize()
    for (key, _, _, _, head), p_, st in zip(items, packed, stored):
        if head is None:
            check(key, "fp4", p_)
            check(key, "fp4s", st)
        else:  # the first rows of the same tensor: the same words
            assert torch.equal(p_.cpu(), packed[0][:head].cpu()) and torch.equal(st.cpu(), stored[0][:head].cpu())


# ---- static q / k / v QDQ -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("strategy", ["attn_head", "tensor"])
@pytest.mark.parametrize("key", ["attn.int8.sym", "attn.fp8.sym", "attn.int8.i4"])
def test_static_attention_qdq(cta, dev, key, strategy, dt):
    """ct_attn_qdq: a (1, H, S, D) state whose heads hold one edge scale each — read in place, whole 16-byte units; `attn_head` in one launch,
    `tensor` a head at a time under that head's scale (the same rows)"""
    key = f"{key}.{dt}"
    r = CASES[key]
    B, H, S, D = r["attn"]
    x, s, z = on(dev, cpu_side(key)[0], "x", "scale", "zero_point")
    x, s, z = x.reshape(B, H, S, D), s.reshape(H, 1, 1), None if z is None else z.reshape(H, 1, 1)
    c = cta.codec
    kw = dict(num_bits=8, qtype="float" if r["qtype"] == "fp8" else "int")
    plan = c.plan_attn_qdq(x.shape, x.stride(), x.dtype, s.shape, "attn_head")
    assert plan.in_place and plan.vector and plan.per_head and (plan.B, plan.H, plan.S, plan.D) == (B, H, S, D)
    heads = range(H) if H <= 17 else range(0, H, 16)  # (272 heads: every 16th a head at a time — each edge scale once)
    for op in r["ops"]:
        def qdq(xx, ss, zz, st):
            if op in ("fq", "fq8"):
                return c.attn_fake_quantize(xx, ss, zz, strategy=st, **kw)
            return c.attn_quantize(xx, ss, zz, strategy=st, dtype=torch.int8 if op == "q" else C.F8, **kw)

        if strategy == "attn_head":
            check(key, op, qdq(x, s, z, "attn_head").reshape(H, S * D))
            continue
        want = cpu_side(key)[1][op]
        for h in heads:
            one = x[:, h:h + 1]
            p1 = c.plan_attn_qdq(one.shape, one.stride(), one.dtype, (1,), "tensor")
            assert p1.in_place and p1.vector and not p1.per_head
            got = qdq(one, s[h].reshape(1), None if z is None else z[h].reshape(1), "tensor").reshape(S * D).cpu()
            assert eq_f8(got, want[h]) if want.dtype is C.F8 else eq(got, want[h]), (key, op, h)


# ---- class level -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key", ["w4.g128.sym", "w4.g128.ib", "w3.guard.g128.ib"])
def test_packed_compressor_compress(cta, dev, key, dt):
    """PackedQuantizationCompressor.compress: a symmetric W4 scheme through ct_quant_pack's lean branch, an asymmetric one through
    ct_quant_pack_w4_zp (w4_quant_pack_one_kernel: words and stored zero points from one launch), another width through wb_quant_pack_lean_kernel"""
    key = f"{key}.{dt}"
    r, t = CASES[key], cpu_side(key)[0]
    x, s, z = on(dev, t, "x", "scale", "zero_point")
    if r["bits"] != 4:
        assert wb_ok(r, s, z)
    elif z is None:
        assert w4_lean(r) and w4_variant(r) == "plain"
    else:  # _w4_zp_fused_ok
        assert z.dtype is torch.int8 and r["shape"][1] % 32 == 0 and r["group"] % 32 == 0 and tuple(s.shape) == (r["shape"][0], r["shape"][1] // r["group"])
        assert cta.codec.quantize_and_pack_with_zp(x, s, z, **C.kw_of(r)) is not None
    args = cta.QuantizationArgs(num_bits=r["bits"], group_size=r["group"], symmetric=z is None, strategy="group")
    sd = {"weight": x, "weight_scale": s, **({} if z is None else {"weight_zero_point": z})}
    out = cta.PackedQuantizationCompressor.compress(sd, cta.QuantizationScheme(targets=["Linear"], weights=args))
    check(key, "pack", out["weight_packed"])
    if z is not None:
        assert torch.equal(out["weight_zero_point"].cpu(), O.pack_to_int32(t["zero_point"], r["bits"], packed_dim=0).contiguous())
    else:
        assert "weight_zero_point" not in out
