"""Every observer kernel over the whole domain of group extremes (tests/_observer_range_cases.py): every 16-bit pattern as a group's extreme
(`sweep16`, bfloat16 and float16), every exponent (`exp16`), the edge patterns crossed with each other (`cross`: one-sided and all-zero groups, inf
with -inf, NaN with inf), the half-integer ties of the zero point (`ties`) and the fp32 sweep — through each form of `minmax_qparams` /
`minmax_qparams_float` (ct_qparams.hip: absmax, subwave with 4 and 1 units per lane, the three bodies of the wave kernel), `generate_gparam`, and
the observer halves of the one-pass RTN kernels.  A result is compared bit for bit (`eq` of test_oracle_golden: NaN == NaN, -0.0 != +0.0; zero
points exactly) with the pinned oracle on the CPU and, as canonical sha256 and NaN / inf / zero counts (whole tensors for `cross`), with what the
reference recorded (tests/golden/observer_ranges_manifest.json).  The one property not compared with the record is the MX scale of a group that
holds a NaN (`_observer_range_cases.masked`); kernel and oracle are compared there too (inf).
Every test asserts, with `form` — a mirror of minmax_qparams_impl's dispatch rule — which kernel form its case takes, so a later change of the
rule cannot silently move a case to another kernel.
Every test here needs an MI355X:  python -m pytest tests -m gpu"""
import functools

import pytest
import torch
from test_oracle_golden import eq, eq_f8

import _observer_range_cases as R
import oracle as O

pytestmark = pytest.mark.gpu

CASES = dict(R.case_list())
DTS = ("bf16", "f16")
BLOCK, ABSMAX_U = 256, 4  # kBlock of ct_common.h, the units per lane of qparams_absmax_kernel


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


def form(shape, cdiv, dt, symmetric, aligned=True) -> str:
    """minmax_qparams_impl's dispatch: from cdiv % 8, cols % cdiv, the units per group a power of two <= 64 / <= 256, the dtype, the symmetry and
    the 16-byte alignment of the weight"""
    rows, cols = shape
    upg = cdiv // 8
    subwave = cdiv % 8 == 0 and cols % cdiv == 0 and upg >= 1 and upg & (upg - 1) == 0 and upg <= 256 and aligned
    if subwave and symmetric and dt != "f32" and upg <= 64:
        return "absmax"
    if subwave:
        return "subwave4" if upg >= 4 else "subwave1"
    vec = cols % 8 == 0 and (cdiv % 8 == 0 or cdiv >= cols) and aligned
    if vec and symmetric and dt != "f32":
        return "wave.pairs"
    return "wave.vector" if vec else "wave.element"


def pairs_tail(cols) -> tuple:
    """(full trips of 512 units, the tail's loads in flight: 0, 4 or 8, how many of them read units of the row — the others are clamped to its
    last unit) of the raw-pair body of qparams_wave_kernel for a row of `cols`"""
    nu = cols // 8
    rem = nu % 512
    return nu // 512, 8 if rem > 256 else 4 if rem else 0, -(-rem // 64)


@functools.lru_cache(maxsize=3)
def weight(key):
    """a case's weight on the CPU; never written to"""
    return R.weight(CASES[key])


@functools.lru_cache(maxsize=2)
def weight_on(key, dev):
    x = weight(key).to(dev)
    assert x.data_ptr() % 16 == 0 and x.is_contiguous()
    return x


@functools.lru_cache(maxsize=None)
def want(key, op):
    """(scale, zero point or None) of the pinned oracle; never written to"""
    return R.oracle_output(O, CASES[key], weight(key), op)


def check(key, op, scale, zp=None, fixture=True):
    r = CASES[key]
    ws, wz = want(key, op)
    scale = scale.reshape(ws.shape).cpu()
    assert scale.dtype is ws.dtype and eq(scale, ws), (key, op, int((R.canonical(scale) != R.canonical(ws)).sum()))
    if wz is not None:
        zp = zp.reshape(wz.shape).cpu()
        assert zp.dtype is torch.int8 and torch.equal(zp, wz), (key, op, int((zp != wz).sum()))
    if fixture:
        assert R.fixture_mismatch(key, op, r, weight(key), scale, zp if wz is not None else None) == "", (key, op)


def observe(cta, dev, key, op, x=None):
    """the product's observer for an op of a case: (scale, zero point or None)"""
    r = CASES[key]
    p = R.parse_op(op)
    x = weight_on(key, dev) if x is None else x
    if p["kind"] == "int":
        return cta.codec.minmax_qparams(x, num_bits=p["bits"], group_size=r["group"], symmetric=p["symmetric"])
    gs = R.global_scale(O, r, weight(key), op).to(dev) if p["kind"] == "nvfp4" else None
    return cta.codec.minmax_qparams_float(x, kind=p["kind"], group_size=r["group"], global_scale=gs), None


def case_form(key, op, aligned=True):
    r = CASES[key]
    p = R.parse_op(op)
    return form(r["shape"], r["group"] or r["shape"][1], r["dt"], p.get("symmetric", True), aligned)


def every(cases, body):
    """`body(*case)` for every case, all failures reported together: one test per kernel form and dtype rather than one per case — there are some
    five hundred of them — and a failure still names its case"""
    cases, bad = list(cases), []
    for case in cases:
        case = case if isinstance(case, tuple) else (case,)
        try:
            body(*case)
        except AssertionError as e:
            bad.append(f"{case}: {str(e)[:400]}")
    assert cases and not bad, f"{len(bad)} of {len(cases)} cases fail:\n" + "\n".join(bad)


INT48 = ("i4s", "i8s", "i4a", "i8a")
FP32 = [("s32.g32", "subwave4"), ("s32.g128", "subwave4"), ("c32.g32", "subwave4"), ("c32.g128", "subwave4"), ("s32.g8", "subwave1"), ("c32.g8", "subwave1"),
        ("s32.chan96", "wave.vector"), ("c32.chan5632", "wave.vector")]


def run_and_check(cta, dev, key, op, expect):
    assert case_form(key, op) == expect, (key, op, case_form(key, op))
    assert op in CASES[key]["ops"]
    check(key, op, *observe(cta, dev, key, op))


# ---- qparams_absmax_kernel ----------------------------------------------------------------------------------------------------------------------
ABSMAX = ([("s16.g32", f"i{b}s") for b in range(1, 9)] + [(k, op) for k in ("s16.g8", "s16.g16", "s16.g128", "e16.g512", "e16.row.g32", "c16.g32", "c16.g128")
                                                          for op in ("i4s", "i8s")])


@pytest.mark.parametrize("dt", DTS)
def test_absmax(cta, dev, dt):
    """16-bit weights, symmetric, at most 64 units per group: the raw bit patterns reduced as integers (a NaN is a pattern above inf).  A wave
    holds 4 * 64 / upg groups and evaluates 64 per trip of the `g0` loop: four trips at g = 8, two at g = 16, one from g = 32 on; g = 512: all 64
    lanes of a load in one group; the single row of 2049 (257) groups: units that are no whole number of workgroups — the clamped loads and the
    `live` mask"""
    def one(key, op):
        key = f"{key}.{dt}"
        r = CASES[key]
        upg = r["group"] // 8
        trips = -(-(ABSMAX_U * (64 // upg)) // 64)
        assert trips == {8: 4, 16: 2}.get(r["group"], 1)
        units = r["shape"][0] * r["shape"][1] // 8
        assert (units % (BLOCK * ABSMAX_U) != 0) is (key.startswith(("e16.row", "c16")))
        run_and_check(cta, dev, key, op, "absmax")

    every(ABSMAX, one)


# ---- qparams_subwave_kernel ---------------------------------------------------------------------------------------------------------------------
SUBWAVE4 = ([("s16.g32", f"i{b}a") for b in range(1, 9)] + [("ties.g32", f"i{b}a") for b in range(1, 9)]
            + [(k, op) for k in ("s16.g128", "c16.g32", "c16.g128") for op in ("i4a", "i8a")]
            + [("e16.g2048", op) for op in ("i4a", "i8a", "i4s", "i8s")] + [("e16.g1024", op) for op in ("i4s", "i8s")])


@pytest.mark.parametrize("dt", DTS)
def test_subwave_four_units_per_lane(cta, dev, dt):
    """qparams_subwave_kernel<., 4>: float min / max with a NaN flag, DPP inside a row of 16 lanes and ds_bpermute beyond it (g = 2048: 64 lanes);
    symmetric 16-bit groups of more than 64 units take the raw-pair branch INSIDE this kernel"""
    def one(key, op):
        key = f"{key}.{dt}"
        r = CASES[key]
        if op[2] == "s":
            assert r["group"] // 8 > 64
        run_and_check(cta, dev, key, op, "subwave4")

    every(SUBWAVE4, one)


@pytest.mark.parametrize("dt", DTS)
def test_subwave_one_unit_per_lane(cta, dev, dt):
    def one(key, op):
        run_and_check(cta, dev, f"{key}.{dt}", op, "subwave1")

    every([(k, op) for k in ("s16.g8", "s16.g16") for op in ("i4a", "i8a")], one)


def test_fp32_weights(cta, dev):
    """fp32 weights take the float forms whatever the symmetry: no raw-pair reduction"""
    def one(key, expect, op):
        run_and_check(cta, dev, key, op, expect)

    every([(k, f, op) for k, f in FP32 for op in INT48], one)


# ---- qparams_wave_kernel ------------------------------------------------------------------------------------------------------------------------
WIDTHS = {96: (0, 4, 1), 1992: (0, 4, 4), 2056: (0, 8, 5), 4000: (0, 8, 8), 4096: (1, 0, 0), 5632: (1, 4, 3), 6496: (1, 8, 5)}


@pytest.mark.parametrize("dt", DTS)
def test_wave_channel_wise(cta, dev, dt):
    """a wave per row.  Symmetric: the raw pairs with eight loads in flight — a 4-load tail (96 columns), an 8-load tail (2056), one full trip and
    no tail (4096), a trip and a short tail (5632), a trip and a long tail (6496); 1992 and 4000: a tail whose LAST load still reads units of the row
    (in the others it is clamped to the row's last unit).  Asymmetric: the vector float form on the same rows"""
    def one(cols, op):
        key = f"e16.chan{cols}.{dt}"
        assert pairs_tail(cols) == WIDTHS[cols] and CASES[key]["shape"][1] == cols and sorted(WIDTHS) == list(R.CHANNEL_WIDTHS)
        run_and_check(cta, dev, key, op, "wave.pairs" if op[2] == "s" else "wave.vector")

    every([(c, op) for c in sorted(WIDTHS) for op in INT48], one)


@pytest.mark.parametrize("dt", DTS)
def test_wave_tensor_strategy(cta, dev, dt):
    """the `tensor` strategy: the exp16 tensor of groups of 32 as ONE row of 16 (2) full trips"""
    def one(op):
        key = f"e16.tensor.{dt}"
        assert CASES[key]["shape"][0] == 1 and pairs_tail(CASES[key]["shape"][1]) == (16 if dt == "bf16" else 2, 0, 0)
        run_and_check(cta, dev, key, op, "wave.pairs" if op[2] == "s" else "wave.vector")

    every(INT48, one)


@pytest.mark.parametrize("dt", DTS)
def test_wave_element_form(cta, dev, dt):
    """rows of 20 columns; groups of 48 in rows of 100 (a ragged last group of 4); groups of 20 (no 16-byte units)"""
    def one(key, op):
        key = f"{key}.{dt}"
        r = CASES[key]
        assert (r["shape"][1] % (r["group"] or r["shape"][1]) != 0) is key.startswith("c16.g48")
        run_and_check(cta, dev, key, op, "wave.element")

    every([(k, op) for k in ("s16.chan20", "c16.g48", "c16.g20") for op in INT48], one)


@pytest.mark.parametrize("dt", DTS)
def test_wave_element_form_of_a_misaligned_view(cta, dev, dt):
    """the g = 32 `cross` tensor read through a contiguous view that starts 2 bytes into its storage: no 16-byte loads, the element form (the
    Python entry would clone such a view to an aligned one, so the library is called as a C caller would)"""
    from compressed_tensors_amd._lib import DT, call, ptr, stream_of

    def one(op):
        key = f"c16.g32.{dt}"
        r, p = CASES[key], R.parse_op(op)
        assert case_form(key, op, aligned=False) == "wave.element" and case_form(key, op) in ("absmax", "subwave4")
        x = weight_on(key, dev)
        store = torch.zeros(x.numel() + 8, dtype=x.dtype, device=dev)
        view = store[1:1 + x.numel()].view(x.shape)
        view.copy_(x)
        assert store.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 2 and view.is_contiguous()
        rows, cols = x.shape
        scale = torch.empty(R.grid(r), dtype=x.dtype, device=dev)
        zp = torch.empty(R.grid(r), dtype=torch.int8, device=dev)
        call("ct_minmax_qparams", ptr(view), DT[x.dtype], rows, cols, r["group"], p["bits"], int(p["symmetric"]), ptr(scale), ptr(zp), stream_of(view))
        check(key, op, scale, zp)

    every(INT48, one)


# ---- FLOAT kinds --------------------------------------------------------------------------------------------------------------------------------
FLOAT16 = ([(k, "fp8", f) for k, f in (("s16.g32", "absmax"), ("s16.g128", "absmax"), ("c16.g32", "absmax"), ("c16.g128", "absmax"), ("e16.chan5632", "wave.pairs"),
                                       ("e16.chan96", "wave.pairs"), ("e16.chan2056", "wave.pairs"))]
           + [(k, op, "absmax") for k in ("s16.g16", "c16.g16") for op in R.NV_OPS] + [(k, op, "absmax") for k in ("s16.g32", "c16.g32") for op in ("mxfp4", "mxfp8")])


@pytest.mark.parametrize("dt", DTS)
def test_float_kinds(cta, dev, dt):
    """minmax_qparams_float: fp8 (amax / 448, the eps substitution), nvfp4 under the global scales 1, 2^-10, 896, 2^12 and generate_gparam of the
    case's finite part (clamp at 448, the float8 rounding, 0 -> 0.125), mxfp4 / mxfp8 (a NaN group: inf)"""
    def one(key, op, expect):
        key = f"{key}.{dt}"
        run_and_check(cta, dev, key, op, expect)
        if op in R.MASKED_OPS:
            got = observe(cta, dev, key, op)[0].cpu()
            nang = R.nan_groups(CASES[key], weight(key))
            assert int(nang.sum()) > 0 and bool(torch.isposinf(got[nang]).all())

    every(FLOAT16, one)


def test_float_kinds_fp32(cta, dev):
    def one(key, op):
        run_and_check(cta, dev, key, op, "subwave4")

    every([(k, op) for k in ("s32.g32", "c32.g32") for op in ("fp8", "mxfp4", "mxfp8")], one)


# ---- generate_gparam ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_generate_gparam(cta, dev, dt):
    """one tensor per exp16 pattern and per edge, the extreme its last element: (4, 64) rows take the absmax kernel, (3, 20) rows the element form
    of the wave kernel; then gparam_finish_kernel (clamp at tiny, reciprocal, x 2688, non-finite -> 1)"""
    def one(shape):
        assert form(shape, shape[1], dt, True) == ("absmax" if shape[1] == 64 else "wave.element")
        xs = R.weight(R.gparam_case(dt, shape)).reshape(-1, *shape)
        xd = xs.to(dev)
        got = torch.cat([cta.codec.generate_gparam(t) for t in xd]).cpu()
        ref = torch.cat([O.generate_gparam(t).reshape(1) for t in xs])
        assert got.dtype is torch.float32 and eq(got, ref), int((got != ref).sum())
        assert R.gparam_mismatch(dt, shape, got) == ""

    every([(shape,) for shape in R.gparam_shapes()], one)


# ---- the observer halves of the one-pass kernels ------------------------------------------------------------------------------------------------
def check_both(cta, dev, key, op, scale, zp):
    """a one-pass kernel's scale and zero point: the oracle's, the record's, and the observer kernel's of the same weight"""
    check(key, op, scale, zp)
    os_, oz = observe(cta, dev, key, op)
    assert eq(scale.cpu().reshape(os_.shape), os_.cpu()) and (oz is None or torch.equal(zp.cpu().reshape(oz.shape), oz.cpu())), (key, op)


GROUPED = ["s16.g32", "c16.g32", "s16.g128", "c16.g128"]


@pytest.mark.parametrize("dt", DTS)
def test_rtn_quantize_and_pack_observer(cta, dev, dt):
    def one(key, bits, sym):
        key = f"{key}.{dt}"
        r = CASES[key]
        assert cta.codec.rtn_w4_group(r["shape"], r["group"]) == r["group"]
        _, s, z = cta.codec.rtn_quantize_and_pack(weight_on(key, dev), group_size=r["group"], symmetric=sym == "s", num_bits=bits)
        check_both(cta, dev, key, f"i{bits}{sym}", s, z)

    every([(k, b, s) for k in GROUPED for b in (2, 3, 4, 5, 6, 7) for s in "sa"], one)


@pytest.mark.parametrize("dt", DTS)
def test_rtn_quantize_group8_observer(cta, dev, dt):
    def one(key, kind):
        key = f"{key}.{dt}"
        r = CASES[key]
        if kind == "mxfp8" and r["group"] != 32:
            with pytest.raises(NotImplementedError):
                cta.codec.rtn_quantize_group8(weight_on(key, dev), group_size=r["group"], qtype="float", mx=True)
            return
        assert cta.codec.rtn_group8_group(r["shape"], r["group"]) == r["group"]
        x = weight_on(key, dev)
        if kind[0] == "i":
            _, s, z = cta.codec.rtn_quantize_group8(x, group_size=r["group"], qtype="int", symmetric=kind == "i8s")
        else:
            got = cta.codec.rtn_quantize_group8(x, group_size=r["group"], qtype="float", mx=kind == "mxfp8")
            s, z = got[1], None
            if kind == "mxfp8":  # the stored E8M0 codes: compress_mx_scale of the observer's scale
                assert torch.equal(got[3], cta.codec.compress_mx_scale(observe(cta, dev, key, kind)[0]))
        check_both(cta, dev, key, kind, s, z)

    every([(k, kind) for k in GROUPED for kind in ("i8s", "i8a", "fp8", "mxfp8")], one)


@pytest.mark.parametrize("dt", DTS)
def test_rtn_quantize_channel8_observer(cta, dev, dt):
    def one(cols, kind):
        key = f"e16.chan{cols}.{dt}"
        assert cta.codec.rtn_channel8_form(CASES[key]["shape"], kind != "i8a") == ("wave" if cols == 96 or kind == "i8a" else "row")
        for other in (cta.codec.rtn_quantize_and_pack, cta.codec.rtn_quantize_group8):  # such a row is no group of 32 * 2^k: theirs to refuse
            with pytest.raises(NotImplementedError):
                other(weight_on(key, dev), group_size=None)
        _, s, z = cta.codec.rtn_quantize_channel8(weight_on(key, dev), qtype="float" if kind == "fp8" else "int", symmetric=kind != "i8a")
        if kind == "fp8":
            assert z.dtype is R.F8 and int(z.view(torch.uint8).count_nonzero()) == 0
        check_both(cta, dev, key, kind, s, z if kind != "fp8" else None)

    every([(c, kind) for c in (96, 2056, 5632) for kind in ("i8s", "i8a", "fp8")], one)


@pytest.mark.parametrize("dt", DTS)
def test_rtn_quantize_block8_observer(cta, dev, dt):
    """the block observer (`codes=False`): the sweep16 groups of 64 laid out as blocks [4, 16], exp16 in blocks [128, 128], the cross in blocks
    [16, 64] — equal to the oracle over the blocks as rows, to the record, and to `_block_rows` + the observer kernel"""
    from compressed_tensors_amd.quantization.utils import _block_rows

    def one(key, kind):
        key = f"{key}.{dt}"
        r = CASES[key]
        x = weight_on(key, dev)
        assert cta.codec.rtn_block8_group(r["shape"], r["block"]) != 0
        none, s, z = cta.codec.rtn_quantize_block8(x, block_structure=r["block"], qtype="float" if kind == "fp8" else "int", symmetric=kind != "i8a", codes=False)
        assert none is None and tuple(s.shape) == R.grid(r)
        check(key, kind, s, z if kind != "fp8" else None)
        blocks, grid = _block_rows(x, r["block"])
        assert tuple(grid) == R.grid(r) and torch.equal(blocks.cpu().view(torch.int16), R.to_groups(r, weight(key)).view(torch.int16))
        if kind == "fp8":
            s2, z2 = cta.codec.minmax_qparams_float(blocks, kind="fp8"), None
        else:
            s2, z2 = cta.codec.minmax_qparams(blocks, num_bits=8, symmetric=kind == "i8s")
        check(key, kind, s2, z2)

    every([(k, kind) for k in ("s16.blk4x16", "e16.blk128", "c16.blk16x64") for kind in ("i8s", "i8a", "fp8")], one)


@pytest.mark.parametrize("dt", DTS)
def test_rtn_mxfp4_stored_scales(cta, dev, dt):
    """the stored E8M0 codes are compress_mx_scale of the observer's scale; the float scale it returns is the observer's"""
    def one(key):
        key = f"{key}.{dt}"
        _, code, s = cta.codec.rtn_mxfp4_quantize_and_pack(weight_on(key, dev), return_scale=True)
        check_both(cta, dev, key, "mxfp4", s, None)
        assert code.dtype is torch.uint8 and torch.equal(code, cta.codec.compress_mx_scale(observe(cta, dev, key, "mxfp4")[0]))

    every(["s16.g32", "c16.g32"], one)


@pytest.mark.parametrize("dt", DTS)
def test_rtn_nvfp4_stored_scales(cta, dev, dt):
    """the stored float8 scales are the float8 cast of the observer's (float8-representable) float32 scale"""
    def one(key, op):
        key = f"{key}.{dt}"
        gs = R.global_scale(O, CASES[key], weight(key), op).to(dev)
        _, s8, gs_out, s = cta.codec.rtn_nvfp4_quantize_and_pack(weight_on(key, dev), gs, return_scale=True)
        assert torch.equal(gs_out.cpu().view(torch.int32), gs.cpu().view(torch.int32))
        check_both(cta, dev, key, op, s, None)
        ws = want(key, op)[0]
        assert s8.dtype is R.F8 and eq_f8(s8.cpu(), ws.to(R.F8)) and bool((ws.to(R.F8).float() == ws)[~torch.isnan(ws)].all())

    every([(k, op) for k in ("s16.g16", "c16.g16") for op in R.NV_OPS], one)


# ---- class level --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_calculate_qparams_from_weight(cta, dev, dt):
    """`calculate_qparams_from_weight` on the `cross` weight: the shapes the reference initialises — tensor (1,), channel (R, 1), group (R, G), block
    (ceil(R / bh), ceil(C / bw)) — and the oracle's bits (group and block: the record's too)"""
    from compressed_tensors_amd.quantization import calculate_qparams_from_weight

    def one(strategy, sym):
        key = f"c16.blk16x64.{dt}" if strategy == "block" else f"c16.g32.{dt}"
        r = CASES[key]
        op = "i8s" if sym else "i8a"
        x = weight_on(key, dev)
        extra = dict(group_size=32) if strategy == "group" else dict(block_structure=r["block"]) if strategy == "block" else {}
        s, z = calculate_qparams_from_weight(x, cta.QuantizationArgs(num_bits=8, symmetric=sym, strategy=strategy, **extra))
        rows, cols = r["shape"]
        assert tuple(s.shape) == tuple(z.shape) == {"tensor": (1,), "channel": (rows, 1), "group": (rows, cols // 32), "block": R.grid(r)}[strategy]
        assert s.dtype is x.dtype and z.dtype is torch.int8
        if strategy in ("group", "block"):
            check(key, op, s, z)
            return
        xc = weight(key)
        ws, wz = O.calculate_qparams_minmax(xc.reshape(1, -1) if strategy == "tensor" else xc, num_bits=8, symmetric=sym)
        assert eq(s.cpu().reshape(ws.shape), ws) and torch.equal(z.cpu().reshape(wz.shape), wz)

    every([(st, sym) for st in ("tensor", "channel", "group", "block") for sym in (True, False)], one)
