"""Host side of the one-pass round-to-nearest compress of the widths next to 4 and 8 (pack-quantized W2 / W3 / W5 / W6 / W7 from a dense model): the
C ABI's three symbols, the planner of the table form (ct_rtn_wb_batch_plan) and its named refusals, the argument errors of the codec entries, the
gates, PackQuantizedQuantizer's name-only methods, and the fixture tests/golden/packw_rtn.safetensors against the pinned oracle and, where the
reference sources exist, against the reference itself.  No GPU: the planner is a host function."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import _packw_rtn_cases as C
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "packw_rtn.safetensors")
NEW = ("ct_rtn_quant_pack_wb", "ct_rtn_wb_batch_plan", "ct_rtn_quant_pack_wb_batch")


@pytest.fixture(scope="module")
def lib():
    from compressed_tensors_amd import _lib

    return _lib.load()


def table(items):
    """a host table of (rows, cols, group) with made-up, aligned addresses: the planner looks at pointers, it never follows them"""
    from compressed_tensors_amd import _lib

    tab = (_lib.W4Item * max(len(items), 1))()
    for i, (rows, cols, group) in enumerate(items):
        it, base = tab[i], 0x100000 * (i + 1)
        it.src, it.dst, it.scale, it.zp = base, base + 0x80000, base + 0xC0000, base + 0xE0000
        it.rows, it.cols, it.group = rows, cols, group
    return tab


def plan(lib, tab, bits=3, n=None):
    return int(lib.ct_rtn_wb_batch_plan(ctypes.cast(tab, ctypes.c_void_p), len(tab) if n is None else n, bits))


FAST_ITEMS = [(shape[0], shape[1], group or 0) for shape, group, _ in C.FAST]


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_prototyped(lib):
    from compressed_tensors_amd import _lib, codec

    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ct_hip.h")).read(), flags=re.S)
    header = re.sub(r"\s+", " ", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NEW:
        assert name in exported and name in _lib._PROTOTYPES and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert ("int ct_rtn_quant_pack_wb(const void* x, int xdt, int64_t rows, int64_t cols, int64_t group, int bits, int symmetric, int32_t* packed, "
            "void* scale_out, int8_t* zp_out, ct_stream_t stream);") in header
    assert "int64_t ct_rtn_wb_batch_plan(ct_w4_item* items_host, int n, int bits);" in header
    assert "int ct_rtn_quant_pack_wb_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int dt, int bits, int symmetric, ct_stream_t stream);" in header
    assert [len(_lib._PROTOTYPES[name][0]) for name in NEW] == [11, 3, 7]
    assert lib.ct_abi_version() == 2 and ctypes.sizeof(_lib.W4Item) == 13 * 8  # additive: nothing an existing caller sees moved
    for name in ("rtn_quantize_and_pack", "rtn_quantize_and_pack_many", "rtn_wb_table_item", "launch_rtn_wb_words", "RTN_PACKW_BITS"):
        assert hasattr(codec, name) and name in codec.__all__
    assert codec.RTN_PACKW_BITS == C.BITS
    assert codec._TABLES["rtn_wb"] == ("ct_rtn_wb_batch_plan", True, "ct_rtn_quant_pack_wb_batch")  # the plan's third argument is the width
    assert codec.launch_rtn_wb_words(None, 0, None, torch.device("cpu"), 3, True) is None  # an empty table: nothing is touched


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", C.BITS)
def test_plan_counts_workgroups_of_256_lanes_of_32_elements_and_fills_the_derived_fields(lib, bits):
    tab = table(FAST_ITEMS)
    want = [-(-(rows * cols) // 8192) for rows, cols, _ in FAST_ITEMS]
    assert want[:5] == [1, 1, 1, 2, 2] and plan(lib, tab, bits) == sum(want)  # 8224 / 8320 elements: one full workgroup and a partial one
    first = 0
    for it, (rows, cols, g), blocks in zip(tab, FAST_ITEMS, want):
        g = g or cols
        assert it.first_block == first and it.units == rows * cols // 8 and it.main_blocks == blocks, (rows, cols, g)
        assert it.upg == g // 8 and 1 << it.upg_shift == it.upg and 1 <= (1 << (it.upg_shift - 2)) <= 64  # lanes per group
        first += blocks
    assert plan(lib, table([(8192, 8192, 128)]), bits) == 8192 * 8192 // 8192
    assert plan(lib, table(FAST_ITEMS), bits, 0) == 0
    sym = table([(4, 64, 32)])
    sym[0].zp = None  # a symmetric table may leave the zero-point output out
    assert plan(lib, sym, bits) == 1
    four = table([(4, 64, 32)])
    four[0].dst += 4  # the packed words need 4-byte alignment only
    assert plan(lib, four, bits) == 1


@pytest.mark.parametrize("what", ["ragged_cols", "group48", "group16", "group96", "too_large", "channel40", "misaligned_src", "misaligned_dst", "no_scale",
                                  "no_dst", "no_rows", "zp_packed"])
def test_plan_refuses_and_names_the_item(lib, what):
    from compressed_tensors_amd import _lib

    items = [(4, 128, 32), (8, 256, 128), (2, 2048, 2048)]
    change = dict(ragged_cols=(8, 200, 128), group48=(8, 96, 48), group16=(8, 256, 16), group96=(8, 192, 96), too_large=(8, 4096, 4096),
                  channel40=(2, 40, 0), no_rows=(0, 256, 128))
    if what in change:
        items[1] = change[what]
    tab = table(items)
    if what == "misaligned_src":
        tab[1].src += 8
    elif what == "misaligned_dst":
        tab[1].dst += 2
    elif what == "no_scale":
        tab[1].scale = None
    elif what == "no_dst":
        tab[1].dst = None
    elif what == "zp_packed":
        tab[1].zp_packed = 0x4000
    assert plan(lib, tab) == -1
    msg = _lib.last_error()
    assert "ct_rtn_wb_batch_plan" in msg and "item 1" in msg, msg
    assert ("ct_pack_int32_dim0" if what == "zp_packed" else "32 * 2^k") in msg, msg


def test_plan_and_launches_refuse_other_widths_naming_what_serves_them(lib):
    from compressed_tensors_amd import _lib

    a = 0x100000
    for bits, names in ((4, "ct_rtn_quant_pack_w4"), (8, "ct_rtn_quant_group8"), (1, "ct_minmax_qparams"), (0, "ct_minmax_qparams"), (9, "ct_minmax_qparams")):
        assert plan(lib, table([(4, 128, 32)]), bits) == -1 and names in _lib.last_error(), bits
        assert lib.ct_rtn_quant_pack_wb(a, _lib.BF16, 4, 128, 32, bits, 1, a, a, a, None) == _lib.CT_ERR_UNSUPPORTED and names in _lib.last_error(), bits
        assert lib.ct_rtn_quant_pack_wb_batch(a, 1, 1, _lib.BF16, bits, 1, None) == _lib.CT_ERR_UNSUPPORTED and names in _lib.last_error(), bits
    assert plan(lib, table(FAST_ITEMS), 3, -1) == -1 and "bad arguments" in _lib.last_error()
    assert int(lib.ct_rtn_wb_batch_plan(None, 1, 3)) == -1 and "bad arguments" in _lib.last_error()
    assert plan(lib, table([(1 << 22, 1 << 22, 32)] * 2)) == -1 and "exceed one launch" in _lib.last_error()
    # the dtype belongs to the launch, not to the plan: refused before anything touches a GPU
    assert lib.ct_rtn_quant_pack_wb(a, _lib.F32, 4, 64, 32, 3, 1, a, a, a, None) == _lib.CT_ERR_INVALID_ARG and "16-bit float weights" in _lib.last_error()
    assert lib.ct_rtn_quant_pack_wb_batch(a, 1, 1, _lib.F32, 3, 1, None) == _lib.CT_ERR_INVALID_ARG and "16-bit weights only" in _lib.last_error()
    assert lib.ct_rtn_quant_pack_wb(a, _lib.BF16, 4, 96, 48, 3, 1, a, a, a, None) == _lib.CT_ERR_INVALID_ARG and "32 * 2^k" in _lib.last_error()
    assert lib.ct_rtn_quant_pack_wb(a, _lib.BF16, 4, 96, 64, 3, 1, a, a, a, None) == _lib.CT_ERR_INVALID_ARG and "multiple of the group size" in _lib.last_error()
    assert lib.ct_rtn_quant_pack_wb(a + 8, _lib.BF16, 4, 64, 32, 3, 1, a, a, a, None) == _lib.CT_ERR_INVALID_ARG and "16-byte aligned" in _lib.last_error()
    assert lib.ct_rtn_quant_pack_wb(a, _lib.BF16, 4, 64, 32, 3, 1, a + 2, a, a, None) == _lib.CT_ERR_INVALID_ARG and "4-byte aligned" in _lib.last_error()
    assert lib.ct_rtn_quant_pack_wb(a, _lib.BF16, 4, 64, 32, 3, 0, a, a, None, None) == _lib.CT_ERR_INVALID_ARG and "zero-point outputs" in _lib.last_error()
    assert lib.ct_rtn_quant_pack_wb(a, _lib.BF16, 0, 64, 32, 3, 1, a, a, a, None) == _lib.CT_OK  # an empty tensor: nothing to do
    assert lib.ct_rtn_quant_pack_wb_batch(a, 0, 0, _lib.BF16, 3, 1, None) == _lib.CT_OK  # an empty table


def test_codec_group_rule_is_the_plans(lib):
    """`codec.rtn_w4_group`, which admits a weight to the W4 table, decides for this table too what its plan decides in the library"""
    from compressed_tensors_amd import codec

    for rows in (1, 3):
        for cols in (32, 40, 96, 200, 256, 1024, 2048, 4096):
            for g in (0, 16, 32, 48, 64, 96, 128, 256, 512, 1024, 2048, 4096):
                if g > cols:  # the table reads a group beyond the row as the row, the Python rule as ragged
                    continue
                took = plan(lib, table([(rows, cols, g)])) >= 0
                assert bool(codec.rtn_w4_group((rows, cols), g or None)) == took, (rows, cols, g)
                assert not took or codec.rtn_w4_group((rows, cols), g or None) == (g or cols)


# ---- the codec: argument errors ----------------------------------------------------------------------------------------------------------
def test_codec_refuses_by_name_before_any_device_is_touched():
    from compressed_tensors_amd import codec

    x = torch.zeros((2, 96), dtype=C.BF16)
    for b in C.BITS + (4,):
        with pytest.raises(ValueError, match="divisble by the given group_size"):
            codec.rtn_quantize_and_pack(x, group_size=64, num_bits=b)
        with pytest.raises(NotImplementedError, match="32 \\* 2\\^k"):
            codec.rtn_quantize_and_pack(x, group_size=48, num_bits=b)
        with pytest.raises(NotImplementedError, match="16-bit float"):
            codec.rtn_quantize_and_pack(x.float(), group_size=32, num_bits=b)
        with pytest.raises(ValueError, match="2-D"):
            codec.rtn_quantize_and_pack(x[0], group_size=32, num_bits=b)
        with pytest.raises(ValueError, match="group sizes for"):
            codec.rtn_quantize_and_pack_many([x], group_size=[32, 32], num_bits=b)
    for fn in (lambda **kw: codec.rtn_quantize_and_pack(x, group_size=32, **kw), lambda **kw: codec.rtn_quantize_and_pack_many([x], group_size=32, **kw)):
        with pytest.raises(NotImplementedError, match="minmax_qparams \\+ quantize_and_pack"):
            fn(num_bits=1)
        with pytest.raises(NotImplementedError, match="rtn_quantize_group8\\(words=True\\)"):
            fn(num_bits=8)
        for b in (0, 9, -3):
            with pytest.raises(ValueError, match="num_bits"):
                fn(num_bits=b)
    with pytest.raises(NotImplementedError, match="num_bits"):
        codec.launch_rtn_wb_words([], 0, C.BF16, torch.device("cpu"), 4, True)
    assert codec.rtn_quantize_and_pack_many([], num_bits=3) == []
    assert codec.rtn_wb_table_item(x, 32, 3) is None  # a CPU tensor is no table item


# ---- the gates ---------------------------------------------------------------------------------------------------------------------------
def test_both_gates_have_a_key_for_every_width_and_symmetry():
    from compressed_tensors_amd.compressors.pack_quantized import base

    keys = {(b, s) for b in C.BITS for s in (True, False)}
    for gate in (base.RTN_PACKW_MEASURED_FASTER, base.RTN_PACKW_TABLE_MEASURED_FASTER):
        assert set(gate) == keys and all(isinstance(v, bool) for v in gate.values())
    assert "compress_rtn_modules" in vars(base.PackedQuantizationCompressor) and "compress_rtn" in vars(base.PackedQuantizationCompressor)


def test_the_window_hook_asks_the_table_gate_per_scheme(monkeypatch):
    import compressed_tensors_amd as cta
    from compressed_tensors_amd.compressors.pack_quantized import base

    def info(bits, symmetric, **kw):
        scheme = cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(num_bits=bits, symmetric=symmetric, **kw))
        return base._rtn_scheme_info({}, scheme)

    monkeypatch.setattr(base, "RTN_PACKW_TABLE_MEASURED_FASTER", dict.fromkeys(base.RTN_PACKW_TABLE_MEASURED_FASTER, False))
    assert info(4, True, strategy="group", group_size=128) == (128, True, 4) and info(4, False, strategy="channel") == (None, False, 4)
    assert all(info(b, s, strategy="group", group_size=128) is None for b in C.BITS for s in (True, False))
    monkeypatch.setattr(base, "RTN_PACKW_TABLE_MEASURED_FASTER", {**dict.fromkeys(base.RTN_PACKW_TABLE_MEASURED_FASTER, False), (3, True): True, (6, False): True})
    assert info(3, True, strategy="group", group_size=64) == (64, True, 3) and info(6, False, strategy="channel") == (None, False, 6)
    assert info(3, False, strategy="group", group_size=64) is None and info(6, True, strategy="channel") is None
    assert info(8, True, strategy="group", group_size=128) is None and info(3, True, strategy="tensor") is None
    assert info(4, True, type="float", strategy="group", group_size=32) is None


# ---- PackQuantizedQuantizer: names only ----------------------------------------------------------------------------------------------------
NAMES = ("model.embed_tokens.weight", "model.layers.0.self_attn.q_proj.weight", "model.layers.0.mlp.down_proj.weight",
         "model.layers.0.input_layernorm.weight", "model.norm.weight", "lm_head.weight")


def test_quantizer_constructor_validate_dependencies_and_config():
    from compressed_tensors_amd.compressors.pack_quantized.base import PackedQuantizationCompressor
    from compressed_tensors_amd.entrypoints import convert
    from compressed_tensors_amd.entrypoints.convert import PackQuantizedQuantizer
    from compressed_tensors_amd.entrypoints.convert.converters import Converter

    assert "PackQuantizedQuantizer" in convert.__all__ and issubclass(PackQuantizedQuantizer, Converter)
    c = PackQuantizedQuantizer()
    assert (c.num_bits, c.group_size, c.symmetric, c.strategy) == (4, 128, True, "group")
    assert tuple(c.ignore) == ("lm_head", "re:.*embed_tokens$") and tuple(c.targets) == () and c.device is None
    assert PackQuantizedQuantizer(device="cuda:1").device == torch.device("cuda", 1)
    assert PackQuantizedQuantizer(3, 64, False, "channel").group_size is None
    with pytest.raises(TypeError):
        PackQuantizedQuantizer(4, 128, True, "group", (), (), "cuda:0")  # device is keyword-only
    for bad in (1, 8, 0, 9):
        with pytest.raises(ValueError, match="num_bits"):
            PackQuantizedQuantizer(bad)
    with pytest.raises(ValueError, match="strategies"):
        PackQuantizedQuantizer(strategy="tensor")
    with pytest.raises(ValueError, match="group_size"):
        PackQuantizedQuantizer(group_size=None)

    meta = torch.empty((4, 128), dtype=C.BF16, device="meta")
    names = dict.fromkeys(NAMES, meta)
    c.validate(names)  # names only: the values are meta tensors
    c.validate({k: None for k in names})
    c.validate(dict(names, **{"lm_head.weight_scale": None}))  # ignored modules may carry anything
    for partner in ("weight_scale", "weight_packed", "weight_shape", "weight_zero_point"):
        with pytest.raises(ValueError, match="q_proj"):
            c.validate(dict(names, **{f"model.layers.0.self_attn.q_proj.{partner}": None}))
    assert c._targeted(names) == ["model.layers.0.self_attn.q_proj", "model.layers.0.mlp.down_proj"]
    assert PackQuantizedQuantizer(targets=["re:.*q_proj$"])._targeted(names) == ["model.layers.0.self_attn.q_proj"]
    for name in names:
        assert c.get_dependencies(name) == set()
    untouched = {"model.norm.weight": torch.ones(8), "lm_head.weight": torch.ones((4, 64), dtype=C.BF16)}
    out = c.process(dict(untouched))  # nothing targeted: no device is asked for
    assert list(out) == list(untouched) and all(out[k] is untouched[k] for k in untouched)

    for bits, group, symmetric, strategy in ((4, 128, True, "group"), (4, 128, False, "group"), (3, 64, True, "group"), (6, 128, False, "channel")):
        q = PackQuantizedQuantizer(bits, group, symmetric, strategy, ignore=["lm_head"], targets=["re:.*proj$"])
        cfg = q.create_config().model_dump()
        assert cfg["quant_method"] == "compressed-tensors" and cfg["quantization_status"] == "compressed" and cfg["format"] == "pack-quantized"
        assert cfg["ignore"] == ["lm_head"] and list(cfg["config_groups"]) == ["config_group_0"]
        g = cfg["config_groups"]["config_group_0"]
        assert g["format"] == "pack-quantized" and g["targets"] == ["re:.*proj$"] and g["input_activations"] is None and g["output_activations"] is None
        w = g["weights"]
        assert (w["num_bits"], w["type"], w["strategy"], w["symmetric"], w["dynamic"], w["group_size"], w["zp_dtype"]) == \
            (bits, "int", strategy, symmetric, False, group if strategy == "group" else None, None if symmetric else "torch.int8")
        json.dumps(cfg)  # what write_checkpoint_quantization_config stores
        assert PackedQuantizationCompressor.can_compress(torch.nn.Linear, q._scheme())


def test_quantizer_config_is_the_references_preset():
    """the weights of create_config are the reference's W<n>A16 presets — and their asymmetric and channel-wise forms — as model_dump() writes them"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_import

    if not ref_import.available():
        pytest.skip("the reference sources are not on this machine")
    ref_import.import_reference()
    from compressed_tensors.quantization import QuantizationArgs
    from compressed_tensors.quantization.quant_scheme import PRESET_SCHEMES

    from compressed_tensors_amd.entrypoints.convert import PackQuantizedQuantizer

    def dumped(args):
        return {k: (str(v) if isinstance(v, torch.dtype) else getattr(v, "value", v)) for k, v in json.loads(args.model_dump_json()).items()}

    for bits in (2, 3, 4, 5, 6, 7):
        group = PackQuantizedQuantizer(bits).create_config().model_dump()["config_groups"]["config_group_0"]
        assert group["weights"] == dumped(PRESET_SCHEMES[f"W{bits}A16"]["weights"]) and group["input_activations"] is None, bits
    group = PackQuantizedQuantizer(4, symmetric=False).create_config().model_dump()["config_groups"]["config_group_0"]
    assert group["weights"] == dumped(PRESET_SCHEMES["W4A16_ASYM"]["weights"])
    group = PackQuantizedQuantizer(3, symmetric=False, strategy="channel").create_config().model_dump()["config_groups"]["config_group_0"]
    assert group["weights"] == dumped(QuantizationArgs(num_bits=3, type="int", symmetric=False, strategy="channel", dynamic=False))


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_fixture_inputs_and_oracle_composition_reproduce_the_fixture():
    """the recipes give the recorded inputs, and the oracle composition the GPU tests use (O.calculate_qparams_minmax, O.quantize, O.pack_to_int32) gives
    the reference's recorded scale, zero point, packed words and stored zero points for every case, width and symmetry, bit for bit; the fixture holds
    nothing else and fits the size limit"""
    from safetensors.torch import load_file

    stored = load_file(GOLDEN)
    assert os.path.getsize(GOLDEN) < (1 << 20)
    seen = set()
    for key, r in C.case_list():
        x = C.make_weight(r)
        assert x.dtype == C.DTYPES[r["dtype"]] and list(x.shape) == r["shape"] and bool(torch.isfinite(x.float()).all())
        assert torch.equal(C.bits_of(stored[f"{key}.x"]), C.bits_of(x)), key
        seen.add(f"{key}.x")
        for b in r["bits"]:
            for symmetric in (True, False):
                for name, t in C.oracle_outputs(O, x, r["group"], b, symmetric).items():
                    want = stored[f"{key}.{C.tag(b, symmetric)}.{name}"]
                    assert t.shape == want.shape and t.dtype == want.dtype, (key, b, symmetric, name)
                    assert torch.equal(C.bits_of(t.contiguous()), C.bits_of(want)), (key, b, symmetric, name)
                    seen.add(f"{key}.{C.tag(b, symmetric)}.{name}")
    assert seen == set(stored)


def test_the_cases_hold_what_they_are_there_for():
    cases = dict(C.case_list())
    assert {b for r in cases.values() for b in r["bits"]} == set(C.BITS)
    for b in C.BITS:
        for g, dtype in ((32, "bf16"), (128, "f16")):
            key = C.key_of((3, 3 * g), g, dtype, "planted", b)
            x = C.make_weight(cases[key])
            qmax = 2 ** (b - 1) - 1
            assert bool((x[0, :g] >= 0).all()) and not x[0, g:2 * g].any() and bool((x[0, 2 * g:] <= 0).all())
            assert bool((x[1, :g] < 0).any()) and float(x[1, :g].abs().max()) == 4.0
            assert torch.equal(C.bits_of(x[1, g + 4:g + 5]), C.bits_of(torch.tensor([-0.0], dtype=x.dtype)))
            # the symmetric group's scale is exactly 2^-7 and +-qmax * scale are in it; the asymmetric group's ends are qmin and qmax times 2^-7
            s, z = O.calculate_qparams_minmax(x, num_bits=b, group_size=g, symmetric=True)
            assert float(s[2, 0]) == 2.0 ** -7 and float(x[2, 5]) == qmax * 2.0 ** -7 and float(x[2, 9]) == -qmax * 2.0 ** -7
            s, z = O.calculate_qparams_minmax(x, num_bits=b, group_size=g, symmetric=False)
            assert float(s[2, 1]) == 2.0 ** -7 and int(z[2, 1]) == 0
            assert float(x[2, g:2 * g].min()) == -(qmax + 1) * 2.0 ** -7 and float(x[2, g:2 * g].max()) == qmax * 2.0 ** -7
            q = O.quantize(x, s, z, num_bits=b, strategy="group", group_size=g, dtype=torch.int8)
            assert int(q[2, g + 7]) == -(qmax + 1) and int(q[2, g + 11]) == qmax
    for dtype in ("bf16", "f16"):
        x = C.make_weight(cases[f"3x128.g32.{dtype}.extremes"])
        fi = torch.finfo(x.dtype)
        assert float(x[0].abs().min()) == fi.max and float(x[1].abs().max()) == fi.tiny and 0 < float(x[2].abs().max()) < fi.tiny
        x = C.make_weight(cases[f"2x256.g128.{dtype}.maxima"])
        assert float(x[0, 0]) == 3.0 and float(x[0, 255]) == -5.0 and float(x[1, 255]) == 7.0 and float(x.abs().flatten()[1:255].max()) < 1.0
    assert {tuple(r["shape"]) for r in cases.values() if r["fast"]} >= {(1, 32), (3, 96), (3, 384), (1, 8224), (1, 8320), (4, 512), (2, 2048), (3, 256), (2, 256), (3, 128)}
    assert {(tuple(r["shape"]), r["group"], r["dtype"]) for r in cases.values() if not r["fast"]} >= {((4, 64), 32, "f32"), ((2, 96), 48, "bf16"),
                                                                                                      ((1, 4096), 4096, "bf16"), ((2, 40), None, "bf16")}


def test_generator_check_mode_matches_the_reference():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_import

    if not ref_import.available():
        pytest.skip("the reference sources are not on this machine")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_packw_rtn.py"), "--check"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
