"""Host side of channel-wise 8-bit round-to-nearest (FP8_DYNAMIC and W8A8 from a dense model): the C ABI's two new symbols and the widened bound of
ct_rtn_quant_channel8, the planner of the table form (ct_rtn_channel8_batch_plan) and its named refusals, the Python form of its rule, the name-only
methods of FP8DynamicQuantizer / W8A8Quantizer, and the fixture tests/golden/channel8_rtn.safetensors against the pinned oracle and, where the
reference sources exist, against the reference itself.  No GPU: the planner is a host function."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import _channel8_rtn_cases as C
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "channel8_rtn.safetensors")
MANIFEST = os.path.join(ROOT, "tests", "golden", "channel8_rtn_manifest.json")
NEW = ("ct_rtn_channel8_batch_plan", "ct_rtn_quant_channel8_batch")
FORM_CODE = {"wave": 0, "row": 1, "long": 2}
CASES = dict(C.case_list())


@pytest.fixture(scope="module")
def lib():
    from compressed_tensors_amd import _lib

    return _lib.load()


def table(items):
    """a host table of (rows, cols, symmetric) with made-up, aligned addresses: the planner looks at pointers, it never follows them.  An item
    with a zero-point output is an asymmetric one."""
    from compressed_tensors_amd import _lib

    tab = (_lib.W4Item * max(len(items), 1))()
    for i, (rows, cols, symmetric) in enumerate(items):
        it, base = tab[i], 0x100000 * (i + 1)
        it.src, it.dst, it.scale, it.zp = base, base + 0x80000, base + 0xC0000, None if symmetric else base + 0xE0000
        it.rows, it.cols = rows, cols
    return tab


def plan(lib, tab, n=None):
    return int(lib.ct_rtn_channel8_batch_plan(ctypes.cast(tab, ctypes.c_void_p), len(tab) if n is None else n))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_prototyped(lib):
    from compressed_tensors_amd import _lib, codec

    text = open(os.path.join(ROOT, "include", "ct_hip.h")).read()
    assert "#define CT_RTN_CHANNEL8_MAX_COLS 65536" in text and "cols <= CT_RTN_CHANNEL8_MAX_COLS" in text
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NEW:
        assert name in exported and name in _lib._PROTOTYPES and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "int64_t ct_rtn_channel8_batch_plan(ct_w4_item* items_host, int n);" in header
    assert ("int ct_rtn_quant_channel8_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int xdt, int fp8, int symmetric, "
            "ct_stream_t stream);") in header
    assert [len(_lib._PROTOTYPES[name][0]) for name in NEW] == [2, 7]
    assert _lib._PROTOTYPES["ct_rtn_quant_channel8_batch"] == _lib._PROTOTYPES["ct_rtn_quant_block8_batch"]
    assert lib.ct_abi_version() == 2 and ctypes.sizeof(_lib.W4Item) == 13 * 8  # additive: nothing an existing caller sees moved
    declared = set(re.findall(r"\b(ct_\w+)\s*\(", header))
    assert set(NEW) <= declared and declared <= exported  # the library exports what the header declares
    for name in ("rtn_quantize_channel8", "rtn_quantize_channel8_many", "rtn_channel8_table_item", "rtn_channel8_form", "launch_rtn_channel8_words"):
        assert callable(getattr(codec, name)) and name in codec.__all__
    assert codec.RTN_CHANNEL8_MAX_COLS == C.MAX_COLS == 65536
    assert codec._TABLES["rtn_channel8"] == ("ct_rtn_channel8_batch_plan", False, "ct_rtn_quant_channel8_batch")
    assert codec.launch_rtn_channel8_words(None, 0, None, torch.device("cpu"), True, True) is None  # an empty table: nothing is touched


def test_launch_entries_refuse_by_name(lib):
    """the dtype belongs to the launch, not to the plan; the single launch names its bound: refused before anything touches a GPU"""
    from compressed_tensors_amd import _lib

    a = 0x100000
    assert lib.ct_rtn_quant_channel8_batch(a, 1, 1, _lib.F32, 1, 1, None) == _lib.CT_ERR_INVALID_ARG and "16-bit weights only" in _lib.last_error()
    assert lib.ct_rtn_quant_channel8_batch(a, 1, 1, _lib.BF16, 1, 0, None) == _lib.CT_ERR_INVALID_ARG and "symmetric" in _lib.last_error()
    assert lib.ct_rtn_quant_channel8_batch(a, 1, 1 << 31, _lib.BF16, 1, 1, None) == _lib.CT_ERR_INVALID_ARG and "bad batch size" in _lib.last_error()
    assert lib.ct_rtn_quant_channel8(a, _lib.BF16, 1, C.MAX_COLS + 8, 1, 1, a, a, None, None) == _lib.CT_ERR_INVALID_ARG
    assert "CT_RTN_CHANNEL8_MAX_COLS = 65536" in _lib.last_error()
    assert lib.ct_rtn_quant_channel8(a, _lib.BF16, 2, 100, 1, 1, a, a, None, None) == _lib.CT_ERR_INVALID_ARG and "multiple of 8" in _lib.last_error()
    with pytest.raises(NotImplementedError, match="cols <= 65536"):
        __import__("compressed_tensors_amd").codec.rtn_quantize_channel8(torch.zeros((1, C.MAX_COLS + 8), dtype=C.BF16))


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [True, False])
def test_plan_counts_workgroups_per_form_and_fills_the_derived_fields(lib, symmetric):
    """ceil(rows / 4) workgroups in the wave form (four rows per workgroup), rows in the workgroup and long forms; the form in upg_shift, the units per
    row in upg"""
    from compressed_tensors_amd import codec

    items = [(shape[0], shape[1], symmetric) for shape, _ in C.FAST] + [(7, 2048, symmetric), (9, 8192, symmetric), (3, 16392, symmetric)]
    forms = [codec.rtn_channel8_form((rows, cols), symmetric) for rows, cols, _ in items]
    want = [-(-rows // 4) if form == "wave" else rows for (rows, _, _), form in zip(items, forms)]
    by_shape = dict(zip([(r, c) for r, c, _ in items], zip(forms, want)))
    assert by_shape[(1, 8)] == ("wave", 1) and by_shape[(5, 512)] == ("wave", 2) and by_shape[(2, 2048)] == ("wave", 1) and by_shape[(7, 2048)] == ("wave", 2)
    assert by_shape[(2, 2056)] == (("row", 2) if symmetric else ("wave", 1)) and by_shape[(1, 8192)] == (("row", 1) if symmetric else ("wave", 1))
    assert by_shape[(9, 8192)] == (("row", 9) if symmetric else ("wave", 3)) and by_shape[(1, 8200)] == ("row", 1) and by_shape[(1, 16384)] == ("row", 1)
    assert by_shape[(1, 16392)] == ("long", 1) and by_shape[(3, 16392)] == ("long", 3) and by_shape[(1, 29568)] == ("long", 1) and by_shape[(1, 65536)] == ("long", 1)
    tab = table(items)
    assert plan(lib, tab) == sum(want)
    first = 0
    for it, (rows, cols, _), form, blocks in zip(tab, items, forms, want):
        assert it.first_block == first and it.units == rows * cols // 8 and it.main_blocks == blocks, (rows, cols)
        assert it.upg == cols // 8 and it.upg_shift == FORM_CODE[form] and it.g_magic == 0 and it.g_shift == 0, (rows, cols, form)
        first += blocks
    assert plan(lib, table(items), 0) == 0
    assert plan(lib, table([(1 << 20, 4096, symmetric)])) == ((1 << 20) if symmetric else (1 << 18))


@pytest.mark.parametrize("what,names", [("no_rows", "empty"), ("no_cols", "empty"), ("cols100", "multiple of 8"), ("too_wide", "CT_RTN_CHANNEL8_MAX_COLS = 65536"),
                                        ("misaligned_src", "misaligned"), ("misaligned_dst", "misaligned"), ("no_src", "are required"),
                                        ("no_dst", "are required"), ("no_scale", "are required"), ("too_many", "2^31 workgroups")])
def test_plan_refuses_and_names_the_reason(lib, what, names):
    from compressed_tensors_amd import _lib

    items = [(4, 128, True), (8, 256, True), (2, 32768, True)]
    change = dict(no_rows=(0, 256, True), no_cols=(8, 0, True), cols100=(2, 100, True), too_wide=(1, C.MAX_COLS + 8, True), too_many=(1 << 31, 4096, True))
    if what in change:
        items[1] = change[what]
    tab = table(items)
    if what == "misaligned_src":
        tab[1].src += 8
    elif what == "misaligned_dst":
        tab[1].dst += 8
    elif what == "no_src":
        tab[1].src = None
    elif what == "no_dst":
        tab[1].dst = None
    elif what == "no_scale":
        tab[1].scale = None
    assert plan(lib, tab) == -1
    msg = _lib.last_error()
    assert "ct_rtn_channel8_batch_plan" in msg and "item 1" in msg and names in msg, msg


def test_plan_refuses_bad_arguments_and_two_to_the_31_workgroups(lib):
    from compressed_tensors_amd import _lib

    assert plan(lib, table([(4, 128, True)]), -1) == -1 and "bad arguments" in _lib.last_error()
    assert int(lib.ct_rtn_channel8_batch_plan(None, 1)) == -1 and "bad arguments" in _lib.last_error()
    assert plan(lib, table([(1 << 30, 4096, True)] * 2)) == -1 and "exceed one launch" in _lib.last_error()


def test_python_form_agrees_with_the_plan_on_every_case_and_around_every_boundary(lib):
    from compressed_tensors_amd import codec

    shapes = [tuple(r["shape"]) for r in CASES.values()]
    shapes += [(3, c) for c in (8, 2048, 2056, 8192, 8200, 16384, 16392, C.MAX_COLS, C.MAX_COLS + 8, 100, 0)] + [(0, 64)]
    for shape in shapes:
        for symmetric in (True, False):
            form = codec.rtn_channel8_form(shape, symmetric)
            tab = table([(shape[0], shape[1], symmetric)])
            blocks = plan(lib, tab)
            assert (blocks == -1) == (form == ""), (shape, symmetric, form, blocks)
            if form:
                assert tab[0].upg_shift == FORM_CODE[form], (shape, symmetric, form)
    f = codec.rtn_channel8_form
    assert (f((3, 2048), True), f((3, 2056), True)) == ("wave", "row") and (f((3, 8192), False), f((3, 8200), False)) == ("wave", "row")
    assert (f((3, 16384), True), f((3, 16392), True), f((3, 16384), False), f((3, 16392), False)) == ("row", "long", "row", "long")
    assert (f((3, C.MAX_COLS), True), f((3, C.MAX_COLS + 8), True), f((3, C.MAX_COLS), False), f((3, C.MAX_COLS + 8), False)) == ("long", "", "long", "")
    assert f((4, 64, 2), True) == "" and f((64,), True) == ""
    for key, r in CASES.items():  # the case matrix: what is fast has a form, what falls back has none or is float32
        assert bool(f(r["shape"], True)) == (r["fast"] or r["dtype"] == "f32"), key


# ---- the converters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fmt,qtype", [("FP8DynamicQuantizer", "float-quantized", "float"), ("W8A8Quantizer", "int-quantized", "int")])
def test_quantizer_name_only_methods_and_config(name, fmt, qtype):
    from compressed_tensors_amd.entrypoints import convert

    cls = getattr(convert, name)
    assert name in convert.__all__
    c = cls()
    assert tuple(c.ignore) == ("lm_head", "re:.*embed_tokens$") and tuple(c.targets) == () and c.device is None
    names = {"model.embed_tokens.weight": None, "model.layers.0.mlp.down_proj.weight": None, "model.norm.weight": None, "lm_head.weight": None}
    c.validate(names)
    assert c._targeted(names) == ["model.layers.0.mlp.down_proj"]
    with pytest.raises(ValueError, match="quantized already"):
        c.validate(dict(names, **{"model.layers.0.mlp.down_proj.weight_scale": None}))
    assert c.get_dependencies("model.layers.0.mlp.down_proj.weight") == set()
    untouched = {"model.norm.weight": torch.ones(8), "lm_head.weight": torch.ones((4, 64), dtype=C.BF16)}
    out = c.process(dict(untouched))  # nothing targeted: no device is asked for
    assert list(out) == list(untouched) and all(out[k] is untouched[k] for k in untouched)

    cfg = cls(ignore=["lm_head"], targets=["re:.*proj$"]).create_config().model_dump()
    assert cfg["quant_method"] == "compressed-tensors" and cfg["quantization_status"] == "compressed" and cfg["format"] == fmt
    assert cfg["ignore"] == ["lm_head"] and list(cfg["config_groups"]) == ["config_group_0"]
    group = cfg["config_groups"]["config_group_0"]
    assert group["format"] == fmt and group["targets"] == ["re:.*proj$"] and group["output_activations"] is None
    assert group["weights"]["type"] == qtype and group["weights"]["strategy"] == "channel" and group["weights"]["dynamic"] is False
    assert group["input_activations"]["type"] == qtype and group["input_activations"]["strategy"] == "token" and group["input_activations"]["dynamic"] is True
    assert cls().create_config().model_dump()["config_groups"]["config_group_0"]["targets"] == ["Linear"]
    scheme = c._scheme()  # the scheme the fallback compresses under is the preset, and its codec is the format's
    import compressed_tensors_amd as cta

    assert c._compressor() is cta.BaseCompressor.get_value_from_registry(fmt) and c._compressor().can_compress(torch.nn.Linear, scheme)
    assert scheme.weights.symmetric and str(getattr(scheme.weights.strategy, "value", scheme.weights.strategy)) == "channel"


@pytest.mark.parametrize("name,preset", [("FP8DynamicQuantizer", "FP8_DYNAMIC"), ("W8A8Quantizer", "INT8_W8A8")])
def test_quantizer_config_is_the_references_preset(name, preset):
    """the weights and input activations of create_config are the reference's preset as its model_dump() writes it"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_import

    if not ref_import.available():
        pytest.skip("the reference sources are not on this machine")
    ref_import.import_reference()
    from compressed_tensors.quantization import quant_scheme

    from compressed_tensors_amd.entrypoints import convert

    want_preset = getattr(quant_scheme, preset)
    group = getattr(convert, name)().create_config().model_dump()["config_groups"]["config_group_0"]
    for key in ("weights", "input_activations"):
        want = {k: (str(v) if isinstance(v, torch.dtype) else getattr(v, "value", v)) for k, v in want_preset[key].model_dump().items()}
        assert group[key] == want, key


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_fixture_holds_every_stored_case_and_equals_the_oracle():
    from safetensors.torch import load_file

    golden = load_file(GOLDEN)
    manifest = json.load(open(MANIFEST))
    assert os.path.getsize(GOLDEN) < (1 << 20)
    assert list(manifest) == sorted(CASES) and len(CASES) == 2 * len(C.FAST) + len(C.FALLBACK)
    expected = set()
    for key, r in CASES.items():
        x = C.make_weight(r)
        assert manifest[key]["x_sha256"] == C.sha(x) and manifest[key]["shape"] == r["shape"] and manifest[key]["stored"] == r["stored"], key
        if not r["stored"]:
            assert not any(k.startswith(key + ".") for k in golden), key
            continue
        if C.x_stored(r):
            expected.add(f"{key}.x")
            assert torch.equal(C.bits(golden[f"{key}.x"]), C.bits(x)), key
        for kind in C.KINDS:
            for name, t in C.oracle_outputs(O, x, kind).items():
                expected.add(f"{key}.{kind}.{name}")
                g = golden[f"{key}.{kind}.{name}"]
                assert g.shape == t.shape and torch.equal(C.bits(g), C.bits(t.contiguous())), (key, kind, name)
    assert set(golden) == expected
    not_stored = {tuple(r["shape"]) for r in CASES.values() if not r["stored"]}
    assert not_stored == {(1, 16384), (1, C.MAX_COLS), (1, C.MAX_COLS + 8)}


def test_long_rows_carry_their_extremes_at_the_ends():
    """every row beyond 16384 columns has its maximum in its last unit and its minimum in its first; the specials are where the matrix says"""
    for key, r in CASES.items():
        x = C.make_weight(r).float()
        if r["shape"][1] > 16384:
            assert int(x[0].argmax()) == r["shape"][1] - 1 and int(x[0].argmin()) == 0 and int(x[0].abs().argmax()) == r["shape"][1] - 1, key
    x = C.make_weight(CASES["5x512.bf16"])
    assert not x[0].any() and bool((x[1] > 0).all()) and bool(torch.signbit(x[2, 9])) and x[2, 9] == 0 and x[2, 5] == 3.5
    assert bool((x[3].float().abs() == torch.finfo(C.BF16).max).all()) and bool((x[4].float().abs() == torch.finfo(C.BF16).tiny).all())
    sub = C.make_weight(CASES["2x1032.f16"])[0].float().abs()
    assert bool((sub == torch.finfo(C.F16).tiny / 4).all())


def test_generator_check_mode_matches_the_reference():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_import

    if not ref_import.available():
        pytest.skip("the reference sources are not on this machine")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_channel8_rtn.py"), "--check"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
