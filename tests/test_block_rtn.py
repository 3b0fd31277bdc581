"""Host side of block-wise 8-bit round-to-nearest (FP8_BLOCK from a dense model): the C ABI's three symbols, the planner of the table form
(ct_rtn_block8_batch_plan) and its named refusals, FP8BlockQuantizer's name-only methods, and the fixtures of tests/golden/block_rtn.* against the
pinned oracle and, where the reference sources exist, against the reference itself.  No GPU: the planner is a host function."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import _block_rtn_cases as C
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("ct_rtn_quant_block8", "ct_rtn_block8_batch_plan", "ct_rtn_quant_block8_batch")


@pytest.fixture(scope="module")
def lib():
    from compressed_tensors_amd import _lib

    return _lib.load()


def group_of(block):
    return -((block[0] << 24) | block[1])


def table(items):
    """a host table of (rows, cols, block) with made-up, aligned addresses: the planner looks at pointers, it never follows them"""
    from compressed_tensors_amd import _lib

    tab = (_lib.W4Item * max(len(items), 1))()
    for i, (rows, cols, block) in enumerate(items):
        it, base = tab[i], 0x100000 * (i + 1)
        it.src, it.dst, it.scale, it.zp = base, base + 0x80000, base + 0xC0000, base + 0xE0000
        it.rows, it.cols, it.group = rows, cols, group_of(block)
    return tab


def plan(lib, tab, n=None):
    return int(lib.ct_rtn_block8_batch_plan(ctypes.cast(tab, ctypes.c_void_p), len(tab) if n is None else n))


FAST_ITEMS = [(shape[0], shape[1], block) for shape, block, _ in C.FAST]


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_prototyped(lib):
    from compressed_tensors_amd import _lib, codec

    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ct_hip.h")).read(), flags=re.S)
    header = re.sub(r"\s+", " ", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NEW:
        assert name in exported and name in _lib._PROTOTYPES and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert ("int ct_rtn_quant_block8(const void* x, int xdt, int64_t rows, int64_t cols, int64_t block_h, int64_t block_w, int fp8, int symmetric, "
            "void* out, void* scale_out, int8_t* zp_out, ct_stream_t stream);") in header
    assert "int64_t ct_rtn_block8_batch_plan(ct_w4_item* items_host, int n);" in header
    assert ("int ct_rtn_quant_block8_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int xdt, int fp8, int symmetric, "
            "ct_stream_t stream);") in header
    assert [len(_lib._PROTOTYPES[name][0]) for name in NEW] == [12, 2, 7]
    assert lib.ct_abi_version() == 2 and ctypes.sizeof(_lib.W4Item) == 13 * 8  # additive: nothing an existing caller sees moved
    for name in ("rtn_quantize_block8", "rtn_quantize_block8_many", "rtn_block8_table_item"):
        assert callable(getattr(codec, name)) and name in codec.__all__
    assert codec._TABLES["rtn_block8"] == ("ct_rtn_block8_batch_plan", False, "ct_rtn_quant_block8_batch")
    assert codec.launch_rtn_block8_words(None, 0, None, torch.device("cpu"), True, True) is None  # an empty table: nothing is touched


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def test_plan_counts_one_workgroup_per_block_and_fills_the_derived_fields(lib):
    tab = table(FAST_ITEMS)
    want = [-(-rows // b[0]) * (cols // b[1]) for rows, cols, b in FAST_ITEMS]
    assert want == [1, 6, 2, 4, 9, 6, 16] and plan(lib, tab) == sum(want)
    first = 0
    for it, (rows, cols, b), blocks in zip(tab, FAST_ITEMS, want):
        assert it.first_block == first and it.units == rows * cols // 8, (rows, cols, b)
        assert it.upg == b[1] // 8 and 1 << it.upg_shift == it.upg and 1 << (it.main_blocks - 1) == b[0]
        G = cols // b[1]
        for n in (0, 1, G - 1, G, blocks - 1, 12345, (1 << 31) - 1):  # the multiply-high is the division by the blocks per row of blocks
            assert (n * it.g_magic) >> it.g_shift == n // G
        first += blocks
    assert plan(lib, table([(8192, 8192, (128, 128))])) == 4096
    assert plan(lib, table(FAST_ITEMS), 0) == 0
    one = table([(100, 256, (128, 128))])
    one[0].dst = None  # the observer form: no codes
    assert plan(lib, one) == 2


@pytest.mark.parametrize("what,names", [("ragged_cols", "ragged columns"), ("bw8", "at least 16"), ("bh96", "powers of two"), ("bw96", "powers of two"),
                                        ("too_large", "16384"), ("misaligned_src", "misaligned"), ("misaligned_dst", "misaligned"),
                                        ("no_scale", "scale output"), ("no_rows", "empty"), ("group128", "must encode a block")])
def test_plan_refuses_and_names_the_reason(lib, what, names):
    from compressed_tensors_amd import _lib

    items = [(128, 128, (128, 128)), (256, 256, (128, 128)), (64, 64, (64, 64))]
    change = dict(ragged_cols=(256, 200, (128, 128)), bw8=(256, 256, (128, 8)), bh96=(192, 256, (96, 128)), bw96=(256, 192, (128, 96)),
                  too_large=(256, 256, (256, 128)), no_rows=(0, 256, (128, 128)))
    if what in change:
        items[1] = change[what]
    tab = table(items)
    if what == "misaligned_src":
        tab[1].src += 8
    elif what == "misaligned_dst":
        tab[1].dst += 4
    elif what == "no_scale":
        tab[1].scale = None
    elif what == "group128":
        tab[1].group = 128
    assert plan(lib, tab) == -1
    msg = _lib.last_error()
    assert "ct_rtn_block8_batch_plan" in msg and "item 1" in msg and names in msg, msg


def test_plan_refuses_bad_arguments_and_two_to_the_31_workgroups(lib):
    from compressed_tensors_amd import _lib

    assert plan(lib, table(FAST_ITEMS), -1) == -1 and "bad arguments" in _lib.last_error()
    assert int(lib.ct_rtn_block8_batch_plan(None, 1)) == -1 and "bad arguments" in _lib.last_error()
    assert plan(lib, table([(1 << 20, 1 << 17, (1, 128))] * 2)) == -1 and "exceed one launch" in _lib.last_error()
    assert plan(lib, table([(1 << 24, 1 << 20, (1, 16))])) == -1 and "2^31 blocks" in _lib.last_error()


def test_codec_group_rule_is_the_plans(lib):
    """`codec.rtn_block8_group` and `quantization.utils.block_one_pass` decide in Python what the plan decides in the library"""
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.quantization.utils import block_one_pass

    cases = FAST_ITEMS + [(256, 200, (128, 128)), (130, 136, (128, 128)), (256, 256, (128, 8)), (192, 256, (96, 128)), (256, 256, (256, 128)),
                          (256, 256, (1, 16384)), (256, 256, (2, 16384)), (64, 32, (16, 16))]
    for rows, cols, b in cases:
        took = plan(lib, table([(rows, cols, b)])) >= 0
        assert bool(codec.rtn_block8_group((rows, cols), b)) == took, (rows, cols, b)
        assert not took or codec.rtn_block8_group((rows, cols), b) == group_of(b)
        for dtype, ok in ((C.BF16, True), (C.F16, True), (C.F32, False)):
            w = torch.empty((rows, cols), dtype=dtype, device="meta")
            args = cta.QuantizationArgs(num_bits=8, type="float", strategy="block", block_structure=list(b))
            assert block_one_pass(w, args) == (took and ok)
    w = torch.empty((128, 128), dtype=C.BF16, device="meta")
    assert not block_one_pass(w, cta.QuantizationArgs(num_bits=4, strategy="block", block_structure=[128, 128]))
    assert block_one_pass(w, cta.QuantizationArgs(num_bits=8, strategy="block", block_structure=[128, 128], symmetric=False))


def test_block_qparams_and_compress_rtn_no_longer_refuse_the_strategy():
    """the block branch exists: without a GPU it ends at the device check, not at NotImplementedError("strategy 'block' not supported")"""
    import compressed_tensors_amd as cta
    from compressed_tensors_amd.compressors.naive_quantized.base import NaiveQuantizationCompressor, rtn_block8_windows
    from compressed_tensors_amd.quantization.utils import _block_rows

    x = C.make_weight(dict(shape=[130, 136], block=[128, 128], dtype="bf16", special=None, salt=3))
    rows, grid = _block_rows(x, [128, 128])
    want, want_grid = C.block_rows(x, [128, 128])
    assert grid == want_grid == (2, 2) and torch.equal(C.bits(rows), C.bits(want))
    assert NaiveQuantizationCompressor.RTN_TABLE_MEASURED_FASTER is False and callable(rtn_block8_windows)
    assert "block" in cta.ModelCompressor.compress_model_rtn.__doc__


# ---- FP8BlockQuantizer: names only ----------------------------------------------------------------------------------------------------
def test_quantizer_constructor_validate_dependencies_and_config():
    from compressed_tensors_amd.entrypoints import convert
    from compressed_tensors_amd.entrypoints.convert import FP8BlockQuantizer
    from compressed_tensors_amd.entrypoints.convert.converters import Converter

    assert "FP8BlockQuantizer" in convert.__all__ and issubclass(FP8BlockQuantizer, Converter)
    c = FP8BlockQuantizer()
    assert tuple(c.ignore) == ("lm_head", "re:.*embed_tokens$") and tuple(c.targets) == () and tuple(c.weight_block_size) == (128, 128) and c.device is None
    assert FP8BlockQuantizer(device="cuda:1").device == torch.device("cuda", 1)
    with pytest.raises(TypeError):
        FP8BlockQuantizer((), (), (128, 128), "cuda:0")  # device is keyword-only
    for block in ((128,), (128, 0), "128x128", (128.0, 128)):
        with pytest.raises(ValueError):
            FP8BlockQuantizer(weight_block_size=block)

    names = {"model.embed_tokens.weight": None, "model.layers.0.self_attn.q_proj.weight": None, "model.layers.0.mlp.down_proj.weight": None,
             "model.layers.0.input_layernorm.weight": None, "model.norm.weight": None, "lm_head.weight": None}
    c.validate(names)  # names only: the values are None
    c.validate(dict(names, **{"lm_head.weight_scale": None}))  # ignored modules may carry anything
    for partner in ("weight_scale", "weight_scale_inv", "weight_packed"):
        with pytest.raises(ValueError, match="q_proj"):
            c.validate(dict(names, **{f"model.layers.0.self_attn.q_proj.{partner}": None}))
    assert c._targeted(names) == ["model.layers.0.self_attn.q_proj", "model.layers.0.mlp.down_proj"]
    assert FP8BlockQuantizer(targets=["re:.*q_proj$"])._targeted(names) == ["model.layers.0.self_attn.q_proj"]
    for name in names:
        assert c.get_dependencies(name) == set()

    cfg = FP8BlockQuantizer(ignore=["lm_head"], targets=["re:.*proj$"], weight_block_size=(64, 128)).create_config().model_dump()
    assert cfg["quant_method"] == "compressed-tensors" and cfg["quantization_status"] == "compressed" and cfg["format"] == "float-quantized"
    assert cfg["ignore"] == ["lm_head"] and list(cfg["config_groups"]) == ["config_group_0"]
    group = cfg["config_groups"]["config_group_0"]
    assert group["format"] == "float-quantized" and group["targets"] == ["re:.*proj$"] and group["output_activations"] is None
    w, a = group["weights"], group["input_activations"]
    assert (w["num_bits"], w["type"], w["strategy"], w["symmetric"], w["dynamic"], w["block_structure"], w["group_size"]) == (8, "float", "block", True, False, [64, 128], None)
    assert (a["num_bits"], a["type"], a["strategy"], a["symmetric"], a["dynamic"], a["block_structure"], a["group_size"]) == (8, "float", "group", True, True, None, 128)
    json.dumps(cfg)  # what write_checkpoint_quantization_config stores


def test_quantizer_config_is_the_references_preset():
    """the weights and input activations of create_config are the reference's FP8_BLOCK preset as its model_dump() writes it"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_import

    if not ref_import.available():
        pytest.skip("the reference sources are not on this machine")
    ref_import.import_reference()
    from compressed_tensors.quantization.quant_scheme import FP8_BLOCK

    from compressed_tensors_amd.entrypoints.convert import FP8BlockQuantizer

    group = FP8BlockQuantizer().create_config().model_dump()["config_groups"]["config_group_0"]
    for key, args in (("weights", FP8_BLOCK["weights"]), ("input_activations", FP8_BLOCK["input_activations"])):
        want = {k: (str(v) if isinstance(v, torch.dtype) else getattr(v, "value", v)) for k, v in args.model_dump().items()}
        assert group[key] == want, key


# ---- the fixtures --------------------------------------------------------------------------------------------------------------------
def test_golden_inputs_and_oracle_recipe_reproduce_the_fixture():
    """the seeded inputs hash to the manifest, and the oracle recipe the GPU tests use gives the reference's recorded scale, zero point and codes
    bit for bit — every case and kind, the float32 one and the planted zero / negative-zero blocks included"""
    from safetensors.torch import load_file

    stored = load_file(os.path.join(GOLDEN, "block_rtn.safetensors"))
    manifest = json.load(open(os.path.join(GOLDEN, "block_rtn_manifest.json")))["cases"]
    assert list(manifest) == sorted(k for k, _ in C.case_list()) and os.path.getsize(os.path.join(GOLDEN, "block_rtn.safetensors")) < 400 << 10
    for key, r in C.case_list():
        x = C.make_weight(r)
        assert C.sha(x) == manifest[key]["x_sha256"] and manifest[key]["recipe"] == r, key
        for kind in C.KINDS:
            for name, t in zip(("scale", "zero_point", "q"), C.oracle_triple(O, x, r["block"], kind)):
                m = manifest[key]["out"][f"{kind}.{name}"]
                assert (str(t.dtype).replace("torch.", ""), list(t.shape), C.sha(t)) == (m["dtype"], m["shape"], m["sha256"]), (key, kind, name)
                full = stored.get(f"{key}.{kind}.{name}")
                assert (full is not None) == (name != "q" or C.stores_codes(r, kind)), (key, kind, name)
                if full is not None:
                    assert torch.equal(C.bits(full), C.bits(t)), (key, kind, name)
    q = C.oracle_triple(O, C.make_weight(dict(C.case_list()[2][1])), [128, 128], "fp8")[2].view(torch.uint8)
    # the planted block: tiny negatives become -0.0 codes in the cast, the -0.0 element met the zero-point add first and is +0.0; the zero block is +0.0
    assert C.case_list()[2][1]["special"] == "planted" and int(q[128 + 4, 7]) == 0x00 and int(q[128 + 5, 7]) == 0x80 and int(q[128 + 3, 5]) == 0x7E
    assert int((q[128:, :128] == 0x80).sum()) == 128 * 128 - 2 and not bool(q[:128, 128:256].any())


def test_golden_regenerates_to_the_committed_bytes():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_import

    if not ref_import.available():
        pytest.skip("the reference sources are not on this machine")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_block_rtn.py"), "--check"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
