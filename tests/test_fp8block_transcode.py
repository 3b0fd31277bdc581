"""FP8BlockToMXFP8Converter, FP8BlockToNVFP4Converter and the C planners of `ct_fp8block_mxfp8_batch` / `ct_fp8block_nvfp4_batch` (CPU tests: the ABI,
the plans through ctypes, the converters' host logic on name-only dicts, the refusals that must come before any device is touched, the fixture).  The
GPU half is tests/test_gpu_fp8block_transcode.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import _fp8block_transcode_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = {"mxfp8": "ct_fp8block_mxfp8_plan", "nvfp4": "ct_fp8block_nvfp4_plan"}
LAUNCHES = {"mxfp8": ("ct_fp8block_mxfp8_batch",), "nvfp4": ("ct_fp8block_nvfp4_amax_batch", "ct_fp8block_nvfp4_batch")}
DEFINE = {"mxfp8": "CT_FP8BLOCK_MXFP8_GROUPS_PER_BLOCK", "nvfp4": "CT_FP8BLOCK_NV_GROUPS_PER_BLOCK"}
TARGETS = pytest.mark.parametrize("target", C.TARGETS)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    from compressed_tensors_amd import _lib

    return _lib


def _item_type(target):
    from compressed_tensors_amd import _lib

    return _lib.Fp8BlockMxItem if target == "mxfp8" else _lib.Fp8BlockNvItem


def _item(target, rows, cols, block=(128, 128), scale_shape=None, sdt=None, base=0x100000):
    from compressed_tensors_amd import _lib

    it = _item_type(target)()
    it.w, it.scale, it.packed = base, base + 0x1000, base + 0x2000
    if target == "mxfp8":
        it.e8m0 = base + 0x3000
    else:
        it.scale_f8, it.key, it.global_scale = base + 0x3000, base + 0x4000, base + 0x4004
    it.rows, it.cols, it.block_h, it.block_w = rows, cols, block[0], block[1]
    it.scale_shape[0], it.scale_shape[1] = scale_shape or (-(-rows // max(block[0], 1)), -(-cols // max(block[1], 1)))
    it.sdt = _lib.F32 if sdt is None else sdt
    it.reserved, it.units_per_row, it.units, it.first_block = -7, -7, -7, -7  # the plan writes every derived field of an admitted item
    return it


def _plan(target, items, n=None):
    from compressed_tensors_amd import _lib

    table = (_item_type(target) * max(len(items), 1))(*items)
    return int(getattr(_lib.load(), PLAN[target])(ctypes.cast(table, ctypes.c_void_p), len(items) if n is None else n)), table


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_the_new_symbols_are_declared_prototyped_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "ct_hip.h")).read()
    for line in ("int64_t ct_fp8block_mxfp8_plan(ct_fp8block_mx_item* items_host, int n);",
                 "int ct_fp8block_mxfp8_batch(const ct_fp8block_mx_item* items_dev, int n, int64_t total_blocks, int xdt, const uint8_t* code_table, ct_stream_t stream);",
                 "int64_t ct_fp8block_nvfp4_plan(ct_fp8block_nv_item* items_host, int n);",
                 "int ct_fp8block_nvfp4_amax_batch(const ct_fp8block_nv_item* items_dev, int n, int64_t total_blocks, int xdt, ct_stream_t stream);",
                 "int ct_fp8block_nvfp4_batch(const ct_fp8block_nv_item* items_dev, int n, int64_t total_blocks, int xdt, ct_stream_t stream);"):
        assert line in header, line
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in (*PLAN.values(), *LAUNCHES["mxfp8"], *LAUNCHES["nvfp4"]):
        assert re.search(rf"\bT {name}\b", exported), name
        assert name in lib._PROTOTYPES and name in lib.EXPORTED_SYMBOLS and hasattr(lib.load(), name)
    words = int(re.search(r"\} ct_fp8block_nv_item;\s*/\* (\d+) 64-bit words \*/", header).group(1))
    assert ctypes.sizeof(lib.Fp8BlockNvItem) == 8 * words == 144
    assert lib.Fp8BlockNvItem.key.offset == 32 and lib.Fp8BlockNvItem.sdt.offset == 96 and lib.Fp8BlockNvItem.first_block.offset == 136
    assert ctypes.sizeof(lib.Fp8BlockMxItem) == 128  # the MXFP8 table reuses the MXFP4 row, unchanged
    # the workgroups' shares: the header, the binding and the case matrix (whose share_m1 / share_p1 shapes are derived from them) agree
    binding = {"mxfp8": lib.FP8BLOCK_MXFP8_GROUPS_PER_BLOCK, "nvfp4": lib.FP8BLOCK_NV_GROUPS_PER_BLOCK}
    for t in C.TARGETS:
        assert int(re.search(rf"#define {DEFINE[t]} (\d+)", header).group(1)) == binding[t] == C.GROUPS_PER_BLOCK[t], t
        for tag, n in (("m1", binding[t] - 1), ("p1", binding[t] + 1)):
            c = C.CASES[f"share_{tag}.{t}"]
            assert c["rows"] * c["cols"] // C.GROUP[t] == n and c["cols"] % C.GROUP[t] == 0, (t, tag)
    assert C.load_fixture()[1]["groups_per_block"] == C.GROUPS_PER_BLOCK


# ------------------------------------------------------------------------------------------------------------------- the plans
@TARGETS
def test_plan_counts_workgroups_and_fills_the_derived_fields(lib, target):
    g, gpb = C.GROUP[target], C.GROUPS_PER_BLOCK[target]
    m1, p1 = (C.CASES[f"share_{tag}.{target}"] for tag in ("m1", "p1"))
    # (rows, cols, block, scale shape, sdt)
    shapes = [(576, 7168, (128, 128), None, lib.F32), (200, 320, (64, 32), None, lib.BF16), (256, 256, (1, 128), (1, 2), lib.F16),
              (m1["rows"], m1["cols"], (128, 128), (1, 1), lib.F32), (p1["rows"], p1["cols"], (128, 128), None, lib.F32), (1, g, (128, 128), None, lib.F32)]
    n, table = _plan(target, [_item(target, r, c, b, s, d, base=0x100000 * (i + 1)) for i, (r, c, b, s, d) in enumerate(shapes)])
    expect, first = [], 0
    for r, c, _, _, _ in shapes:
        expect.append((first, c // g, r * (c // g), 0))
        first += -(-(r * (c // g)) // gpb)
    assert n == first
    assert [(t.first_block, t.units_per_row, t.units, t.reserved) for t in table] == expect
    assert expect[4][0] - expect[3][0] == 1 and expect[5][0] - expect[4][0] == 2  # one group fewer: one workgroup; one more: two
    # scale strides in elements, 0 along a broadcast dimension (a single block row or column is one)
    ncb_p1 = -(-p1["cols"] // 128)
    assert [tuple(t.scale_stride) for t in table] == [(56, 1), (10, 1), (0, 1), (0, 0), (0 if p1["rows"] <= 128 else ncb_p1, 1 if ncb_p1 > 1 else 0), (0, 0)]
    for shape in ((3, 2), (1, 2), (3, 1), (1, 1)):  # every broadcast torch accepts
        assert _plan(target, [_item(target, 300, 256, scale_shape=shape)])[0] == -(-(300 * (256 // g)) // gpb), shape


@TARGETS
def test_plan_refuses_one_item_per_branch_and_names_it(lib, target):
    g = C.GROUP[target]
    ragged, odd_bw = (48, 80) if target == "mxfp8" else (40, 40)
    mk = lambda *a, **k: _item(target, *a, **k)  # noqa: E731
    bad = {
        f"columns ({ragged}) must be a multiple of the {'MX' if target == 'mxfp8' else 'NVFP4'} group size {g}": mk(64, ragged),
        f"block width {odd_bw} is not a multiple of {g}": mk(200, 320, (96, odd_bw)),
        "weight is not 16-byte aligned": mk(64, 64),
        "is not 16-byte aligned": mk(64, 64),
        "weight_scale_inv of shape (2, 2)": mk(128, 128, scale_shape=(2, 2)),
        "weight_scale_inv of shape (0, 1)": mk(128, 128, scale_shape=(0, 1)),
        "weight_scale_inv must be float32, bfloat16 or float16 (dtype code 8)": mk(64, 64, sdt=lib.F8),
        "weight_scale_inv must be float32, bfloat16 or float16 (dtype code 4)": mk(64, 64, sdt=lib.I32),
        "has a NULL pointer": mk(64, 64),
        "has a NULL pointer ": mk(64, 64),
        "has shape (0, 64)": mk(0, 64, scale_shape=(1, 1)),
        "has shape (64, -32)": mk(64, -32, scale_shape=(1, 1)),
        "has shape (64, 2147483648)": mk(64, 1 << 31, scale_shape=(1, 1)),
        "has block size (0, 128)": mk(64, 64, (0, 128), scale_shape=(1, 1)),
        "has block size (128, -128)": mk(64, 64, (128, -128), scale_shape=(1, 1)),
    }
    bad["weight is not 16-byte aligned"].w += 8
    bad["is not 16-byte aligned"].packed += 8
    bad["has a NULL pointer "].scale = None
    if target == "mxfp8":
        bad["has a NULL pointer"].e8m0 = None
    else:
        bad["has a NULL pointer"].key = None
        bad["has a NULL pointer  "] = mk(64, 64)
        bad["has a NULL pointer  "].global_scale = None
        bad["has a NULL pointer   "] = mk(64, 64)
        bad["has a NULL pointer   "].scale_f8 = None
        bad["the amax key and weight_global_scale must be 4-byte aligned"] = mk(64, 64)
        bad["the amax key and weight_global_scale must be 4-byte aligned"].key += 2
    for why, it in bad.items():
        ret, table = _plan(target, [mk(64, 64), it, mk(64, 64)])
        assert ret == -1, why
        assert lib.last_error().startswith(f"{PLAN[target]}: item 1") and why.strip() in lib.last_error(), (why, lib.last_error())
        assert table[2].first_block == -7  # the loop stopped at the refused item
    if target == "nvfp4":  # what the MX plans refuse and this one admits: columns and a block width of 16 and not of 32
        assert _plan(target, [mk(3, 48), mk(200, 320, (96, 80))])[0] == 1 + 4


@TARGETS
def test_plan_of_empty_null_negative_and_oversized_tables(lib, target):
    g, gpb = C.GROUP[target], C.GROUPS_PER_BLOCK[target]
    plan = getattr(lib.load(), PLAN[target])
    ret, table = _plan(target, [_item(target, 64, 64)], n=0)
    assert ret == 0 and table[0].first_block == -7  # n = 0: nothing is read or written
    assert plan(None, 0) == 0
    assert plan(None, 1) == -1 and lib.last_error() == f"{PLAN[target]}: bad arguments"
    assert _plan(target, [_item(target, 64, 64)], n=-1)[0] == -1 and lib.last_error() == f"{PLAN[target]}: bad arguments"
    # a table past the launch cap: 2^31 workgroups or more are refused, one short of it is admitted
    rows = (1 << 31) - 1
    cap = _item(target, rows, g * gpb, scale_shape=(1, 1))
    assert _plan(target, [cap])[0] == rows
    assert _plan(target, [cap, _item(target, 1, g)])[0] == -1 and "workgroups exceed one launch; split the batch" in lib.last_error()
    # the launches: a bad dense dtype is refused whatever the table, an empty table returns before anything is launched
    for name in LAUNCHES[target]:
        batch = getattr(lib.load(), name)
        extra = (None,) if target == "mxfp8" else ()
        assert batch(None, 0, 0, lib.F32, *extra, None) != 0 and "dense dtype must be bfloat16 or float16" in lib.last_error()
        assert batch(None, 0, 0, lib.BF16, *extra, None) == 0 and batch(None, 1, 1 << 31, lib.BF16, *extra, None) != 0


@TARGETS
def test_python_never_hands_the_plan_a_row_it_would_refuse(lib, target):
    from compressed_tensors_amd.entrypoints.convert import fp8block_transcode as ft

    class T:  # what `fused_admits` reads of a tensor
        def __init__(self, ptr):
            self.ptr = ptr

        def data_ptr(self):
            return self.ptr

    tgt = {"mxfp8": ft.MXFP8, "nvfp4": ft.NVFP4}[target]
    for block, wp, pp in (((128, 128), 0x1000, 0x2000), ((128, 80), 0x1000, 0x2000), ((128, 40), 0x1000, 0x2000), ((128, 128), 0x1008, 0x2000),
                          ((128, 128), 0x1000, 0x2008), ((64, 32), 0x1000, 0x2000), ((64, 16), 0x1000, 0x2000)):
        it = _item(target, 200, 320, block)
        it.w, it.packed = wp, pp
        assert ft.fused_admits(tgt, T(wp), T(pp), block) == (_plan(target, [it])[0] >= 0), (block, wp, pp)


# ------------------------------------------------------------------------------------------------------------------- the converters
def _names(*names):
    return dict.fromkeys(names)


def _classes():
    from compressed_tensors_amd.entrypoints.convert import FP8BlockToMXFP8Converter, FP8BlockToNVFP4Converter

    return {"mxfp8": FP8BlockToMXFP8Converter, "nvfp4": FP8BlockToNVFP4Converter}


def test_both_classes_are_exported_converters_over_one_body():
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.entrypoints import convert
    from compressed_tensors_amd.entrypoints.convert import Converter, FP8BlockToMXFP4Converter
    from compressed_tensors_amd.entrypoints.convert.fp8block_transcode import FP8BlockTranscoder

    for cls in _classes().values():
        assert cls.__name__ in convert.__all__ and issubclass(cls, Converter) and issubclass(cls, FP8BlockTranscoder)
    assert issubclass(FP8BlockToMXFP4Converter, FP8BlockTranscoder)  # the third user of the body
    for cls in (*_classes().values(), FP8BlockToMXFP4Converter):
        assert cls.process is FP8BlockTranscoder.process and cls.validate is FP8BlockTranscoder.validate
    for name in ("fp8block_to_mxfp8", "fp8block_to_nvfp4"):
        assert callable(getattr(codec, name)) and name in codec.__all__
    assert [c.format for c in _classes().values()] == ["mxfp8-quantized", "nvfp4-pack-quantized"]


@TARGETS
def test_validate_and_dependencies_on_names_alone(target):
    cls = _classes()[target]
    conv = cls(ignore=["re:lm_head.*"], targets=["re:.*proj$"])
    conv.validate(_names("m.q_proj.weight", "m.q_proj.weight_scale_inv", "lm_head.weight", "lm_head.weight_scale_inv", "m.norm.weight"))
    with pytest.raises(ValueError, match="Found weight without corresponding weight_scale_inv m.q_proj.weight"):
        conv.validate(_names("m.q_proj.weight"))
    with pytest.raises(ValueError, match="Found weight_scale_inv without corresponding weight m.q_proj.weight_scale_inv"):
        conv.validate(_names("m.q_proj.weight_scale_inv"))
    with pytest.raises(ValueError, match="Found unexpected non-targeted tensor m.gate.weight_scale_inv"):
        conv.validate(_names("m.gate.weight", "m.gate.weight_scale_inv"))
    assert conv.get_dependencies("m.q_proj.weight") == {"m.q_proj.weight_scale_inv"}
    assert conv.get_dependencies("m.q_proj.weight_scale_inv") == set()
    assert conv.get_dependencies("lm_head.weight") == set() and conv.get_dependencies("m.norm.weight") == set()
    assert conv.param_names == ["weight", "weight_scale_inv"] and conv.stream_results is False
    for bad in (dict(dtype=torch.float32), dict(weight_block_size=(128,)), dict(weight_block_size=(0, 128))):
        with pytest.raises(ValueError, match=cls.__name__):
            cls(**bad)


@TARGETS
def test_fused_follows_the_measured_flag_unless_forced(monkeypatch, target):
    from compressed_tensors_amd.entrypoints.convert import fp8block_transcode as ft

    cls = _classes()[target]
    name = f"FP8BLOCK_{target.upper()}_MEASURED_FASTER"
    assert name in ft.__all__ and isinstance(getattr(ft, name), bool)
    for flag in (True, False):
        monkeypatch.setattr(ft, name, flag)
        assert cls()._fused() is flag
        assert cls(fused=True)._fused() is True and cls(fused=False)._fused() is False


@pytest.mark.parametrize("target, activations, preset", [("mxfp8", False, "MXFP8"), ("mxfp8", True, "MXFP8"), ("nvfp4", False, "NVFP4A16"), ("nvfp4", True, "NVFP4")])
def test_create_config_is_the_reference_preset(target, activations, preset):
    from compressed_tensors_amd.entrypoints.convert import FP8BlockQuantizer

    want = C.load_fixture()[1]["presets"][preset]
    assert (want["input_activations"] is not None) == (preset != "NVFP4A16")
    shape = FP8BlockQuantizer(ignore=["lm_head"], targets=["re:.*proj$"]).create_config().model_dump()
    conv = _classes()[target](["lm_head"], ["re:.*proj$"], activations=activations)
    cfg = conv.create_config().model_dump()
    group = cfg["config_groups"]["config_group_0"]
    assert group["weights"] == want["weights"] and group["input_activations"] == want["input_activations"]
    assert cfg["format"] == group["format"] == conv.format and group["targets"] == ["re:.*proj$"] and cfg["ignore"] == ["lm_head"]
    # the shape `_DenseQuantizer.create_config` produces
    assert list(cfg) == list(shape) and list(group) == list(shape["config_groups"]["config_group_0"])
    assert {k: v for k, v in cfg.items() if k not in ("config_groups", "format")} == {k: v for k, v in shape.items() if k not in ("config_groups", "format")}


# ------------------------------------------------------------------------------------------------------------------- early refusal
@TARGETS
def test_ragged_columns_raise_the_reference_text_before_any_device_is_touched(monkeypatch, target):
    from compressed_tensors_amd import _lib, codec

    def no_device():
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(_lib, "require_device", no_device)
    g = C.GROUP[target]
    cols = 48 if target == "mxfp8" else 40
    entry = getattr(codec, f"fp8block_to_{target}")
    w = C.synth_codes(64, cols, 1)
    s = C.synth_scales(1, 1, 1, torch.float32)
    text = f"tensor column shape must be divisble by the given group_size {g} but got {cols}"
    with pytest.raises(ValueError, match=text):
        entry(w, s)
    good_w, good_s = C.inputs("sq128")
    shard = {"a.q_proj.weight": good_w, "a.q_proj.weight_scale_inv": good_s, "b.q_proj.weight": w, "b.q_proj.weight_scale_inv": s}
    with pytest.raises(ValueError, match="b.q_proj: " + text):
        _classes()[target](targets=["re:.*proj$"], fused=True).process(dict(shard))
    with pytest.raises(ValueError, match="expected a 2-D float8_e4m3fn tensor"):
        entry(torch.zeros(4, 64), s)
    with pytest.raises(ValueError, match="dtype must be torch.bfloat16 or torch.float16"):
        entry(good_w, good_s, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------------------- the fixture
def test_the_fixture_is_complete_and_small():
    blob, manifest = C.load_fixture()
    keys = [f"{t}.{case}.{dtype}.{name}" for t in C.TARGETS for case in C.cases_of(t) for dtype in C.DENSE_DTYPES for name, _ in C.OUTPUTS[t]]
    assert sorted(manifest["outputs"]) == sorted(keys)
    assert sorted(blob) == sorted(k for k, rec in manifest["outputs"].items() if rec["whole"])
    assert sorted(manifest["presets"]) == ["MXFP8", "NVFP4", "NVFP4A16"]
    for t in C.TARGETS:
        assert not manifest["outputs"][f"{t}.kv_a_576x7168.bfloat16.{C.OUTPUTS[t][0][0]}"]["whole"]  # the kv_a shape keeps its sha256 alone
        assert manifest["outputs"][f"{t}.allcodes_b1x256.float16.{C.OUTPUTS[t][0][0]}"]["whole"]
        # the matrix: the MXFP4 one, the shapes around each kernel's share, and for NVFP4 columns and a block width of 16 and not of 32
        assert set(C.M.CASES) <= set(C.cases_of(t)) and {f"share_m1.{t}", f"share_p1.{t}"} <= set(C.cases_of(t))
    assert C.CASES["nv_r3x48"]["cols"] % 32 == 16 and C.CASES["nv_r64x96_b32x48"]["block"][1] % 32 == 16 and C.CASES["refused_b96x80"]["block"] == (96, 80)
    for name in ("fp8block_transcode.safetensors", "fp8block_transcode_manifest.json"):
        assert os.path.getsize(os.path.join(C.GOLDEN, name)) < 2 * os.path.getsize(os.path.join(C.GOLDEN, "fp8block.safetensors")), name
    # bytes the generator took from the pinned oracle: none in a case without NaN codes (there the fixture is the reference's output in every byte)
    for key, rec in manifest["outputs"].items():
        case = key.split(".", 1)[1].rsplit(".", 2)[0]
        assert case in C.CASES and (rec["bytes_from_oracle"] == 0 or case in C.HOLDS_NAN_CODES), key
    w, _ = C.inputs("share_m1.nvfp4")
    assert not bool(((w.view(torch.uint8) & 0x7F) == 0x7F).any())  # `finite_codes`


# ------------------------------------------------------------------------------------------------------------------- reading it back
def test_the_dequantizer_reads_an_nvfp4_checkpoint_without_input_global_scales(tmp_path):
    """the NVFP4 preset's activations are `dynamic="local"`: a calibrated checkpoint carries an `input_global_scale` per module, the data-free
    conversion none — the name is a partner of the weight only where the checkpoint holds it"""
    import json

    from compressed_tensors_amd.entrypoints.convert import CompressedTensorsDequantizer, FP8BlockToNVFP4Converter

    cfg = FP8BlockToNVFP4Converter(targets=["re:.*proj$"], activations=True).create_config().model_dump()
    parts = ["weight_packed", "weight_scale", "weight_global_scale"]
    names = [f"{m}.{p}" for m in ("a.q_proj", "b.q_proj") for p in parts] + ["b.q_proj.input_global_scale", "a.norm.weight"]
    (tmp_path / "config.json").write_text(json.dumps({"quantization_config": cfg}))
    (tmp_path / "model.safetensors.index.json").write_text(json.dumps({"metadata": {}, "weight_map": dict.fromkeys(names, "model-00001-of-00001.safetensors")}))
    conv = CompressedTensorsDequantizer(str(tmp_path))
    conv.validate(dict.fromkeys(names))
    assert conv.get_dependencies("a.q_proj.weight_packed") == {"a.q_proj.weight_scale", "a.q_proj.weight_global_scale"}
    assert conv.get_dependencies("b.q_proj.weight_packed") == {"b.q_proj.weight_scale", "b.q_proj.weight_global_scale", "b.q_proj.input_global_scale"}
    with pytest.raises(ValueError, match="Expected key a.q_proj.weight_global_scale not found"):
        conv.validate(dict.fromkeys(n for n in names if n != "a.q_proj.weight_global_scale"))
