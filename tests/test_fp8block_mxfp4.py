"""FP8BlockToMXFP4Converter, MXFP4Quantizer and the C planner of `ct_fp8block_mxfp4_batch` (CPU tests: the ABI, the plan through ctypes, the converters'
host logic on name-only dicts, the refusals that must come before any device is touched).  The GPU half is tests/test_gpu_fp8block_mxfp4.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import _fp8block_mxfp4_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = "ct_fp8block_mxfp4_plan"
GPB = C.GROUPS_PER_BLOCK


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    from compressed_tensors_amd import _lib

    return _lib


def _item(rows, cols, block=(128, 128), scale_shape=None, sdt=None, base=0x100000):
    from compressed_tensors_amd import _lib

    it = _lib.Fp8BlockMxItem()
    it.w, it.scale, it.packed, it.e8m0 = base, base + 0x1000, base + 0x2000, base + 0x3000
    it.rows, it.cols, it.block_h, it.block_w = rows, cols, block[0], block[1]
    it.scale_shape[0], it.scale_shape[1] = scale_shape or (-(-rows // max(block[0], 1)), -(-cols // max(block[1], 1)))
    it.sdt = _lib.F32 if sdt is None else sdt
    it.reserved, it.units_per_row, it.units, it.first_block = -7, -7, -7, -7  # the plan writes every derived field of an admitted item
    return it


def _plan(items, n=None):
    from compressed_tensors_amd import _lib

    table = (_lib.Fp8BlockMxItem * max(len(items), 1))(*items)
    return int(getattr(_lib.load(), PLAN)(ctypes.cast(table, ctypes.c_void_p), len(items) if n is None else n)), table


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_the_two_symbols_are_declared_prototyped_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "ct_hip.h")).read()
    assert "int64_t ct_fp8block_mxfp4_plan(ct_fp8block_mx_item* items_host, int n);" in header
    assert "int ct_fp8block_mxfp4_batch(const ct_fp8block_mx_item* items_dev, int n, int64_t total_blocks, int xdt, ct_stream_t stream);" in header
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in (PLAN, "ct_fp8block_mxfp4_batch"):
        assert re.search(rf"\bT {name}\b", exported), name
        assert name in lib._PROTOTYPES and name in lib.EXPORTED_SYMBOLS and hasattr(lib.load(), name)
    words = int(re.search(r"\} ct_fp8block_mx_item;\s*/\* (\d+) 64-bit words \*/", header).group(1))
    assert ctypes.sizeof(lib.Fp8BlockMxItem) == 8 * words == 128
    assert lib.Fp8BlockMxItem.sdt.offset == 80 and lib.Fp8BlockMxItem.first_block.offset == 120
    # the workgroup's share of groups: the header, the binding and the case matrix (whose 511- and 513-group shapes depend on it) agree
    assert int(re.search(r"#define CT_FP8BLOCK_MX_GROUPS_PER_BLOCK (\d+)", header).group(1)) == lib.FP8BLOCK_MX_GROUPS_PER_BLOCK == GPB
    assert C.CASES["g511_r73x224"]["rows"] * C.CASES["g511_r73x224"]["cols"] // 32 == GPB - 1
    assert C.CASES["g513_r27x608"]["rows"] * C.CASES["g513_r27x608"]["cols"] // 32 == GPB + 1


# ------------------------------------------------------------------------------------------------------------------- the plan
def test_plan_counts_workgroups_and_fills_the_derived_fields(lib):
    # (rows, cols, block, scale shape, sdt)
    shapes = [(576, 7168, (128, 128), None, lib.F32), (200, 320, (64, 32), None, lib.BF16), (256, 256, (1, 128), (1, 2), lib.F16),
              (73, 224, (128, 128), (1, 1), lib.F32), (27, 608, (128, 128), None, lib.F32), (1, 32, (128, 128), None, lib.F32)]
    n, table = _plan([_item(r, c, b, s, d, base=0x100000 * (i + 1)) for i, (r, c, b, s, d) in enumerate(shapes)])
    expect, first = [], 0
    for r, c, _, _, _ in shapes:
        expect.append((first, c // 32, r * (c // 32), 0))
        first += -(-(r * (c // 32)) // GPB)
    assert n == first == 252 + 4 + 4 + 1 + 2 + 1
    assert [(t.first_block, t.units_per_row, t.units, t.reserved) for t in table] == expect
    # scale strides in elements, 0 along a broadcast dimension (a single block row or column is one)
    assert [tuple(t.scale_stride) for t in table] == [(56, 1), (10, 1), (0, 1), (0, 0), (0, 1), (0, 0)]
    # every broadcast torch accepts
    for shape in ((3, 2), (1, 2), (3, 1), (1, 1)):
        assert _plan([_item(300, 256, scale_shape=shape)])[0] == -(-(300 * 8) // GPB), shape


def test_plan_refuses_one_item_per_branch_and_names_it(lib):
    bad = {
        "columns (48) must be a multiple of the MX group size 32": _item(64, 48),
        "block width 80 is not a multiple of 32": _item(200, 320, (96, 80)),
        "weight is not 16-byte aligned": _item(64, 64),
        "weight_packed is not 16-byte aligned": _item(64, 64),
        "weight_scale_inv of shape (2, 2)": _item(128, 128, scale_shape=(2, 2)),
        "weight_scale_inv of shape (0, 1)": _item(128, 128, scale_shape=(0, 1)),
        "weight_scale_inv must be float32, bfloat16 or float16 (dtype code 8)": _item(64, 64, sdt=lib.F8),
        "weight_scale_inv must be float32, bfloat16 or float16 (dtype code 4)": _item(64, 64, sdt=lib.I32),
        "has a NULL pointer": _item(64, 64),
        "has a NULL pointer ": _item(64, 64),
        "has shape (0, 64)": _item(0, 64, scale_shape=(1, 1)),
        "has shape (64, -32)": _item(64, -32, scale_shape=(1, 1)),
        "has shape (64, 2147483648)": _item(64, 1 << 31, scale_shape=(1, 1)),
        "has block size (0, 128)": _item(64, 64, (0, 128), scale_shape=(1, 1)),
        "has block size (128, -128)": _item(64, 64, (128, -128), scale_shape=(1, 1)),
    }
    bad["weight is not 16-byte aligned"].w += 8
    bad["weight_packed is not 16-byte aligned"].packed += 8
    bad["has a NULL pointer"].e8m0 = None
    bad["has a NULL pointer "].scale = None
    for why, it in bad.items():
        ret, table = _plan([_item(64, 64), it, _item(64, 64)])
        assert ret == -1, why
        assert lib.last_error().startswith(f"{PLAN}: item 1") and why.strip() in lib.last_error(), (why, lib.last_error())
        assert table[2].first_block == -7  # the loop stopped at the refused item


def test_plan_of_empty_null_negative_and_oversized_tables(lib):
    plan = getattr(lib.load(), PLAN)
    ret, table = _plan([_item(64, 64)], n=0)
    assert ret == 0 and table[0].first_block == -7  # n = 0: nothing is read or written
    assert plan(None, 0) == 0
    assert plan(None, 1) == -1 and lib.last_error() == f"{PLAN}: bad arguments"
    assert _plan([_item(64, 64)], n=-1)[0] == -1 and lib.last_error() == f"{PLAN}: bad arguments"
    # a table past the launch cap: 2^31 workgroups or more are refused, one short of it is admitted
    rows = (1 << 31) - 1
    cap = _item(rows, 32 * GPB, scale_shape=(1, 1))
    assert _plan([cap])[0] == rows
    assert _plan([cap, _item(1, 32)])[0] == -1 and "workgroups exceed one launch; split the batch" in lib.last_error()
    # the launch: a bad dense dtype is refused whatever the table, an empty table returns before anything is launched
    batch = lib.load().ct_fp8block_mxfp4_batch
    assert batch(None, 0, 0, lib.F32, None) != 0 and "dense dtype must be bfloat16 or float16" in lib.last_error()
    assert batch(None, 0, 0, lib.BF16, None) == 0 and batch(None, 1, 1 << 31, lib.BF16, None) != 0


def test_python_never_hands_the_plan_a_row_it_would_refuse(lib):
    from compressed_tensors_amd.entrypoints.convert import fp8block_mxfp4 as fx

    class T:  # what `_fused_admits` reads of a tensor
        def __init__(self, ptr):
            self.ptr = ptr

        def data_ptr(self):
            return self.ptr

    for block, wp, pp in (((128, 128), 0x1000, 0x2000), ((128, 80), 0x1000, 0x2000), ((128, 128), 0x1008, 0x2000), ((128, 128), 0x1000, 0x2008), ((64, 32), 0x1000, 0x2000)):
        it = _item(200, 320, block)
        it.w, it.packed = wp, pp
        assert fx._fused_admits(T(wp), T(pp), block) == (_plan([it])[0] >= 0), (block, wp, pp)


# ------------------------------------------------------------------------------------------------------------------- the converters
def _names(*names):
    return dict.fromkeys(names)


def test_both_classes_are_exported_converters():
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.entrypoints import convert
    from compressed_tensors_amd.entrypoints.convert import Converter, FP8BlockToMXFP4Converter, MXFP4Quantizer

    for cls in (FP8BlockToMXFP4Converter, MXFP4Quantizer):
        assert cls.__name__ in convert.__all__ and issubclass(cls, Converter)
    for name in ("fp8block_to_mxfp4", "rtn_mxfp4_outputs", "rtn_mxfp4_launch"):
        assert callable(getattr(codec, name)) and name in codec.__all__
    assert "rtn_mxfp4" in codec._TABLES and len(codec._TABLES) == 12  # the transcoding's table is no `ct_w4_item` table: no kind of its own
    assert codec.rtn_mxfp4_launch(torch.float16) == ("rtn_mxfp4", 0, (codec.DT[torch.float16],))
    assert codec.rtn_mxfp4_outputs(3, 64) == [("dst", (3, 32), torch.uint8), ("zp_packed", (3, 2), torch.uint8)]
    assert MXFP4Quantizer.entry_of == {"dst": "weight_packed", "zp_packed": "weight_scale"}


def test_validate_and_dependencies_on_names_alone():
    from compressed_tensors_amd.entrypoints.convert import FP8BlockToMXFP4Converter

    conv = FP8BlockToMXFP4Converter(ignore=["re:lm_head.*"], targets=["re:.*proj$"])
    ok = _names("m.q_proj.weight", "m.q_proj.weight_scale_inv", "lm_head.weight", "lm_head.weight_scale_inv", "m.norm.weight")
    conv.validate(ok)
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
        with pytest.raises(ValueError):
            FP8BlockToMXFP4Converter(**bad)


def test_fused_follows_the_measured_flag_unless_forced(monkeypatch):
    from compressed_tensors_amd.entrypoints.convert import fp8block_mxfp4 as fx

    for flag in (True, False):
        monkeypatch.setattr(fx, "FP8BLOCK_MXFP4_MEASURED_FASTER", flag)
        assert fx.FP8BlockToMXFP4Converter()._fused() is flag
        assert fx.FP8BlockToMXFP4Converter(fused=True)._fused() is True and fx.FP8BlockToMXFP4Converter(fused=False)._fused() is False


@pytest.mark.parametrize("activations, preset", [(False, "MXFP4A16"), (True, "MXFP4")])
def test_create_config_is_the_reference_preset(activations, preset):
    from compressed_tensors_amd.entrypoints.convert import FP8BlockToMXFP4Converter, FP8BlockQuantizer, MXFP4Quantizer

    want = C.load_fixture()[1]["presets"][preset]
    assert (want["input_activations"] is not None) == activations
    shape = FP8BlockQuantizer(ignore=["lm_head"], targets=["re:.*proj$"]).create_config().model_dump()
    for conv in (FP8BlockToMXFP4Converter(["lm_head"], ["re:.*proj$"], activations=activations),
                 MXFP4Quantizer(["lm_head"], ["re:.*proj$"], activations=activations)):
        cfg = conv.create_config().model_dump()
        group = cfg["config_groups"]["config_group_0"]
        assert group["weights"] == want["weights"] and group["input_activations"] == want["input_activations"]
        assert cfg["format"] == group["format"] == "mxfp4-pack-quantized" and group["targets"] == ["re:.*proj$"] and cfg["ignore"] == ["lm_head"]
        # the shape `_DenseQuantizer.create_config` produces
        assert list(cfg) == list(shape) and list(group) == list(shape["config_groups"]["config_group_0"])
        assert {k: v for k, v in cfg.items() if k not in ("config_groups", "format")} == {k: v for k, v in shape.items() if k not in ("config_groups", "format")}


def test_mxfp4_quantizer_refuses_a_module_that_is_quantized_already():
    from compressed_tensors_amd.entrypoints.convert import MXFP4Quantizer

    conv = MXFP4Quantizer(targets=["re:.*proj$"])
    conv.validate(_names("m.q_proj.weight", "m.norm.weight", "lm_head.weight"))
    for partner in ("weight_packed", "weight_scale"):
        with pytest.raises(ValueError, match=f"Found m.q_proj.{partner} beside the targeted m.q_proj.weight"):
            conv.validate(_names("m.q_proj.weight", f"m.q_proj.{partner}"))
    assert conv.get_dependencies("m.q_proj.weight") == set()


# ------------------------------------------------------------------------------------------------------------------- early refusal
def test_ragged_columns_raise_the_reference_text_before_any_device_is_touched(monkeypatch):
    from compressed_tensors_amd import _lib, codec
    from compressed_tensors_amd.entrypoints.convert import FP8BlockToMXFP4Converter, MXFP4Quantizer

    def no_device():
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(_lib, "require_device", no_device)
    w = C.synth_codes(64, 48, 1)
    s = C.synth_scales(1, 1, 1, torch.float32)
    text = "tensor column shape must be divisble by the given group_size 32 but got 48"
    with pytest.raises(ValueError, match=text):
        codec.fp8block_to_mxfp4(w, s)
    good_w, good_s = C.inputs("sq128")
    shard = {"a.q_proj.weight": good_w, "a.q_proj.weight_scale_inv": good_s, "b.q_proj.weight": w, "b.q_proj.weight_scale_inv": s}
    with pytest.raises(ValueError, match="b.q_proj: " + text):
        FP8BlockToMXFP4Converter(targets=["re:.*proj$"], fused=True).process(dict(shard))
    with pytest.raises(ValueError, match="b.q_proj: " + text):
        MXFP4Quantizer(targets=["re:.*proj$"]).process({"a.q_proj.weight": torch.zeros(4, 64, dtype=torch.bfloat16), "b.q_proj.weight": torch.zeros(4, 48, dtype=torch.bfloat16)})
    with pytest.raises(ValueError, match="expected a 2-D float8_e4m3fn tensor"):
        codec.fp8block_to_mxfp4(torch.zeros(4, 64), s)
    with pytest.raises(ValueError, match="dtype must be torch.bfloat16 or torch.float16"):
        codec.fp8block_to_mxfp4(good_w, good_s, dtype=torch.float32)


def test_the_fixture_is_complete_and_small():
    blob, manifest = C.load_fixture()
    keys = [f"{case}.{dtype}" for case in C.CASES for dtype in C.DENSE_DTYPES] + [f"quantizer.{n}.{d}" for n in C.QUANTIZER_SHAPES for d in C.DENSE_DTYPES]
    assert sorted(manifest["outputs"]) == sorted(f"{k}.{name}" for k in keys for name in ("packed", "e8m0"))
    assert sorted(blob) == sorted(k for k, rec in manifest["outputs"].items() if rec["whole"])
    assert not manifest["outputs"]["kv_a_576x7168.bfloat16.packed"]["whole"]  # the kv_a shape keeps its sha256 alone
    assert manifest["outputs"]["allcodes_b1x256.float16.packed"]["whole"] and manifest["outputs"]["allcodes_b1x32.bfloat16.e8m0"]["whole"]
    assert os.path.getsize(os.path.join(C.GOLDEN, "fp8block_mxfp4.safetensors")) < 2 * os.path.getsize(os.path.join(C.GOLDEN, "fp8block.safetensors"))
    # the all-codes rows hold every byte, the sweep a zero of either sign, negatives and a float16 overflow
    w, s = C.inputs("allcodes_b1x32")
    assert sorted(set(w.view(torch.uint8)[0].tolist())) == list(range(256)) and s.shape == (20, 8)
    assert {0.0, -1.0, 2.0 ** 100} <= set(s[:, 0].tolist()) and torch.signbit(s[:, 0]).sum() >= 5
