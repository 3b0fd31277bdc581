"""NVFP4ToMXFP4Converter, `codec.nvfp4_to_mxfp4` and the C planner of `ct_nvfp4_mxfp4_batch` (CPU tests: the ABI, the plan through ctypes, the
converter's host logic, the refusals that must come before any device is touched).  The GPU half is tests/test_gpu_nvfp4_mxfp4.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import _nvfp4_mxfp4_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = "ct_nvfp4_mxfp4_plan"
GPB = C.GROUPS_PER_BLOCK
TARGETS = ["re:.*proj$"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    from compressed_tensors_amd import _lib

    return _lib


def _item(rows, cols, base=0x100000):
    from compressed_tensors_amd import _lib

    it = _lib.Nvfp4MxItem()
    it.packed_in, it.scale_f8, it.global_scale, it.packed_out, it.e8m0 = base, base + 0x1000, base + 0x2000, base + 0x3000, base + 0x4000
    it.rows, it.cols = rows, cols
    it.units, it.first_block = -7, -7  # the plan writes every derived field of an admitted item
    return it


def _plan(items, n=None):
    from compressed_tensors_amd import _lib

    table = (_lib.Nvfp4MxItem * max(len(items), 1))(*items)
    return int(getattr(_lib.load(), PLAN)(ctypes.cast(table, ctypes.c_void_p), len(items) if n is None else n)), table


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_the_two_symbols_are_declared_prototyped_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "ct_hip.h")).read()
    assert "int64_t ct_nvfp4_mxfp4_plan(ct_nvfp4_mx_item* items_host, int n);" in header
    assert "int ct_nvfp4_mxfp4_batch(const ct_nvfp4_mx_item* items_dev, int n, int64_t total_blocks, ct_stream_t stream);" in header
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in (PLAN, "ct_nvfp4_mxfp4_batch"):
        assert re.search(rf"\bT {name}\b", exported), name
        assert name in lib._PROTOTYPES and name in lib.EXPORTED_SYMBOLS and hasattr(lib.load(), name)
    words = int(re.search(r"\} ct_nvfp4_mx_item;\s*/\* (\d+) 64-bit words \*/", header).group(1))
    assert ctypes.sizeof(lib.Nvfp4MxItem) == 8 * words == 72
    assert lib.Nvfp4MxItem.rows.offset == 40 and lib.Nvfp4MxItem.first_block.offset == 64
    fields = re.search(r"typedef struct ct_nvfp4_mx_item \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"(\w+)(?:, (\w+))?;", fields) == [("packed_in", ""), ("scale_f8", ""), ("global_scale", ""), ("packed_out", ""), ("e8m0", ""),
                                                          ("rows", "cols"), ("units", ""), ("first_block", "")]
    assert [f[0] for f in lib.Nvfp4MxItem._fields_] == ["packed_in", "scale_f8", "global_scale", "packed_out", "e8m0", "rows", "cols", "units", "first_block"]


def test_the_header_constant_the_binding_and_the_case_matrix_agree(lib):
    header = open(os.path.join(ROOT, "include", "ct_hip.h")).read()
    assert int(re.search(r"#define CT_NVFP4_MX_GROUPS_PER_BLOCK (\d+)", header).group(1)) == lib.NVFP4_MX_GROUPS_PER_BLOCK == GPB
    groups = {key: c["rows"] * c["cols"] // 32 for key, c in C.CASES.items()}
    assert (groups["g_minus_1"], groups["g_exact"], groups["g_plus_1"]) == (GPB - 1, GPB, GPB + 1)
    # 27 rows whose boundaries fall inside the first workgroup, and a second workgroup
    assert GPB < groups["r27x1216"] < 2 * GPB and GPB % (C.CASES["r27x1216"]["cols"] // 32) != 0
    # the mixed table: a module of one group, so that neighbouring workgroups belong to different items, and a global scale per module
    assert min(groups[k] for k in C.MIXED_KEYS) == 1 and len({C.CASES[k]["gs"] for k in C.MIXED_KEYS}) == len(C.MIXED_KEYS)


# ------------------------------------------------------------------------------------------------------------------- the plan
def test_plan_counts_workgroups_and_fills_the_derived_fields(lib):
    shapes = [(576, 7168), (200, 320), (1, 32 * (GPB - 1)), (1, 32 * GPB), (1, 32 * (GPB + 1)), (27, 1216), (1, 32)]
    n, table = _plan([_item(r, c, base=0x100000 * (i + 1)) for i, (r, c) in enumerate(shapes)])
    expect, first = [], 0
    for r, c in shapes:
        expect.append((first, r * (c // 32)))
        first += -(-(r * (c // 32)) // GPB)
    assert n == first == 126 + 2 + 1 + 1 + 2 + 2 + 1
    assert [(t.first_block, t.units) for t in table] == expect


def test_plan_refuses_one_item_per_branch_and_names_it(lib):
    bad = {
        "columns (48) must be a multiple of the MX group size 32": _item(64, 48),
        "the NVFP4 weight_packed is not 16-byte aligned": _item(64, 64),
        "the MXFP4 weight_packed is not 16-byte aligned": _item(64, 64),
        "the NVFP4 weight_scale is not 2-byte aligned": _item(64, 64),
        "weight_global_scale is not 4-byte aligned": _item(64, 64),
        "has a NULL pointer": _item(64, 64),
        "has a NULL pointer ": _item(64, 64),
        "has a NULL pointer  ": _item(64, 64),
        "has a NULL pointer   ": _item(64, 64),
        "has a NULL pointer    ": _item(64, 64),
        "has shape (0, 64)": _item(0, 64),
        "has shape (64, -32)": _item(64, -32),
        "has shape (64, 2147483648)": _item(64, 1 << 31),
        "has shape (2147483648, 64)": _item(1 << 31, 64),
    }
    bad["the NVFP4 weight_packed is not 16-byte aligned"].packed_in += 8
    bad["the MXFP4 weight_packed is not 16-byte aligned"].packed_out += 8
    bad["the NVFP4 weight_scale is not 2-byte aligned"].scale_f8 += 1
    bad["weight_global_scale is not 4-byte aligned"].global_scale += 2
    for pad, field in enumerate(("packed_in", "scale_f8", "global_scale", "packed_out", "e8m0")):
        setattr(bad["has a NULL pointer" + " " * pad], field, None)
    for why, it in bad.items():
        ret, table = _plan([_item(64, 64), it, _item(64, 64)])
        assert ret == -1, why
        assert lib.last_error().startswith(f"{PLAN}: item 1") and why.strip() in lib.last_error(), (why, lib.last_error())
        assert table[2].first_block == -7  # the loop stopped at the refused item
    # what the plan does admit: an even scale address, a global scale at any multiple of four
    ok = _item(64, 64)
    ok.scale_f8 += 2
    ok.global_scale += 4
    assert _plan([ok])[0] == 1


def test_plan_of_empty_null_negative_and_oversized_tables(lib):
    plan = getattr(lib.load(), PLAN)
    ret, table = _plan([_item(64, 64)], n=0)
    assert ret == 0 and table[0].first_block == -7  # n = 0: nothing is read or written
    assert plan(None, 0) == 0
    assert plan(None, 1) == -1 and lib.last_error() == f"{PLAN}: bad arguments"
    assert _plan([_item(64, 64)], n=-1)[0] == -1 and lib.last_error() == f"{PLAN}: bad arguments"
    # a table past the launch cap: 2^31 workgroups or more are refused, one short of it is admitted
    rows = (1 << 31) - 1
    cap = _item(rows, 32 * GPB)
    assert _plan([cap])[0] == rows
    assert _plan([cap, _item(1, 32)])[0] == -1 and "workgroups exceed one launch; split the batch" in lib.last_error()
    # the launch: an empty table returns before anything is launched, a bad size or a NULL table is refused
    batch = lib.load().ct_nvfp4_mxfp4_batch
    assert batch(None, 0, 0, None) == 0 and batch(None, 1, 0, None) == 0
    assert batch(None, 1, 1 << 31, None) != 0 and batch(None, -1, 1, None) != 0
    assert batch(None, 1, 1, None) != 0 and "table is NULL" in lib.last_error()


def test_python_never_hands_the_plan_a_row_it_would_refuse(lib):
    from compressed_tensors_amd.entrypoints.convert import nvfp4_mxfp4 as nm

    class T:  # what `_fused_admits` reads of a tensor
        def __init__(self, ptr, shape=(200, 160), dtype=torch.float32):
            self.ptr, self.shape, self.dtype = ptr, shape, dtype

        def data_ptr(self):
            return self.ptr

    for pi, sc, gs, po in ((0x1000, 0x2000, 0x3000, 0x4000), (0x1008, 0x2000, 0x3000, 0x4000), (0x1000, 0x2001, 0x3000, 0x4000), (0x1000, 0x2002, 0x3000, 0x4000),
                           (0x1000, 0x2000, 0x3002, 0x4000), (0x1000, 0x2000, 0x3004, 0x4000), (0x1000, 0x2000, 0x3000, 0x4008), (0x1004, 0x2000, 0x3000, 0x4000)):
        it = _item(200, 320)
        it.packed_in, it.scale_f8, it.global_scale, it.packed_out = pi, sc, gs, po
        assert nm._fused_admits(T(pi), T(sc), T(gs), T(po)) == (_plan([it])[0] >= 0), (pi, sc, gs, po)
    # a global scale that is not float32 is the composition's, whatever its address
    assert not nm._fused_admits(T(0x1000), T(0x2000), T(0x3000, dtype=torch.bfloat16), T(0x4000))
    assert not nm._fused_admits(T(0x1000, shape=(1 << 31, 160)), T(0x2000), T(0x3000), T(0x4000))


# ------------------------------------------------------------------------------------------------------------------- the converter
def _names(*names):
    return dict.fromkeys(names)


def _no_device(monkeypatch):
    from compressed_tensors_amd import _lib

    def no_device():
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(_lib, "require_device", no_device)


def _stub_transcode(monkeypatch, seen):
    """`transcode` without a device: records its modules and fills the places `process` left"""
    from compressed_tensors_amd.entrypoints.convert import nvfp4_mxfp4 as nm

    def stub(out, modules, triples, dev, fused, to_host=True, stream_results=False):
        seen.append((list(modules), fused))
        for m, (p, s, g) in zip(modules, triples):
            assert p.dtype == torch.uint8 and s.dtype == C.F8 and g.numel() == 1
            out[f"{m}.weight_packed"] = torch.zeros_like(p)
            out[f"{m}.weight_scale"] = torch.zeros(p.shape[0], p.shape[1] // 16, dtype=torch.uint8)

    monkeypatch.setattr(nm, "transcode", stub)
    monkeypatch.setattr(nm._lib, "require_device", lambda: torch.device("cpu"))


def test_the_class_and_the_codec_entry_are_exported():
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.entrypoints import convert
    from compressed_tensors_amd.entrypoints.convert import Converter, NVFP4ToMXFP4Converter, nvfp4_mxfp4

    assert "NVFP4ToMXFP4Converter" in convert.__all__ and issubclass(NVFP4ToMXFP4Converter, Converter)
    assert callable(codec.nvfp4_to_mxfp4) and "nvfp4_to_mxfp4" in codec.__all__
    assert NVFP4ToMXFP4Converter.format == "mxfp4-pack-quantized" and isinstance(nvfp4_mxfp4.NVFP4_MXFP4_MEASURED_FASTER, bool)
    with pytest.raises(ValueError, match="source must be one of"):
        NVFP4ToMXFP4Converter(source="awq")


def test_process_replaces_the_packed_weight_in_place_and_drops_the_global_scales(monkeypatch):
    from compressed_tensors_amd.entrypoints.convert import NVFP4ToMXFP4Converter

    seen = []
    _stub_transcode(monkeypatch, seen)
    p, s, g = C.inputs("r3x32")
    norm, head = torch.ones(4), torch.zeros(2, 16, dtype=torch.uint8)
    shard = {"m.norm.weight": norm, "m.q_proj.weight_scale": s, "m.q_proj.weight_packed": p, "m.q_proj.input_global_scale": g.clone(),
             "m.q_proj.weight_global_scale": g, "m.q_proj.bias": norm, "lm_head.weight_packed": head, "lm_head.weight_scale": s,
             "lm_head.weight_global_scale": g, "lm_head.input_global_scale": g, "m.k_proj.input_global_scale": g,
             "m.k_proj.weight_packed": p, "m.k_proj.weight_global_scale": g, "m.k_proj.weight_scale": s}
    out = NVFP4ToMXFP4Converter(ignore=["lm_head"], targets=TARGETS, fused=True).process(dict(shard))
    assert seen == [(["m.q_proj", "m.k_proj"], True)]
    assert list(out) == ["m.norm.weight", "m.q_proj.weight_packed", "m.q_proj.weight_scale", "m.q_proj.bias", "lm_head.weight_packed", "lm_head.weight_scale",
                         "lm_head.weight_global_scale", "lm_head.input_global_scale", "m.k_proj.weight_packed", "m.k_proj.weight_scale"]
    assert out["m.norm.weight"] is norm and out["lm_head.weight_packed"] is head and out["lm_head.weight_global_scale"] is g
    assert out["m.q_proj.weight_scale"].dtype == torch.uint8 and tuple(out["m.q_proj.weight_scale"].shape) == (3, 1)
    # nothing targeted: nothing is staged, everything passes through
    seen.clear()
    plain = {"m.norm.weight": norm, "lm_head.weight_packed": head}
    out = NVFP4ToMXFP4Converter(ignore=["lm_head"], targets=TARGETS).process(dict(plain))
    assert seen == [] and list(out) == list(plain) and all(out[k] is plain[k] for k in plain)


def test_process_of_a_modelopt_shard_goes_through_the_modelopt_converter_first(monkeypatch):
    from compressed_tensors_amd.entrypoints.convert import ModelOptNvfp4Converter, NVFP4ToMXFP4Converter
    from compressed_tensors_amd.quantization.quant_args import QuantizationArgs

    seen = []
    _stub_transcode(monkeypatch, seen)
    p, s, _ = C.inputs("r3x32")
    kv = QuantizationArgs(num_bits=8, type="float", strategy="tensor")
    shard = {"m.k_proj.weight": p, "m.k_proj.weight_scale": s, "m.k_proj.weight_scale_2": torch.tensor([0.5]), "m.k_proj.input_scale": torch.tensor([0.25]),
             "m.k_proj.k_scale": torch.tensor([2.0]), "m.norm.weight": torch.ones(4)}
    given = dict(shard)
    out = NVFP4ToMXFP4Converter(targets=TARGETS, source="modelopt", kv_cache_scheme=kv).process(given)
    assert list(given) == list(shard)  # the caller's dict is left alone
    renamed = ModelOptNvfp4Converter(targets=TARGETS, kv_cache_scheme=kv).process(dict(shard))
    assert list(renamed) == ["m.k_proj.weight_scale", "m.k_proj.k_scale", "m.norm.weight", "m.k_proj.weight_packed", "m.k_proj.weight_global_scale",
                             "m.k_proj.input_global_scale"]
    assert list(out) == ["m.k_proj.k_scale", "m.norm.weight", "m.k_proj.weight_packed", "m.k_proj.weight_scale"]
    assert out["m.k_proj.k_scale"].dtype == torch.bfloat16 and out["m.norm.weight"] is shard["m.norm.weight"]
    assert seen == [(["m.k_proj"], False)]  # (the flag is False until the measurement says otherwise; see the flag's comment)


def test_every_refusal_comes_before_a_device_is_asked_for(monkeypatch):
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.entrypoints.convert import NVFP4ToMXFP4Converter

    _no_device(monkeypatch)
    p, s, g = C.inputs("r3x32")
    conv = NVFP4ToMXFP4Converter(targets=TARGETS, fused=True)
    good = {"a.q_proj.weight_packed": p, "a.q_proj.weight_scale": s, "a.q_proj.weight_global_scale": g}

    def shard(**changes):
        sd = dict(good)
        for k, v in changes.items():
            key = f"b.q_proj.{k}"
            if v is not None:
                sd[key] = v
        return sd

    full = dict(weight_packed=p, weight_scale=s, weight_global_scale=g)
    with pytest.raises(ValueError, match="Found weight_packed without corresponding weight_scale b.q_proj.weight_packed"):
        conv.process(shard(**dict(full, weight_scale=None)))
    with pytest.raises(ValueError, match="Found weight_packed without corresponding weight_global_scale b.q_proj.weight_packed"):
        conv.process(shard(**dict(full, weight_global_scale=None)))
    with pytest.raises(ValueError, match="b.q_proj: weight_packed: expected a 2-D uint8 tensor"):
        conv.process(shard(**dict(full, weight_packed=p.view(torch.int8))))
    with pytest.raises(ValueError, match="b.q_proj: weight_packed: expected a 2-D uint8 tensor"):
        conv.process(shard(**dict(full, weight_packed=p.reshape(-1))))
    with pytest.raises(ValueError, match="b.q_proj: weight_scale: expected a 2-D float8_e4m3fn tensor"):
        conv.process(shard(**dict(full, weight_scale=s.view(torch.uint8))))
    with pytest.raises(ValueError, match=r"b.q_proj: weight_scale of shape \(3, 1\) for a weight_packed of shape \(3, 16\)"):
        conv.process(shard(**dict(full, weight_scale=s[:, :1])))
    with pytest.raises(ValueError, match=r"b.q_proj: weight_scale of shape \(3, 2\) for a weight_packed of shape \(3, 20\)"):
        conv.process(shard(**dict(full, weight_packed=torch.zeros(3, 20, dtype=torch.uint8))))  # 40 columns: no whole NVFP4 groups
    with pytest.raises(ValueError, match="b.q_proj: weight_global_scale: expected one floating-point element"):
        conv.process(shard(**dict(full, weight_global_scale=torch.ones(2))))
    with pytest.raises(ValueError, match="b.q_proj: weight_global_scale: expected one floating-point element"):
        conv.process(shard(**dict(full, weight_global_scale=torch.ones(1, dtype=torch.int32))))
    # 48 columns: legal NVFP4 (three groups of 16), no whole MX group — the reference's GROUP-strategy text
    text = "tensor column shape must be divisble by the given group_size 32 but got 48"
    p48, s48 = C.synth_nibbles(4, 48, 1), C.finite_scales(C.synth_scale_bytes(4, 48, 1)).view(C.F8)
    with pytest.raises(ValueError, match="b.q_proj: " + text):
        conv.process(shard(weight_packed=p48, weight_scale=s48, weight_global_scale=g))
    with pytest.raises(ValueError, match="b.q_proj: " + text):
        NVFP4ToMXFP4Converter(targets=TARGETS, source="modelopt").process(
            {"b.q_proj.weight": p48, "b.q_proj.weight_scale": s48, "b.q_proj.weight_scale_2": torch.ones(1), "b.q_proj.input_scale": torch.ones(1)})
    with pytest.raises(ValueError, match="^" + text):
        codec.nvfp4_to_mxfp4(p48, s48, g)
    with pytest.raises(ValueError, match="^weight_packed: expected a 2-D uint8 tensor"):
        codec.nvfp4_to_mxfp4(p.float(), s, g)
    with pytest.raises(ValueError, match="^weight_scale: expected a 2-D float8_e4m3fn tensor"):
        codec.nvfp4_to_mxfp4(p, s.float(), g)
    with pytest.raises(ValueError, match="^weight_global_scale: expected one floating-point element"):
        codec.nvfp4_to_mxfp4(p, s, None)


def test_validate_and_dependencies_on_names_alone():
    from compressed_tensors_amd.entrypoints.convert import ModelOptNvfp4Converter, NVFP4ToMXFP4Converter
    from compressed_tensors_amd.quantization.quant_args import QuantizationArgs

    conv = NVFP4ToMXFP4Converter(ignore=["re:lm_head.*"], targets=TARGETS)
    module = ("weight_packed", "weight_scale", "weight_global_scale")
    conv.validate(_names(*(f"m.q_proj.{p}" for p in module), "m.q_proj.input_global_scale", *(f"lm_head.{p}" for p in module), "m.norm.weight",
                         "m.gate.weight_packed", "m.gate.weight_scale"))
    with pytest.raises(ValueError, match="Found weight_packed without corresponding weight_scale m.q_proj.weight_packed"):
        conv.validate(_names("m.q_proj.weight_packed", "m.q_proj.weight_global_scale"))
    with pytest.raises(ValueError, match="Found weight_packed without corresponding weight_global_scale m.q_proj.weight_packed"):
        conv.validate(_names("m.q_proj.weight_packed", "m.q_proj.weight_scale"))
    with pytest.raises(ValueError, match="Found unexpected non-targeted tensor m.gate.weight_global_scale"):
        conv.validate(_names(*(f"m.gate.{p}" for p in module)))
    assert conv.get_dependencies("m.q_proj.weight_packed") == {"m.q_proj.weight_scale", "m.q_proj.weight_global_scale"}
    assert conv.get_dependencies("m.q_proj.weight_scale") == set() and conv.get_dependencies("m.q_proj.input_global_scale") == set()
    assert conv.get_dependencies("lm_head.weight_packed") == set() and conv.get_dependencies("m.norm.weight") == set()
    assert conv.param_names == ["weight_packed", "weight_scale", "weight_global_scale", "input_global_scale"] and conv.stream_results is False

    # ModelOpt's names: what ModelOptNvfp4Converter answers
    kv = QuantizationArgs(num_bits=8, type="float", strategy="tensor")
    mo, ref = NVFP4ToMXFP4Converter(targets=TARGETS, source="modelopt", kv_cache_scheme=kv), ModelOptNvfp4Converter(targets=TARGETS, kv_cache_scheme=kv)
    assert mo.param_names == ref.param_names
    for name in ("m.k_proj.weight", "m.v_proj.weight", "m.q_proj.weight", "m.q_proj.weight_scale", "m.norm.weight"):
        assert mo.get_dependencies(name) == ref.get_dependencies(name), name
    assert mo.get_dependencies("m.k_proj.weight") == {"m.k_proj.input_scale", "m.k_proj.weight_scale", "m.k_proj.weight_scale_2", "m.k_proj.k_scale"}
    mo.validate(_names("m.q_proj.weight", "m.q_proj.weight_scale", "m.q_proj.weight_scale_2", "m.q_proj.input_scale", "m.norm.weight"))
    with pytest.raises(ValueError, match="Hit unexpected non-targeted tensor m.gate.weight_scale_2"):
        mo.validate(_names("m.gate.weight", "m.gate.weight_scale_2"))


def test_fused_follows_the_measured_flag_unless_forced(monkeypatch):
    from compressed_tensors_amd.entrypoints.convert import nvfp4_mxfp4 as nm

    for flag in (True, False):
        monkeypatch.setattr(nm, "NVFP4_MXFP4_MEASURED_FASTER", flag)
        assert nm.NVFP4ToMXFP4Converter()._fused() is flag
        assert nm.NVFP4ToMXFP4Converter(fused=True)._fused() is True and nm.NVFP4ToMXFP4Converter(fused=False)._fused() is False


@pytest.mark.parametrize("activations, preset", [(False, "MXFP4A16"), (True, "MXFP4")])
def test_create_config_is_the_reference_preset(activations, preset):
    from compressed_tensors_amd.entrypoints.convert import ModelOptNvfp4Converter, MXFP4Quantizer, NVFP4ToMXFP4Converter
    from compressed_tensors_amd.quantization.quant_args import QuantizationArgs

    want = C.load_fixture()["presets"][preset]
    assert (want["input_activations"] is not None) == activations
    shape = MXFP4Quantizer(["lm_head"], TARGETS, activations=activations).create_config().model_dump()
    kv = QuantizationArgs(num_bits=8, type="float", strategy="tensor")
    for source in ("compressed-tensors", "modelopt"):
        cfg = NVFP4ToMXFP4Converter(["lm_head"], TARGETS, activations, source=source).create_config().model_dump()
        assert cfg == shape  # the dense-checkpoint quantizer's config, key for key
        group = cfg["config_groups"]["config_group_0"]
        assert group["weights"] == want["weights"] and group["input_activations"] == want["input_activations"]
        assert cfg["format"] == group["format"] == "mxfp4-pack-quantized" and group["targets"] == TARGETS and cfg["ignore"] == ["lm_head"]
        assert cfg["kv_cache_scheme"] is None
        with_kv = NVFP4ToMXFP4Converter(["lm_head"], TARGETS, activations, source=source, kv_cache_scheme=kv).create_config().model_dump()
        assert with_kv["kv_cache_scheme"] == ModelOptNvfp4Converter(kv_cache_scheme=kv).create_config().model_dump()["kv_cache_scheme"]
        assert with_kv["kv_cache_scheme"]["num_bits"] == 8 and {k: v for k, v in with_kv.items() if k != "kv_cache_scheme"} == {
            k: v for k, v in shape.items() if k != "kv_cache_scheme"}


def test_the_fixture_is_complete_and_small():
    fixture = C.load_fixture()
    keys = list(C.CASES) + [C.sweep_key(layout, name) for layout in C.SWEEP_LAYOUTS for name in C.GOLDEN_SCALES]
    assert sorted(fixture["outputs"]) == sorted(f"{k}.{name}" for k in keys for name in ("packed", "e8m0"))
    assert fixture["groups_per_block"] == GPB and os.path.getsize(C.FIXTURE) < (512 << 10)
    assert all(("base64" in rec) == rec["whole"] == (rec["shape"][0] * rec["shape"][1] <= C.WHOLE_MAX) for rec in fixture["outputs"].values())
    assert not fixture["outputs"]["kv_a_576x7168.packed"]["whole"] and fixture["outputs"]["sweep_first.gs_1.packed"]["whole"]
    # no golden input holds a NaN scale byte or a degenerate global scale; the sweep's rows hold every scale byte in both roles and all 16 codes per group
    for key, (p, s, g) in C.golden_inputs().items():
        assert not bool(((s.view(torch.uint8) & 0x7F) == 0x7F).any()) and bool(torch.isfinite(g).all()) and float(g) != 0.0, key
    assert set(C.SWEEP_SCALES) - set(C.GOLDEN_SCALES) == {"0", "-1", "inf"}
    for layout, own in (("first", 0), ("second", 1)):
        p, s, _ = C.sweep_inputs(layout, "1")
        b = s.view(torch.uint8)
        assert b[:, own].tolist() == list(range(256)) and b[:, own + 2].tolist() == list(range(256))
        assert {0x7F, 0xFF} <= set(b[:, 1 - own].tolist()) | set(b[:, own].tolist())
        codes = torch.stack([p & 0xF, p >> 4], dim=-1).reshape(256, 4, 16)
        assert bool((codes.sort(dim=-1).values == torch.arange(16, dtype=torch.uint8)).all())
