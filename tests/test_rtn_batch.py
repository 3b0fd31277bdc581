"""Host side of the table form of the one-pass round-to-nearest compress (ct_rtn_quant_pack_w4_batch / ct_rtn_mxfp4_quant_pack_batch): the C ABI's
symbols and planners, and the grouping compress_model_rtn(batched=True) does.  No GPU: the planners are host functions, the launches are replaced."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ct_rtn_w4_batch_plan", "ct_rtn_quant_pack_w4_batch", "ct_rtn_mxfp4_batch_plan", "ct_rtn_mxfp4_quant_pack_batch")
# (rows, cols, group; 0 = one group per row): the table of tests/test_gpu_rtn_batch.py
ITEMS = [(5, 256, 32), (8, 512, 128), (3, 2048, 0), (16, 64, 64), (64, 4096, 128), (7, 1024, 0), (1, 32, 32)]


@pytest.fixture(scope="module")
def lib():
    from compressed_tensors_amd import _lib

    return _lib.load()


def table(items, mx=False):
    """a host table with made-up, 16-byte aligned addresses: the planners look at pointers, they never follow them"""
    from compressed_tensors_amd import _lib

    tab = (_lib.W4Item * len(items))()
    for i, (rows, cols, group) in enumerate(items):
        it = tab[i]
        it.src, it.dst, it.rows, it.cols, it.group = 0x10000 * (i + 1), 0x10000 * (i + 1) + 0x8000, rows, cols, group
        if mx:
            it.zp_packed = 0x10000 * (i + 1) + 0x4000
        else:
            it.scale, it.zp = 0x10000 * (i + 1) + 0x4000, 0x10000 * (i + 1) + 0x6000
    return tab


def plan(lib, name, tab):
    return int(getattr(lib, name)(ctypes.cast(tab, ctypes.c_void_p), len(tab)))


def test_symbols_exported_declared_and_prototyped(lib):
    from compressed_tensors_amd import _lib

    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ct_hip.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NEW:
        assert name in exported and name in _lib._PROTOTYPES and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"int64_t\s+ct_rtn_w4_batch_plan\(ct_w4_item\* items_host, int n\);", header)
    assert re.search(r"int\s+ct_rtn_quant_pack_w4_batch\(const ct_w4_item\* items_dev, int n, int64_t total_blocks, int dt, int symmetric, ct_stream_t stream\);", header)
    assert re.search(r"int64_t\s+ct_rtn_mxfp4_batch_plan\(ct_w4_item\* items_host, int n\);", header)
    assert re.search(r"int\s+ct_rtn_mxfp4_quant_pack_batch\(const ct_w4_item\* items_dev, int n, int64_t total_blocks, int xdt, ct_stream_t stream\);", header)
    assert lib.ct_abi_version() == 2 and ctypes.sizeof(_lib.W4Item) == 13 * 8
    from compressed_tensors_amd import codec

    for name in ("rtn_quantize_and_pack_many", "rtn_mxfp4_quantize_and_pack_many", "launch_rtn_w4_words", "launch_rtn_mxfp4_words"):
        assert callable(getattr(codec, name)) and name in codec.__all__


def test_w4_plan_fills_the_derived_fields(lib):
    tab = table(ITEMS)
    want = sum(-(-(rows * cols // 32) // 256) for rows, cols, _ in ITEMS)
    assert plan(lib, "ct_rtn_w4_batch_plan", tab) == want == 38
    first = 0
    for it, (rows, cols, group) in zip(tab, ITEMS):
        g = group or cols
        assert it.first_block == first and it.units == rows * cols // 8 and it.upg == g // 8 and 1 << it.upg_shift == g // 8
        assert it.main_blocks == -(-(rows * cols // 32) // 256) and 1 <= 1 << (it.upg_shift - 2) <= 64
        first += it.main_blocks
    assert [it.first_block for it in tab] == sorted(it.first_block for it in tab)
    assert plan(lib, "ct_rtn_w4_batch_plan", table([])) == 0
    sym = table(ITEMS)
    for it in sym:
        it.zp = None  # a symmetric table may leave the zero-point output out
    assert plan(lib, "ct_rtn_w4_batch_plan", sym) == want


def test_mxfp4_plan_fills_the_derived_fields(lib):
    items = [(4, 64, 32), (5, 96, 32), (64, 4096, 32), (1, 32, 32)]
    tab = table(items, mx=True)
    assert plan(lib, "ct_rtn_mxfp4_batch_plan", tab) == 1 + 1 + 32 + 1
    assert [it.first_block for it in tab] == [0, 1, 2, 34] and all(it.units == r * c // 8 and it.upg_shift == 2 for it, (r, c, _) in zip(tab, items))


@pytest.mark.parametrize("what", ["group48", "cols_not_multiple", "misaligned_src", "misaligned_dst", "zp_packed", "no_scale", "group4096"])
def test_w4_plan_refuses(lib, what):
    from compressed_tensors_amd import _lib

    items = list(ITEMS)
    if what == "group48":
        items[2] = (8, 96, 48)
    elif what == "cols_not_multiple":
        items[2] = (8, 160, 64)
    elif what == "group4096":
        items[2] = (2, 4096, 0)
    tab = table(items)
    if what == "misaligned_src":
        tab[2].src += 8
    elif what == "misaligned_dst":
        tab[2].dst += 4
    elif what == "zp_packed":
        tab[2].zp_packed = 0x7000
    elif what == "no_scale":
        tab[2].scale = None
    assert plan(lib, "ct_rtn_w4_batch_plan", tab) == -1
    msg = _lib.last_error()
    assert "ct_rtn_w4_batch_plan" in msg and "item 2" in msg, msg


@pytest.mark.parametrize("what", ["group16", "group64", "cols48", "misaligned_src", "no_codes"])
def test_mxfp4_plan_refuses(lib, what):
    from compressed_tensors_amd import _lib

    items = [(4, 64, 32), (5, 96, 32), (8, 128, 32)]
    if what in ("group16", "group64"):
        items[1] = (5, 128, 16 if what == "group16" else 64)
    elif what == "cols48":
        items[1] = (4, 48, 32)
    tab = table(items, mx=True)
    if what == "misaligned_src":
        tab[1].src += 2
    elif what == "no_codes":
        tab[1].zp_packed = None
    assert plan(lib, "ct_rtn_mxfp4_batch_plan", tab) == -1
    msg = _lib.last_error()
    assert "ct_rtn_mxfp4_batch_plan" in msg and "item 1" in msg, msg


def test_plans_refuse_two_to_the_31_workgroups(lib):
    from compressed_tensors_amd import _lib

    big = [(1 << 24, 1 << 20, 128)]  # 2^39 lanes of 32 elements / 256 = 2^31 workgroups
    assert plan(lib, "ct_rtn_w4_batch_plan", table(big)) == -1 and "exceed one launch" in _lib.last_error()
    assert plan(lib, "ct_rtn_mxfp4_batch_plan", table([(r, c, 32) for r, c, _ in big], mx=True)) == -1 and "exceed one launch" in _lib.last_error()


def test_many_on_cpu_tensors_behaves_like_the_single_call():
    """a CPU weight is not a table item: it takes the single-tensor function, which stages it onto the GPU — or raises where there is none"""
    from compressed_tensors_amd import codec

    w = torch.randn(8, 256).to(torch.bfloat16)
    pairs = ((lambda: [codec.rtn_quantize_and_pack(w, group_size=128)] * 2, lambda: codec.rtn_quantize_and_pack_many([w, w], group_size=128)),
             (lambda: [codec.rtn_mxfp4_quantize_and_pack(w)] * 2, lambda: codec.rtn_mxfp4_quantize_and_pack_many([w, w])))
    for single, many in pairs:
        if torch.cuda.is_available():
            for a, b in zip(single(), many()):
                assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) and not y.is_cuda for x, y in zip(a, b))
            continue
        with pytest.raises(RuntimeError) as e1:
            single()
        with pytest.raises(RuntimeError) as e2:
            many()
        assert str(e1.value) == str(e2.value)
    with pytest.raises(ValueError):
        codec.rtn_quantize_and_pack_many([w, w], group_size=[128])
    assert codec.rtn_quantize_and_pack_many([]) == [] and codec.rtn_mxfp4_quantize_and_pack_many([]) == []


def test_compress_model_rtn_groups_by_compressor_in_module_order(monkeypatch):
    """compress_model_rtn(batched=True) hands each compressor class with a `compress_rtn_modules` whose gate holds ONE list, in module order; NVFP4
    (its gate is off) and the 8-bit codecs (they have no hook) go through `compress_rtn` per module; batched=False calls `compress_rtn` for every
    module and no table entry"""
    import compressed_tensors_amd as cta
    from compressed_tensors_amd.compressors.base import BaseCompressor

    def scheme(act=None, **kw):
        return cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(**kw), input_activations=act)

    w4, w4a = scheme(num_bits=4, group_size=128, symmetric=True), scheme(num_bits=4, group_size=128, symmetric=False)
    mx = scheme(num_bits=4, type="float", strategy="group", group_size=32, scale_dtype=torch.uint8)
    nv = scheme(num_bits=4, type="float", strategy="tensor_group", group_size=16, scale_dtype=torch.float8_e4m3fn)
    f8 = scheme(act=cta.QuantizationArgs(num_bits=8, type="float", strategy="tensor"), num_bits=8, type="float", strategy="channel")
    i8 = scheme(act=cta.QuantizationArgs(num_bits=8, strategy="tensor"), num_bits=8, strategy="channel")
    order = [w4, mx, nv, w4a, f8, mx, w4, i8]

    def build():
        model = torch.nn.Sequential(*[torch.nn.Linear(128, 128, bias=False) for _ in order]).to(torch.bfloat16)
        for m, s in zip(model, order):
            m.quantization_scheme = s
        return model

    names = ("pack-quantized", "mxfp4-pack-quantized", "nvfp4-pack-quantized", "float-quantized", "int-quantized", "naive-quantized")
    classes = {n: BaseCompressor.get_value_from_registry(n) for n in names}
    assert hasattr(classes["pack-quantized"], "compress_rtn_modules") and hasattr(classes["mxfp4-pack-quantized"], "compress_rtn_modules")
    assert not any(hasattr(classes[n], "compress_rtn_modules") for n in names[3:])
    assert "compress_rtn_modules" in vars(classes["nvfp4-pack-quantized"]) and classes["nvfp4-pack-quantized"].RTN_TABLE_MEASURED_FASTER is False
    calls = []
    for n, c in classes.items():
        if "compress_rtn_modules" in vars(c):
            monkeypatch.setattr(c, "compress_rtn_modules", classmethod(lambda cls, ms, _n=n: calls.append(("many", cls, list(ms)))))
        if "compress_rtn" in vars(c):
            monkeypatch.setattr(c, "compress_rtn", classmethod(lambda cls, w, s, _n=n: calls.append(("one", cls, w)) or {"weight": w}))

    model = build()
    cta.ModelCompressor().compress_model_rtn(model)
    many = {c: ms for k, c, ms in calls if k == "many"}
    assert list(many) == [classes["pack-quantized"], classes["mxfp4-pack-quantized"]] and len(calls) == 2 + 3
    assert [id(m) for m in many[classes["pack-quantized"]]] == [id(model[i]) for i in (0, 3, 6)]
    assert [id(m) for m in many[classes["mxfp4-pack-quantized"]]] == [id(model[i]) for i in (1, 5)]
    ones = [(c, w) for k, c, w in calls if k == "one"]
    assert [c for c, _ in ones] == [classes["nvfp4-pack-quantized"], classes["float-quantized"], classes["int-quantized"]]
    assert [w.data_ptr() for _, w in ones] == [model[i].weight.data_ptr() for i in (2, 4, 7)]
    assert [m.quantization_scheme.format.value for m in model] == ["pack-quantized", "mxfp4-pack-quantized", "nvfp4-pack-quantized", "pack-quantized",
                                                                   "float-quantized", "mxfp4-pack-quantized", "pack-quantized", "int-quantized"]

    calls.clear()
    model = build()
    cta.ModelCompressor().compress_model_rtn(model, batched=False)
    assert [k for k, _, _ in calls] == ["one"] * len(order)
    assert [w.data_ptr() for _, _, w in calls] == [m.weight.data_ptr() for m in model]
