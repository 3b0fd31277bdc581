"""Host side of NVFP4 from a dense model: the table form of the one-pass round-to-nearest compress (ct_rtn_nvfp4_batch_plan / ct_rtn_nvfp4_amax_batch /
ct_rtn_nvfp4_quant_pack_batch) — symbols, planner, the window hook's grouping — and the calibrated global scale (MinMaxObserver.get_global_scale,
modeling.calibrate_global_scales).  No GPU: the planner is a host function, the launches are replaced."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ct_rtn_nvfp4_batch_plan", "ct_rtn_nvfp4_amax_batch", "ct_rtn_nvfp4_quant_pack_batch")
# (rows, cols): the table of tests/test_gpu_nvfp4_rtn_table.py
ITEMS = [(1, 32), (5, 96), (3, 64), (64, 4096), (7, 1024), (2, 32)]
BF16, F16, F32, F8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn


@pytest.fixture(scope="module")
def lib():
    from compressed_tensors_amd import _lib

    return _lib.load()


def table(items):
    """a host table with made-up, aligned addresses: the planner looks at pointers, it never follows them"""
    from compressed_tensors_amd import _lib

    tab = (_lib.W4Item * max(len(items), 1))()
    for i, (rows, cols) in enumerate(items):
        it, base = tab[i], 0x10000 * (i + 1)
        it.src, it.dst, it.zp_packed, it.zp, it.scale = base, base + 0x8000, base + 0x4000, 0x1000 + 4 * i, base + 0x6000
        it.rows, it.cols, it.group = rows, cols, 16
    return tab


def plan(lib, tab, n=None):
    return int(lib.ct_rtn_nvfp4_batch_plan(ctypes.cast(tab, ctypes.c_void_p), len(tab) if n is None else n))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_prototyped(lib):
    from compressed_tensors_amd import _lib, codec, modeling
    from compressed_tensors_amd.quantization import MinMaxObserver

    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ct_hip.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NEW:
        assert name in exported and name in _lib._PROTOTYPES and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"int64_t\s+ct_rtn_nvfp4_batch_plan\(ct_w4_item\* items_host, int n\);", header)
    for name in NEW[1:]:
        assert re.search(rf"int\s+{name}\(const ct_w4_item\* items_dev, int n, int64_t total_blocks, int xdt, ct_stream_t stream\);", header)
        assert len(_lib._PROTOTYPES[name][0]) == 5
    assert lib.ct_abi_version() == 2 and ctypes.sizeof(_lib.W4Item) == 13 * 8  # additive: nothing an existing caller sees moved
    for name in ("rtn_nvfp4_quantize_and_pack_many", "launch_rtn_nvfp4_words", "rtn_nvfp4_table_item", "attn_observe_global_scale"):
        assert callable(getattr(codec, name)) and name in codec.__all__
    assert callable(MinMaxObserver.get_global_scale)
    assert callable(modeling.calibrate_global_scales) and "calibrate_global_scales" in modeling.__all__
    # one shared device function carries generate_gparam's arithmetic for the three kernels that need it
    csrc = os.path.join(ROOT, "compressed_tensors_amd", "csrc")
    assert "float gparam_from_amax(float amax)" in open(os.path.join(csrc, "ct_minmax.h")).read()
    for src in ("ct_qparams.hip", "ct_fp4.hip", "ct_attn_observe.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert "gparam_from_amax<" in text and "2688" not in text, src


def test_plan_fills_the_derived_fields(lib):
    tab = table(ITEMS)
    want = [-(-(rows * cols // 32) // 256) for rows, cols in ITEMS]
    assert want == [1, 1, 1, 32, 1, 1] and plan(lib, tab) == sum(want)
    first = 0
    for it, (rows, cols), blocks in zip(tab, ITEMS, want):
        assert it.first_block == first and it.units == rows * cols // 8 and it.upg == 2 and it.upg_shift == 1 and it.main_blocks == blocks
        first += blocks
    assert plan(lib, table([(300, 4096)])) == 150


@pytest.mark.parametrize("what", ["cols48", "cols16", "group32", "misaligned_src", "misaligned_dst", "misaligned_key", "no_key", "no_global_scale", "no_scales",
                                  "no_rows"])
def test_plan_refuses(lib, what):
    from compressed_tensors_amd import _lib

    items = [(4, 64), (5, 96), (8, 128)]
    if what in ("cols48", "cols16"):
        items[1] = (4, 48 if what == "cols48" else 16)  # whole groups of 16, but a lane is two of them
    elif what == "no_rows":
        items[1] = (0, 64)
    tab = table(items)
    if what == "group32":
        tab[1].group = 32
    elif what == "misaligned_src":
        tab[1].src += 8
    elif what == "misaligned_dst":
        tab[1].dst += 4
    elif what == "misaligned_key":
        tab[1].zp += 2
    elif what == "no_key":
        tab[1].zp = None
    elif what == "no_global_scale":
        tab[1].scale = None
    elif what == "no_scales":
        tab[1].zp_packed = None
    assert plan(lib, tab) == -1
    msg = _lib.last_error()
    assert "ct_rtn_nvfp4_batch_plan" in msg and "item 1" in msg, msg


def test_plan_refuses_an_empty_table_and_two_to_the_31_workgroups(lib):
    from compressed_tensors_amd import _lib

    for n in (0, -1):
        assert plan(lib, table(ITEMS), n) == -1 and "ct_rtn_nvfp4_batch_plan" in _lib.last_error() and "bad arguments" in _lib.last_error()
    assert int(lib.ct_rtn_nvfp4_batch_plan(None, 1)) == -1 and "bad arguments" in _lib.last_error()
    assert plan(lib, table([(1 << 24, 1 << 20)])) == -1 and "exceed one launch" in _lib.last_error()


# ---- codec: one plan, one upload, two launches ----------------------------------------------------------------------------------------
def test_launch_words_plans_once_and_launches_fold_then_quantize(monkeypatch):
    from compressed_tensors_amd import _lib, codec

    assert codec.launch_rtn_nvfp4_words(None, 0, None, torch.device("cpu")) is None  # an empty table: before anything is looked at
    calls = []
    monkeypatch.setattr(codec, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(_lib, "stream_on", lambda device, handle=None: ("stream", device))  # (no GPU here to have a current stream)
    flat = []
    for i, (rows, cols) in enumerate(ITEMS):
        base = 0x10000 * (i + 1)
        flat += codec.item_row(base, base + 0x6000, 0x1000 + 4 * i, base + 0x8000, rows, cols, 16, base + 0x4000)
    cpu = torch.device("cpu")
    tab = codec.launch_rtn_nvfp4_words(flat, len(ITEMS), BF16, cpu)
    assert [name for name, _ in calls] == ["ct_rtn_nvfp4_amax_batch", "ct_rtn_nvfp4_quant_pack_batch"]
    for _, (ptr, n, blocks, xdt, _stream) in calls:
        assert ptr == tab.data_ptr() and n == len(ITEMS) and blocks == 37 and xdt == _lib.BF16
    items = (_lib.W4Item * len(ITEMS)).from_buffer_copy(tab.numpy().tobytes())  # the uploaded table is the planned one
    assert [it.first_block for it in items] == [0, 1, 2, 3, 35, 36] and [it.zp for it in items] == [0x1000 + 4 * i for i in range(len(ITEMS))]
    refused = codec.item_row(0x10000, 0x20000, 0x1000, 0x40000, rows=4, cols=48, group=16, zp_packed=0x30000)
    with pytest.raises(ValueError, match="ct_rtn_nvfp4_batch_plan: item 0"):
        codec.launch_rtn_nvfp4_words(list(refused), 1, BF16, cpu)
    assert len(calls) == 2
    assert codec.rtn_nvfp4_keys(5, cpu).tolist() == [0] * 5 and codec.rtn_nvfp4_keys(5, cpu).dtype == torch.int32


def test_table_item_and_many_leave_cpu_tensors_to_the_single_call():
    from compressed_tensors_amd import codec

    w = torch.randn(8, 256).to(BF16)
    assert not codec.rtn_nvfp4_takes(w) and codec.rtn_nvfp4_table_item(w, 0x1000) is None
    assert codec.rtn_nvfp4_quantize_and_pack_many([]) == []
    if torch.cuda.is_available():
        for a, b in zip([codec.rtn_nvfp4_quantize_and_pack(w)] * 2, codec.rtn_nvfp4_quantize_and_pack_many([w, w])):
            assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) and not y.is_cuda for x, y in zip(a, b))
        return
    with pytest.raises(RuntimeError) as e1:
        codec.rtn_nvfp4_quantize_and_pack(w)
    with pytest.raises(RuntimeError) as e2:
        codec.rtn_nvfp4_quantize_and_pack_many([w, w])
    assert str(e1.value) == str(e2.value)


# ---- the window hook against a recording fake ------------------------------------------------------------------------------------------
class _Fake:
    """stands in for the pieces of the table path that need a GPU: every weight the predicate names is `taken`, tables and keys are recorded"""

    class Recorded:
        def __init__(self, log, what):
            self.log, self.what = log, what

        def data_ptr(self):
            return 0x5000

        def record_stream(self, stream):
            self.log.append(("record", self.what, stream))

    def __init__(self, monkeypatch, takes):
        from compressed_tensors_amd import codec

        self.log, self.single = [], []
        monkeypatch.setattr(codec, "rtn_nvfp4_takes", takes)
        monkeypatch.setattr(codec, "rtn_nvfp4_keys", lambda n, device: self.log.append(("keys", n, device)) or self.Recorded(self.log, "keys"))

        def item(x, key):
            rows, cols = x.shape
            packed, s8, gs = torch.zeros(rows, cols // 2, dtype=torch.uint8), torch.zeros(rows, cols // 16, dtype=F8), torch.full((1,), 2.0)
            return packed, s8, gs, codec.item_row(x.data_ptr(), gs.data_ptr(), key, packed.data_ptr(), rows, cols, 16, s8.data_ptr())

        monkeypatch.setattr(codec, "rtn_nvfp4_table_item", item)

        def launch(flat, n, dtype, device):
            assert len(flat) == n * codec._ITEM_WORDS
            rows = [flat[i * codec._ITEM_WORDS:(i + 1) * codec._ITEM_WORDS] for i in range(n)]
            self.log.append(("launch", n, dtype, device, [tuple(r) for r in rows]))
            return self.Recorded(self.log, "table")

        monkeypatch.setattr(codec, "launch_rtn_nvfp4_words", launch)
        monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: ("stream", device))


def _nv_scheme(**kw):
    import compressed_tensors_amd as cta

    return cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(**dict(dict(num_bits=4, type="float", strategy="tensor_group", group_size=16), **kw)))


def test_window_hook_groups_by_device_and_dtype_and_hands_the_rest_on(monkeypatch):
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import _lib, codec
    from compressed_tensors_amd.compressors.base import RTN_WINDOW

    NV, MX = cta.NVFP4PackedCompressor, cta.MXFP4PackedCompressor
    assert "compress_rtn_modules" in vars(NV) and "compress_rtn_modules" in vars(MX)  # the subclass keeps its own hook and does not inherit this one
    for c in (NV, MX):  # one hook name: nothing else that begins like it
        assert {n for n in dir(c) if n.startswith("compress_rtn")} == {"compress_rtn", "compress_rtn_module", "compress_rtn_modules"}
    fake = _Fake(monkeypatch, lambda x: x.dim() == 2 and x.dtype in (BF16, F16) and x.shape[1] % 32 == 0)
    monkeypatch.setattr(NV, "compress_rtn", classmethod(lambda cls, w, s: fake.single.append(w) or {"weight_packed": w}))
    n = RTN_WINDOW + 2
    model = torch.nn.Sequential(*[torch.nn.Linear(64, 32, bias=(k == 1)) for k in range(n)]).to(BF16)
    model[3] = torch.nn.Linear(48, 32, bias=False).to(BF16)  # cols % 32: not a table item
    model[4] = model[4].to(F16)                              # another dtype: a table of its own
    model[5] = model[5].to(F32)                              # float32: per module
    plain, f8, bf16_scales = _nv_scheme(), _nv_scheme(scale_dtype=F8), _nv_scheme(scale_dtype=BF16)
    for k, m in enumerate(model):
        m.quantization_scheme = bf16_scales if k == 6 else (f8 if k % 2 else plain)  # a non-float8 scale_dtype: per module
    weights = [m.weight.data for m in model]
    bias1 = model[1].bias.data_ptr()
    NV.compress_rtn_modules(list(model))
    # window 0: one table of the bf16 modules, one of the fp16 module; window 1: the last two modules
    launches = [e for e in fake.log if e[0] == "launch"]
    taken0 = [k for k in range(RTN_WINDOW) if k not in (3, 4, 5, 6)]
    assert [(e[1], e[2]) for e in launches] == [(len(taken0), BF16), (1, F16), (2, BF16)]
    assert [e[1] for e in fake.log if e[0] == "keys"] == [RTN_WINDOW, RTN_WINDOW, 2]  # one key buffer per table, sized by its window
    order = [e[0] for e in fake.log]
    assert order == ["keys", "keys", "launch", "record", "record", "launch", "record", "record", "keys", "launch", "record", "record"]
    assert {e[1] for e in fake.log if e[0] == "record"} == {"table", "keys"}
    for rows, ks in zip([e[4] for e in launches], [taken0, [4], [RTN_WINDOW, RTN_WINDOW + 1]]):
        at = {name: getattr(_lib.W4Item, name).offset // 8 for name in ("src", "zp", "group")}
        assert [r[at["src"]] for r in rows] == [weights[k].data_ptr() for k in ks]
        assert [r[at["zp"]] for r in rows] == [0x5000 + 4 * i for i in range(len(ks))] and {r[at["group"]] for r in rows} == {16}  # each item its own key
    # the rest reached compress_rtn, in module order, from this call
    assert [w.data_ptr() for w in fake.single] == [weights[k].data_ptr() for k in (3, 5, 6)]
    for k, m in enumerate(model):
        assert m.quantization_status == cta.QuantizationStatus.COMPRESSED and "weight" not in m._parameters, k
        want = ["weight_packed"] if k in (3, 5, 6) else ["weight_packed", "weight_scale", "weight_global_scale"]
        assert [name for name in m._parameters if name.startswith("weight")] == want, k
    assert model[1].bias.data_ptr() == bias1 and list(model[1]._parameters) == ["bias", "weight_packed", "weight_scale", "weight_global_scale"]
    assert model[0].weight_scale.dtype == F8 and model[0].weight_global_scale.dtype == F32 and not model[0].weight_packed.requires_grad


def test_compress_model_rtn_honours_the_table_hooks_gate(monkeypatch):
    import compressed_tensors_amd as cta

    NV, MX = cta.NVFP4PackedCompressor, cta.MXFP4PackedCompressor
    calls = []
    monkeypatch.setattr(NV, "compress_rtn_modules", classmethod(lambda cls, ms: calls.append(("tables", cls, len(list(ms))))))
    monkeypatch.setattr(MX, "compress_rtn_modules", classmethod(lambda cls, ms: calls.append(("modules", cls, len(list(ms))))))
    for c in (NV, MX):
        monkeypatch.setattr(c, "compress_rtn", classmethod(lambda cls, w, s: calls.append(("one", cls, 1)) or {"weight": w}))
    mx = cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(num_bits=4, type="float", strategy="group", group_size=32, scale_dtype=torch.uint8))
    order = [_nv_scheme(), mx, _nv_scheme(), mx]

    def build():
        model = torch.nn.Sequential(*[torch.nn.Linear(64, 64, bias=False) for _ in order]).to(BF16)
        for m, s in zip(model, order):
            m.quantization_scheme = s
        return model

    monkeypatch.setattr(NV, "RTN_TABLE_MEASURED_FASTER", True)
    cta.ModelCompressor().compress_model_rtn(build())
    assert calls == [("tables", NV, 2), ("modules", MX, 2)]
    calls.clear()
    monkeypatch.setattr(NV, "RTN_TABLE_MEASURED_FASTER", False)  # the dispatch rule declined: per module, and MXFP4 is untouched
    cta.ModelCompressor().compress_model_rtn(build())
    assert calls == [("one", NV, 1), ("one", NV, 1), ("modules", MX, 2)]
    calls.clear()
    cta.ModelCompressor().compress_model_rtn(build(), batched=False)
    assert [c[:2] for c in calls] == [("one", NV), ("one", MX), ("one", NV), ("one", MX)]


# ---- the observer's constructor rules -----------------------------------------------------------------------------------------------------
def _args(**kw):
    import compressed_tensors_amd as cta

    return cta.QuantizationArgs(**dict(dict(num_bits=4, type="float", symmetric=True, strategy="tensor_group", group_size=16, dynamic="local",
                                            observer="static_minmax", scale_dtype=torch.float8_e4m3fn,
                                            zp_dtype=torch.float8_e4m3fn), **kw))


def test_observer_takes_the_presets_activation_arguments(monkeypatch):
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.quantization import MinMaxObserver

    module = torch.nn.Module()
    for base in ("input", "output"):
        obs = MinMaxObserver(base, _args(), module)  # the parent raises NotImplementedError "dynamic" here
        assert obs.keep is True and obs.observer == "static_minmax" and obs.global_only
        with pytest.raises(NotImplementedError, match="dynamic arguments are not observed"):
            obs(torch.zeros(2, 3, 64, dtype=BF16))
    assert MinMaxObserver("input", _args(observer="memoryless_minmax"), module).keep is False
    assert MinMaxObserver("input", _args(), module, observer="memoryless_minmax").keep is False
    # what stays refused
    with pytest.raises(NotImplementedError, match="dynamic"):
        MinMaxObserver("input", _args(strategy="tensor", group_size=None, dynamic=True, num_bits=8), module)
    with pytest.raises(NotImplementedError, match="input activations"):
        MinMaxObserver("input", _args(dynamic=False), module)  # a STATIC tensor_group observer
    with pytest.raises(NotImplementedError, match="input activations"):
        MinMaxObserver("input", _args(strategy="group", group_size=32, dynamic=False), module)
    with pytest.raises(NotImplementedError, match="calculate_qparams_from_weight"):
        MinMaxObserver("weight", _args(dynamic=False), module)
    for name in ("minmax", "mse"):
        with pytest.raises(NotImplementedError, match=name):
            MinMaxObserver("input", _args(observer=name), module)
    for base in ("q", "k", "v"):
        with pytest.raises(NotImplementedError, match="dynamic"):
            MinMaxObserver(base, _args(), module)
        static = MinMaxObserver(base, _args(dynamic=False), module)
        monkeypatch.setattr(codec, "call", lambda *a: pytest.fail("launched"))
        with pytest.raises(ValueError, match="Group quantization cannot be applied to attention"):  # upstream's words
            static(torch.zeros(2, 8, 5, 64, dtype=BF16))


def test_get_global_scale_keeps_its_own_state_and_hands_the_parameter_through(monkeypatch):
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.quantization import MinMaxObserver

    calls = []

    def fake(x, state, *, keep=False, global_scale=None):
        calls.append(dict(x=x, state=state, keep=keep, global_scale=global_scale))
        state[1, 0] = 9  # what a fold leaves behind
        return global_scale if global_scale is not None else torch.ones(1)

    monkeypatch.setattr(codec, "attn_observe_global_scale", fake)
    x = torch.zeros(2, 3, 64, dtype=BF16)
    static, memoryless = MinMaxObserver("input", _args(), None), MinMaxObserver("input", _args(observer="memoryless_minmax"), None)
    out = static.get_global_scale(x)
    assert out.shape == (1,) and calls[-1]["keep"] is True and calls[-1]["x"] is x and calls[-1]["global_scale"] is None
    state = calls[-1]["state"]
    assert state.shape == (2, 1) and state.dtype == torch.int32
    p = torch.nn.Parameter(torch.empty(1), requires_grad=False)
    assert static.get_global_scale(x, p) is p and calls[-1]["global_scale"] is p and calls[-1]["state"] is state
    static.reset()
    assert static._global_state is state and state.tolist() == [[0x7FFFFFFF], [-0x80000000]]
    memoryless.get_global_scale(x)
    assert calls[-1]["keep"] is False and calls[-1]["state"] is not state
    # a static tensor observer has one too, beside the state its forward folds into
    tensor = MinMaxObserver("input", _args(strategy="tensor", group_size=None, dynamic=False, num_bits=8), None)
    tensor.get_global_scale(x)
    assert tensor._state is None and tensor._global_state is calls[-1]["state"]


def test_global_scale_entry_refuses_before_any_launch(monkeypatch):
    from compressed_tensors_amd import codec

    monkeypatch.setattr(codec, "call", lambda *a: pytest.fail("launched"))
    x = torch.zeros(2, 3, 64, dtype=BF16)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        codec.attn_observe_global_scale(x, codec.attn_observe_state(1, "cpu"))
    with pytest.raises(NotImplementedError, match="float64"):
        codec.attn_observe_global_scale(x.double(), codec.attn_observe_state(1, "cpu"))


# ---- the calibration context manager ----------------------------------------------------------------------------------------------------
def test_calibrate_global_scales_registers_and_removes(monkeypatch):
    import inspect

    import compressed_tensors_amd as cta
    from compressed_tensors_amd import codec, install, modeling

    assert "global_scales" not in inspect.getsource(install)  # install() gets no new patch
    seen = []

    def fake(x, state, *, keep=False, global_scale=None):
        seen.append((x, keep, global_scale))
        global_scale.data.fill_(float(len(seen)))
        return global_scale

    monkeypatch.setattr(codec, "attn_observe_global_scale", fake)
    act = _args()
    nv = cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(num_bits=4, type="float", strategy="tensor_group", group_size=16),
                                input_activations=act)
    both = cta.QuantizationScheme(targets=["Linear"], weights=None, input_activations=act, output_activations=act)
    static = cta.QuantizationScheme(targets=["Linear"], weights=None, input_activations=cta.QuantizationArgs(num_bits=8, strategy="tensor"))
    model = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 64)).to(BF16)
    model[0].quantization_scheme, model[2].quantization_scheme, model[3].quantization_scheme = nv, both, static
    given = torch.nn.Parameter(torch.full((1,), 5.0), requires_grad=False)
    model[2].register_parameter("input_global_scale", given)
    before = {k: (list(m._parameters), list(m._modules), len(m._forward_pre_hooks), len(m._forward_hooks)) for k, m in enumerate(model)}
    x = torch.randn(2, 3, 64).to(BF16)
    with modeling.calibrate_global_scales(model) as inside:
        assert inside is model
        p = model[0].input_global_scale
        assert isinstance(p, torch.nn.Parameter) and p.dtype == F32 and p.shape == (1,) and not p.requires_grad and p.device == model[0].weight.device
        assert model[2].input_global_scale is given  # only a missing parameter is registered
        assert model[2].output_global_scale.shape == (1,) and not hasattr(model[3], "input_global_scale") and not hasattr(model[4], "input_global_scale")
        assert isinstance(model[0].input_observer, cta.quantization.MinMaxObserver) and model[0].input_observer.keep is True
        assert len(model[0]._forward_pre_hooks) == 1 and len(model[2]._forward_pre_hooks) == 1 and len(model[2]._forward_hooks) == 1
        assert not model[3]._forward_pre_hooks and not model[4]._forward_pre_hooks
        y = model(x)
        # the input before the module's forward, the output behind it, each into the module's own parameter
        assert [(g is model[0].input_global_scale, k) for _, k, g in seen[:1]] == [(True, True)] and seen[0][0] is x
        assert seen[1][2] is given and seen[2][2] is model[2].output_global_scale and len(seen) == 3
        assert seen[2][0].shape == y.shape
        assert p.item() == 1.0 and given.item() == 2.0 and p.data_ptr() == model[0].input_global_scale.data_ptr()
    with modeling.calibrate_global_scales(model, observer="memoryless_minmax"):
        assert model[0].input_observer.keep is False and model[0].input_global_scale is p  # kept, not registered again
    for k, m in enumerate(model):
        params, modules, pre, post = before[k]
        assert list(m._modules) == modules and len(m._forward_pre_hooks) == pre and len(m._forward_hooks) == post, k
        extra = [name for name in m._parameters if name not in params]
        assert extra == {0: ["input_global_scale"], 2: ["output_global_scale"]}.get(k, []), k  # the parameters keep what the last forward wrote
    # an exception inside still cleans up
    with pytest.raises(RuntimeError, match="boom"):
        with modeling.calibrate_global_scales(model):
            raise RuntimeError("boom")
    assert not model[0]._forward_pre_hooks and "input_observer" not in model[0]._modules
