"""Host side of the attention min-max observer (codec.plan_attn_observe, the ct_attn_observe ABI, quantization.MinMaxObserver's
host logic, the fixtures against the repo's own CPU oracle): everything here runs without a GPU."""
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_observe_cases as C  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "attn_observe_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
TORCH_DT = {"bfloat16": C.BF16, "float16": C.F16, "float32": C.F32, "int8": torch.int8, "float8_e4m3fn": C.F8}
_GOLDEN = {}


def _golden(key, name):
    if not _GOLDEN:
        from safetensors.torch import load_file

        _GOLDEN.update(load_file(os.path.join(GOLDEN, "attn_observe.safetensors")))
    t = _GOLDEN[f"{key}.{name}"]
    return t.view(C.F8) if MANIFEST[key]["out"][name]["dtype"] == "float8_e4m3fn" else t


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def test_manifest_matches_the_case_list():
    cases = C.case_list()
    assert [k for k, _ in cases] == sorted(MANIFEST, key=[k for k, _ in cases].index) and len(cases) == len(MANIFEST)
    for key, recipe in cases:
        assert MANIFEST[key]["recipe"] == recipe, key
    # the matrix the issue names: every layout at every D, every kind / dtype / strategy / base, the special cases
    recipes = [r for _, r in cases]
    assert {(r["layout"], r["D"]) for r in recipes} >= {(layout, D) for layout in C.LAYOUTS for D in C.D_VALUES}
    for factor, values in C.FACTORS.items():
        assert {r[factor] for r in recipes} >= set(values), factor
    assert {r["special"] for r in recipes} == {None, "zero_head", "signed_heads", "nan_inf", "arange"}
    assert {r["kind"] for r in recipes if r["special"] == "nan_inf"} == {"fp8", "int8_zp"}


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_inputs_reproduce_and_goldens_equal_the_oracle(key):
    """the recipe synthesises the input the reference saw, and the reference's scale / zero point equal the repo's own CPU
    restatement of calculate_qparams on each entry's values viewed as one row"""
    import oracle as O

    entry = MANIFEST[key]
    r = entry["recipe"]
    x = C.make_observed(r)
    assert C.sha(x) == entry["x_sha256"] and list(x.stride()) == entry["x_strides"]
    for name in ("min_vals", "max_vals", "scale", "zero_point"):
        t = _golden(key, name)
        assert tuple(t.shape) == C.expected_shape(r) == tuple(entry["out"][name]["shape"]), (name, t.shape)
        assert t.dtype == TORCH_DT[entry["out"][name]["dtype"]] == (C.zp_dtype(r) if name == "zero_point" else x.dtype), (name, t.dtype)
    rows = C.head_rows(r, x).contiguous()
    kind = C.KINDS[r["kind"]]
    if kind["type"] == "float":
        scale = O.calculate_qparams_float(rows, kind="fp8")
        zp = torch.zeros(scale.shape, dtype=C.F8)
    else:
        scale, zp = O.calculate_qparams_minmax(rows, num_bits=kind["num_bits"], symmetric=kind["symmetric"])
    shape = C.expected_shape(r)
    assert C.canonical_bytes(scale.reshape(shape)) == C.canonical_bytes(_golden(key, "scale")), "scale"
    assert C.canonical_bytes(zp.reshape(shape)) == C.canonical_bytes(_golden(key, "zero_point")), "zero point"
    # and the extremes are the values' own
    nan = torch.isnan(rows.float()).any(dim=1)
    want_mn = torch.where(nan, torch.tensor(float("nan")), rows.float().amin(dim=1)).to(x.dtype).reshape(shape)
    want_mx = torch.where(nan, torch.tensor(float("nan")), rows.float().amax(dim=1)).to(x.dtype).reshape(shape)
    assert C.canonical_bytes(want_mn + 0.0) == C.canonical_bytes(_golden(key, "min_vals") + 0.0)
    assert C.canonical_bytes(want_mx + 0.0) == C.canonical_bytes(_golden(key, "max_vals") + 0.0)


def test_the_references_known_answer_is_in_the_fixtures():
    """test_static_attention_quantization: arange(24) as (1, 2, 3, 4) bf16, INT4 symmetric"""
    key = "k.int4.attn_head.bf16.contiguous.1x2x3x4.arange"
    assert _golden(key, "min_vals").flatten().tolist() == [0.0, 12.0] and _golden(key, "max_vals").flatten().tolist() == [11.0, 23.0]
    key = "k.int4.tensor.bf16.contiguous.1x2x3x4.arange"
    assert _golden(key, "min_vals").tolist() == [0.0] and _golden(key, "max_vals").tolist() == [23.0]
    assert _golden(key, "scale").tolist() == [3.0625]  # 23 / 7.5 in bfloat16


# ---- plan_attn_observe ---------------------------------------------------------------------------------------------------------------
def _plan(x, strategy="attn_head", **kw):
    from compressed_tensors_amd import codec

    return codec.plan_attn_observe(x.shape, x.stride(), x.dtype, strategy, offset_bytes=(x.storage_offset() * x.element_size()) % 16, **kw)


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_plan_reads_every_fixture_case_in_place(key):
    r = MANIFEST[key]["recipe"]
    x = C.make_observed(r)
    p = _plan(x, r["strategy"])
    assert p.in_place and p.reason is None
    assert p.per_head == (r["strategy"] == "attn_head") and p.entries == (r["H"] if p.per_head else 1)
    if r["base"] == "input":  # (batch, seq, hidden): the padded batch dimension, then rows of `hidden`
        assert (p.B, p.H, p.S, p.D) == (1, r["B"], r["S"], r["H"] * r["D"])
    else:
        assert (p.B, p.H, p.S, p.D) == C.logical_shape(r)
        want = tuple(x.stride()[:-1]) if x.ndim == 4 else (0,) + tuple(x.stride()[:-1])
        sizes = C.logical_shape(r)[:3]  # the stride of a dimension of one entry is never used
        assert [s for s, n in zip(p.strides, sizes) if n > 1] == [s for s, n in zip(want, sizes) if n > 1]
        assert p.vector ==(r["D"] % 8 == 0 and r["layout"] != "misaligned"), (x.stride(), x.storage_offset())
    if r["layout"] == "expanded":
        assert p.strides[0] == 0  # read as it is: a read-only kernel does not mind


def test_plan_copies_only_what_the_kernel_cannot_index():
    from compressed_tensors_amd import codec

    x = torch.zeros(2, 8, 5, 128, dtype=C.BF16)
    p = _plan(x.transpose(2, 3))
    assert not p.in_place and "stride" in p.reason and p.strides == (8 * 5 * 128, 128 * 5, 5)
    p = codec.plan_attn_observe((2, 8, 5, 128), (5120, -640, 128, 1), C.BF16, "attn_head")
    assert not p.in_place and p.reason == "negative strides"
    # a view that overlaps itself is fine for a reader (plan_attn_qdq copies it: it has an output to lay out)
    overlapping = torch.zeros(4096, dtype=C.BF16).as_strided((2, 8, 5, 128), (64, 8, 128, 1))
    p = _plan(overlapping)
    assert p.in_place and p.strides == (64, 8, 128) and p.vector
    five = torch.zeros(3, 2, 8, 5, 128, dtype=C.BF16)
    p = _plan(five)
    assert p.in_place and (p.B, p.H, p.S, p.D) == (6, 8, 5, 128)
    assert not _plan(five.transpose(0, 1)).in_place
    # the vector rule is ct_attn_qdq's: whole units, an aligned base, strides that keep the units aligned
    assert not codec.plan_attn_observe((2, 4, 5, 64), (1280, 320, 64, 1), C.F32, "attn_head", offset_bytes=8).vector
    assert not codec.plan_attn_observe((1, 4, 5, 64), (0, 324, 64, 1), C.BF16, "attn_head").vector
    assert codec.plan_attn_observe((1, 1, 5, 64), (0, 324, 64, 1), C.BF16, "attn_head").vector
    # a static activation: one entry, rows of `hidden`
    p = codec.plan_attn_observe((2, 5, 4096), (5 * 4096, 4096, 1), C.BF16, "tensor")
    assert p.in_place and p.vector and not p.per_head and p.entries == 1 and p.D == 4096


def test_plan_error_contract():
    from compressed_tensors_amd import codec

    cap = codec.ATTN_OBSERVE_MAX_ENTRIES
    assert cap >= 1024
    src = open(os.path.join(ROOT, "compressed_tensors_amd", "csrc", "ct_attn_observe.hip")).read()
    assert int(re.search(r"kObsMaxEntries = (\d+);", src).group(1)) == cap
    with pytest.raises(ValueError, match="at least 3 observed dimensions"):
        codec.plan_attn_observe((5, 64), (64, 1), C.BF16, "attn_head")
    assert codec.plan_attn_observe((5, 64), (64, 1), C.BF16, "tensor").entries == 1
    with pytest.raises(NotImplementedError, match="float64"):
        codec.plan_attn_observe((2, 8, 5, 64), (2560, 320, 64, 1), torch.float64, "attn_head")
    with pytest.raises(NotImplementedError, match="cpu"):
        codec.plan_attn_observe((2, 8, 5, 64), (2560, 320, 64, 1), C.BF16, "attn_head", device_type="cpu")
    assert codec.plan_attn_observe((1, cap, 1, 8), (cap * 8, 8, 8, 1), C.BF16, "attn_head").entries == cap
    with pytest.raises(NotImplementedError, match=f"{cap + 1} heads"):
        codec.plan_attn_observe((1, cap + 1, 1, 8), ((cap + 1) * 8, 8, 8, 1), C.BF16, "attn_head")
    assert codec.plan_attn_observe((1, cap + 1, 1, 8), ((cap + 1) * 8, 8, 8, 1), C.BF16, "tensor").entries == 1  # no table entry per head
    for strategy, word in (("token", "Token"), ("channel", "Channel"), ("group", "Group"), ("tensor_group", "Group"), ("block", "Block")):
        with pytest.raises(ValueError, match=f"{word} quantization cannot be applied to attention"):
            codec.plan_attn_observe((2, 8, 5, 64), (2560, 320, 64, 1), C.BF16, strategy)
    with pytest.raises(ValueError, match="empty"):
        codec.plan_attn_observe((2, 8, 0, 64), (0, 0, 64, 1), C.BF16, "attn_head")


def test_cpu_tensors_and_unserved_arguments_raise_before_any_launch(monkeypatch):
    from compressed_tensors_amd import codec

    monkeypatch.setattr(codec, "call", lambda *a: pytest.fail("launched"))
    x = torch.zeros(2, 8, 5, 64, dtype=C.BF16)
    state = codec.attn_observe_state(8, "cpu")
    assert state.dtype == torch.int32 and state.tolist() == [[0x7FFFFFFF] * 8, [-0x80000000] * 8]
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        codec.attn_observe(x, state, num_bits=8, qtype="float")
    with pytest.raises(NotImplementedError, match="FLOAT 4-bit"):
        codec.attn_observe(x, state, num_bits=4, qtype="float")
    with pytest.raises(NotImplementedError, match="global scale"):
        codec.attn_observe(x, state, num_bits=8, qtype="float", global_scale=torch.ones(1))
    with pytest.raises(NotImplementedError, match="global scale"):
        codec.attn_observe_pair(x, x, state, state, num_bits=8, qtype="float", global_scale=torch.ones(1))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_prototyped_and_exported():
    import ctypes

    from compressed_tensors_amd import _lib

    header = open(os.path.join(ROOT, "include", "ct_hip.h")).read()
    assert re.search(r"int ct_attn_observe\(const ct_attn_observe_tensor\* tensors, int n, int kind, int bits, int symmetric, int xdt, int sdt, "
                     r"int zdt, int keep,\s+ct_stream_t stream\);", header)
    assert "ct_attn_observe" in _lib.EXPORTED_SYMBOLS
    argtypes, restype = _lib._PROTOTYPES["ct_attn_observe"]
    assert len(argtypes) == 10 and restype is ctypes.c_int
    # the descriptor: the header's fields in the header's order, 14 64-bit words
    body = re.search(r"typedef struct ct_attn_observe_tensor \{(.*?)\} ct_attn_observe_tensor;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == ["x", "state", "scale", "zp", "min_vals", "max_vals", "B", "H", "S", "D", "x_stride", "per_head"]
    assert [f[0] for f in _lib.AttnObserveTensor._fields_] == names and ctypes.sizeof(_lib.AttnObserveTensor) == 14 * 8
    src = open(os.path.join(ROOT, "compressed_tensors_amd", "csrc", "ct_attn_observe.hip")).read()
    assert '#include "ct_attn.h"' in src and '#include "ct_minmax.h"' in src
    assert 'extern "C" int ct_attn_observe(' in src
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "ct_attn_observe")


# ---- the observer's host logic, with the launch replaced ----------------------------------------------------------------------------
class _Recorded:
    def __init__(self, monkeypatch):
        from compressed_tensors_amd import codec

        self.calls = []

        def attn_observe(x, state, **kw):
            self.calls.append(dict(kw, state=state, x=x))
            shape = (x.shape[-3], 1, 1) if kw["strategy"] == "attn_head" else (1,)
            if kw["keep"]:
                state[0, 0] = 7  # what a fold leaves behind
            out = torch.ones(shape, dtype=x.dtype)
            return out, torch.zeros(shape, dtype=torch.int8), -out, out

        monkeypatch.setattr(codec, "attn_observe", attn_observe)


def _args(**kw):
    import compressed_tensors_amd as cta

    return cta.QuantizationArgs(**dict(dict(num_bits=8, type="float", symmetric=True, strategy="attn_head"), **kw))


def test_observer_names_select_keep(monkeypatch):
    from compressed_tensors_amd.quantization import MinMaxObserver

    rec = _Recorded(monkeypatch)
    x = torch.zeros(2, 8, 5, 64, dtype=C.BF16)
    module = torch.nn.Module()
    memoryless = MinMaxObserver("k", _args(), module)  # no name anywhere: the reference's default for static arguments
    assert memoryless.observer == "memoryless_minmax" and memoryless.min_vals is None
    scale, zp = memoryless(x)
    assert rec.calls[-1]["keep"] is False and rec.calls[-1]["want_minmax"] and scale.shape == (8, 1, 1) and zp.dtype == torch.int8
    assert memoryless.min_vals is not None and memoryless.max_vals is not None
    assert dict(num_bits=8, symmetric=True, qtype="float", strategy="attn_head").items() <= rec.calls[-1].items()
    static = MinMaxObserver("k", _args(observer="static_minmax"), module)
    static(x)
    assert rec.calls[-1]["keep"] is True
    assert MinMaxObserver("k", _args(observer="static_minmax"), module, observer="memoryless_minmax").keep is False  # the argument wins
    # the state: armed on first use, the same buffer afterwards, armed again by reset()
    state = rec.calls[-1]["state"]
    assert state.shape == (2, 8) and state[0, 0] == 7
    static(x)
    assert rec.calls[-1]["state"] is state
    static.reset()
    assert static._state is state and state.tolist() == [[0x7FFFFFFF] * 8, [-0x80000000] * 8] and static.min_vals is None
    # another entry count: a new state
    static(torch.zeros(2, 4, 5, 64, dtype=C.BF16))
    assert rec.calls[-1]["state"].shape == (2, 4)
    # the module's parameters are handed through
    p = torch.nn.Parameter(torch.empty(8, 1, 1, dtype=C.BF16), requires_grad=False)
    memoryless(x, scale=p)
    assert rec.calls[-1]["scale"] is p and rec.calls[-1]["zero_point"] is None


def test_observer_refuses_what_it_does_not_serve():
    from compressed_tensors_amd.quantization import MinMaxObserver

    module = torch.nn.Module()
    for name in ("minmax", "mse", "static_mse"):
        with pytest.raises(NotImplementedError, match=name):
            MinMaxObserver("k", _args(observer=name), module)
        with pytest.raises(NotImplementedError, match=name):
            MinMaxObserver("k", _args(), module, observer=name)
    with pytest.raises(NotImplementedError, match="calculate_qparams_from_weight"):
        MinMaxObserver("weight", _args(strategy="tensor"), module)
    with pytest.raises(ValueError, match="Unknown quantization base name"):
        MinMaxObserver("bias", _args(), module)
    with pytest.raises(NotImplementedError, match="input activations"):
        MinMaxObserver("input", _args(strategy="group", group_size=32), module)
    with pytest.raises(NotImplementedError, match="dynamic"):
        MinMaxObserver("input", _args(strategy="tensor", dynamic=True), module)
    for base in ("input", "output", "q", "v"):
        assert MinMaxObserver(base, _args(strategy="tensor"), module).base_name == base


def test_calibration_changes_no_default_and_the_pair_dispatch_follows_the_bench():
    """nothing launches an observer unless asked (install() patches nothing new), and K and V share a launch only where
    profiles/attn_observe_bench.jsonl says the pair is faster at every k+v row by more than the spread between its runs"""
    import inspect

    from compressed_tensors_amd import install, modeling

    assert "observe" not in inspect.getsource(install)
    with open(os.path.join(ROOT, "profiles", "attn_observe_bench.jsonl")) as f:
        lines = [json.loads(line) for line in f if line.strip()]
    verdicts = [v for v in lines if v.get("path") == "pair"]
    assert {v["verdict"] for v in verdicts} == {"prefill_kv", "decode_kv"} and len({r["run"] for r in lines if "run" in r}) >= 2
    for v in verdicts:
        assert v["faster"] == (v["path_worst_us"] + v["run_spread_us"] < v["baseline_best_us"])
    may = all(v["faster"] for v in verdicts)
    assert lines[-1] == {"OBSERVE_PAIR_MEASURED_FASTER_may_be": may}
    assert modeling.OBSERVE_PAIR_MEASURED_FASTER in (False, may) and modeling.calibration.OBSERVE_PAIR_MEASURED_FASTER is modeling.OBSERVE_PAIR_MEASURED_FASTER
