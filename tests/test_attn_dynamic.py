"""The host half of the dynamic q / k / v QDQ (codec.plan_attn_dynamic, the dispatch in forward_quantize and quantize_key_value,
the C ABI) and its fixtures: no GPU needed.  The kernel itself is tests/test_gpu_attn_dynamic.py's."""
import ctypes
import hashlib
import itertools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_dynamic_cases as C  # noqa: E402

import compressed_tensors_amd as cta  # noqa: E402
from compressed_tensors_amd import _lib, codec  # noqa: E402
from compressed_tensors_amd.modeling import kvcache  # noqa: E402
from compressed_tensors_amd.quantization import dynamic  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "attn_dynamic_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
CASES = C.case_list()


def _args(r):
    return cta.QuantizationArgs(**C.preset_args(r))


def _plan(r, x):
    return codec.plan_attn_dynamic(x.shape, x.stride(), x.dtype, _args(r), offset_bytes=x.storage_offset() * x.element_size(),
                                   global_scale=C.global_scale(r) is not None)


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------------
def test_matrix_covers_every_pair_of_factor_values():
    names = list(C.FACTORS)
    have = set()
    for _, r in CASES:
        have |= {(a, r[a], b, r[b]) for a, b in itertools.combinations(names, 2)}
    missing = C.possible_pairs() - have
    assert not missing, sorted(missing, key=repr)[:10]
    for name, values in C.FACTORS.items():  # and every value of every factor survives `normalise` somewhere
        assert {r[name] for _, r in CASES} == set(values), name
    keys = [k for k, _ in CASES]
    assert len(keys) == len(set(keys)) and set(keys) == set(MANIFEST)
    # every layout at every D for bf16 MXFP4 and NVFP4 + gs; every preset on the prefill and the decode view
    for layout in C.LAYOUTS:
        B = 1 if layout == "3d" else 2
        for D in C.D_VALUES:
            if D % 16 == 0:  # (D = 20 has no NVFP4 group: normalised to the group that is the row)
                assert f"nvfp4_gs.bf16.{layout}.{B}x8x5x{D}" in MANIFEST
            if D % 32 == 0:
                assert f"mxfp4.bf16.{layout}.{B}x8x5x{D}" in MANIFEST
    for preset in C.PRESETS:
        for S in (33, 1):
            assert f"{preset}.bf16.transposed.2x8x{S}x128" in MANIFEST


def test_manifest_inputs_resynthesise():
    for key, r in CASES:
        entry = MANIFEST[key]
        assert entry["recipe"] == r, key
        x = C.make_input(r)
        assert C.sha(x) == entry["x_sha256"] and list(x.stride()) == entry["x_strides"], key


def test_golden_files_are_small_and_match_their_hashes():
    from safetensors.torch import load_file

    for name in ("attn_dynamic_manifest.json", "attn_dynamic.safetensors"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 512 * 1024, name
    stored = load_file(os.path.join(GOLDEN, "attn_dynamic.safetensors"))
    want = {f"{k}.out" for k, e in MANIFEST.items() if e["stored"]}
    assert set(stored) == want and want
    for name, t in stored.items():
        e = MANIFEST[name[:-4]]
        assert C.stored(e["recipe"]) and t.dtype == torch.bfloat16 and list(t.shape) == e["out"]["shape"]
        assert C.sha(t) == e["out"]["sha256"], name


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
def test_plan_gives_the_expected_form_the_references_strides_and_qparam_layouts():
    forms = {"strided": 0, "copy": 0}
    for key, r in CASES:
        entry = MANIFEST[key]
        x = C.make_input(r)
        p = _plan(r, x)
        assert p.form == C.expected_form(r), (key, p.form, p.reason)
        assert (p.reason is None) == (p.form == "strided") and (p.form == "strided" or isinstance(p.reason, str) and p.reason), key
        forms[p.form] += 1
        assert list(p.out_strides) == entry["out"]["strides"], (key, p.out_strides, entry["out"]["strides"])  # the meta-tensor stride rule
        for what, shape, dtype in (("scale", p.scale_shape, p.scale_dtype), ("zp", p.scale_shape, p.zp_dtype)):
            assert list(shape) == entry[what]["shape"] and str(dtype).replace("torch.", "") == entry[what]["dtype"], (key, what)
            # contiguous whatever x's strides are: the kernel writes them in logical (b, h, s, group) order
            assert entry[what]["strides"] == list(torch.empty(shape, device="meta").stride()), (key, what)
        assert entry["out"]["dtype"] == str(x.dtype).replace("torch.", "") and entry["out"]["shape"] == list(x.shape), key
        if p.form == "strided":
            assert (p.B, p.H, p.S, p.D) == C.logical_shape(r) and p.group in (C.preset_args(r).get("group_size"), r["D"]) and p.D % p.group == 0
    assert forms["strided"] > 100 and forms["copy"] > 30, forms
    # the copy-form cases are exactly the five kinds the kernel's contract leaves out
    for key, r in CASES:
        if C.expected_form(r) == "copy":
            st = C.preset_args(r)["strategy"]
            assert (r["layout"] == "misaligned" or r["D"] == 20 or st == "tensor" or (st == "token" and (r["S"] > 1 or r["D"] & (r["D"] - 1)))), key


def test_stride_examples_of_the_decode_and_fused_views():
    mx, tok = cta.QuantizationArgs(**C.DYN_PRESETS["mxfp4"]), cta.QuantizationArgs(**C.DYN_PRESETS["fp8_token"])
    bf = torch.bfloat16
    assert codec.plan_attn_dynamic((2, 8, 1, 128), (1024, 128, 1024, 1), bf, mx).out_strides == (1024, 128, 128, 1)
    assert codec.plan_attn_dynamic((2, 8, 1, 128), (1024, 128, 1024, 1), bf, tok).out_strides == (1024, 128, 1024, 1)
    p = codec.plan_attn_dynamic((2, 2, 5, 128), (4480, 128, 896, 1), bf, mx)
    assert p.form == "strided" and p.out_strides == (1280, 128, 256, 1)
    # what _attn_view refuses is copied: a last dimension that is not contiguous, a view that overlaps itself
    assert codec.plan_attn_dynamic((2, 8, 5, 128), (5120, 1, 1024, 8), bf, mx).form == "copy"
    assert "overlaps" in codec.plan_attn_dynamic((2, 8, 5, 128), (64, 128, 1024, 1), bf, mx).reason
    # rows longer than one pass, groups that are no 8 * 2^k
    assert "exceed" in codec.plan_attn_dynamic((1, 2, 3, 4096), (24576, 4096, 8192, 1), bf, mx).reason
    g24 = cta.QuantizationArgs(num_bits=8, type="float", strategy="group", group_size=24, symmetric=True, dynamic=True)
    assert "8 * 2^k" in codec.plan_attn_dynamic((1, 2, 3, 96), (576, 96, 192, 1), bf, g24).reason


def test_the_references_errors_surface_unchanged():
    bf = torch.bfloat16
    shape, strides = (2, 8, 5, 128), (5120, 128, 1024, 1)
    with pytest.raises(ValueError, match="Dynamic quantization is only supported for"):
        codec.plan_attn_dynamic(shape, strides, bf, cta.QuantizationArgs(num_bits=8, type="float", strategy="channel", symmetric=True, dynamic=True))
    with pytest.raises(NotImplementedError, match="has no kernel"):  # FLOAT asymmetric
        codec.plan_attn_dynamic(shape, strides, bf, cta.QuantizationArgs(num_bits=8, type="float", strategy="group", group_size=32, symmetric=False, dynamic=True))
    with pytest.raises(NotImplementedError, match="has no kernel"):  # a scale dtype no kernel writes
        codec.plan_attn_dynamic(shape, strides, bf, cta.QuantizationArgs(num_bits=8, type="int", strategy="group", group_size=32, symmetric=True, dynamic=True,
                                                                         scale_dtype=torch.float16))
    with pytest.raises(NotImplementedError, match="not a whole number of groups"):
        codec.plan_attn_dynamic(shape, strides, bf, cta.QuantizationArgs(num_bits=8, type="float", strategy="group", group_size=48, symmetric=True, dynamic=True))
    with pytest.raises(NotImplementedError, match="empty tensor"):
        codec.plan_attn_dynamic((2, 8, 0, 128), (0, 128, 1024, 1), bf, cta.QuantizationArgs(**C.DYN_PRESETS["mxfp4"]))
    with pytest.raises(NotImplementedError, match="global scale"):
        codec.plan_attn_dynamic(shape, strides, bf, cta.QuantizationArgs(**C.DYN_PRESETS["mxfp4"]), global_scale=True)
    # the static entries keep refusing what they refused
    with pytest.raises(NotImplementedError, match="FLOAT 4-bit"):
        codec._attn_refusals(None, "float", 4, True, "attention states")
    with pytest.raises(NotImplementedError, match="global scale"):
        codec._attn_refusals(torch.ones(1), "float", 8, True, "attention states")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_symbol_is_declared_and_bound():
    argtypes, restype = _lib._PROTOTYPES["ct_attn_dyn_qdq"]
    assert len(argtypes) == 9 and restype is ctypes.c_int
    assert "ct_attn_dyn_qdq" in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.load(), "ct_attn_dyn_qdq")  # exported by the built library
    with open(os.path.join(ROOT, "include", "ct_hip.h")) as f:
        header = f.read()
    assert "int ct_attn_dyn_qdq(const ct_attn_dyn_tensor* tensors, int n, int group, int kind, int bits, int symmetric, int xdt, int zdt," in header
    assert "} ct_attn_dyn_tensor;" in header
    assert ctypes.sizeof(_lib.AttnDynTensor) == 15 * 8  # "15 64-bit words"
    assert [f[0] for f in _lib.AttnDynTensor._fields_] == ["x", "out", "scale_out", "zp_out", "global_scale", "B", "H", "S", "D", "x_stride", "out_stride"]
    assert ctypes.sizeof(_lib.AttnTensor) == 120  # ct_attn_tensor is unchanged
    with open(os.path.join(ROOT, "compressed_tensors_amd", "csrc", "ct_attn_dyn.hip")) as f:
        src = f.read()
    assert 'extern "C" int ct_attn_dyn_qdq(' in src and '#include "ct_attn.h"' in src and '#include "ct_dynamic.h"' in src
    for name in ("plan_attn_dynamic", "attn_dynamic_fake_quantize", "attn_dynamic_fake_quantize_pair", "attn_dynamic_qparams"):
        assert callable(getattr(codec, name)) and name in codec.__all__
    assert kvcache.DYNAMIC_MEASURED_FASTER is codec.ATTN_DYNAMIC_MEASURED_FASTER


# ---- the dispatch, with stubs --------------------------------------------------------------------------------------------------------------
class _Stub:
    def __init__(self, result=None):
        self.calls, self.result = [], result

    def __call__(self, *a, **kw):
        self.calls.append((a, kw))
        return self.result if self.result is not None else a[0]


def test_forward_quantize_sends_dynamic_attention_states_to_the_strided_entry(monkeypatch):
    ours, old = _Stub(), _Stub()
    monkeypatch.setattr(codec, "attn_dynamic_fake_quantize", ours)
    monkeypatch.setattr(dynamic, "dynamic_fake_quantize", old)
    mod = torch.nn.Module()
    mod.k_global_scale = torch.ones(1)
    x = torch.ones(2, 5, 8, 32).transpose(1, 2)
    for preset in ("mxfp4", "nvfp4", "fp8_token"):
        args = cta.QuantizationArgs(**C.DYN_PRESETS[preset])
        old.calls.clear()
        for name in ("q", "k", "v"):
            ours.calls.clear()
            assert dynamic.forward_quantize(mod, x, name, args) is x
            (a, kw), = ours.calls
            assert a[0] is x and a[1] is args and a[2] is (mod.k_global_scale if name == "k" else None) and not kw
        assert not old.calls
        for name in ("input", "output", "weight"):
            old.calls.clear()
            ours.calls.clear()
            dynamic.forward_quantize(mod, x, name, args)
            assert len(old.calls) == 1 and not ours.calls and old.calls[0][0][:2] == (x, args)
    # a static scheme never reaches either
    static = cta.QuantizationArgs(num_bits=8, type="float", strategy="tensor", symmetric=True)
    mod.k_scale = torch.ones(1)
    attn = _Stub()
    monkeypatch.setattr(codec, "attn_fake_quantize", attn)
    old.calls.clear()
    ours.calls.clear()
    mod.k_global_scale = None
    dynamic.forward_quantize(mod, x, "k", static)
    assert len(attn.calls) == 1 and not old.calls and not ours.calls


def test_quantize_key_value_takes_the_dynamic_pair_only_where_it_is_served(monkeypatch):
    class _Cuda(torch.Tensor):  # a CPU tensor that says it lives on the GPU: the dispatch reads nothing else
        is_cuda = True

    k = torch.ones(2, 5, 2, 32).transpose(1, 2).as_subclass(_Cuda)
    v = torch.ones(2, 5, 2, 32).transpose(1, 2).as_subclass(_Cuda)
    pair = _Stub(result=("K", "V"))
    monkeypatch.setattr(codec, "attn_dynamic_fake_quantize_pair", pair)
    single = _Stub(result="S")
    mx = cta.QuantizationArgs(**C.DYN_PRESETS["mxfp4"])
    nv = cta.QuantizationArgs(**C.DYN_PRESETS["nvfp4"])
    mod = torch.nn.Module()

    def run(args, **kw):
        pair.calls.clear()
        single.calls.clear()
        out = kvcache.quantize_key_value(mod, k, v, args, single=single, **kw)
        return out, len(pair.calls), len(single.calls)

    assert run(mx, pair=True) == (("K", "V"), 1, 0)
    (a, kw), = pair.calls
    assert a[0] is k and a[1] is v and a[2] is mx and a[3] is None and a[4] is None
    assert run(mx, pair=False) == (("S", "S"), 0, 2)
    for on in (False, True):  # None: the constant decides
        monkeypatch.setitem(kvcache.DYNAMIC_MEASURED_FASTER, "pair", on)
        assert run(mx) == ((("K", "V"), 1, 0) if on else (("S", "S"), 0, 2))
    # both global scales, or neither
    mod.k_global_scale = torch.ones(1)
    assert run(nv, pair=True) == (("S", "S"), 0, 2)
    mod.v_global_scale = torch.ones(1) * 2
    assert run(nv, pair=True) == (("K", "V"), 1, 0)
    assert pair.calls[0][0][3] is mod.k_global_scale and pair.calls[0][0][4] is mod.v_global_scale
    mod.k_global_scale = mod.v_global_scale = None
    # group schemes only: token and tensor go through the two calls, and so does a static scheme without scales
    for preset in ("fp8_token", "fp8_tensor"):
        assert run(cta.QuantizationArgs(**C.DYN_PRESETS[preset]), pair=True) == (("S", "S"), 0, 2)
    assert run(cta.QuantizationArgs(num_bits=8, type="float", strategy="tensor", symmetric=True), pair=True) == (("S", "S"), 0, 2)
    # CPU states: the two calls
    out = kvcache.quantize_key_value(mod, torch.ones(1, 1, 1, 32), torch.ones(1, 1, 1, 32), mx, single=single, pair=True)
    assert out == ("S", "S")


# ---- the dispatch constants --------------------------------------------------------------------------------------------------------------
ROWS = (("dyn_prefill_q", [1, 32, 8192, 128], "single"), ("dyn_prefill_kv", [1, 8, 8192, 128], "pair"), ("dyn_decode_kv", [64, 8, 1, 128], "pair"))
BENCH_SCHEMES = ("fp8_group128", "mxfp4", "nvfp4_gs")


def test_as_shipped_the_dispatch_constants_are_measured_faster():
    """a key of ATTN_DYNAMIC_MEASURED_FASTER is True only if every verdict of profiles/attn_dynamic_bench.jsonl that speaks for it, in
    both runs, is "faster"; the file holds two runs of the three rows x three schemes"""
    consts = codec.ATTN_DYNAMIC_MEASURED_FASTER
    assert set(consts) == {"single", "pair"} and all(isinstance(v, bool) for v in consts.values())
    with open(os.path.join(ROOT, "profiles", "attn_dynamic_bench.jsonl")) as f:
        lines = [json.loads(line) for line in f if line.strip()]
    rows = [r for r in lines if "row" in r]
    verdicts = [v for v in lines if "verdict" in v]
    for name, shape, key in ROWS:
        for scheme in BENCH_SCHEMES:
            mine = [r for r in rows if r["row"] == name and r["scheme"] == scheme]
            assert len(mine) >= 2 and {r["run"] for r in mine} >= {0, 1} and all(r["shape"] == shape and r["transposed_view"] and r["dtype"] == "bfloat16" for r in mine)
            vs = [v for v in verdicts if v["verdict"] == name and v["scheme"] == scheme]
            assert vs and key in {v["key"] for v in vs}
            for v in vs:  # the rule of tools/rotated_bench.py and tools/attn_bench.py
                assert v["faster"] == (v["path_worst_us"] + v["run_spread_us"] < v["baseline_best_us"])
    for key, on in consts.items():
        speaking = [v for v in verdicts if v["key"] == key]
        assert speaking
        if on:
            assert all(v["faster"] for v in speaking), (key, [v for v in speaking if not v["faster"]])


def test_manifest_hash_is_stable():
    """the manifest is what the generator writes for this matrix: sorted keys, one recipe per case"""
    with open(os.path.join(GOLDEN, "attn_dynamic_manifest.json"), "rb") as f:
        raw = f.read()
    again = (json.dumps(json.loads(raw), indent=1, sort_keys=True) + "\n").encode()
    assert hashlib.sha256(raw).hexdigest() == hashlib.sha256(again).hexdigest()
