"""Host side of the head-dim rotation in the attention QDQ's launch (codec.plan_attn_rot_qdq, the ct_attn_rot_qdq ABI, the fixtures of
tools/gen_golden_attn_rotated.py, the hand-off between transform.fuse_attention_quantization's hooks and forward_quantize /
quantize_key_value with the launches replaced by stand-ins, and the dispatch constants against the measurement).  No GPU needed."""
import ctypes
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_cases as A  # noqa: E402
import _attn_rotated_cases as C  # noqa: E402

import compressed_tensors_amd as cta  # noqa: E402
from compressed_tensors_amd import _lib, codec, modeling, transform  # noqa: E402
from compressed_tensors_amd.modeling import kvcache  # noqa: E402
from compressed_tensors_amd.quantization import dynamic  # noqa: E402
from compressed_tensors_amd.transform import apply as tapply  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "attn_rotated_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
BF16 = torch.bfloat16


def _plan(x, n, scale_shape=None, strategy="attn_head", **kw):
    scale_shape = (x.shape[-3], 1, 1) if scale_shape is None else scale_shape
    return codec.plan_attn_rot_qdq(x.shape, x.stride(), x.dtype, n, scale_shape, strategy, offset_bytes=(x.storage_offset() * x.element_size()) % 16, **kw)


# ---- plan_attn_rot_qdq -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", A.LAYOUTS)
@pytest.mark.parametrize("D", [8, 16, 64, 128, 256, 384, 512])
def test_plan_fuses_every_fixture_layout(layout, D):
    r = A.normalise(dict(D=D, B=2, H=8, S=5, layout=layout, dtypes="bf16/bf16", kind="fp8", strategy="attn_head", mode="fake", salt=1))
    x = A.make_input(r)
    for n in sorted({2, 8, D & -D, min(D & -D, 128)}):  # powers of two that divide D
        p = _plan(x, n)
        if layout == "misaligned":
            assert not p.fused and "alignment" in p.reason
            continue
        assert p.fused and p.reason is None and p.in_place, (layout, D, n, p.reason)
        assert p.hadamard.size == n and p.attn.D == D
        assert p.out_strides == tuple(torch.empty(x.shape).stride())  # the rotated tensor is a new, contiguous one


def test_plan_declines_with_a_reason():
    x = torch.zeros(2, 8, 5, 20, dtype=BF16)
    p = _plan(x, 4)
    assert not p.fused and "8-element units" in p.reason
    p = _plan(torch.zeros(1, 2, 3, 1024, dtype=BF16), 1024)
    assert not p.fused and "512" in p.reason
    p = _plan(torch.zeros(2 * 8 * 5 * 64 + 1, dtype=BF16)[1:].view(2, 8, 5, 64), 64)  # one element into its storage
    assert not p.fused and "alignment" in p.reason
    p = _plan(torch.zeros(1, 2, 3, 4096, dtype=BF16), 128)  # D / 8 = 512 lanes
    assert not p.fused and "one pass" in p.reason
    p = _plan(torch.zeros(2, 8, 5, 64, dtype=BF16), 64, precision=torch.float64)
    assert not p.fused and "float32" in p.reason
    p = _plan(torch.zeros(2, 8, 64, 5, dtype=BF16).transpose(2, 3), 64)  # last stride != 1: copied first
    assert not p.fused and not p.in_place and "stride" in p.reason
    assert codec.ATTN_ROTATED_MAX_SIZE == 512 and codec.ATTN_ROTATED_MAX_UNITS == 256


def test_plan_raises_the_rotations_errors_first():
    x = torch.zeros(2, 8, 5, 24, dtype=BF16)
    for n, msg in ((0, "size <= 0"), (-4, "size <= 0"), (12, "size != 2\\^n"), (16, "16 must divide 24")):
        with pytest.raises(ValueError, match=msg):
            _plan(x, n, strategy="channel")  # ... before the strategy is looked at
    with pytest.raises(NotImplementedError, match="tensor and attn_head"):
        _plan(x, 8, strategy="channel")
    with pytest.raises(RuntimeError, match=r"must match the size of tensor b \(3\)"):
        _plan(x, 8, scale_shape=(3, 1, 1))
    with pytest.raises(ValueError, match="at least 3"):
        _plan(torch.zeros(5, 24, dtype=BF16), 8, scale_shape=(1, 1, 1))


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------------
def test_the_fixture_matrix():
    cases = C.fixture_cases()
    assert sorted(k for k, _ in cases) == sorted(MANIFEST) and 20 <= len(cases) <= 60
    flagship = {(r["D"], r["n"]) for _, r in cases if (r["layout"], r["dtypes"], r["kind"], r["strategy"], r["mode"]) ==
                ("transposed", "bf16/bf16", "fp8", "attn_head", "fake")}
    assert set(C.DN_PAIRS) <= flagship
    assert {r["layout"] for _, r in cases} == set(C.LAYOUTS) and {r["kind"] for _, r in cases} == set(C.KINDS)
    assert {r["mode"] for _, r in cases} == {"fake", "quantize"} and {"attn_head", "tensor"} <= {r["strategy"] for _, r in cases}
    for key, r in cases:
        assert MANIFEST[key]["recipe"] == r and MANIFEST[key]["stored"] == C.stored(r)


def test_the_identity_matrix_covers_every_pair():
    cases = C.identity_cases()
    names = list(C.ID_FACTORS)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            want = {(va, vb) for va in C.ID_FACTORS[a] for vb in C.ID_FACTORS[b]}
            assert want <= {(c[a], c[b]) for c in cases}, (a, b)
    assert len(cases) < 150
    flagship = {c["dn"] for c in cases if (c["layout"], c["dtype"], c["kind"], c["strategy"]) == ("transposed", "bf16", "fp8", "attn_head")}
    assert set(C.DN_PAIRS) <= flagship


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_manifest_inputs_resynthesise_and_the_plan_gives_the_references_strides(key):
    entry = MANIFEST[key]
    r = entry["recipe"]
    x = C.make_input(r)
    assert C.sha(x) == entry["x_sha256"] and list(x.stride()) == entry["x_strides"]
    rows = x.reshape(-1, r["D"]) if x.is_contiguous() else x.contiguous().reshape(-1, r["D"])
    assert not rows[0].any() and int((rows[1] != 0).sum()) == 1 and bool((rows[2] == 3).all())  # zero, single non-zero, constant
    ints = rows.double() * torch.pow(2.0, 4 - ((torch.arange(rows.shape[0]) * 7 + r["salt"]) % 9 - 4).double()).unsqueeze(1)
    assert torch.equal(ints, ints.round())  # integers times a per-row power of two
    scale, _ = C.make_qparams(r)
    p = _plan(x, r["n"], scale_shape=tuple(scale.shape), strategy=A.strategy_of(r))
    assert p.fused and list(p.out_strides) == entry["out"]["strides"] == entry["rotated"]["strides"], key
    assert entry["rotated"]["dtype"] == str(x.dtype).replace("torch.", "") and entry["out"]["shape"] == list(x.shape)


def test_golden_files_are_small_and_match_their_hashes():
    from safetensors.torch import load_file

    for name in ("attn_rotated_manifest.json", "attn_rotated.safetensors"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 512 * 1024, name
    g = load_file(os.path.join(GOLDEN, "attn_rotated.safetensors"))
    assert set(g) == {f"{k}.out" for k, e in MANIFEST.items() if e["stored"]} and g
    for name, t in g.items():
        want = MANIFEST[name[:-4]]["out"]
        t = t.view(C.F8) if want["dtype"] == "float8_e4m3fn" else t
        assert C.sha(t) == want["sha256"] and list(t.shape) == want["shape"], name


def test_rotation64_is_the_float32_butterfly_on_fixture_inputs():
    import _hadamard_cases as H

    for key, r in C.fixture_cases()[:12]:
        x = C.fixture_values(r)
        assert C.equal_by_value(C.rotation64(x, r["n"]), H.butterfly(x, r["n"])), key


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbol_is_declared_and_bound():
    argtypes, restype = _lib._PROTOTYPES["ct_attn_rot_qdq"]
    assert len(argtypes) == 13 and restype is ctypes.c_int
    assert "ct_attn_rot_qdq" in _lib.EXPORTED_SYMBOLS
    with open(os.path.join(ROOT, "include", "ct_hip.h")) as f:
        header = f.read()
    assert "int ct_attn_rot_qdq(const ct_attn_tensor* tensors, int n, int rot_size, int rot_mask, int mode, int kind, int bits, int xdt, int sdt," in header
    assert ctypes.sizeof(_lib.AttnTensor) == 120  # ct_attn_tensor is unchanged: 15 64-bit words
    with open(os.path.join(ROOT, "compressed_tensors_amd", "csrc", "ct_attn_rot.hip")) as f:
        src = f.read()
    assert 'extern "C" int ct_attn_rot_qdq(' in src and '#include "ct_attn.h"' in src and '#include "ct_hadamard.h"' in src
    for name in ("plan_attn_rot_qdq", "attn_rotated_fake_quantize", "attn_rotated_quantize", "attn_rotated_fake_quantize_pair"):
        assert callable(getattr(codec, name)) and name in codec.__all__
    assert callable(transform.fuse_attention_quantization) and modeling.ROTATED_MEASURED_FASTER is codec.ATTN_ROTATED_MEASURED_FASTER


# ---- the hand-off ----------------------------------------------------------------------------------------------------------------------
def test_take_prequantized_per_base_name():
    mod = torch.nn.Module()
    q, k, v, x = (torch.ones(2) for _ in range(4))
    for name, t in (("q", q), ("k", k), ("v", v)):
        dynamic.remember_prequantized(mod, t, name)
    dynamic.remember_prequantized(mod, x)  # "input": the default, the attribute it always had
    assert dynamic._PREQUANTIZED in mod.__dict__ and dynamic._PREQUANTIZED == "_ct_prequantized_input"
    assert not dynamic.take_prequantized(mod, k, "q")  # another tensor: no, and the reference is gone
    assert not dynamic.take_prequantized(mod, q, "q")
    assert dynamic.take_prequantized(mod, k, "k") and not dynamic.take_prequantized(mod, k, "k")  # once
    assert not dynamic.take_prequantized(mod, v, "weight") and not dynamic.take_prequantized(mod, v, "output")  # other names never hit ...
    assert dynamic.take_prequantized(mod, v, "v")  # ... and clear nothing
    assert dynamic.take_prequantized(mod, x, "input") and not any(a.startswith("_ct_prequantized") for a in mod.__dict__)
    gone = torch.ones(2)
    dynamic.remember_prequantized(mod, gone, "q")
    clone = gone.clone()
    del gone
    assert not dynamic.take_prequantized(mod, clone, "q")  # a weak reference: nothing is kept alive


class _Stubs:
    """the launches replaced by CPU arithmetic: rotate = +1, quantize = *2; the fused calls do both and are counted"""

    def __init__(self, monkeypatch, fusable=True):
        self.calls = []
        monkeypatch.setitem(codec.ATTN_ROTATED_MEASURED_FASTER, "single", True)
        monkeypatch.setitem(codec.ATTN_ROTATED_MEASURED_FASTER, "pair", True)
        monkeypatch.setattr(codec, "_attn_rot_fusable", lambda *a, **k: fusable)
        monkeypatch.setattr(codec, "_attn_rot_pair_fusable", lambda *a, **k: fusable)
        monkeypatch.setattr(kvcache, "_static_pair_args", lambda module, k, v, args: getattr(module, "k_scale", None) is not None)
        monkeypatch.setattr(codec, "hadamard_transform", lambda x, size, **kw: self.calls.append("rotate") or x + 1)
        monkeypatch.setattr(codec, "attn_fake_quantize", lambda x, s, z=None, **kw: self.calls.append("qdq") or x * 2)
        monkeypatch.setattr(codec, "attn_fake_quantize_pair", lambda k, v, *a, **kw: self.calls.append("pair") or (k * 2, v * 2))
        monkeypatch.setattr(codec, "attn_rotated_fake_quantize", lambda x, size, s, z=None, **kw: self.calls.append("rot_qdq") or (x + 1) * 2)
        monkeypatch.setattr(codec, "attn_rotated_fake_quantize_pair", lambda k, v, size, *a, **kw: self.calls.append("rot_pair") or ((k + 1) * 2, v * 2))


def _attention(static=True):
    """an attention module as the hooks see it: a scheme, scales, and the two rotations of apply_transform_config"""
    attn = torch.nn.Module()
    args = cta.QuantizationArgs(num_bits=8, type="float", symmetric=True, strategy="attn_head", dynamic=not static)
    attn.quantization_scheme = cta.QuantizationScheme(targets=["LlamaAttention"], input_activations=args)
    for name in ("q_scale", "k_scale", "v_scale"):
        setattr(attn, name, torch.ones(2, 1, 1))
    scheme = cta.TransformScheme("hadamard", [cta.TransformArgs("LlamaAttention", "q_attn")], head_dim=16)
    rot = transform.HadamardTransform(16, scheme, scheme.apply[0], torch.nn.Module)
    q, k = tapply.QueryRotation(rot), tapply.KeyRotation(rot)
    q.fuse_quantization = k.fuse_quantization = True
    return attn, args, q, k


def test_fused_hooks_hand_their_tensors_to_the_consumers(monkeypatch):
    stubs = _Stubs(monkeypatch)
    attn, args, qrot, krot = _attention()
    x = torch.ones(1, 2, 3, 16)
    q = qrot(attn, x)
    assert stubs.calls == ["rot_qdq"] and torch.equal(q, (x + 1) * 2)
    assert dynamic.forward_quantize(attn, q, "q", args) is q and stubs.calls == ["rot_qdq"]  # identity: untouched, nothing launched
    k, v = krot(attn, x, x * 3)
    assert stubs.calls == ["rot_qdq", "rot_pair"]
    k2, v2 = modeling.quantize_key_value(attn, k, v, args)
    assert k2 is k and v2 is v and stubs.calls == ["rot_qdq", "rot_pair"]
    assert not any(a.startswith("_ct_prequantized") for a in attn.__dict__)
    # identity only: a clone of the remembered tensor is quantized again
    q = qrot(attn, x)
    out = dynamic.forward_quantize(attn, q.clone(), "q", args)
    assert stubs.calls[-2:] == ["rot_qdq", "qdq"] and torch.equal(out, q * 2)
    # K replaced by a later hook, V not: K goes through the ordinary single call, V comes back untouched
    k, v = krot(attn, x, x * 3)
    stubs.calls.clear()
    k2, v2 = modeling.quantize_key_value(attn, k.clone(), v, args)
    assert stubs.calls == ["qdq"] and v2 is v and torch.equal(k2, k * 2)
    # nobody pre-quantized: the pair launch, as always
    stubs.calls.clear()
    modeling.quantize_key_value(attn, x, x, args)
    assert stubs.calls == ["pair"]


@pytest.mark.parametrize("how", ["disabled", "no_scheme", "dynamic", "global_scale", "no_scale", "plan", "constants", "not_opted_in"])
def test_predicate_false_rotates_only(monkeypatch, how):
    stubs = _Stubs(monkeypatch, fusable=how != "plan")
    attn, args, qrot, krot = _attention(static=how != "dynamic")
    if how == "disabled":
        attn.quantization_enabled = False
    elif how == "no_scheme":
        del attn.quantization_scheme
    elif how == "global_scale":
        attn.q_global_scale = attn.k_global_scale = torch.ones(1)
    elif how == "no_scale":
        del attn.q_scale, attn.k_scale
    elif how == "constants":
        monkeypatch.setitem(codec.ATTN_ROTATED_MEASURED_FASTER, "single", False)
        monkeypatch.setitem(codec.ATTN_ROTATED_MEASURED_FASTER, "pair", False)
    elif how == "not_opted_in":
        qrot.fuse_quantization = krot.fuse_quantization = False
    x = torch.ones(1, 2, 3, 16)
    assert torch.equal(qrot(attn, x), x + 1)
    k, v = krot(attn, x, x * 3)
    assert torch.equal(k, x + 1) and torch.equal(v, x * 3)
    assert stubs.calls == ["rotate", "rotate"] and not any(a.startswith("_ct_prequantized") for a in attn.__dict__)


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=32, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2, head_dim=16,
                      max_position_embeddings=16)
    return LlamaForCausalLM(cfg).eval()


def test_fuse_attention_quantization_wants_the_rotation_to_be_the_last_pre_hook():
    pytest.importorskip("transformers")
    m = _tiny_llama()
    attns = [mod for name, mod in m.named_modules() if name.endswith("self_attn")]
    modeling.initialize_hooked_attention(m, attns[1])
    modeling.register_query_hook(attns[1], lambda mod, q: None)  # before the rotation: does not matter
    cfg = cta.TransformConfig({"r": cta.TransformScheme("hadamard", [cta.TransformArgs("LlamaAttention", "q_attn"), cta.TransformArgs("LlamaAttention", "k_cache")],
                                                        head_dim=16)})
    cta.apply_transform_config(m, cfg)
    rots = [attn.__dict__[tapply._ATTN_ROTATIONS] for attn in attns]
    assert all(isinstance(r["q"], tapply.QueryRotation) and isinstance(r["k"], tapply.KeyRotation) for r in rots)  # named hooks, findable
    assert all(r["q"].handle.id in attn.impl._forward_pre_hooks and r["k"].handle.id in attn.kv_cache._forward_pre_hooks for r, attn in zip(rots, attns))
    # layer 0: a hook AFTER each rotation -> skipped entirely; layer 1: untouched -> fused
    modeling.register_query_hook(attns[0], lambda mod, q: None)
    modeling.register_value_hook(attns[0], lambda mod, v: None)
    assert transform.fuse_attention_quantization(m) == ["model.layers.1.self_attn"]
    assert not rots[0]["q"].fuse_quantization and not rots[0]["k"].fuse_quantization
    assert rots[1]["q"].fuse_quantization and rots[1]["k"].fuse_quantization
    # only the key side of layer 0 is followed by another hook once the later query hook is gone: the query side alone qualifies
    m2 = _tiny_llama()
    cta.apply_transform_config(m2, cfg)
    a0 = next(mod for name, mod in m2.named_modules() if name.endswith("layers.0.self_attn"))
    modeling.register_key_hook(a0, lambda mod, k: None)
    assert transform.fuse_attention_quantization(m2) == ["model.layers.0.self_attn", "model.layers.1.self_attn"]
    r0 = a0.__dict__[tapply._ATTN_ROTATIONS]
    assert r0["q"].fuse_quantization and not r0["k"].fuse_quantization
    # a float64 rotation is not fused; a model without attention rotations has nothing to fuse
    m3 = _tiny_llama()
    cta.apply_transform_config(m3, cta.TransformConfig({"r": cta.TransformScheme("hadamard", [cta.TransformArgs("LlamaAttention", "q_attn")], head_dim=16,
                                                                                precision=torch.float64)}))
    assert transform.fuse_attention_quantization(m3) == [] and transform.fuse_attention_quantization(_tiny_llama()) == []


def test_the_rotation_hooks_rotate_as_before_the_opt_in(monkeypatch):
    """apply_transform_config is unchanged in effect: the named hooks rotate the query and the key, and pass the value through"""
    stubs = _Stubs(monkeypatch)
    attn, args, qrot, krot = _attention()
    qrot.fuse_quantization = krot.fuse_quantization = False
    x, v = torch.ones(1, 2, 3, 16), torch.zeros(1, 2, 3, 16)
    assert torch.equal(qrot(attn, x), x + 1)
    k2, v2 = krot(attn, x, v)
    assert torch.equal(k2, x + 1) and v2 is v and stubs.calls == ["rotate", "rotate"]


# ---- dispatch follows measurement ------------------------------------------------------------------------------------------------------
def test_as_shipped_the_dispatch_constants_are_measured_faster():
    """a key of ROTATED_MEASURED_FASTER is True only if every row of profiles/attn_rot_bench.jsonl that speaks for it has the verdict
    "faster"; the file holds two runs of the three rows"""
    consts = modeling.ROTATED_MEASURED_FASTER
    assert set(consts) == {"single", "pair"} and all(isinstance(v, bool) for v in consts.values())
    with open(os.path.join(ROOT, "profiles", "attn_rot_bench.jsonl")) as f:
        lines = [json.loads(line) for line in f if line.strip()]
    rows = [r for r in lines if "row" in r]
    verdicts = [v for v in lines if "verdict" in v]
    for name, shape, key in (("rot_prefill_q", [1, 32, 8192, 128], "single"), ("rot_prefill_kv", [1, 8, 8192, 128], "pair"), ("rot_decode_kv", [64, 8, 1, 128], "pair")):
        mine = [r for r in rows if r["row"] == name]
        assert len(mine) >= 2 and {r["run"] for r in mine} >= {0, 1} and all(r["shape"] == shape and r["rotation"] == 128 and r["transposed_view"] for r in mine)
        vs = [v for v in verdicts if v["verdict"] == name]
        assert vs and all(v["key"] == key for v in vs)
        for v in vs:  # the rule of tools/rotated_bench.py
            assert v["faster"] == (v["path_worst_us"] + v["run_spread_us"] < v["baseline_best_us"])
    for key, on in consts.items():
        if on:
            speaking = [v for v in verdicts if v["key"] == key]
            assert speaking and all(v["faster"] for v in speaking), (key, speaking)
