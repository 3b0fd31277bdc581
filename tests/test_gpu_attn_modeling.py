"""The attention / KV-cache hooks (compressed_tensors_amd.modeling) on a 2-layer random Llama on the MI355X: registration, what
reaches the cache and the attention function, launch counts, generate(), the reference's own hooks on the same weights, upstream's
objects under install(patch_forward=True, patch_modeling=True), and the q_attn / k_cache transform locations."""
import collections
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_import  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
LAYERS, HEADS, KV_HEADS, HEAD_DIM = 2, 4, 2, 16


def _model(attn_implementation=None, seed=0):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                      num_key_value_heads=KV_HEADS, head_dim=HEAD_DIM, max_position_embeddings=64)
    m = LlamaForCausalLM(cfg).to(BF16).to(DEV).eval()
    if attn_implementation is not None:
        m.set_attn_implementation(attn_implementation)
    return m


def _ids():
    return (torch.arange(10, device=DEV).reshape(2, 5) * 7 + 3) % 64


def _attentions(m):
    return [mod for name, mod in m.named_modules() if name.endswith("self_attn")]


def _scales(strategy, layer):
    """distinct per head and per layer, so that a wrong head or a wrong module's scale cannot pass"""
    def per(heads, base):
        if strategy == "tensor":
            return torch.tensor([base], dtype=BF16, device=DEV)
        return (base * (1.0 + 0.5 * torch.arange(heads, dtype=torch.float32))).to(BF16).reshape(heads, 1, 1).to(DEV)

    return dict(q_scale=per(HEADS, 0.011 * (layer + 1)), k_scale=per(KV_HEADS, 0.017 * (layer + 1)), v_scale=per(KV_HEADS, 0.007 * (layer + 1)))


def _attach(m, strategy, args_cls, scheme_cls, status=None):
    args = args_cls(num_bits=8, type="float", symmetric=True, strategy=strategy)
    for layer, attn in enumerate(_attentions(m)):
        attn.quantization_scheme = scheme_cls(targets=["LlamaAttention"], input_activations=args)
        if status is not None:
            attn.quantization_status = status
        for name, value in _scales(strategy, layer).items():
            attn.register_parameter(name, torch.nn.Parameter(value, requires_grad=False))
    return args


def _hook_ours(m):
    from compressed_tensors_amd import modeling

    for attn in _attentions(m):
        modeling.initialize_hooked_attention(m, attn)


@pytest.fixture()
def counted():
    from compressed_tensors_amd import _lib

    counts = collections.Counter()
    orig = _lib.call

    def call(name, *a):
        counts[name] += 1
        return orig(name, *a)

    _lib.call = call
    import compressed_tensors_amd.codec as codec_mod

    saved = codec_mod.call
    codec_mod.call = call
    try:
        yield counts
    finally:
        _lib.call = orig
        codec_mod.call = saved


# ---- hooks ---------------------------------------------------------------------------------------------------------------------------
def test_hooks_register_once_fire_everywhere_and_change_nothing():
    from compressed_tensors_amd import modeling

    m = _model()
    ids = _ids()
    with torch.no_grad():
        base = m(ids).logits
    _hook_ours(m)
    fired = collections.Counter()
    for attn in _attentions(m):
        impl, cache, hooks = attn.impl, attn.kv_cache, len(attn._forward_pre_hooks)
        modeling.initialize_hooked_attention(m, attn)  # again: nothing new
        modeling.initialize_hooked_kv_cache(m, attn)
        assert attn.impl is impl and attn.kv_cache is cache and len(attn._forward_pre_hooks) == hooks == 1
        assert isinstance(impl, modeling.QuantizedAttentionImpl) and isinstance(cache, modeling.QuantizedKVCache)
        modeling.register_query_hook(attn, lambda mod, q: fired.update(["q"]))
        modeling.register_key_hook(attn, lambda mod, k: fired.update(["k"]))
        modeling.register_value_hook(attn, lambda mod, v: fired.update(["v"]))
    assert m.config._attn_implementation == modeling.HOOKED_ATTENTION_NAME
    with torch.no_grad():
        got = m(ids).logits
    assert dict(fired) == {"q": LAYERS, "k": LAYERS, "v": LAYERS}
    assert torch.equal(got.view(torch.int16), base.view(torch.int16))  # no scheme: the unhooked model's logits, bit for bit


def test_eager_attention_runs_without_a_registry_entry():
    """"eager" is not in transformers' registry; our impl finds the modeling file's function.  No scheme: the unhooked logits"""
    m = _model("eager")
    ids = _ids()
    with torch.no_grad():
        base = m(ids).logits
    _hook_ours(m)
    from compressed_tensors_amd import modeling

    assert modeling.QuantizedAttentionImpl._original_impl == "eager"
    with torch.no_grad():
        got = m(ids).logits
    assert torch.equal(got.view(torch.int16), base.view(torch.int16))


class _Recorder:
    """the q / k / v states the hooks see, and what then reaches the attention function and the model's cache"""

    def __init__(self, m, monkeypatch):
        from transformers import DynamicCache
        from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS

        from compressed_tensors_amd import modeling

        self.seen = {"q": [], "k": [], "v": []}
        self.query_in, self.cache_in = [], []
        for attn in _attentions(m):
            modeling.register_query_hook(attn, lambda mod, t: self.seen["q"].append((mod, t)))
            modeling.register_key_hook(attn, lambda mod, t: self.seen["k"].append((mod, t)))
            modeling.register_value_hook(attn, lambda mod, t: self.seen["v"].append((mod, t)))
        original = modeling.QuantizedAttentionImpl._original_impl

        def recording_attention(module, query, key, value, *args, **kwargs):
            self.query_in.append(query)
            return modeling.attention._original_attention(module, original)(module, query, key, value, *args, **kwargs)

        ALL_ATTENTION_FUNCTIONS.register("ct_test_recording_attention", recording_attention)
        monkeypatch.setattr(modeling.QuantizedAttentionImpl, "_original_impl", "ct_test_recording_attention")
        update = DynamicCache.update

        def recording_update(cache, key_states, value_states, *args, **kwargs):
            self.cache_in.append((key_states, value_states))
            return update(cache, key_states, value_states, *args, **kwargs)

        monkeypatch.setattr(DynamicCache, "update", recording_update)

    def check(self, strategy):
        from compressed_tensors_amd import codec

        kw = dict(num_bits=8, qtype="float", strategy=strategy)
        assert len(self.query_in) == len(self.seen["q"]) == len(self.cache_in) == len(self.seen["k"]) == len(self.seen["v"]) > 0
        for (mod, q), got in zip(self.seen["q"], self.query_in):
            want = codec.attn_fake_quantize(q, mod.q_scale, None, **kw)
            assert got.stride() == want.stride() and torch.equal(got.view(torch.int16), want.view(torch.int16))
        for (mod, k), (_, v), (got_k, got_v) in zip(self.seen["k"], self.seen["v"], self.cache_in):
            want_k, want_v = codec.attn_fake_quantize(k, mod.k_scale, None, **kw), codec.attn_fake_quantize(v, mod.v_scale, None, **kw)
            assert torch.equal(got_k.view(torch.int16), want_k.view(torch.int16)) and torch.equal(got_v.view(torch.int16), want_v.view(torch.int16))
            assert not torch.equal(got_k, k)  # and it IS quantized


@pytest.mark.parametrize("strategy", ["attn_head", "tensor"])
def test_quantized_states_reach_the_cache_and_the_attention_function(strategy, counted, monkeypatch):
    import compressed_tensors_amd as cta
    from compressed_tensors_amd.modeling import kvcache

    m = _model()
    ids = _ids()
    with torch.no_grad():
        base = m(ids).logits
    _hook_ours(m)
    _attach(m, strategy, cta.QuantizationArgs, cta.QuantizationScheme)
    rec = _Recorder(m, monkeypatch)
    per_forward = 1 + (1 if kvcache.PAIR_MEASURED_FASTER else 2)  # one entry for q; K+V: one (pair) or two
    counted.clear()
    with torch.no_grad():
        logits = m(ids).logits
    assert dict(counted) == {"ct_attn_qdq": LAYERS * per_forward}, counted
    assert rec.seen["k"][0][1].shape == (2, KV_HEADS, 5, HEAD_DIM) and not rec.seen["k"][0][1].is_contiguous()  # the transposed view, as passed
    rec.check(strategy)
    assert not torch.equal(logits, base)
    # generate with the default dynamic cache: the decode steps pass S = 1 states
    counted.clear()
    for lst in (*rec.seen.values(), rec.query_in, rec.cache_in):
        lst.clear()
    with torch.no_grad():
        out = m.generate(ids[:1], max_new_tokens=3, do_sample=False)
    assert out.shape == (1, 8)
    steps = len(rec.query_in) // LAYERS
    assert steps == 3 and dict(counted) == {"ct_attn_qdq": steps * LAYERS * per_forward}, (steps, counted)
    assert {t.shape[2] for _, t in rec.seen["k"]} == {5, 1}
    rec.check(strategy)
    # quantization_enabled = False: the base logits again
    for attn in _attentions(m):
        attn.quantization_enabled = False
    counted.clear()
    with torch.no_grad():
        off = m(ids).logits
    assert torch.equal(off.view(torch.int16), base.view(torch.int16)) and not counted


def test_pair_form_in_the_cache_equals_two_calls(counted):
    """whatever PAIR_MEASURED_FASTER dispatches today, both forms of quantize_key_value give the same states"""
    import compressed_tensors_amd as cta
    from compressed_tensors_amd.modeling import quantize_key_value

    m = _model()
    args = _attach(m, "attn_head", cta.QuantizationArgs, cta.QuantizationScheme)
    attn = _attentions(m)[1]
    k = torch.randn(2, 5, KV_HEADS, HEAD_DIM, device=DEV).to(BF16).transpose(1, 2)
    v = torch.randn(2, 5, KV_HEADS, HEAD_DIM, device=DEV).to(BF16).transpose(1, 2)
    counted.clear()
    k1, v1 = quantize_key_value(attn, k, v, args, pair=True)
    assert dict(counted) == {"ct_attn_qdq": 1}
    k2, v2 = quantize_key_value(attn, k, v, args, pair=False)
    assert dict(counted) == {"ct_attn_qdq": 3}
    assert torch.equal(k1.view(torch.int16), k2.view(torch.int16)) and torch.equal(v1.view(torch.int16), v2.view(torch.int16))
    assert k1.stride() == k2.stride() == k.stride()


# ---- against the reference itself ------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not ref_import.available(), reason="no reference on this machine")
@pytest.mark.parametrize("impl", ["sdpa", "eager"])
@pytest.mark.parametrize("strategy", ["attn_head", "tensor"])
def test_logits_equal_the_references_hooks(strategy, impl, counted, monkeypatch):
    ref_import.import_reference()
    import compressed_tensors.modeling as up_modeling
    from compressed_tensors.quantization import QuantizationArgs as UpArgs
    from compressed_tensors.quantization import QuantizationScheme as UpScheme
    from compressed_tensors.quantization import QuantizationStatus

    import compressed_tensors_amd as cta
    import compressed_tensors_amd.install as ct_amd

    if impl == "eager":
        # transformers keeps "eager" out of ALL_ATTENTION_FUNCTIONS (it is the modeling file's eager_attention_forward, passed as a
        # default by the attention module), and upstream's QuantizedAttentionImpl looks its original up there: give it the entry
        from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS
        from transformers.models.llama.modeling_llama import eager_attention_forward

        if "eager" not in ALL_ATTENTION_FUNCTIONS:
            monkeypatch.setitem(ALL_ATTENTION_FUNCTIONS._global_mapping, "eager", eager_attention_forward)
    ids = _ids()

    def upstream_model():
        m = _model(impl)
        for attn in _attentions(m):
            up_modeling.initialize_hooked_attention(m, attn)
        _attach(m, strategy, UpArgs, UpScheme, status=QuantizationStatus.FROZEN)
        return m

    up = upstream_model()
    with torch.no_grad():
        want = up(ids).logits  # upstream's hooks, upstream's eager forward_quantize
    assert not counted
    ours = _model(impl)
    _hook_ours(ours)
    _attach(ours, strategy, cta.QuantizationArgs, cta.QuantizationScheme)
    with torch.no_grad():
        got = ours(ids).logits
    assert counted["ct_attn_qdq"] >= 2 * LAYERS
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # upstream's objects with the HIP path installed underneath them
    counted.clear()
    ct_amd.install(patch_forward=True, patch_modeling=True)
    try:
        with torch.no_grad():
            patched = up(ids).logits
    finally:
        ct_amd.uninstall()
    assert counted["ct_attn_qdq"] >= 2 * LAYERS, counted
    assert torch.equal(patched.view(torch.int16), want.view(torch.int16))
    counted.clear()
    with torch.no_grad():
        restored = up(ids).logits  # uninstall() put upstream's forward back
    assert not counted and torch.equal(restored.view(torch.int16), want.view(torch.int16))


# ---- q_attn / k_cache rotations -----------------------------------------------------------------------------------------------------------
def test_attention_transform_locations(monkeypatch):
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import codec, modeling

    m = _model()
    ids = _ids()
    with torch.no_grad():
        base = m(ids).logits
    _hook_ours(m)
    raw = {"q": [], "k": []}
    for attn in _attentions(m):  # registered first: they see the states before the rotation
        modeling.register_query_hook(attn, lambda mod, t: raw["q"].append(t))
        modeling.register_key_hook(attn, lambda mod, t: raw["k"].append(t))
    cfg = cta.TransformConfig({"r": cta.TransformScheme("hadamard", [cta.TransformArgs("LlamaAttention", "q_attn"), cta.TransformArgs("LlamaAttention", "k_cache")],
                                                        head_dim=HEAD_DIM)})
    cta.apply_transform_config(m, cfg)
    assert m.transform_config is cfg and all(len(attn._forward_pre_hooks) == 1 for attn in _attentions(m))  # initialised once
    _attach(m, "attn_head", cta.QuantizationArgs, cta.QuantizationScheme)
    rec = _Recorder(m, monkeypatch)  # registered last: they see the rotated states, which is what is quantized
    with torch.no_grad():
        rotated_logits = m(ids).logits
    assert len(raw["q"]) == len(rec.seen["q"]) == LAYERS
    for name in ("q", "k"):
        for before, (_, after) in zip(raw[name], rec.seen[name]):
            want = codec.hadamard_transform(before.contiguous(), HEAD_DIM)
            assert torch.equal(after.view(torch.int16), want.view(torch.int16))
    rec.check("attn_head")  # the K QDQ's input is the rotated K: rotation first, then quantization
    print("max |logits(rotated q, k) - logits(unrotated, unquantized)| =", float((rotated_logits.float() - base.float()).abs().max()))
    # what is not built raises as before; a model that is not a PreTrainedModel raises upstream's ValueError
    with pytest.raises(ValueError, match="Cannot hook attention of model"):
        cta.apply_transform_config(torch.nn.Sequential(torch.nn.Linear(16, 16)), cfg)
    bad = cta.TransformConfig({"r": cta.TransformScheme("hadamard", [cta.TransformArgs("LlamaAttention", "q_attn")], head_dim=HEAD_DIM, randomize=True)})
    with pytest.raises(NotImplementedError, match="randomize"):
        cta.apply_transform_config(_model(), bad)
