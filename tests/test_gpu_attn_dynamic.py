"""The dynamic group QDQ of strided q / k / v states (csrc/ct_attn_dyn.hip) on the MI355X: against the reference's outputs, scales
and zero points on every fixture case (tests/golden/attn_dynamic*, tools/gen_golden_attn_dynamic.py) with dtype, shape AND strides,
in the strided and in the copy form; against the contiguous kernel on the same values; the pair against the two single calls; scales
only; launch counts and no copies; every bf16 bit pattern as one value of a group; and a 2-layer Llama whose KV cache and query states
run MXFP4 / NVFP4 / FP8 per-(token, head).  Every comparison is bit-exact."""
import collections
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_dynamic_cases as C  # noqa: E402
import ref_import  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "attn_dynamic_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
_GOLDEN = {}
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float8_e4m3fn: torch.uint8,
         torch.uint8: torch.uint8, torch.int8: torch.int8}


def _golden_tensors():
    if not _GOLDEN:
        from safetensors.torch import load_file

        _GOLDEN.update(load_file(os.path.join(GOLDEN, "attn_dynamic.safetensors")))
    return _GOLDEN


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


def _args(r):
    import compressed_tensors_amd as cta

    return cta.QuantizationArgs(**C.preset_args(r))


def _gs(r):
    g = C.global_scale(r)
    return None if g is None else g.to(DEV)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(_BITS[a.dtype]), b.contiguous().view(_BITS[b.dtype]))


def _check(t, want, what):
    assert str(t.dtype).replace("torch.", "") == want["dtype"], (what, t.dtype)
    assert list(t.shape) == want["shape"] and list(t.stride()) == want["strides"], (what, t.shape, t.stride(), want["strides"])
    assert C.sha(t) == want["sha256"], f"{what} differs from the reference"


def _kernels_of(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    events = list(prof.events())
    kernels = [e.name for e in events if e.device_type == torch.autograd.DeviceType.CUDA]
    ops = [e.name for e in events if e.device_type == torch.autograd.DeviceType.CPU]
    return kernels, ops


# ---- every fixture case ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_attn_dynamic_matches_the_reference(key, counted):
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.quantization import dynamic

    entry = MANIFEST[key]
    r = entry["recipe"]
    x = C.make_input(r, DEV)
    assert C.sha(x) == entry["x_sha256"] and list(x.stride()) == entry["x_strides"], "the recipe no longer synthesises the reference's input"
    args, gs = _args(r), _gs(r)
    before = x.clone()
    ref = dynamic.dynamic_fake_quantize(x.contiguous(), args, gs, return_qparams=True)
    tensor_form = dynamic.plan_dynamic(x.shape, x.dtype, args, gs).launches() == 2
    expected = C.expected_form(r)
    for form in (("strided", "copy") if expected == "strided" else ("copy",)):
        counted.clear()
        out, scale, zp = codec.attn_dynamic_fake_quantize(x, args, gs, return_qparams=True, form=form)
        torch.cuda.synchronize()
        want = {"ct_attn_dyn_qdq": 1} if form == "strided" else {"ct_dynamic_qdq_tensor" if tensor_form else "ct_dynamic_qdq": 1}
        assert dict(counted) == want, (form, counted)
        _check(out, entry["out"], f"{form}: the output")
        _check(scale, entry["scale"], f"{form}: the scale")
        _check(zp, entry["zp"], f"{form}: the zero point")
        if entry["stored"]:
            stored = _golden_tensors()[f"{key}.out"]
            assert C.canonical_bytes(out) == C.canonical_bytes(stored), f"{form}: the output differs from the stored reference"
        for got, old, what in zip((out, scale, zp), ref, ("output", "scale", "zero point")):
            assert _bits_equal(got, old), f"{form}: the {what} differs from the contiguous kernel's"
        assert C.canonical_bytes(x) == C.canonical_bytes(before), "the input was written"


# ---- the pair ------------------------------------------------------------------------------------------------------------------------
def _pair_inputs(preset):
    rk = C.normalise(dict(D=64, B=2, H=2, S=5, layout="transposed", dtypes="bf16/bf16", preset=preset, salt=3))
    rv = C.normalise(dict(D=96 if preset != "fp8_group64" else 192, B=2, H=2, S=7, layout="fused_v", dtypes="bf16/bf16", preset=preset, salt=4))
    assert rk["preset"] == rv["preset"] == preset
    return rk, C.make_input(rk, DEV), C.make_input(rv, DEV)


@pytest.mark.parametrize("preset", ["mxfp4", "nvfp4_gs", "fp8_group64", "int4_group32_asym"])
def test_pair_equals_the_two_single_calls_in_one_launch(preset, counted):
    """K and V of different head dims, shapes and layouts (and different global scales) in ONE launch"""
    from compressed_tensors_amd import codec

    rk, k, v = _pair_inputs(preset)
    args, kg = _args(rk), _gs(rk)
    vg = None if kg is None else kg * 3.0
    want_k = codec.attn_dynamic_fake_quantize(k, args, kg, return_qparams=True, form="strided")
    want_v = codec.attn_dynamic_fake_quantize(v, args, vg, return_qparams=True, form="strided")
    counted.clear()
    got_k, got_v = codec.attn_dynamic_fake_quantize_pair(k, v, args, kg, vg, return_qparams=True, form="strided", pair=True)
    torch.cuda.synchronize()
    assert dict(counted) == {"ct_attn_dyn_qdq": 1}, counted
    for got, want in ((got_k, want_k), (got_v, want_v)):
        for g, w in zip(got, want):
            assert _bits_equal(g, w) and g.stride() == w.stride()
    kernels, _ = _kernels_of(lambda: codec.attn_dynamic_fake_quantize_pair(k, v, args, kg, vg, form="strided", pair=True))
    assert len(kernels) == 1 and "attn_dyn" in kernels[0], kernels
    counted.clear()
    two_k, two_v = codec.attn_dynamic_fake_quantize_pair(k, v, args, kg, vg, form="strided", pair=False)
    assert dict(counted) == {"ct_attn_dyn_qdq": 2}, counted
    assert _bits_equal(two_k, want_k[0]) and _bits_equal(two_v, want_v[0])


def test_pair_with_one_global_scale_is_two_launches(counted):
    from compressed_tensors_amd import codec

    rk, k, v = _pair_inputs("nvfp4_gs")
    args, kg = _args(rk), _gs(rk)
    got_k, got_v = codec.attn_dynamic_fake_quantize_pair(k, v, args, kg, None, form="strided", pair=True)
    assert dict(counted) == {"ct_attn_dyn_qdq": 2}, counted
    assert _bits_equal(got_k, codec.attn_dynamic_fake_quantize(k, args, kg, form="strided"))
    assert _bits_equal(got_v, codec.attn_dynamic_fake_quantize(v, args, None, form="strided"))


# ---- scales only -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["mxfp4.bf16.transposed.2x8x33x128", "nvfp4_gs.bf16.transposed.2x8x1x128", "int4_group32_asym.bf16.transposed.2x8x33x128",
                                 "fp8_token.bf16.transposed.2x8x1x128", "fp8_token.bf16.transposed.2x8x33x128"])
def test_scales_only(key, counted):
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.quantization import dynamic

    entry = MANIFEST[key]
    r = entry["recipe"]
    x, args, gs = C.make_input(r, DEV), _args(r), _gs(r)
    for form in ("strided", "copy"):
        scale, zp = codec.attn_dynamic_qparams(x, args, gs, form=form)
        _check(scale, entry["scale"], "the scale")
        _check(zp, entry["zp"], "the zero point")
    counted.clear()
    scale, zp = dynamic.compute_dynamic_scales_and_zp(x, args, None, gs)  # the public entry on the view: it raised on the parent
    assert sum(counted.values()) == 1, counted
    _check(scale, entry["scale"], "the scale")
    _check(zp, entry["zp"], "the zero point")


# ---- launches and copies ---------------------------------------------------------------------------------------------------------------
def test_transposed_view_is_read_in_place():
    from compressed_tensors_amd import codec

    r = MANIFEST["mxfp4.bf16.transposed.2x8x33x128"]["recipe"]
    x, args = C.make_input(r, DEV), _args(r)
    kernels, ops = _kernels_of(lambda: codec.attn_dynamic_fake_quantize(x, args, form="strided"))
    assert len(kernels) == 1 and "attn_dyn" in kernels[0], kernels
    assert not [o for o in ops if o in ("aten::contiguous", "aten::clone", "aten::copy_", "aten::_to_copy")], ops
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = codec.attn_dynamic_fake_quantize(x, args, form="strided")
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert out.stride() == x.stride()
    # the copy form: the copy in, the contiguous kernel, the copy into the reference's strides
    kernels, ops = _kernels_of(lambda: codec.attn_dynamic_fake_quantize(x, args, form="copy"))
    assert len(kernels) == 3 and sum("dyn_group_kernel" in k for k in kernels) == 1, kernels
    torch.cuda.synchronize()


# ---- every bf16 bit pattern ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,group", [("fp8_groupD", 128), ("mxfp4", 32), ("nvfp4_gs", 16)])
def test_every_bf16_bit_pattern_as_one_value_of_a_group(preset, group):
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.quantization import dynamic

    D = 128
    groups = 65536
    rows = groups * group // D
    g = torch.Generator().manual_seed(group)
    body = (torch.randn(groups, group, generator=g) * 3.0).to(BF16)
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16)
    body[torch.arange(groups), torch.arange(groups) % group] = pats  # the pattern sits at every position of a group in turn
    B, H = 2, 4
    x = body.reshape(B, rows // (B * H), H, D).to(DEV).transpose(1, 2)  # strided as a Llama's states are
    r = dict(D=D, preset=preset)
    args, gs = _args(r), _gs(r)
    out, scale, zp = codec.attn_dynamic_fake_quantize(x, args, gs, return_qparams=True, form="strided")
    ref = dynamic.dynamic_fake_quantize(x.contiguous(), args, gs, return_qparams=True)
    assert out.stride() == x.stride()
    for got, old in zip((out, scale, zp), ref):
        assert _bits_equal(got, old)


# ---- what the parent could not do --------------------------------------------------------------------------------------------------------
def test_forward_quantize_takes_a_transposed_key_state(counted):
    """on the parent this raised NotImplementedError("the dynamic QDQ kernels take contiguous GPU activations")"""
    from compressed_tensors_amd import _lib, codec
    from compressed_tensors_amd.quantization import dynamic

    assert hasattr(_lib.load(), "ct_attn_dyn_qdq") and callable(codec.attn_dynamic_fake_quantize)
    entry = MANIFEST["mxfp4.bf16.transposed.2x8x33x128"]
    r = entry["recipe"]
    x, args = C.make_input(r, DEV), _args(r)
    attn = torch.nn.Module()
    out = dynamic.forward_quantize(attn, x, "k", args)
    _check(out, entry["out"], "forward_quantize's output")
    assert sum(counted.values()) == 1, counted


# ---- modelling ---------------------------------------------------------------------------------------------------------------------------
LAYERS, HEADS, KV_HEADS, HEAD_DIM = 2, 4, 2, 32
SCHEMES = {
    "mxfp4": dict(C.DYN_PRESETS["mxfp4"]),
    "nvfp4": dict(C.DYN_PRESETS["nvfp4"]),
    "fp8_head": dict(num_bits=8, type="float", strategy="group", group_size=HEAD_DIM, symmetric=True, dynamic=True),
}


def _model(impl, seed=0):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                      num_key_value_heads=KV_HEADS, head_dim=HEAD_DIM, max_position_embeddings=64)
    m = LlamaForCausalLM(cfg).to(BF16).to(DEV).eval()
    m.set_attn_implementation(impl)
    return m


def _attentions(m):
    return [mod for name, mod in m.named_modules() if name.endswith("self_attn")]


def _ids():
    return (torch.arange(10, device=DEV).reshape(2, 5) * 7 + 3) % 64


def _calibrated_global_scales(m, ids):
    """generate_gparam of the states one forward passes, by the strided observer (codec.attn_observe_global_scale)"""
    from compressed_tensors_amd import codec, modeling

    found = collections.defaultdict(dict)
    handles = []
    for i, attn in enumerate(_attentions(m)):
        modeling.initialize_hooked_attention(m, attn)
        for name, register in (("q", modeling.register_query_hook), ("k", modeling.register_key_hook), ("v", modeling.register_value_hook)):
            def hook(mod, t, i=i, name=name):
                found[i][f"{name}_global_scale"] = codec.attn_observe_global_scale(t, codec.attn_observe_state(1, DEV)).reshape(1).clone()

            handles.append(register(attn, hook))
    with torch.no_grad():
        m(ids)
    for h in handles:
        h.remove()
    return found


def _decode(m, ids, steps=2):
    """prefill plus `steps` greedy decode steps through the model's own cache: the logits of every step"""
    from transformers import DynamicCache

    cache, logits, cur = DynamicCache(), [], ids
    with torch.no_grad():
        for _ in range(steps + 1):
            out = m(cur, past_key_values=cache, use_cache=True)
            logits.append(out.logits)
            cur = out.logits[:, -1:].argmax(-1)
    return logits


@pytest.mark.parametrize("impl", ["sdpa", "eager"])
@pytest.mark.parametrize("scheme", sorted(SCHEMES))
def test_llama_logits_equal_the_contiguous_kernels_in_hooks(scheme, impl, counted, monkeypatch):
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import modeling
    from compressed_tensors_amd.quantization import dynamic

    monkeypatch.setitem(cta.codec.ATTN_DYNAMIC_MEASURED_FASTER, "single", True)  # the strided launch, whatever is dispatched today
    monkeypatch.setitem(cta.codec.ATTN_DYNAMIC_MEASURED_FASTER, "pair", True)
    ids = _ids()
    args = cta.QuantizationArgs(**SCHEMES[scheme])
    scales = _calibrated_global_scales(_model(impl), ids) if scheme == "nvfp4" else collections.defaultdict(dict)

    # ours: the scheme on the attention modules, the hooks of compressed_tensors_amd.modeling
    ours = _model(impl)
    for i, attn in enumerate(_attentions(ours)):
        modeling.initialize_hooked_attention(ours, attn)
        attn.quantization_scheme = cta.QuantizationScheme(targets=["LlamaAttention"], input_activations=args)
        for name, value in scales[i].items():
            attn.register_parameter(name, torch.nn.Parameter(value.clone(), requires_grad=False))
    counted.clear()
    got = _decode(ours, ids)
    per_forward = 2  # q alone; K and V in one launch
    assert dict(counted) == {"ct_attn_dyn_qdq": 3 * LAYERS * per_forward}, counted

    # the same model without a scheme: hooks make the states contiguous and send them through the parent's dynamic_fake_quantize
    plain = _model(impl)

    def through_parent(name):
        def hook(mod, *states):
            res = []
            for n, t in zip(name, states):
                q = dynamic.dynamic_fake_quantize(t.contiguous(), args, getattr(mod, f"{n}_global_scale", None))
                res.append(torch.empty_like(t).copy_(q))  # the view's own strides, as the attention function got them before
            return res[0] if len(res) == 1 else tuple(res)

        return hook

    for i, attn in enumerate(_attentions(plain)):
        modeling.initialize_hooked_attention(plain, attn)
        for name, value in scales[i].items():
            attn.register_parameter(name, torch.nn.Parameter(value.clone(), requires_grad=False))
        modeling.register_query_hook(attn, through_parent("q"))
        modeling.register_key_value_hook(attn, through_parent("kv"))
    counted.clear()
    want = _decode(plain, ids)
    assert "ct_attn_dyn_qdq" not in counted and counted["ct_dynamic_qdq"] == 3 * LAYERS * 3, counted
    unquantized = _decode(_model(impl), ids)
    for g, w, u in zip(got, want, unquantized):
        assert torch.equal(g.view(torch.int16), w.view(torch.int16))
        assert not torch.equal(g, u)  # and the states ARE quantized

    if not ref_import.available():
        return
    # upstream's hooks and upstream's eager ops, then the same objects with the HIP path installed underneath them
    ref_import.import_reference()
    import compressed_tensors.modeling as up_modeling
    from compressed_tensors.quantization import QuantizationArgs as UpArgs
    from compressed_tensors.quantization import QuantizationScheme as UpScheme
    from compressed_tensors.quantization import QuantizationStatus

    import compressed_tensors_amd.install as ct_amd

    if impl == "eager":
        from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS
        from transformers.models.llama.modeling_llama import eager_attention_forward

        if "eager" not in ALL_ATTENTION_FUNCTIONS:
            monkeypatch.setitem(ALL_ATTENTION_FUNCTIONS._global_mapping, "eager", eager_attention_forward)
    up = _model(impl)
    for i, attn in enumerate(_attentions(up)):
        up_modeling.initialize_hooked_attention(up, attn)
        attn.quantization_scheme = UpScheme(targets=["LlamaAttention"], input_activations=UpArgs(**SCHEMES[scheme]))
        attn.quantization_status = QuantizationStatus.FROZEN
        for name, value in scales[i].items():
            attn.register_parameter(name, torch.nn.Parameter(value.clone(), requires_grad=False))
    counted.clear()
    eager = _decode(up, ids)
    assert "ct_attn_dyn_qdq" not in counted and "ct_dynamic_qdq" not in counted, counted  # upstream's own ops (its fp4 cast may be a registered backend)
    for g, e in zip(got, eager):
        assert torch.equal(g.view(torch.int16), e.view(torch.int16))
    ct_amd.install(patch_forward=True, patch_modeling=True)
    try:
        patched = _decode(up, ids)
    finally:
        ct_amd.uninstall()
    assert counted["ct_attn_dyn_qdq"] >= 3 * LAYERS, counted
    for p, e in zip(patched, eager):
        assert torch.equal(p.view(torch.int16), e.view(torch.int16))
