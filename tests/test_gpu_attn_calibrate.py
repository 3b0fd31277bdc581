"""The calibration lifecycle of the static q / k / v QDQ on the 2-layer random Llama of test_gpu_attn_modeling.py, on the MI355X:
initialize_attn_qparams registers the reference's parameters, calibrate_attention fills them from the states the hooks see —
before the QDQ of the same forward reads them — and leaves nothing behind."""
import collections
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_import  # noqa: E402
from test_gpu_attn_modeling import BF16, DEV, HEADS, KV_HEADS, LAYERS, _attentions, _hook_ours, _model  # noqa: E402

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn


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


def _initialised(strategy="attn_head", **args_kw):
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import modeling

    m = _model()
    _hook_ours(m)
    args = cta.QuantizationArgs(**dict(dict(num_bits=8, type="float", symmetric=True, strategy=strategy), **args_kw))
    for attn in _attentions(m):
        modeling.initialize_attn_qparams(attn, cta.QuantizationScheme(targets=["LlamaAttention"], input_activations=args))
    return m, args


def _batches():
    return (torch.arange(10, device=DEV).reshape(2, 5) * 7 + 3) % 64, (torch.arange(14, device=DEV).reshape(2, 7) * 11 + 5) % 64


@pytest.mark.parametrize("strategy", ["attn_head", "tensor"])
def test_initialize_attn_qparams_registers_the_references_parameters(strategy):
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import modeling

    m, _ = _initialised(strategy)
    for attn in _attentions(m):
        q_shape, kv_shape = ((HEADS, 1, 1), (KV_HEADS, 1, 1)) if strategy == "attn_head" else ((1,), (1,))
        for name, shape in (("q", q_shape), ("k", kv_shape), ("v", kv_shape)):
            scale, zp = getattr(attn, f"{name}_scale"), getattr(attn, f"{name}_zero_point")
            assert isinstance(scale, torch.nn.Parameter) and not scale.requires_grad and scale.shape == shape and scale.dtype == BF16 and scale.device == DEV
            assert isinstance(zp, torch.nn.Parameter) and zp.shape == shape and zp.dtype == F8 and not zp.float().any()  # zp_dtype of FLOAT arguments
    # INT arguments: int8 zero points; a symmetric scheme without force_zero_point registers none; q only with the impl, k / v only with the cache
    m = _model()
    _hook_ours(m)
    attn = _attentions(m)[0]
    int8 = cta.QuantizationScheme(targets=["LlamaAttention"], input_activations=cta.QuantizationArgs(num_bits=8, symmetric=True, strategy="attn_head"))
    modeling.initialize_attn_qparams(attn, int8, force_zero_point=False)
    assert attn.k_scale.shape == (KV_HEADS, 1, 1) and not hasattr(attn, "k_zero_point") and attn.quantization_scheme is int8
    modeling.initialize_attn_qparams(attn, int8)
    assert attn.q_zero_point.dtype == torch.int8 and attn.v_zero_point.shape == (KV_HEADS, 1, 1)
    bare = _attentions(_model())[0]
    with pytest.raises(ValueError, match="no impl or kv_cache attributes"):
        modeling.initialize_attn_qparams(bare, int8)
    modeling.initialize_hooked_kv_cache(m, bare)  # the cache alone: k and v, no q
    modeling.initialize_attn_qparams(bare, int8)
    assert hasattr(bare, "k_scale") and hasattr(bare, "v_scale") and not hasattr(bare, "q_scale")
    with pytest.raises(ValueError, match="Cannot apply weight quantization to attention"):
        modeling.initialize_attn_qparams(attn, cta.QuantizationScheme(targets=[], weights=int8.input_activations, input_activations=int8.input_activations))


def _reference_qparams(mn, mx, args_kw):
    """calculate_qparams of the extremes: the reference's own where it is on this machine, and the repo's CPU oracle always"""
    import oracle as O

    rows = torch.stack([mn.flatten(), mx.flatten()], dim=1).cpu()  # one row per entry holding exactly its extremes
    want = O.calculate_qparams_float(rows, kind="fp8").reshape(mn.shape)
    if ref_import.available():
        ref_import.import_reference()
        from compressed_tensors.quantization import QuantizationArgs as UpArgs
        from compressed_tensors.quantization.utils import calculate_qparams

        up_scale, up_zp = calculate_qparams(mn.cpu(), mx.cpu(), UpArgs(**args_kw))
        assert torch.equal(up_scale, want) and up_zp.dtype == F8 and not up_zp.float().any()
    return want


@pytest.mark.parametrize("strategy", ["attn_head", "tensor"])
def test_calibrate_attention_fills_the_scales_the_same_forward_reads(strategy, counted):
    from compressed_tensors_amd import modeling

    m, args = _initialised(strategy)
    seen = collections.defaultdict(list)  # (layer, name) -> the states of every forward, as the hooks see them
    for layer, attn in enumerate(_attentions(m)):
        modeling.register_query_hook(attn, lambda mod, t, layer=layer: seen[layer, "q"].append(t.clone()))
        modeling.register_key_hook(attn, lambda mod, t, layer=layer: seen[layer, "k"].append(t.clone()))
        modeling.register_value_hook(attn, lambda mod, t, layer=layer: seen[layer, "v"].append(t.clone()))
    first, second = _batches()
    pair = modeling.calibration.OBSERVE_PAIR_MEASURED_FASTER
    counted.clear()
    with modeling.calibrate_attention(m, observer="static_minmax"), torch.no_grad():
        assert all(hasattr(attn, "q_observer") and hasattr(attn, "k_observer") and hasattr(attn, "v_observer") for attn in _attentions(m))
        m(first)
        logits = m(second).logits
    assert counted["ct_attn_observe"] == 2 * LAYERS * (2 if pair else 3), counted
    dims = (0, 2, 3) if strategy == "attn_head" else (0, 1, 2, 3)
    shape_of = lambda t: (t.shape[1], 1, 1) if strategy == "attn_head" else (1,)  # noqa: E731
    for layer, attn in enumerate(_attentions(m)):
        for name in ("q", "k", "v"):
            a, b = seen[layer, name]
            assert a.shape[2] == 5 and b.shape[2] == 7
            mn = torch.minimum(a.amin(dim=dims), b.amin(dim=dims)).reshape(shape_of(a))
            mx = torch.maximum(a.amax(dim=dims), b.amax(dim=dims)).reshape(shape_of(a))
            want = _reference_qparams(mn, mx, dict(num_bits=8, type="float", symmetric=True, strategy=strategy))
            got = getattr(attn, f"{name}_scale")
            assert got.shape == want.shape and torch.equal(got.data.cpu().view(torch.int16), want.view(torch.int16)), (layer, name, got.flatten().tolist(), want.flatten().tolist())
            assert not getattr(attn, f"{name}_zero_point").float().any()
    # a model that carries those scales by hand computes the second batch's logits bit for bit: the QDQ read what the observer wrote
    by_hand, _ = _initialised(strategy)
    for src, dst in zip(_attentions(m), _attentions(by_hand)):
        for name in ("q", "k", "v"):
            getattr(dst, f"{name}_scale").data.copy_(getattr(src, f"{name}_scale").data)
    counted.clear()
    with torch.no_grad():
        want_logits = by_hand(second).logits
    assert "ct_attn_observe" not in counted and counted["ct_attn_qdq"] > 0
    assert torch.equal(logits, want_logits)
    # nothing is left behind: no hook, no observer, no observer launch
    for attn in _attentions(m):
        assert len(attn.impl._forward_pre_hooks) == 1 and len(attn.kv_cache._forward_pre_hooks) == 2  # the recording hooks of this test only
        assert not any(hasattr(attn, f"{name}_observer") for name in ("q", "k", "v"))
    counted.clear()
    with torch.no_grad():
        after = m(second).logits
    assert "ct_attn_observe" not in counted and torch.equal(after, want_logits)


def test_memoryless_calibration_keeps_the_last_forward_only():
    from compressed_tensors_amd import modeling

    m, _ = _initialised("attn_head")
    first, second = _batches()
    with modeling.calibrate_attention(m), torch.no_grad():  # the arguments name no observer: memoryless_minmax
        m(first)
        m(second)
    last = [attn.k_scale.data.clone() for attn in _attentions(m)]
    with modeling.calibrate_attention(m), torch.no_grad():
        m(second)
    assert all(torch.equal(a, attn.k_scale.data) for a, attn in zip(last, _attentions(m)))
    with pytest.raises(NotImplementedError, match="minmax"):
        with modeling.calibrate_attention(m, observer="minmax"):
            pass
    assert all(len(attn.impl._forward_pre_hooks) == 0 and not hasattr(attn, "q_observer") for attn in _attentions(m))
