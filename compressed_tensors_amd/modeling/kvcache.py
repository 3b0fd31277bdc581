"""A hookable KV cache for attention modules (the surface of upstream's modeling/kvcache.py): `QuantizedKVCache` sits in front of
whatever cache the model was called with, quantizes the key and value states on their way in, and passes them on to that cache's
`update`.  Being a torch.nn.Module, it takes forward pre-hooks: `register_key_hook` / `register_value_hook` (transforms,
calibration observers).

The QDQ itself is the strided launch of csrc/ct_attn.hip: the states arrive as `(B, S, H, D).transpose(1, 2)` views and are read
in place.  transformers is only imported inside `initialize_hooked_kv_cache`'s callers' models: nothing here imports it."""
import inspect
import weakref
from typing import Callable, Optional, Tuple

import torch

from .. import codec
from ..quantization.dynamic import forward_quantize, take_prequantized
from ..quantization.quant_args import enum_value

__all__ = ["QuantizedKVCache", "initialize_hooked_kv_cache", "register_key_hook", "register_value_hook", "register_key_value_hook", "KV_CACHE_ATTR",
           "PAIR_MEASURED_FASTER", "ROTATED_MEASURED_FASTER", "DYNAMIC_MEASURED_FASTER", "quantize_key_value"]

KV_CACHE_ATTR = "kv_cache"

# K and V of one cache update in ONE launch (codec.attn_fake_quantize_pair) instead of two: dispatched only where
# tools/attn_bench.py measured the pair faster than the two single launches by more than the spread between its runs, at the
# prefill AND the decode shape.  profiles/attn_bench.jsonl: k+v (1, 8, 8192, 128) 32.1-32.3 us against 36.5-37.4, k+v
# (64, 8, 1, 128) 16.1-16.2 against 22.7-23.1, run spreads 0.9 and 0.3 us.  False would mean: two launches.
PAIR_MEASURED_FASTER = True

# the head-dim rotation of q / k in the QDQ's launch (csrc/ct_attn_rot.hip): {"single": bool, "pair": bool}, the very dict
# codec.attn_rotated_* dispatch by — held to profiles/attn_rot_bench.jsonl by tests/test_attn_rotated.py
ROTATED_MEASURED_FASTER = codec.ATTN_ROTATED_MEASURED_FASTER

# dynamic group schemes (MXFP4 / MXFP8 / NVFP4 / FP8 groups) on K and V: {"single": bool, "pair": bool}, the very dict
# codec.attn_dynamic_* dispatch by — held to profiles/attn_dynamic_bench.jsonl by tests/test_attn_dynamic.py
DYNAMIC_MEASURED_FASTER = codec.ATTN_DYNAMIC_MEASURED_FASTER


def _static_pair_args(module, key_states, value_states, quant_args) -> bool:
    """the pair launch serves: static tensor / attn_head arguments, GPU states, scales on the module, no global scale"""
    if enum_value(getattr(quant_args, "dynamic", False)) in (True, "local"):
        return False
    if enum_value(quant_args.strategy) not in ("tensor", "attn_head"):
        return False
    if not (key_states.is_cuda and value_states.is_cuda and key_states.numel() and value_states.numel()):
        return False
    if getattr(module, "k_global_scale", None) is not None or getattr(module, "v_global_scale", None) is not None:
        return False
    return getattr(module, "k_scale", None) is not None and getattr(module, "v_scale", None) is not None


def _dynamic_pair_args(module, key_states, value_states, quant_args) -> bool:
    """the dynamic pair launch serves: dynamic group / tensor_group arguments, GPU states of one dtype, and global scales on both
    states or on neither (the global scale is a compile-time branch of the kernel)"""
    if enum_value(getattr(quant_args, "dynamic", False)) not in (True, "local"):
        return False
    if enum_value(quant_args.strategy) not in ("group", "tensor_group"):
        return False
    if not (key_states.is_cuda and value_states.is_cuda and key_states.numel() and value_states.numel() and key_states.dtype == value_states.dtype):
        return False
    return (getattr(module, "k_global_scale", None) is None) == (getattr(module, "v_global_scale", None) is None)


def quantize_key_value(module, key_states, value_states, quant_args, single=forward_quantize, pair: Optional[bool] = None):
    """forward_quantize(module, key_states, "k", args), forward_quantize(module, value_states, "v", args): as one launch where the
    pair form is dispatched (`pair`; None: PAIR_MEASURED_FASTER for static arguments, DYNAMIC_MEASURED_FASTER["pair"] for dynamic
    group arguments) and the plan takes both, through `single` twice otherwise.  A state that IS the tensor a fused rotation hook
    handed off (object identity) comes back untouched."""
    done_k, done_v = take_prequantized(module, key_states, "k"), take_prequantized(module, value_states, "v")
    if done_k or done_v:  # transform.fuse_attention_quantization: the rotation's pre-hook quantized these very tensors in its launch
        return (key_states if done_k else single(module, key_states, "k", quant_args),
                value_states if done_v else single(module, value_states, "v", quant_args))
    if (PAIR_MEASURED_FASTER if pair is None else pair) and _static_pair_args(module, key_states, value_states, quant_args):
        try:
            return codec.attn_fake_quantize_pair(
                key_states, value_states, module.k_scale, module.v_scale, getattr(module, "k_zero_point", None), getattr(module, "v_zero_point", None),
                num_bits=int(quant_args.num_bits), strategy=enum_value(quant_args.strategy), qtype=enum_value(getattr(quant_args, "type", "int")))
        except NotImplementedError:
            pass  # a combination the launch does not serve: the two calls decide
    if (DYNAMIC_MEASURED_FASTER["pair"] if pair is None else pair) and _dynamic_pair_args(module, key_states, value_states, quant_args) \
            and getattr(module, "weight_g_idx", None) is None:
        try:
            return codec.attn_dynamic_fake_quantize_pair(key_states, value_states, quant_args, getattr(module, "k_global_scale", None),
                                                         getattr(module, "v_global_scale", None), pair=True)
        except NotImplementedError:
            pass  # arguments no dynamic kernel computes: the two calls decide
    return single(module, key_states, "k", quant_args), single(module, value_states, "v", quant_args)


class QuantizedKVCache(torch.nn.Module):
    """Stands in for the `past_key_values` argument of one attention module.  `update` is the cache protocol's method; it runs this
    module's forward, so hooks registered on it fire for every cache update.  The model's own cache is kept as a weak reference
    for the duration of one attention forward and does the actual caching (sliding windows, static shapes, offloading: all its)."""

    def __init__(self, config, attn_module: torch.nn.Module):
        super().__init__()
        self.config = config
        self.attn_module = weakref.ref(attn_module)  # the parent holds this module: no cycle
        self.past_key_values = None

    def update(self, *args, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        return self(*args, **kwargs)

    def forward(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        module = self.attn_module()
        quant_args = getattr(getattr(module, "quantization_scheme", None), "input_activations", None)
        if quant_args is not None and getattr(module, "quantization_enabled", True):
            key_states, value_states = quantize_key_value(module, key_states, value_states, quant_args)
        wrapped = self.past_key_values() if self.past_key_values is not None else None
        self.past_key_values = None
        if wrapped is None:
            return key_states, value_states
        return wrapped.update(key_states, value_states, *args, **kwargs)

    def add_past_key_values(self, past_key_values) -> None:
        self.past_key_values = None if past_key_values is None else weakref.ref(past_key_values)


def _swap_in_hooked_cache(module: torch.nn.Module, args, kwargs):
    """forward pre-hook of the attention module: the cache the model passed is remembered, the hooked cache goes in its place"""
    name = "past_key_values" if "past_key_values" in inspect.signature(module.forward).parameters else "past_key_value"
    cache: QuantizedKVCache = getattr(module, KV_CACHE_ATTR)
    cache.add_past_key_values(kwargs.get(name))
    kwargs[name] = cache
    return args, kwargs


def initialize_hooked_kv_cache(model, module: torch.nn.Module) -> None:
    """attach a QuantizedKVCache to the attention `module` of `model` (a PreTrainedModel); a module that has one is left alone"""
    if hasattr(module, KV_CACHE_ATTR):
        return
    module.register_module(KV_CACHE_ATTR, QuantizedKVCache(model.config.get_text_config(decoder=True), module))
    module.register_forward_pre_hook(_swap_in_hooked_cache, with_kwargs=True)


def _register_states_hook(module: torch.nn.Module, names: Tuple[str, ...], hook: Callable):
    """a forward pre-hook of the module's cache that hands `hook` the arguments `names` of the cache's forward; what it returns —
    a tensor for one name, a tuple of as many tensors for several, None for nothing — replaces them"""
    cache: QuantizedKVCache = getattr(module, KV_CACHE_ATTR)
    signature = inspect.signature(cache.forward)

    def pre_hook(_cache, args, kwargs):
        bound = signature.bind(*args, **kwargs)
        replaced = hook(module, *(bound.arguments[name] for name in names))
        if replaced is not None:
            bound.arguments.update(zip(names, (replaced,) if len(names) == 1 else replaced, strict=True))
        return bound.args, bound.kwargs

    return cache.register_forward_pre_hook(pre_hook, with_kwargs=True)


def register_key_hook(module: torch.nn.Module, hook: Callable[[torch.nn.Module, torch.Tensor], Optional[torch.Tensor]]):
    """`hook(module, key_states)` sees the post-rope key states before they are quantized and cached; a tensor it returns
    replaces them.  Returns the removable handle."""
    return _register_states_hook(module, ("key_states",), hook)


def register_value_hook(module: torch.nn.Module, hook: Callable[[torch.nn.Module, torch.Tensor], Optional[torch.Tensor]]):
    """the same for the value states"""
    return _register_states_hook(module, ("value_states",), hook)


def register_key_value_hook(module: torch.nn.Module, hook: Callable[[torch.nn.Module, torch.Tensor, torch.Tensor], Optional[Tuple[torch.Tensor, torch.Tensor]]]):
    """`hook(module, key_states, value_states)` sees both states of one cache update; a (key_states, value_states) pair it
    returns replaces them.  Returns the removable handle."""
    return _register_states_hook(module, ("key_states", "value_states"), hook)
