"""The calibration front half of the static q / k / v QDQ: `initialize_attn_qparams` registers the scale / zero-point
parameters of an attention module (the behaviour of upstream's lifecycle/initialize.py:154-335 for attention), and
`calibrate_attention` observes the states of every such module while the model runs and writes those parameters in place — the
launches of csrc/ct_attn_observe.hip, on the views the hooks of this package see, before the QDQ of the same forward reads them.

`calibrate_global_scales` is the same for the NVFP4 preset's activations (`tensor_group`, `dynamic="local"`): it registers `input_global_scale` /
`output_global_scale` and writes them from the inputs / outputs of every such module while the model runs (kind 2 of the same launch).

Nothing here runs unless it is called: no existing path launches an observer."""
import contextlib
from typing import Optional

import torch

from ..quantization.observer import MinMaxObserver, observe_key_value
from ..quantization.quant_args import enum_value
from .attention import IMPL_ATTR, register_query_hook
from .kvcache import KV_CACHE_ATTR, register_key_value_hook

__all__ = ["initialize_attn_qparams", "calibrate_attention", "calibrate_global_scales", "OBSERVE_PAIR_MEASURED_FASTER", "OBSERVER_ATTR"]

# K and V of one cache update through ONE ct_attn_observe (codec.attn_observe_pair) instead of two: dispatched only where
# tools/attn_observe_bench.py measured the pair faster than the two single calls by more than the spread between its runs, at the
# prefill AND the decode shape (the convention of kvcache.PAIR_MEASURED_FASTER; tests/test_attn_observe.py holds it to
# profiles/attn_observe_bench.jsonl).  False would mean: two calls.
OBSERVE_PAIR_MEASURED_FASTER = True

OBSERVER_ATTR = "{}_observer"  # the submodule an observer is registered as while calibrate_attention is active


def _heads_and_dim(config):
    """(query heads, key / value heads, head dim) of a decoder config, by upstream's rules (utils/helpers.py:436-492)"""
    if hasattr(config, "num_attention_heads"):
        heads = config.num_attention_heads
    elif hasattr(config, "hidden_size") and hasattr(config, "head_dim"):
        heads = config.hidden_size // config.head_dim
    else:
        raise ValueError(f"Cannot determine num_attention_heads from config. Config must define either `num_attention_heads` or both "
                         f"`hidden_size` and `head_dim`. {config}")
    if not hasattr(config, "num_key_value_heads"):
        raise ValueError(f"Cannot determine num_key_value_heads from config. Config must define `num_key_value_heads`. {config}")
    if hasattr(config, "head_dim"):
        head_dim = config.head_dim
    elif hasattr(config, "hidden_size") and hasattr(config, "num_attention_heads"):
        head_dim = config.hidden_size // config.num_attention_heads
    else:
        raise ValueError(f"Cannot determine head_dim from config. Config must define either `head_dim` or both `hidden_size` and "
                         f"`num_attention_heads`. {config}")
    return heads, config.num_key_value_heads, head_dim


def _validate_attention_scheme(scheme) -> None:
    if scheme.weights is not None:
        raise ValueError("Cannot apply weight quantization to attention. Instead, target the (q|k|v)_proj submodule layers of attention")
    if scheme.input_activations is None:
        raise ValueError("Cannot apply attention quantization without specifying input activations")
    if scheme.output_activations is not None:
        raise ValueError("Cannot apply output quantization to attention")


def _zp_dtype(args) -> torch.dtype:
    """quant_args.py:401-405 for the arguments attention takes: float8_e4m3fn for FLOAT, int8 for INT up to 8 bits"""
    given = getattr(args, "zp_dtype", None)
    return given if given is not None else args.pytorch_dtype()


def _initialize_qparams(module, base_name: str, args, heads: int, dtype: torch.dtype, device, force_zero_point: bool) -> None:
    dynamic = enum_value(getattr(args, "dynamic", False))
    if dynamic is True:
        return
    strategy = enum_value(args.strategy)
    if strategy == "tensor_group":
        module.register_parameter(f"{base_name}_global_scale", torch.nn.Parameter(torch.empty(1, dtype=torch.float32, device=device), requires_grad=False))
    if dynamic == "local":
        return
    if strategy == "tensor":
        shape = (1,)
    elif strategy == "attn_head":
        shape = (heads, 1, 1)
    elif strategy == "token":
        raise ValueError("Cannot perform static token quantization")
    else:
        raise NotImplementedError(f"static {strategy!r} parameters of attention states are not implemented by the MI355X path (tensor and attn_head are)")
    if dtype not in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        dtype = torch.float16
    module.register_parameter(f"{base_name}_scale", torch.nn.Parameter(torch.empty(shape, dtype=dtype, device=device), requires_grad=False))
    if force_zero_point or not args.symmetric:
        module.register_parameter(f"{base_name}_zero_point", torch.nn.Parameter(torch.zeros(shape, dtype=_zp_dtype(args), device=device), requires_grad=False))


def initialize_attn_qparams(module: torch.nn.Module, scheme=None, force_zero_point: bool = True) -> None:
    """register `{q,k,v}_scale` (empty, in the dtype of the module's parameters) and `{q,k,v}_zero_point` (zeros of
    `args.zp_dtype`; only for asymmetric arguments unless `force_zero_point`) of shape (heads, 1, 1) — `attn_head` — or (1,) —
    `tensor`: q where the hooked attention implementation is attached, k / v where the hooked cache is.  `scheme`: None takes the
    module's `quantization_scheme`; the scheme is kept on the module."""
    scheme = scheme if scheme is not None else getattr(module, "quantization_scheme", None)
    if scheme is None:
        return
    impl, kv_cache = getattr(module, IMPL_ATTR, None), getattr(module, KV_CACHE_ATTR, None)
    if impl is None and kv_cache is None:
        raise ValueError(f"Attention module has quantization scheme but no {IMPL_ATTR} or {KV_CACHE_ATTR} attributes. Please ensure that these "
                         "attributes are initialized using `apply_quantization_config`.")
    _validate_attention_scheme(scheme)
    config = kv_cache.config if kv_cache is not None else impl.config
    if kv_cache is None and hasattr(config, "get_text_config"):
        config = config.get_text_config(decoder=True)
    heads, kv_heads, _ = _heads_and_dim(config)
    first = next(module.parameters())
    args = scheme.input_activations
    if impl is not None:
        _initialize_qparams(module, "q", args, heads, first.dtype, first.device, force_zero_point)
    if kv_cache is not None:
        _initialize_qparams(module, "k", args, kv_heads, first.dtype, first.device, force_zero_point)
        _initialize_qparams(module, "v", args, kv_heads, first.dtype, first.device, force_zero_point)
    module.quantization_scheme = scheme


def _static_attention_args(module):
    """the arguments of an attention module whose scales an observer can fill, or None"""
    if getattr(module, IMPL_ATTR, None) is None and getattr(module, KV_CACHE_ATTR, None) is None:
        return None
    args = getattr(getattr(module, "quantization_scheme", None), "input_activations", None)
    if args is None or enum_value(getattr(args, "dynamic", False)) in (True, "local"):
        return None
    return args


def _observe_into(module, name: str, state: torch.Tensor) -> None:
    observer = getattr(module, OBSERVER_ATTR.format(name))
    observer(state, scale=getattr(module, f"{name}_scale"), zero_point=getattr(module, f"{name}_zero_point", None))


def _query_hook(module, query):
    _observe_into(module, "q", query)


def _key_value_hook(module, key, value):
    pair = OBSERVE_PAIR_MEASURED_FASTER and key.dtype == value.dtype and module.k_scale.dtype == module.v_scale.dtype
    if not pair:
        _observe_into(module, "k", key)
        _observe_into(module, "v", value)
        return
    observe_key_value(module.k_observer, module.v_observer, key, value, k_scale=module.k_scale, v_scale=module.v_scale,
                      k_zero_point=getattr(module, "k_zero_point", None), v_zero_point=getattr(module, "v_zero_point", None))


@contextlib.contextmanager
def calibrate_attention(model: torch.nn.Module, observer: Optional[str] = None):
    """While active, every attention module of `model` that carries a static scheme and `{q,k,v}_scale` parameters
    (initialize_attn_qparams) has its query and key / value states observed on every forward; each observation writes the module's
    own scale / zero-point parameters in place, in stream order BEFORE the QDQ of the same forward reads them — no host wait.
    `observer`: "memoryless_minmax" (each forward's own extremes) or "static_minmax" (the running extremes since entry); None:
    the arguments' own.  On exit the hooks and the observers are removed; the parameters keep what the last forward wrote."""
    handles, registered = [], []
    try:
        for module in list(model.modules()):  # the observers registered below are modules too
            args = _static_attention_args(module)
            if args is None:
                continue
            names = [n for n in ("q", "k", "v") if getattr(module, f"{n}_scale", None) is not None]
            for name in names:
                module.register_module(OBSERVER_ATTR.format(name), MinMaxObserver(name, args, module, observer))
                registered.append((module, OBSERVER_ATTR.format(name)))
            if "q" in names and getattr(module, IMPL_ATTR, None) is not None:
                handles.append(register_query_hook(module, _query_hook))
            if "k" in names and "v" in names and getattr(module, KV_CACHE_ATTR, None) is not None:
                handles.append(register_key_value_hook(module, _key_value_hook))
        yield model
    finally:
        for handle in handles:
            handle.remove()
        for module, attr in registered:
            if attr in module._modules:
                del module._modules[attr]


def _global_scale_args(module, base_name: str):
    """the `tensor_group` activation arguments of a module's scheme whose global scale an observer can fill, or None"""
    args = getattr(getattr(module, "quantization_scheme", None), f"{base_name}_activations", None)
    if args is None or enum_value(args.strategy) != "tensor_group" or enum_value(getattr(args, "dynamic", False)) != "local":
        return None
    return args


def _input_global_scale_hook(module, args):
    if args and isinstance(args[0], torch.Tensor) and args[0].numel():
        module.input_observer.get_global_scale(args[0], module.input_global_scale)


def _output_global_scale_hook(module, args, output):
    if isinstance(output, torch.Tensor) and output.numel():
        module.output_observer.get_global_scale(output, module.output_global_scale)


@contextlib.contextmanager
def calibrate_global_scales(model: torch.nn.Module, observer: Optional[str] = None):
    """While active, every module of `model` whose scheme has `tensor_group`, `dynamic="local"` input (or output) activations — the NVFP4 preset's
    — has `generate_gparam` of its inputs (outputs) written into its `input_global_scale` (`output_global_scale`) on every forward: a forward
    pre-hook (a forward hook for outputs) launches the observer on the tensor as it arrives, in place through its strides, in stream order BEFORE the
    module's own forward_quantize reads the parameter — no host wait, no eager reduction.  A missing parameter is registered as upstream's
    initialize registers it (float32 (1,), no grad, on the device of the module's parameters); an existing one is kept and written in place.
    `observer`: "static_minmax" (the extremes of every forward since entry: the preset's) or "memoryless_minmax" (each forward's own); None: the
    arguments' own.  On exit the hooks and the observers are removed; the parameters keep what the last forward wrote."""
    handles, registered = [], []
    try:
        for module in list(model.modules()):  # the observers registered below are modules too
            for base_name, register, hook in (("input", "register_forward_pre_hook", _input_global_scale_hook),
                                              ("output", "register_forward_hook", _output_global_scale_hook)):
                args = _global_scale_args(module, base_name)
                if args is None:
                    continue
                if getattr(module, f"{base_name}_global_scale", None) is None:
                    first = next(module.parameters(), None)
                    device = first.device if first is not None else None
                    module.register_parameter(f"{base_name}_global_scale", torch.nn.Parameter(torch.empty(1, dtype=torch.float32, device=device), requires_grad=False))
                module.register_module(OBSERVER_ATTR.format(base_name), MinMaxObserver(base_name, args, module, observer))
                registered.append((module, OBSERVER_ATTR.format(base_name)))
                handles.append(getattr(module, register)(hook))
        yield model
    finally:
        for handle in handles:
            handle.remove()
        for module, attr in registered:
            if attr in module._modules:
                del module._modules[attr]
