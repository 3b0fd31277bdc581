"""A hookable attention implementation (the surface of upstream's modeling/attention.py): `QuantizedAttentionImpl` is a module
placed between an attention module and the attention function the model was configured with.  It quantizes the query states
(the strided launch of csrc/ct_attn.hip) and calls the original function; as a module it takes `register_query_hook`.

transformers is imported inside the functions that need its registries, so importing this package does not import it."""
import inspect
from typing import Callable, Optional

import torch

from ..quantization.dynamic import forward_quantize
from .kvcache import initialize_hooked_kv_cache

__all__ = ["QuantizedAttentionImpl", "initialize_hooked_attention", "register_query_hook", "IMPL_ATTR", "HOOKED_ATTENTION_NAME"]

IMPL_ATTR = "impl"
HOOKED_ATTENTION_NAME = "ct_hooked_attention"


def _original_attention(module: torch.nn.Module, name: str):
    """the attention function `name` stood for before hooking.  transformers keeps "eager" out of its registry: it is the
    `eager_attention_forward` of the model's own modeling file, which the attention module's forward passes as the default."""
    from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS

    if name == "eager" and name not in ALL_ATTENTION_FUNCTIONS:
        import sys

        eager = getattr(sys.modules.get(type(module).__module__), "eager_attention_forward", None)
        if eager is None:
            raise KeyError(f"{type(module).__module__} has no eager_attention_forward to run the 'eager' attention implementation with")
        return eager
    return ALL_ATTENTION_FUNCTIONS[name]


class QuantizedAttentionImpl(torch.nn.Module):
    """`impl(module, query, key, value, ...)`: the query states are quantized under the attention module's
    `quantization_scheme.input_activations` (unless `quantization_enabled` is False), then the attention function the model had
    before hooking runs ("eager", which transformers does not register, is looked up in the model's modeling file).  One model is
    hooked at a time: the original implementation's name is kept on the class."""

    _original_impl = "eager"

    def __init__(self, config):
        super().__init__()
        self.config = config

    def forward(self, module: torch.nn.Module, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, *args, **kwargs):
        quant_args = getattr(getattr(module, "quantization_scheme", None), "input_activations", None)
        if quant_args is not None and getattr(module, "quantization_enabled", True):
            query = forward_quantize(module, query, "q", quant_args)
        return _original_attention(module, QuantizedAttentionImpl._original_impl)(module, query, key, value, *args, **kwargs)


def _hooked_attention(module: torch.nn.Module, *args, **kwargs):
    impl = getattr(module, IMPL_ATTR, None)
    if impl is None:
        raise AttributeError(f"attention implementation {HOOKED_ATTENTION_NAME!r} is selected, but {type(module).__name__} has no {IMPL_ATTR!r} submodule")
    return impl(module, *args, **kwargs)


def initialize_hooked_attention(model, module: torch.nn.Module) -> None:
    """attach a QuantizedAttentionImpl (and a QuantizedKVCache) to the attention `module` of `model` (a PreTrainedModel) and point
    the model's attention implementation at it; initialising again changes nothing"""
    from transformers.masking_utils import ALL_MASK_ATTENTION_FUNCTIONS
    from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS

    if not hasattr(module, IMPL_ATTR):
        module.register_module(IMPL_ATTR, QuantizedAttentionImpl(model.config))
    current = model.config._attn_implementation
    if current != HOOKED_ATTENTION_NAME:
        QuantizedAttentionImpl._original_impl = current
        ALL_ATTENTION_FUNCTIONS.register(HOOKED_ATTENTION_NAME, _hooked_attention)
        ALL_MASK_ATTENTION_FUNCTIONS.register(HOOKED_ATTENTION_NAME, ALL_MASK_ATTENTION_FUNCTIONS[current])  # the mask of the original
        model.set_attn_implementation(HOOKED_ATTENTION_NAME)
        if model.config._attn_implementation != HOOKED_ATTENTION_NAME:
            raise RuntimeError(f"the model kept attention implementation {model.config._attn_implementation!r}")
    initialize_hooked_kv_cache(model, module)


def register_query_hook(module: torch.nn.Module, hook: Callable[[torch.nn.Module, torch.Tensor], Optional[torch.Tensor]]):
    """`hook(module, query_states)` sees the post-rope query states before they are quantized; a tensor it returns replaces them.
    Returns the removable handle."""
    impl: QuantizedAttentionImpl = getattr(module, IMPL_ATTR)
    signature = inspect.signature(impl.forward)

    def pre_hook(_impl, args, kwargs):
        bound = signature.bind(*args, **kwargs)
        replaced = hook(module, bound.arguments["query"])
        if replaced is not None:
            bound.arguments["query"] = replaced
        return bound.args, bound.kwargs

    return impl.register_forward_pre_hook(pre_hook, with_kwargs=True)
