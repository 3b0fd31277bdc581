"""Attention and KV-cache hooks (upstream's `compressed_tensors.modeling`) over the strided q / k / v QDQ of csrc/ct_attn.hip."""
from .attention import HOOKED_ATTENTION_NAME, IMPL_ATTR, QuantizedAttentionImpl, initialize_hooked_attention, register_query_hook
from .calibration import OBSERVE_PAIR_MEASURED_FASTER, calibrate_attention, calibrate_global_scales, initialize_attn_qparams
from .kvcache import (KV_CACHE_ATTR, PAIR_MEASURED_FASTER, ROTATED_MEASURED_FASTER, QuantizedKVCache, initialize_hooked_kv_cache, quantize_key_value,
                      register_key_hook, register_key_value_hook, register_value_hook)

__all__ = ["QuantizedAttentionImpl", "QuantizedKVCache", "initialize_hooked_attention", "initialize_hooked_kv_cache", "register_query_hook",
           "register_key_hook", "register_value_hook", "IMPL_ATTR", "KV_CACHE_ATTR", "HOOKED_ATTENTION_NAME", "PAIR_MEASURED_FASTER",
           "ROTATED_MEASURED_FASTER", "quantize_key_value", "register_key_value_hook", "initialize_attn_qparams", "calibrate_attention", "calibrate_global_scales",
           "OBSERVE_PAIR_MEASURED_FASTER"]
