from .dynamic import compute_dynamic_scales_and_zp, forward_quantize
from .forward import calculate_range, dequantize, fake_quantize, quantize
from .observer import MinMaxObserver
from .quant_args import (
    ActivationOrdering,
    DynamicType,
    QuantizationArgs,
    QuantizationScheme,
    QuantizationStatus,
    QuantizationStrategy,
    QuantizationType,
)
from .utils import calculate_qparams_from_weight, is_module_quantized

__all__ = [
    "quantize",
    "dequantize",
    "fake_quantize",
    "calculate_range",
    "compute_dynamic_scales_and_zp",
    "forward_quantize",
    "calculate_qparams_from_weight",
    "is_module_quantized",
    "MinMaxObserver",
    "QuantizationArgs",
    "QuantizationScheme",
    "QuantizationStatus",
    "QuantizationStrategy",
    "QuantizationType",
    "ActivationOrdering",
    "DynamicType",
]
