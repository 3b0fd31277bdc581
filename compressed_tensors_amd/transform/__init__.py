"""Hadamard rotations (upstream `transform/`): the configuration surface, the HadamardTransform module and
apply_transform_config for the deterministic Sylvester type (csrc/ct_hadamard.hip) and, from a given weight constructor, the
random-hadamard type of size K * 2^m (RandomHadamardTransform, csrc/ct_hadamard_k.hip)."""
from .apply import apply_transform_config, fuse_attention_quantization, fuse_input_quantization, match_named_modules
from .config import TRANSFORM_CONFIG_NAME, TransformArgs, TransformConfig, TransformLocation, TransformScheme
from .hadamard import HadamardTransform, get_transform_size, transform_dim
from .random_hadamard import HadamardFactors, RandomHadamardTransform, factor_hadamard_weight, transform_transposed

__all__ = [
    "TransformLocation",
    "TransformArgs",
    "TransformScheme",
    "TransformConfig",
    "TRANSFORM_CONFIG_NAME",
    "HadamardTransform",
    "RandomHadamardTransform",
    "HadamardFactors",
    "factor_hadamard_weight",
    "transform_transposed",
    "get_transform_size",
    "transform_dim",
    "apply_transform_config",
    "fuse_input_quantization",
    "fuse_attention_quantization",
    "match_named_modules",
]
