"""Hadamard rotations (upstream `transform/`): the configuration surface, the HadamardTransform module and
apply_transform_config for the deterministic Sylvester type, on the kernels of csrc/ct_hadamard.hip."""
from .apply import apply_transform_config, fuse_input_quantization, match_named_modules
from .config import TRANSFORM_CONFIG_NAME, TransformArgs, TransformConfig, TransformLocation, TransformScheme
from .hadamard import HadamardTransform, get_transform_size, transform_dim

__all__ = [
    "TransformLocation",
    "TransformArgs",
    "TransformScheme",
    "TransformConfig",
    "TRANSFORM_CONFIG_NAME",
    "HadamardTransform",
    "get_transform_size",
    "transform_dim",
    "apply_transform_config",
    "fuse_input_quantization",
    "match_named_modules",
]
