"""Model-free checkpoint conversion (reference entrypoints/convert/): safetensors in,
GPU decompress, safetensors out — the on-disk consumer of the decompress hot path."""
from .autoawq import AutoAWQConverter
from .convert_checkpoint import convert_checkpoint, convert_file, exec_jobs, validate_file
from .converters import CompressedTensorsDequantizer, Converter, build_inverse_weight_maps
from .dense import FP8BlockQuantizer, FP8DynamicQuantizer, MXFP4Quantizer, MXFP8Quantizer, PackQuantizedQuantizer, W8A8Quantizer
from .fp8block import FP8BlockDequantizer
from .fp8block_mxfp4 import FP8BlockToMXFP4Converter
from .fp8block_transcode import FP8BlockToMXFP8Converter, FP8BlockToNVFP4Converter
from .modelopt import ModelOptNvfp4Converter
from .nvfp4_mxfp4 import NVFP4ToMXFP4Converter

__all__ = ["convert_checkpoint", "convert_file", "validate_file", "exec_jobs", "Converter", "build_inverse_weight_maps",
           "CompressedTensorsDequantizer", "AutoAWQConverter", "FP8BlockDequantizer", "FP8BlockQuantizer", "ModelOptNvfp4Converter",
           "MXFP8Quantizer", "FP8DynamicQuantizer", "W8A8Quantizer", "PackQuantizedQuantizer", "MXFP4Quantizer", "FP8BlockToMXFP4Converter",
           "FP8BlockToMXFP8Converter", "FP8BlockToNVFP4Converter", "NVFP4ToMXFP4Converter"]
