"""ModelOpt NVFP4 checkpoints -> compressed-tensors nvfp4-pack-quantized (reference entrypoints/convert/converters/modelopt_nvfp4.py).

Renames and inverts per-module tensors; the packed FP4 payload and its FP8 block scales move over untouched (the same tensor
objects), so there is no kernel on this path."""
from typing import Any, Dict, Iterable, Optional, Set

import torch

from ...quantization.quant_args import QuantizationArgs
from .converters import Converter, _ConfigDict, match_name, match_quantizable_tensors

__all__ = ["ModelOptNvfp4Converter"]

# the reference's NVFP4 preset (quantization/quant_scheme.py) as its QuantizationArgs.model_dump() writes it
_NVFP4_WEIGHTS = {"num_bits": 4, "type": "float", "symmetric": True, "group_size": 16, "strategy": "tensor_group", "block_structure": None,
                  "dynamic": False, "actorder": None, "scale_dtype": "torch.float8_e4m3fn", "zp_dtype": None,
                  "observer": "memoryless_minmax", "observer_kwargs": {}}
_NVFP4_INPUTS = dict(_NVFP4_WEIGHTS, dynamic="local", observer="static_minmax")


def _value(v):
    return getattr(v, "value", v)


def _args_dump(args) -> Optional[Dict[str, Any]]:
    """a kv_cache_scheme as the reference's QuantizationArgs.model_dump() writes it: the reference's own object dumps itself,
    this package's QuantizationArgs gets the reference's observer inference (quant_args.py, validate_model_after)"""
    if args is None:
        return None
    if hasattr(args, "model_dump"):
        d = args.model_dump()
        return {k: (str(v) if isinstance(v, torch.dtype) else v) for k, v in d.items()}
    dynamic = _value(args.dynamic)
    observer = None if dynamic is True else ("minmax" if dynamic == "local" else "memoryless_minmax")
    zp_dtype = None if args.symmetric else str(args.zp_dtype or args.pytorch_dtype())
    return {"num_bits": args.num_bits, "type": _value(args.type), "symmetric": args.symmetric, "group_size": args.group_size,
            "strategy": _value(args.strategy), "block_structure": args.block_structure, "dynamic": dynamic,
            "actorder": _value(args.actorder), "scale_dtype": str(args.scale_dtype) if args.scale_dtype is not None else None,
            "zp_dtype": zp_dtype, "observer": observer, "observer_kwargs": {}}


class ModelOptNvfp4Converter(Converter):
    """Convert the tensors of a ModelOpt NVFP4 checkpoint to the compressed-tensors NVFP4 convention, and optionally the
    kv_cache_scheme's scales"""

    def __init__(self, ignore: Iterable[str] = tuple(), targets: Iterable[str] = tuple(), kv_cache_scheme: Optional[QuantizationArgs] = None):
        self.ignore = ignore
        self.targets = targets
        self.kv_cache_scheme = kv_cache_scheme
        self.param_names = ["input_scale", "weight", "weight_scale", "weight_scale_2"]
        if self.kv_cache_scheme is not None:
            self.param_names += ["k_scale", "v_scale"]

    def process(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """modelopt_nvfp4.py:38-90, in place:
        - input_scale x    -> input_global_scale 1 / x
        - weight           -> weight_packed (the same tensor)
        - weight_scale     stays (the same tensor)
        - weight_scale_2 x -> weight_global_scale 1 / x
        - k_scale / v_scale cast to kv_cache_scheme.scale_dtype (bfloat16 by default)"""
        for module_name, name in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=self.param_names):
            param_name = name.rpartition(".")[-1]
            if param_name == "input_scale":
                tensors[f"{module_name}.input_global_scale"] = 1 / tensors[name]
                del tensors[name]
            elif param_name == "weight":
                tensors[f"{module_name}.weight_packed"] = tensors[name]
                del tensors[name]
            elif param_name == "weight_scale_2":
                tensors[f"{module_name}.weight_global_scale"] = 1 / tensors[name]
                del tensors[name]
            elif param_name in ("k_scale", "v_scale"):
                tensors[name] = tensors[name].to(self.kv_cache_scheme.scale_dtype or torch.bfloat16)
        return tensors

    def validate(self, tensors: Dict[str, torch.Tensor]):
        """modelopt_nvfp4.py:92-123: no scale tensor may sit outside the targeted modules (names only)"""
        targeted = {name for _, name in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=self.param_names)}
        disallowed_names = ["input_scale", "weight_scale", "weight_scale_2", "k_scale", "v_scale"]
        for name in tensors.keys():
            if name in targeted or any(match_name(name, ign) for ign in self.ignore):
                continue
            if name.rpartition(".")[-1] in disallowed_names:
                raise ValueError(f"Hit unexpected non-targeted tensor {name}")

    def get_dependencies(self, weight_name: str) -> Set[str]:
        module_name, _, param_name = weight_name.rpartition(".")
        if (any(match_name(module_name, t) for t in self.targets) and not any(match_name(module_name, i) for i in self.ignore)
                and param_name == "weight"):
            deps = {f"{module_name}.input_scale", f"{module_name}.weight_scale", f"{module_name}.weight_scale_2"}
            if self.kv_cache_scheme:
                if module_name.endswith("k_proj"):
                    deps.add(f"{module_name}.k_scale")
                if module_name.endswith("v_proj"):
                    deps.add(f"{module_name}.v_scale")
            return deps
        return set()

    def create_config(self) -> _ConfigDict:
        """the reference's `create_config().model_dump()` (modelopt_nvfp4.py:149-163)"""
        return _ConfigDict({
            "config_groups": {"config_group_0": {"targets": list(self.targets), "weights": dict(_NVFP4_WEIGHTS),
                                                 "input_activations": dict(_NVFP4_INPUTS), "output_activations": None,
                                                 "format": "nvfp4-pack-quantized"}},
            "quant_method": "compressed-tensors",
            "kv_cache_scheme": _args_dump(self.kv_cache_scheme),
            "format": "nvfp4-pack-quantized",
            "quantization_status": "compressed",
            "global_compression_ratio": None,
            "ignore": list(self.ignore),
        })
