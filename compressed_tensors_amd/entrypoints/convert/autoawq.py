"""AutoAWQ GEMM checkpoints -> compressed-tensors pack-quantized (reference entrypoints/convert/converters/autoawq.py:24-257).

MI355X design of `AutoAWQConverter.process`: the qweight / qzeros / scales of ALL targeted modules of a shard are staged to the
GPU through one pinned buffer and one copy, and ONE `ct_awq_repack_batch` launch per shard turns them into weight_packed /
weight_zero_point / weight_scale (a 4-bit transpose, csrc/ct_awq.hip); the results come back through one pinned buffer.  Nothing
is unpacked, reordered or re-packed on the host."""
import re
from typing import Any, Dict, Iterable, Set

import torch

from .converters import Converter, _ConfigDict, match_name
from .safetensors_io import CONFIG_NAME, get_checkpoint_files
from .staging import ReadyDict, device_outputs, launch_tables, return_to_host, settle, stage_inputs

__all__ = ["AutoAWQConverter"]


class AutoAWQConverter(Converter):
    """Convert AutoAWQ GEMM tensors (qweight / qzeros / scales) to pack-quantized int4 tensors (weight_packed / weight_zero_point /
    weight_scale / weight_shape)."""

    AWQ_REVERSE_ORDER = [0, 4, 1, 5, 2, 6, 3, 7]

    def __init__(self, bits: int = 4, group_size: int = 128, zero_point: bool = True, version: str = "gemm",
                 ignore: Iterable[str] = ("lm_head",), targets: Iterable[str] = ("Linear",), *, device=None):
        if bits != 4:
            raise ValueError("AutoAWQConverter currently supports only 4-bit weights")
        if version != "gemm":
            raise ValueError(f"Unsupported AutoAWQ version: {version}")
        self.bits = bits
        self.group_size = group_size
        self.zero_point = zero_point
        self.version = version
        self.ignore = list(ignore)
        self.targets = list(targets)
        self.device = torch.device(device) if device is not None else None
        # as CompressedTensorsDequantizer: `process` may return before its D2H copies have landed (a ReadyDict) when this is set or
        # inside `streaming_results()`; otherwise it synchronises first
        self.stream_results = False

    @classmethod
    def from_pretrained(cls, model_name_or_path, targets: Iterable[str] = ("Linear",), trust_remote_code: bool = False) -> "AutoAWQConverter":
        """the quantization_config of a local checkpoint's config.json (or of its text_config), read without transformers"""
        import json

        files = get_checkpoint_files(model_name_or_path)
        path = files.get(CONFIG_NAME)
        if path is None:
            raise ValueError(f"Could not find {CONFIG_NAME} in {model_name_or_path}")
        with open(path) as f:
            config = json.load(f)
        autoawq_config = config.get("quantization_config")
        if autoawq_config is None:
            autoawq_config = (config.get("text_config") or {}).get("quantization_config")
        if autoawq_config is None:
            raise ValueError("Model config does not contain quantization_config")
        if autoawq_config.get("quant_method") != "awq":
            raise ValueError("Model config is not an AutoAWQ config")
        return cls.from_autoawq_config(autoawq_config, targets=targets)

    @classmethod
    def from_autoawq_config(cls, autoawq_config: Dict[str, Any], targets: Iterable[str] = ("Linear",)) -> "AutoAWQConverter":
        ignore = ["lm_head"]
        for module in autoawq_config.get("modules_to_not_convert") or []:
            ignore.append(f"re:.*{re.escape(module)}.*")
        return cls(bits=autoawq_config.get("bits", 4), group_size=autoawq_config.get("group_size", 128),
                   zero_point=autoawq_config.get("zero_point", True), version=autoawq_config.get("version", "gemm"), ignore=ignore,
                   targets=targets)

    def _is_targeted(self, module_name: str) -> bool:
        if any(match_name(module_name, i) for i in self.ignore):
            return False
        if len(self.targets) == 0 or "Linear" in self.targets:
            return True
        return any(match_name(module_name, t) for t in self.targets)

    def process(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """the converted shard: the AWQ tensors of every targeted module are consumed (popped from `tensors`) and replaced by their
        pack-quantized form, every other tensor passes through"""
        from ... import _lib

        modules, inputs = [], []
        for name in list(tensors):
            if not name.endswith(".qweight"):
                continue
            module_name = name[: -len(".qweight")]
            if not self._is_targeted(module_name):
                continue
            qweight = tensors.pop(name)
            qzeros = tensors.pop(f"{module_name}.qzeros", None)
            scales = tensors.pop(f"{module_name}.scales")
            if self.zero_point and qzeros is None:
                raise ValueError("Found qweight without corresponding qzeros")
            sd = {"qweight": qweight, "scales": scales}
            if self.zero_point:
                sd["qzeros"] = qzeros
            _check_module(module_name, sd)
            modules.append(module_name)
            inputs.append(sd)

        out = ReadyDict()
        if modules:
            dev = self.device or _lib.require_device()
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev)
                stage_inputs(out, inputs, dev)
                specs = []  # (name, shape, dtype)
                for m, sd in zip(modules, inputs):
                    K, N, G = sd["qweight"].shape[0], 8 * sd["qweight"].shape[1], sd["scales"].shape[0]
                    specs.append((f"{m}.weight_packed", (N, -(-K // 8)), torch.int32))
                    specs.append((f"{m}.weight_scale", (N, G), sd["scales"].dtype))
                    if self.zero_point:
                        specs.append((f"{m}.weight_zero_point", (N // 8, G), torch.int32))
                    out[f"{m}.weight_shape"] = torch.tensor([N, K], dtype=torch.int64)
                dbuf, dev_out = device_outputs(specs, dev)

                items = []
                for m, sd in zip(modules, inputs):
                    qw, sc, qz = sd["qweight"], sd["scales"], sd.get("qzeros")
                    it = _lib.AwqItem()
                    it.qweight, it.scales, it.scale_dt = qw.data_ptr(), sc.data_ptr(), _lib.DT[sc.dtype]
                    it.weight_packed, it.scale_t = dev_out[f"{m}.weight_packed"].data_ptr(), dev_out[f"{m}.weight_scale"].data_ptr()
                    if qz is not None:
                        it.qzeros, it.zp_packed = qz.data_ptr(), dev_out[f"{m}.weight_zero_point"].data_ptr()
                        it.zp_shape[0], it.zp_shape[1] = qz.shape
                    it.K, it.N, it.G = qw.shape[0], 8 * qw.shape[1], sc.shape[0]
                    it.scale_shape[0], it.scale_shape[1] = sc.shape
                    items.append(it)
                lib = _lib.load()
                launch_tables(items, modules, _lib.AwqItem, lib.ct_awq_repack_plan, lib.ct_awq_repack_batch, dev)
                return_to_host(out, specs, dbuf, stream)
                settle(out, stream, self.stream_results)
        for name, t in tensors.items():
            out[name] = t
        return out

    def validate(self, tensors) -> None:
        """only the NAMES are inspected: `tensors` may map names to None (autoawq.py:155-172)"""
        for name in tensors:
            module_name, _, param_name = name.rpartition(".")
            if param_name in {"qweight", "qzeros", "scales"} and not self._is_targeted(module_name):
                raise ValueError(f"Found unexpected non-targeted tensor {name}")
            if param_name != "qweight" or not self._is_targeted(module_name):
                continue
            for dependency in self.get_dependencies(name):
                if dependency not in tensors:
                    raise ValueError(f"Found qweight without corresponding {dependency}")

    def create_config(self) -> _ConfigDict:
        """the reference's `create_config().model_dump()` (autoawq.py:174-195)"""
        weights = {"num_bits": self.bits, "type": "int", "symmetric": not self.zero_point, "group_size": self.group_size,
                   "strategy": "group", "block_structure": None, "dynamic": False, "actorder": None, "scale_dtype": None,
                   "zp_dtype": None if not self.zero_point else "torch.int8", "observer": "memoryless_minmax", "observer_kwargs": {}}
        return _ConfigDict({
            "config_groups": {"config_group_0": {"targets": list(self.targets), "weights": weights, "input_activations": None,
                                                 "output_activations": None, "format": "pack-quantized"}},
            "quant_method": "compressed-tensors",
            "kv_cache_scheme": None,
            "format": "pack-quantized",
            "quantization_status": "compressed",
            "global_compression_ratio": None,
            "ignore": list(self.ignore),
        })

    def get_dependencies(self, weight_name: str) -> Set[str]:
        module_name, _, suffix = weight_name.rpartition(".")
        if suffix == "qweight" and self._is_targeted(module_name):
            deps = {f"{module_name}.scales"}
            if self.zero_point:
                deps.add(f"{module_name}.qzeros")
            return deps
        return set()


def _check_module(module_name: str, sd: Dict[str, torch.Tensor]) -> None:
    """the dtypes the repack moves (the plan checks the shapes against each other)"""
    qw, sc, qz = sd["qweight"], sd["scales"], sd.get("qzeros")
    if qw.dim() != 2 or qw.dtype != torch.int32:
        raise ValueError(f"{module_name}.qweight: expected a 2-D int32 tensor, got {qw.dtype} {tuple(qw.shape)}")
    if qz is not None and (qz.dim() != 2 or qz.dtype != torch.int32):
        raise ValueError(f"{module_name}.qzeros: expected a 2-D int32 tensor, got {qz.dtype} {tuple(qz.shape)}")
    if sc.dim() != 2 or sc.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"{module_name}.scales: expected a 2-D float16 or bfloat16 tensor, got {sc.dtype} {tuple(sc.shape)}")
