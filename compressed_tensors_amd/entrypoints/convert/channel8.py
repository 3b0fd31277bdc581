"""Dense checkpoints -> compressed-tensors `float-quantized` (FP8_DYNAMIC) and `int-quantized` (W8A8) checkpoints (`FP8DynamicQuantizer`,
`W8A8Quantizer`, no reference counterpart: the reference produces such checkpoints through calibration-free `compress_model`; the bits are
those of calculate_qparams over each output channel's min / max followed by `quantize`).  Both presets are data-free by construction: weights
round-to-nearest under one min-max scale per row, activations dynamic per token.

MI355X design of `process`: the dense weights of ALL targeted modules of a shard are staged to the GPU through one pinned buffer and one copy,
and ONE `ct_rtn_quant_channel8_batch` launch per shard and dtype (observer, scale, codes in one pass over each weight; short, workgroup and long
rows in one table) writes the codes and the scales; the results come back through one pinned buffer."""
from typing import Dict, Iterable, List, Set

import torch

from .converters import Converter, _ConfigDict, match_quantizable_tensors
from .staging import ReadyDict, device_outputs, launch_tables, return_to_host, settle, stage_inputs

__all__ = ["FP8DynamicQuantizer", "W8A8Quantizer"]

# the reference's FP8_DYNAMIC and INT8_W8A8 presets (quantization/quant_scheme.py:365-380, 296-311) as their QuantizationArgs.model_dump() writes them
_FP8_DYNAMIC_WEIGHTS = {"num_bits": 8, "type": "float", "symmetric": True, "group_size": None, "strategy": "channel", "block_structure": None,
                        "dynamic": False, "actorder": None, "scale_dtype": None, "zp_dtype": None, "observer": "memoryless_minmax",
                        "observer_kwargs": {}}
_FP8_DYNAMIC_INPUTS = dict(_FP8_DYNAMIC_WEIGHTS, strategy="token", dynamic=True, observer=None)
_W8A8_WEIGHTS = dict(_FP8_DYNAMIC_WEIGHTS, type="int")
_W8A8_INPUTS = dict(_FP8_DYNAMIC_INPUTS, type="int")
_DENSE_DTYPES = (torch.bfloat16, torch.float16)


class _Channel8Quantizer(Converter):
    """the shared body of the two channel-wise 8-bit presets; a subclass names its number type, format and preset"""

    qtype: str = None  # "float" / "int"
    format: str = None
    code_dtype: torch.dtype = None
    preset_weights: dict = None
    preset_inputs: dict = None

    def __init__(self, ignore: Iterable[str] = ("lm_head", "re:.*embed_tokens$"), targets: Iterable[str] = tuple(), *, device=None):
        self.ignore = ignore
        self.targets = targets
        self.device = torch.device(device) if device is not None else None
        self.param_names = ["weight"]
        self.stream_results = False  # as FP8BlockDequantizer

    def _scheme(self):
        from ...quantization.quant_args import QuantizationArgs, QuantizationScheme

        return QuantizationScheme(targets=["Linear"], weights=QuantizationArgs(num_bits=8, type=self.qtype, strategy="channel", symmetric=True, dynamic=False),
                                  input_activations=QuantizationArgs(num_bits=8, type=self.qtype, strategy="token", symmetric=True, dynamic=True))

    def _compressor(self):
        from ...compressors.naive_quantized.base import FloatQuantizationCompressor, IntQuantizationCompressor

        return FloatQuantizationCompressor if self.qtype == "float" else IntQuantizationCompressor

    def _targeted(self, tensors) -> List[str]:
        return [m for m, _ in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=self.param_names)]

    def process(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """the converted shard, in the input's order: every targeted 2-D bf16 / fp16 `weight` is replaced by its 8-bit codes with its
        `weight_scale` (rows, 1) in the dense dtype behind it (both presets are symmetric: no zero point), every other tensor passes through as
        the same object"""
        from ... import _lib, codec

        def dense(t):
            return t.dim() == 2 and t.dtype in _DENSE_DTYPES and t.numel()

        modules = [m for m in self._targeted(tensors) if dense(tensors[f"{m}.weight"])]
        out = ReadyDict()
        mine = set(modules)
        for name, t in tensors.items():  # the outputs' places: a module's scale directly behind its weight
            out[name] = t
            if name.endswith(".weight") and name[:-7] in mine:
                out[f"{name}_scale"] = None
        if not modules:
            return out
        dev = self.device or _lib.require_device()
        fp8 = self.qtype == "float"
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            inputs = [{"w": tensors[f"{m}.weight"]} for m in modules]
            stage_inputs(out, inputs, dev)
            specs = []
            for m, sd in zip(modules, inputs):
                rows, cols = sd["w"].shape
                specs += [(f"{m}.weight", (rows, cols), self.code_dtype), (f"{m}.weight_scale", (rows, 1), sd["w"].dtype)]
            dbuf, dev_out = device_outputs(specs, dev)

            tables, rest = {}, []  # one table per dtype: the launch takes the weights' dtype
            for m, sd in zip(modules, inputs):
                w = sd["w"]
                if not codec.rtn_channel8_form(w.shape, True) or w.data_ptr() % 16 or dev_out[f"{m}.weight"].data_ptr() % 16:
                    rest.append((m, w))
                    continue
                it = _lib.W4Item()
                it.src, it.dst, it.scale = w.data_ptr(), dev_out[f"{m}.weight"].data_ptr(), dev_out[f"{m}.weight_scale"].data_ptr()
                it.rows, it.cols = w.shape[0], w.shape[1]
                items, names = tables.setdefault(w.dtype, ([], []))
                items.append(it)
                names.append(m)
            lib = _lib.load()
            for dtype, (items, names) in tables.items():
                xdt = _lib.DT[dtype]
                launch_tables(items, names, _lib.W4Item, lib.ct_rtn_channel8_batch_plan,
                              lambda table, n, blocks, handle, xdt=xdt: lib.ct_rtn_quant_channel8_batch(table, n, blocks, xdt, int(fp8), 1, handle), dev)
            if rest:  # what the plan refuses (a misaligned staging slot, cols % 8, rows beyond the kernel's maximum): `compress_rtn`, one by one
                scheme, compressor = self._scheme(), self._compressor()
                for m, w in rest:
                    got = compressor.compress_rtn(w, scheme)
                    dev_out[f"{m}.weight"].copy_(got["weight"])
                    dev_out[f"{m}.weight_scale"].copy_(got["weight_scale"])
            return_to_host(out, specs, dbuf, stream)
            settle(out, stream, self.stream_results)
        return out

    def validate(self, tensors: Dict[str, torch.Tensor]):
        """only the NAMES are inspected (`tensors` may hold meta tensors, or None): a targeted module must still be dense"""
        for m in self._targeted(tensors):
            for partner in ("weight_scale", "weight_scale_inv", "weight_packed"):
                if f"{m}.{partner}" in tensors:
                    raise ValueError(f"Found {m}.{partner} beside the targeted {m}.weight: the module is quantized already")

    def get_dependencies(self, weight_name: str) -> Set[str]:
        """a dense weight has no partner tensors"""
        return set()

    def create_config(self) -> _ConfigDict:
        return _ConfigDict({
            "config_groups": {"config_group_0": {"targets": list(self.targets) or ["Linear"], "weights": dict(self.preset_weights),
                                                 "input_activations": dict(self.preset_inputs), "output_activations": None,
                                                 "format": self.format}},
            "quant_method": "compressed-tensors",
            "kv_cache_scheme": None,
            "format": self.format,
            "quantization_status": "compressed",
            "global_compression_ratio": None,
            "ignore": list(self.ignore),
        })


class FP8DynamicQuantizer(_Channel8Quantizer):
    """Quantize a dense checkpoint to the FP8_DYNAMIC scheme (weights float8_e4m3fn, round-to-nearest under one min-max scale per output channel;
    activations dynamic per token) in the compressed-tensors `float-quantized` format: per targeted module `weight` (float8_e4m3fn) and
    `weight_scale` ((rows, 1), the dense dtype).  `CompressedTensorsDequantizer` reads it back."""

    qtype, format, code_dtype = "float", "float-quantized", torch.float8_e4m3fn
    preset_weights, preset_inputs = _FP8_DYNAMIC_WEIGHTS, _FP8_DYNAMIC_INPUTS


class W8A8Quantizer(_Channel8Quantizer):
    """Quantize a dense checkpoint to the W8A8 scheme (the reference's INT8_W8A8 preset: weights int8, round-to-nearest under one symmetric
    min-max scale per output channel; activations dynamic per token) in the compressed-tensors `int-quantized` format: per targeted module
    `weight` (int8) and `weight_scale` ((rows, 1), the dense dtype).  `CompressedTensorsDequantizer` reads it back."""

    qtype, format, code_dtype = "int", "int-quantized", torch.int8
    preset_weights, preset_inputs = _W8A8_WEIGHTS, _W8A8_INPUTS
