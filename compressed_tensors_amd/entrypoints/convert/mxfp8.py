"""Dense checkpoints -> compressed-tensors `mxfp8-quantized` checkpoints (`MXFP8Quantizer`, no reference counterpart: the reference produces
such checkpoints through calibration-free `compress_model`; the bits are those of calculate_qparams' MX branch over each group's min / max
followed by `quantize` and `compress_mx_scale`).

MI355X design of `MXFP8Quantizer.process`: the dense weights of ALL targeted modules of a shard are staged to the GPU through one pinned buffer
and one copy, and ONE `ct_rtn_quant_group8_batch` launch per shard and dtype (kind MXFP8: observer, E8M0 scale, float8 codes in one pass over
each weight) writes the codes and the exponent bytes; the results come back through one pinned buffer."""
from typing import Dict, Iterable, List, Set

import torch

from .converters import Converter, _ConfigDict, match_quantizable_tensors
from .staging import ReadyDict, device_outputs, launch_tables, return_to_host, settle, stage_inputs

__all__ = ["MXFP8Quantizer"]

# the reference's MXFP8 preset (quantization/quant_scheme.py:253-274) as its QuantizationArgs.model_dump() writes it
_MXFP8_WEIGHTS = {"num_bits": 8, "type": "float", "symmetric": True, "group_size": 32, "strategy": "group", "block_structure": None,
                  "dynamic": False, "actorder": None, "scale_dtype": "torch.uint8", "zp_dtype": None, "observer": "memoryless_minmax",
                  "observer_kwargs": {}}
_MXFP8_INPUTS = dict(_MXFP8_WEIGHTS, dynamic=True, observer=None)
_DENSE_DTYPES = (torch.bfloat16, torch.float16)
_QP_MXFP8 = 4  # the kernel's kind (include/ct_hip.h)


class MXFP8Quantizer(Converter):
    """Quantize a dense checkpoint to the MXFP8 scheme (weights float8_e4m3fn in groups of 32, round-to-nearest under each group's E8M0
    min-max scale; activations dynamic in groups of 32) in the compressed-tensors `mxfp8-quantized` format: per targeted module `weight`
    (float8_e4m3fn) and `weight_scale` (uint8 exponents, (rows, cols / 32)).  `CompressedTensorsDequantizer` reads it back."""

    def __init__(self, ignore: Iterable[str] = ("lm_head", "re:.*embed_tokens$"), targets: Iterable[str] = tuple(), *, device=None):
        self.ignore = ignore
        self.targets = targets
        self.device = torch.device(device) if device is not None else None
        self.param_names = ["weight"]
        self.stream_results = False  # as FP8BlockDequantizer

    def _scheme(self):
        from ...quantization.quant_args import QuantizationArgs, QuantizationScheme

        mx = dict(num_bits=8, type="float", strategy="group", symmetric=True, group_size=32, scale_dtype=torch.uint8, zp_dtype=torch.uint8)
        return QuantizationScheme(targets=["Linear"], weights=QuantizationArgs(dynamic=False, **mx), input_activations=QuantizationArgs(dynamic=True, **mx))

    def _targeted(self, tensors) -> List[str]:
        return [m for m, _ in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=self.param_names)]

    def process(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """the converted shard, in the input's order: every targeted 2-D bf16 / fp16 `weight` is replaced by its float8_e4m3fn codes with its
        `weight_scale` behind it, every other tensor passes through as the same object.  Columns that are no whole groups of 32 raise the
        reference's ValueError."""
        from ... import _lib, codec
        from ...compressors.mxfp8.base import MXFP8QuantizationCompressor

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
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            inputs = [{"w": tensors[f"{m}.weight"]} for m in modules]
            stage_inputs(out, inputs, dev)
            specs = []
            for m, sd in zip(modules, inputs):
                rows, cols = sd["w"].shape
                specs += [(f"{m}.weight", (rows, cols), torch.float8_e4m3fn), (f"{m}.weight_scale", (rows, cols // 32), torch.uint8)]
            dbuf, dev_out = device_outputs(specs, dev)

            tables, rest = {}, []  # one table per dtype: the launch takes the weights' dtype
            for m, sd in zip(modules, inputs):
                w = sd["w"]
                if not codec.rtn_group8_group(w.shape, 32) or w.data_ptr() % 16 or dev_out[f"{m}.weight"].data_ptr() % 16:
                    rest.append((m, w))
                    continue
                it = _lib.W4Item()
                it.src, it.dst, it.zp_packed = w.data_ptr(), dev_out[f"{m}.weight"].data_ptr(), dev_out[f"{m}.weight_scale"].data_ptr()
                it.rows, it.cols, it.group = w.shape[0], w.shape[1], 32
                items, names = tables.setdefault(w.dtype, ([], []))
                items.append(it)
                names.append(m)
            lib = _lib.load()
            for dtype, (items, names) in tables.items():
                xdt, lut = _lib.DT[dtype], codec._mx_code_table(dtype, dev).data_ptr()  # (the table is cached per dtype and device)
                launch_tables(items, names, _lib.W4Item, lib.ct_rtn_group8_batch_plan,
                              lambda table, n, blocks, handle, xdt=xdt, lut=lut: lib.ct_rtn_quant_group8_batch(table, n, blocks, xdt, _QP_MXFP8, 1, 0, lut, handle), dev)
            if rest:  # what the plan refuses (a misaligned staging slot, ragged columns): `compress_rtn`, one by one
                scheme = self._scheme()
                for m, w in rest:
                    got = MXFP8QuantizationCompressor.compress_rtn(w, scheme)
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
            "config_groups": {"config_group_0": {"targets": list(self.targets) or ["Linear"], "weights": dict(_MXFP8_WEIGHTS),
                                                 "input_activations": dict(_MXFP8_INPUTS), "output_activations": None,
                                                 "format": "mxfp8-quantized"}},
            "quant_method": "compressed-tensors",
            "kv_cache_scheme": None,
            "format": "mxfp8-quantized",
            "quantization_status": "compressed",
            "global_compression_ratio": None,
            "ignore": list(self.ignore),
        })
