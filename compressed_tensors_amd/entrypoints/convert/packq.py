"""Dense checkpoints -> compressed-tensors `pack-quantized` checkpoints of the integer weight-only presets (`PackQuantizedQuantizer`: W4A16,
W4A16_ASYM, W2A16 ... W7A16 and their channel-wise forms; no reference counterpart: the reference produces such checkpoints through
calibration-free `compress_model`; the bits are those of calculate_qparams over each group's min / max followed by `quantize`, `pack_to_int32`
and, for an asymmetric scheme, `pack_to_int32(zero_point, bits, packed_dim=0)`).

MI355X design of `process`: the dense weights of ALL targeted modules of a shard are staged to the GPU through one pinned buffer and one copy,
and ONE one-pass table launch per shard and dtype (`ct_rtn_quant_pack_w4_batch` for 4 bits, `ct_rtn_quant_pack_wb_batch` for 2, 3, 5, 6 and 7:
observer, scale, zero point and packed words in one pass over each weight) writes the words and the scales; the stored zero points of an
asymmetric scheme follow in one `ct_zp4_pack_dim0_batch` launch (4 bits) or one `pack_to_int32` per module; the results come back through one
pinned buffer."""
import math
from typing import Dict, Iterable, List, Set

import torch

from .converters import Converter, _ConfigDict, match_quantizable_tensors
from .staging import ReadyDict, device_outputs, launch_tables, return_to_host, settle, stage_inputs

__all__ = ["PackQuantizedQuantizer"]

# the reference's integer weight-only presets (quantization/quant_scheme.py:104-131, _int_wnam) as their QuantizationArgs.model_dump() writes them;
# `zp_dtype` is "torch.int8" for an asymmetric scheme and None for a symmetric one
_PACKQ_WEIGHTS = {"num_bits": 4, "type": "int", "symmetric": True, "group_size": 128, "strategy": "group", "block_structure": None,
                  "dynamic": False, "actorder": None, "scale_dtype": None, "zp_dtype": None, "observer": "memoryless_minmax",
                  "observer_kwargs": {}}
_DENSE_DTYPES = (torch.bfloat16, torch.float16)
_FORMAT = "pack-quantized"


class PackQuantizedQuantizer(Converter):
    """Quantize a dense checkpoint to an integer weight-only scheme of 2..7 bits (round-to-nearest under each group's — or each output channel's —
    min-max scale, symmetric or not) in the compressed-tensors `pack-quantized` format: per targeted module `weight_packed` (int32,
    (rows, ceil(cols * num_bits / 32))), `weight_scale` ((rows, cols / group), the dense dtype), `weight_shape` (int64 [rows, cols]) and, for an
    asymmetric scheme, `weight_zero_point` in its stored form (int32, (ceil(rows * num_bits / 32), cols / group)).  `CompressedTensorsDequantizer`
    reads it back."""

    def __init__(self, num_bits: int = 4, group_size: int = 128, symmetric: bool = True, strategy: str = "group",
                 ignore: Iterable[str] = ("lm_head", "re:.*embed_tokens$"), targets: Iterable[str] = tuple(), *, device=None):
        from ...codec import RTN_PACKW_BITS

        self.num_bits = int(num_bits)
        if self.num_bits != 4 and self.num_bits not in RTN_PACKW_BITS:
            raise ValueError(f"PackQuantizedQuantizer writes 2..7-bit words, got num_bits={num_bits} (8 bits: W8A8Quantizer)")
        strategy = getattr(strategy, "value", strategy)
        if strategy not in ("group", "channel"):
            raise ValueError(f"PackQuantizedQuantizer takes the strategies 'group' and 'channel', got {strategy!r}")
        if strategy == "group" and (group_size is None or int(group_size) <= 0):
            raise ValueError("the group strategy needs a positive group_size")
        self.strategy = strategy
        self.group_size = int(group_size) if strategy == "group" else None
        self.symmetric = bool(symmetric)
        self.ignore = ignore
        self.targets = targets
        self.device = torch.device(device) if device is not None else None
        self.param_names = ["weight"]
        self.stream_results = False  # as FP8BlockDequantizer

    def _scheme(self):
        from ...quantization.quant_args import QuantizationArgs, QuantizationScheme

        return QuantizationScheme(targets=["Linear"], weights=QuantizationArgs(num_bits=self.num_bits, type="int", strategy=self.strategy,
                                                                              group_size=self.group_size, symmetric=self.symmetric, dynamic=False))

    def _targeted(self, tensors) -> List[str]:
        return [m for m, _ in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=self.param_names)]

    def process(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """the converted shard, in the input's order: every targeted 2-D bf16 / fp16 `weight` is replaced by its `weight_packed` with its
        `weight_scale`, (asymmetric) `weight_zero_point` and `weight_shape` behind it, every other tensor passes through as the same object.
        Columns that are no whole groups raise the reference's ValueError."""
        from ... import _lib, codec
        from ...compressors.pack_quantized.base import PackedQuantizationCompressor

        def dense(t):
            return t.dim() == 2 and t.dtype in _DENSE_DTYPES and t.numel()

        bits, symmetric = self.num_bits, self.symmetric
        modules = [m for m in self._targeted(tensors) if dense(tensors[f"{m}.weight"])]
        out = ReadyDict()
        mine = set(modules)
        for name, t in tensors.items():  # the outputs' places: the packed words where the weight was, the module's other entries directly behind
            if name.endswith(".weight") and name[:-7] in mine:
                out[f"{name}_packed"] = None
                out[f"{name}_scale"] = None
                if not symmetric:
                    out[f"{name}_zero_point"] = None
                out[f"{name}_shape"] = torch.tensor(t.shape)  # int64, on the host: as the compressor writes it
            else:
                out[name] = t
        if not modules:
            return out
        dev = self.device or _lib.require_device()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            inputs = [{"w": tensors[f"{m}.weight"]} for m in modules]
            stage_inputs(out, inputs, dev)
            specs, groups = [], {}
            for m, sd in zip(modules, inputs):
                rows, cols = sd["w"].shape
                g = self.group_size or cols
                if cols % g:
                    raise ValueError(f"{m}: tensor column shape must be divisble by the given group_size {g} but got {cols}")
                groups[m] = g
                specs += [(f"{m}.weight_packed", (rows, math.ceil(cols * bits / 32)), torch.int32), (f"{m}.weight_scale", (rows, cols // g), sd["w"].dtype)]
                if not symmetric:
                    specs.append((f"{m}.weight_zero_point", (math.ceil(rows * bits / 32), cols // g), torch.int32))
            dbuf, dev_out = device_outputs(specs, dev)

            dst_align = 16 if bits == 4 else 4
            tables, rest, zps = {}, [], []  # one table per dtype: the launch takes the weights' dtype
            for m, sd in zip(modules, inputs):
                w = sd["w"]
                packed = dev_out[f"{m}.weight_packed"]
                if not codec.rtn_w4_group(w.shape, self.group_size) or w.data_ptr() % 16 or packed.data_ptr() % dst_align:
                    rest.append((m, w))
                    continue
                it = _lib.W4Item()
                it.src, it.dst, it.scale = w.data_ptr(), packed.data_ptr(), dev_out[f"{m}.weight_scale"].data_ptr()
                it.rows, it.cols, it.group = w.shape[0], w.shape[1], groups[m]
                if not symmetric:  # the int8 zero points the launch computes; their stored form follows behind it
                    zp = torch.empty((w.shape[0], w.shape[1] // groups[m]), dtype=torch.int8, device=dev)
                    it.zp = zp.data_ptr()
                    zps.append((m, zp))
                items, names = tables.setdefault(w.dtype, ([], []))
                items.append(it)
                names.append(m)
            lib = _lib.load()
            for dtype, (items, names) in tables.items():
                xdt = _lib.DT[dtype]
                if bits == 4:
                    launch_tables(items, names, _lib.W4Item, lib.ct_rtn_w4_batch_plan,
                                  lambda table, n, blocks, handle, xdt=xdt: lib.ct_rtn_quant_pack_w4_batch(table, n, blocks, xdt, int(symmetric), handle), dev)
                else:
                    launch_tables(items, names, _lib.W4Item, lambda table, n: lib.ct_rtn_wb_batch_plan(table, n, bits),
                                  lambda table, n, blocks, handle, xdt=xdt: lib.ct_rtn_quant_pack_wb_batch(table, n, blocks, xdt, bits, int(symmetric), handle), dev)
            if zps and bits == 4:  # pack_to_int32(zp, 4, packed_dim=0) of every module in one launch
                codec.zp4_batch([(zp, dev_out[f"{m}.weight_zero_point"]) for m, zp in zps], "pack")
            else:
                for m, zp in zps:
                    dev_out[f"{m}.weight_zero_point"].copy_(codec.pack_to_int32(zp, bits, packed_dim=0))
            if rest:  # what the plan refuses (ragged groups, a misaligned staging slot): `compress_rtn`, one by one
                scheme = self._scheme()
                for m, w in rest:
                    got = PackedQuantizationCompressor.compress_rtn(w, scheme)
                    for k in ("weight_packed", "weight_scale") + (() if symmetric else ("weight_zero_point",)):
                        dev_out[f"{m}.{k}"].copy_(got[k])
            return_to_host(out, specs, dbuf, stream)
            settle(out, stream, self.stream_results)
        return out

    def validate(self, tensors: Dict[str, torch.Tensor]):
        """only the NAMES are inspected (`tensors` may hold meta tensors, or None): a targeted module must still be dense"""
        for m in self._targeted(tensors):
            for partner in ("weight_scale", "weight_scale_inv", "weight_packed", "weight_shape", "weight_zero_point"):
                if f"{m}.{partner}" in tensors:
                    raise ValueError(f"Found {m}.{partner} beside the targeted {m}.weight: the module is quantized already")

    def get_dependencies(self, weight_name: str) -> Set[str]:
        """a dense weight has no partner tensors"""
        return set()

    def create_config(self) -> _ConfigDict:
        weights = dict(_PACKQ_WEIGHTS, num_bits=self.num_bits, symmetric=self.symmetric, group_size=self.group_size, strategy=self.strategy,
                       zp_dtype=None if self.symmetric else "torch.int8")
        return _ConfigDict({
            "config_groups": {"config_group_0": {"targets": list(self.targets) or ["Linear"], "weights": weights,
                                                 "input_activations": None, "output_activations": None, "format": _FORMAT}},
            "quant_method": "compressed-tensors",
            "kv_cache_scheme": None,
            "format": _FORMAT,
            "quantization_status": "compressed",
            "global_compression_ratio": None,
            "ignore": list(self.ignore),
        })
