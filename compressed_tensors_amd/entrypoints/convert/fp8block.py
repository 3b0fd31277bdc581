"""FP8 block-quantized checkpoints -> dense weights (reference entrypoints/convert/converters/fp8block_dequantizer.py:15-158), and the way
there: dense checkpoints -> compressed-tensors `float-quantized` FP8_BLOCK checkpoints (`FP8BlockQuantizer`, no reference counterpart: the
reference produces such checkpoints through calibration-free `compress_model`; the bits are those of calculate_qparams over each block's
min / max followed by `quantize`).

MI355X design of `FP8BlockDequantizer.process`: the float8_e4m3fn `weight` and the `weight_scale_inv` of ALL targeted modules of a
shard are staged to the GPU through one pinned buffer and one copy, and ONE `ct_fp8block_dequant_batch` launch per shard writes the
dequantized weights (csrc/ct_fp8block.hip: w * scale_inv per element, no padding, no transposes); the results come back through
one pinned buffer.  Nothing is widened, multiplied or cast on the host."""
from typing import Dict, Iterable, List, Set

import torch

from .converters import Converter, _ConfigDict, match_name, match_quantizable_tensors
from .staging import ReadyDict, device_outputs, launch_tables, return_to_host, settle, stage_inputs

__all__ = ["FP8BlockDequantizer", "FP8BlockQuantizer"]

_OUT_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _block_size(who: str, weight_block_size):
    block = tuple(weight_block_size) if isinstance(weight_block_size, (tuple, list)) else None
    if block is None or len(block) != 2 or not all(isinstance(b, int) and not isinstance(b, bool) and b > 0 for b in block):
        raise ValueError(f"{who}: weight_block_size must be two positive ints, got {weight_block_size!r}")
    return block


class FP8BlockDequantizer(Converter):
    """Dequantize a checkpoint block-quantized with the FP8 quant_method (`weight` float8_e4m3fn, `weight_scale_inv` per
    block) to dense weights of `dtype`."""

    def __init__(self, ignore: Iterable[str] = tuple(), targets: Iterable[str] = tuple(), weight_block_size=(128, 128),
                 dtype=torch.bfloat16, *, device=None):
        if dtype not in _OUT_DTYPES:
            raise ValueError(f"FP8BlockDequantizer: dtype must be torch.bfloat16, torch.float16 or torch.float32, got {dtype}")
        _block_size("FP8BlockDequantizer", weight_block_size)
        self.ignore = ignore
        self.targets = targets
        self.weight_block_size = weight_block_size
        self.dtype = dtype
        self.device = torch.device(device) if device is not None else None
        self.param_names = ["weight", "weight_scale_inv"]
        # as the other converters: `process` may return before its D2H copies have landed (a ReadyDict) when this is set or
        # inside `streaming_results()`; otherwise it synchronises first
        self.stream_results = False

    def process(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """the converted shard, in the input's order: every targeted `weight` is replaced by its dequantized form, its
        `weight_scale_inv` is dropped, every other tensor passes through as the same object"""
        modules = [m for m, name in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=self.param_names)
                   if name.rpartition(".")[-1] == "weight"]
        for m in modules:
            if f"{m}.weight_scale_inv" not in tensors:
                raise ValueError(f"Found weight without corresponding weight_scale_inv {m}.weight")
            _check_module(m, tensors[f"{m}.weight"], tensors[f"{m}.weight_scale_inv"])
        targeted = set(modules)
        out = ReadyDict((name, t) for name, t in tensors.items()
                        if not (name.endswith(".weight_scale_inv") and name.rpartition(".")[0] in targeted))
        if modules:  # every targeted `weight` of `out` is replaced in place, so the order stays
            self._dequantize(out, modules, [(tensors[f"{m}.weight"], tensors[f"{m}.weight_scale_inv"]) for m in modules])
        return out

    def validate(self, tensors: Dict[str, torch.Tensor]):
        """fp8block_dequantizer.py:55-95: only the NAMES are inspected (`tensors` may hold meta tensors, or None)"""
        targeted_names = [name for _, name in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=self.param_names)]
        for name in targeted_names:
            module_name, _, param_name = name.rpartition(".")
            if param_name == "weight" and f"{module_name}.weight_scale_inv" not in tensors:
                raise ValueError(f"Found weight without corresponding weight_scale_inv {name}")
            if param_name == "weight_scale_inv" and f"{module_name}.weight" not in tensors:
                raise ValueError(f"Found weight_scale_inv without corresponding weight {name}")
        disallowed_names = ["weight_scale_inv"]
        targeted = set(targeted_names)
        untargeted_names = [name for name in tensors.keys() if name not in targeted and not any(match_name(name, ign) for ign in self.ignore)]
        for name in untargeted_names:
            if name.rsplit(".", 1)[-1] in disallowed_names:
                raise ValueError(f"Found unexpected non-targeted tensor {name}")

    def create_config(self):
        """a dense checkpoint: `write_checkpoint_quantization_config` removes quantization_config"""
        return None

    def get_dependencies(self, weight_name: str) -> Set[str]:
        module_name, _, param_name = weight_name.rpartition(".")
        if (any(match_name(module_name, t) for t in self.targets) and not any(match_name(module_name, i) for i in self.ignore)
                and param_name == "weight"):
            return {f"{module_name}.weight_scale_inv"}
        return set()

    def _create_dequantized_weight(self, weight: torch.Tensor, weight_scale_inv: torch.Tensor) -> torch.Tensor:
        """the dequantized `weight` of `self.dtype` and the weight's shape, computed on the GPU: a host tensor for host inputs, a
        device tensor for device inputs"""
        _check_module("weight", weight, weight_scale_inv)
        on_device = weight.device.type == "cuda"
        dev = weight.device if on_device else None
        got = ReadyDict()
        self._dequantize(got, ["weight"], [(weight, weight_scale_inv)], device=dev, to_host=not on_device)
        got.wait()
        return got["weight.weight"]

    def _dequantize(self, out: ReadyDict, modules: List[str], pairs, device=None, to_host: bool = True) -> None:
        """`out[f"{module}.weight"]` = the dequantized weight of every (weight, weight_scale_inv) pair, through one staging copy and
        one launch per table the planner accepts"""
        from ... import _lib

        dev = device or self.device or _lib.require_device()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            inputs = [{"w": w, "s": s} for w, s in pairs]
            stage_inputs(out, inputs, dev)
            specs = [(f"{m}.weight", tuple(sd["w"].shape), self.dtype) for m, sd in zip(modules, inputs)]
            dbuf, dev_out = device_outputs(specs, dev)

            items, names = [], []
            bh, bw = self.weight_block_size
            for m, sd in zip(modules, inputs):
                w, s = sd["w"], sd["s"]
                if w.numel() == 0:
                    continue
                s2 = s.reshape((1,) * (2 - s.dim()) + tuple(s.shape))  # torch broadcasting of a 0-D / 1-D scale
                it = _lib.Fp8BlockItem()
                it.w, it.scale, it.out = w.data_ptr(), s2.data_ptr(), dev_out[f"{m}.weight"].data_ptr()
                it.rows, it.cols, it.block_h, it.block_w = w.shape[0], w.shape[1], bh, bw
                it.scale_shape[0], it.scale_shape[1] = s2.shape
                it.sdt = _lib.DT[s.dtype]
                items.append(it)
                names.append(m)
            lib, odt = _lib.load(), _lib.DT[self.dtype]
            launch_tables(items, names, _lib.Fp8BlockItem, lib.ct_fp8block_dequant_plan,
                          lambda table, n, blocks, handle: lib.ct_fp8block_dequant_batch(table, n, blocks, odt, handle), dev)

            if not to_host:
                stream.synchronize()
                out.keep.clear()
                for name, view in dev_out.items():
                    out[name] = view.clone()
                return
            return_to_host(out, specs, dbuf, stream)
            settle(out, stream, self.stream_results)


def _check_module(module_name: str, w: torch.Tensor, s: torch.Tensor) -> None:
    """what the kernel reads (the plan checks the scale's shape against the weight's)"""
    if w.dtype != torch.float8_e4m3fn or w.dim() != 2:
        raise ValueError(f"{module_name}.weight: expected a 2-D float8_e4m3fn tensor, got {w.dtype} {tuple(w.shape)}")
    if s.dtype not in (torch.float32, torch.bfloat16, torch.float16) or s.dim() > 2:
        raise ValueError(f"{module_name}.weight_scale_inv: expected a float32, bfloat16 or float16 tensor of at most 2 dimensions, "
                         f"got {s.dtype} {tuple(s.shape)}")


# the reference's FP8_BLOCK preset (quantization/quant_scheme.py:385-402) as its QuantizationArgs.model_dump() writes it, under the converter's block
_FP8_BLOCK_WEIGHTS = {"num_bits": 8, "type": "float", "symmetric": True, "group_size": None, "strategy": "block", "block_structure": [128, 128],
                      "dynamic": False, "actorder": None, "scale_dtype": None, "zp_dtype": None, "observer": "memoryless_minmax",
                      "observer_kwargs": {}}
_FP8_BLOCK_INPUTS = dict(_FP8_BLOCK_WEIGHTS, group_size=128, strategy="group", block_structure=None, dynamic=True, observer=None)
_DENSE_DTYPES = (torch.bfloat16, torch.float16)


class FP8BlockQuantizer(Converter):
    """Quantize a dense checkpoint to the FP8_BLOCK scheme (weights float8_e4m3fn in blocks of `weight_block_size`, round-to-nearest under each
    block's min-max scale; activations dynamic in groups of 128) in the compressed-tensors `float-quantized` format: per targeted module `weight`
    (float8_e4m3fn) and `weight_scale` (ceil(rows / bh), ceil(cols / bw)) in the dense weight's dtype.  The inverse of `FP8BlockDequantizer` up
    to the layout: that one reads the HF `fp8` layout (`weight_scale_inv`), `CompressedTensorsDequantizer` reads this one."""

    def __init__(self, ignore: Iterable[str] = ("lm_head", "re:.*embed_tokens$"), targets: Iterable[str] = tuple(), weight_block_size=(128, 128), *,
                 device=None):
        _block_size("FP8BlockQuantizer", weight_block_size)
        self.ignore = ignore
        self.targets = targets
        self.weight_block_size = weight_block_size
        self.device = torch.device(device) if device is not None else None
        self.param_names = ["weight"]
        self.stream_results = False  # as FP8BlockDequantizer

    def _scheme(self):
        from ...quantization.quant_args import QuantizationArgs, QuantizationScheme

        return QuantizationScheme(targets=["Linear"],
                                  weights=QuantizationArgs(num_bits=8, type="float", strategy="block", symmetric=True, dynamic=False,
                                                           block_structure=list(self.weight_block_size)),
                                  input_activations=QuantizationArgs(num_bits=8, type="float", strategy="group", symmetric=True, dynamic=True,
                                                                     group_size=128))

    def _targeted(self, tensors) -> List[str]:
        return [m for m, _ in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=self.param_names)]

    def process(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """the converted shard, in the input's order: every targeted 2-D bf16 / fp16 `weight` is replaced by its float8_e4m3fn codes with its
        `weight_scale` behind it, every other tensor passes through as the same object"""
        from ... import _lib, codec
        from ...compressors.naive_quantized.base import FloatQuantizationCompressor

        modules = [m for m in self._targeted(tensors) if tensors[f"{m}.weight"].dim() == 2 and tensors[f"{m}.weight"].dtype in _DENSE_DTYPES
                   and tensors[f"{m}.weight"].numel()]
        out = ReadyDict()
        mine = set(modules)
        for name, t in tensors.items():  # the outputs' places: a module's scale directly behind its weight
            out[name] = t
            if name.endswith(".weight") and name[:-7] in mine:
                out[f"{name}_scale"] = None
        if not modules:
            return out
        bh, bw = self.weight_block_size
        dev = self.device or _lib.require_device()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            inputs = [{"w": tensors[f"{m}.weight"]} for m in modules]
            stage_inputs(out, inputs, dev)
            specs = []
            for m, sd in zip(modules, inputs):
                rows, cols = sd["w"].shape
                specs += [(f"{m}.weight", (rows, cols), torch.float8_e4m3fn), (f"{m}.weight_scale", (-(-rows // bh), -(-cols // bw)), sd["w"].dtype)]
            dbuf, dev_out = device_outputs(specs, dev)

            tables, rest = {}, []  # one table per dtype: the launch takes the weights' dtype
            for m, sd in zip(modules, inputs):
                w = sd["w"]
                group = codec.rtn_block8_group(w.shape, self.weight_block_size)
                if not group or w.data_ptr() % 16:
                    rest.append((m, w))
                    continue
                it = _lib.W4Item()
                it.src, it.dst, it.scale = w.data_ptr(), dev_out[f"{m}.weight"].data_ptr(), dev_out[f"{m}.weight_scale"].data_ptr()
                it.rows, it.cols, it.group = w.shape[0], w.shape[1], group
                items, names = tables.setdefault(w.dtype, ([], []))
                items.append(it)
                names.append(m)
            lib = _lib.load()
            for dtype, (items, names) in tables.items():
                xdt = _lib.DT[dtype]
                launch_tables(items, names, _lib.W4Item, lib.ct_rtn_block8_batch_plan,
                              lambda table, n, blocks, handle, xdt=xdt: lib.ct_rtn_quant_block8_batch(table, n, blocks, xdt, 1, 1, handle), dev)
            if rest:  # what the plan refuses (ragged columns, other block sizes): the observer + compress composition, one by one
                scheme = self._scheme()
                for m, w in rest:
                    got = FloatQuantizationCompressor.compress_rtn(w, scheme)
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
        weights = dict(_FP8_BLOCK_WEIGHTS, block_structure=list(self.weight_block_size))
        return _ConfigDict({
            "config_groups": {"config_group_0": {"targets": list(self.targets) or ["Linear"], "weights": weights,
                                                 "input_activations": dict(_FP8_BLOCK_INPUTS), "output_activations": None,
                                                 "format": "float-quantized"}},
            "quant_method": "compressed-tensors",
            "kv_cache_scheme": None,
            "format": "float-quantized",
            "quantization_status": "compressed",
            "global_compression_ratio": None,
            "ignore": list(self.ignore),
        })
