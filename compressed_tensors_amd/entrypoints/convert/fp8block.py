"""FP8 block-quantized checkpoints -> dense weights (reference entrypoints/convert/converters/fp8block_dequantizer.py:15-158).  The way there,
`FP8BlockQuantizer`, stands with the other dense-checkpoint quantizers in dense.py.

MI355X design of `FP8BlockDequantizer.process`: the float8_e4m3fn `weight` and the `weight_scale_inv` of ALL targeted modules of a
shard are staged to the GPU through one pinned buffer and one copy, and ONE `ct_fp8block_dequant_batch` launch per shard writes the
dequantized weights (csrc/ct_fp8block.hip: w * scale_inv per element, no padding, no transposes); the results come back through
one pinned buffer.  Nothing is widened, multiplied or cast on the host."""
from typing import Dict, Iterable, List, Set

import torch

from .converters import Converter, _ConfigDict, match_name, match_quantizable_tensors
from .staging import ReadyDict, device_outputs, launch_tables, return_to_host, settle, stage_inputs

__all__ = ["FP8BlockDequantizer"]

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
