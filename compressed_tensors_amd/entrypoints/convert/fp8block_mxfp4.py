"""FP8 block-quantized checkpoints -> `mxfp4-pack-quantized` checkpoints without the dense checkpoint in between (no reference counterpart: the
reference reaches MXFP4 from such a checkpoint through `FP8BlockDequantizer`, a model load and `compress_model`).

MI355X design of `FP8BlockToMXFP4Converter.process`: the float8_e4m3fn `weight` and the `weight_scale_inv` of ALL targeted modules of a shard are
staged to the GPU through one pinned buffer and one copy, ONE `ct_fp8block_mxfp4_batch` launch per shard (csrc/ct_fp4.hip: the dequantized element
rounded to `dtype` in registers, then the one-pass MXFP4 compress on those bits) writes every `weight_packed` and `weight_scale` into one output
buffer, and the results come back through one pinned buffer.  The bytes are those of the composition — `FP8BlockDequantizer(dtype=dtype)`, then the
one-pass MXFP4 compress of the dense weights —, which is also the path of what the fused plan refuses and of `fused=False`: one
`ct_fp8block_dequant_batch` launch into a dense device buffer and one `rtn_mxfp4` table launch over it."""
from typing import Dict, Iterable, List, Set

import torch

from ... import _lib
from .converters import Converter, _ConfigDict, match_name, match_quantizable_tensors
from .dense import _DenseQuantizer, mxfp4_preset_args
from .fp8block import _block_size, _check_module
from .staging import ReadyDict, device_outputs, launch_tables, return_to_host, settle, stage_inputs, table_calls

__all__ = ["FP8BlockToMXFP4Converter", "FP8BLOCK_MXFP4_MEASURED_FASTER"]

_DENSE_DTYPES = (torch.bfloat16, torch.float16)

# the dispatch of `fused=None`: True only when tools/fp8block_mxfp4_bench.py has measured the fused launch's median below the composition's MINIMUM
# on both of its tables in both of its runs (the project's dispatch rule).  profiles/fp8block_mxfp4_bench.jsonl, µs, run 1 / run 2:
# DeepSeek-V3.2-shaped table fused 846 / 841 against the composition's minimum 1249 / 1249, Qwen3-4B-shaped one 2658 / 2680 against 4241 / 4233
FP8BLOCK_MXFP4_MEASURED_FASTER = True


def _check_columns(module_name: str, w: torch.Tensor) -> None:
    """the reference's text for a weight whose columns are no whole MX groups (quantization/lifecycle/forward.py, the GROUP strategy)"""
    if w.shape[1] % 32:
        raise ValueError(f"{module_name}: tensor column shape must be divisble by the given group_size 32 but got {w.shape[1]}")


def _source_fields(it, w: torch.Tensor, s: torch.Tensor, block):
    """the fields of a table row that describe the block-quantized weight (`ct_fp8block_item` and `ct_fp8block_mx_item` name them alike)"""
    s2 = s.reshape((1,) * (2 - s.dim()) + tuple(s.shape))  # torch broadcasting of a 0-D / 1-D scale
    it.w, it.scale = w.data_ptr(), s2.data_ptr()
    it.rows, it.cols, it.block_h, it.block_w = w.shape[0], w.shape[1], block[0], block[1]
    it.scale_shape[0], it.scale_shape[1] = s2.shape
    it.sdt = _lib.DT[s.dtype]
    return it


def _fused_admits(w: torch.Tensor, packed: torch.Tensor, block) -> bool:
    """what `ct_fp8block_mxfp4_plan` asks of a row beyond the checks made before anything was staged: the plan is never handed a row it would refuse"""
    return block[1] % 32 == 0 and w.data_ptr() % 16 == 0 and packed.data_ptr() % 16 == 0


def transcode(out: ReadyDict, modules: List[str], pairs, block, dtype, dev, fused: bool, to_host: bool = True, stream_results: bool = False) -> None:
    """`out[f"{module}.weight_packed"]` / `out[f"{module}.weight_scale"]` of every (weight, weight_scale_inv) pair: one staging copy, one fused launch
    over the rows its plan admits (`fused`), the composition over the others, one copy back (`to_host`; else device tensors of their own)"""
    from ... import codec

    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        inputs = [{"w": w, "s": s} for w, s in pairs]
        stage_inputs(out, inputs, dev)
        specs = []
        for m, sd in zip(modules, inputs):
            rows, cols = sd["w"].shape
            specs += [(f"{m}.weight_packed", (rows, cols // 2), torch.uint8), (f"{m}.weight_scale", (rows, cols // 32), torch.uint8)]
        dbuf, dev_out = device_outputs(specs, dev)

        lib, xdt = _lib.load(), _lib.DT[dtype]
        items, names, rest = [], [], []
        for m, sd in zip(modules, inputs):
            w, s = sd["w"], sd["s"]
            if w.numel() == 0:
                continue
            packed, e8m0 = dev_out[f"{m}.weight_packed"], dev_out[f"{m}.weight_scale"]
            if not (fused and _fused_admits(w, packed, block)):
                rest.append((m, w, s))
                continue
            it = _source_fields(_lib.Fp8BlockMxItem(), w, s, block)
            it.packed, it.e8m0 = packed.data_ptr(), e8m0.data_ptr()
            items.append(it)
            names.append(m)
        launch_tables(items, names, _lib.Fp8BlockMxItem, lib.ct_fp8block_mxfp4_plan,
                      lambda table, n, blocks, handle: lib.ct_fp8block_mxfp4_batch(table, n, blocks, xdt, handle), dev)

        if rest:  # the composition: the dequantize table into a dense device buffer, the one-pass MXFP4 table over it
            _, dense = device_outputs([(m, tuple(w.shape), dtype) for m, w, _ in rest], dev)
            ditems, mitems = [], []
            for m, w, s in rest:
                it = _source_fields(_lib.Fp8BlockItem(), w, s, block)
                it.out = dense[m].data_ptr()
                ditems.append(it)
                row = _lib.W4Item()
                row.src, row.rows, row.cols, row.group = it.out, w.shape[0], w.shape[1], 32
                row.dst, row.zp_packed = dev_out[f"{m}.weight_packed"].data_ptr(), dev_out[f"{m}.weight_scale"].data_ptr()
                mitems.append(row)
            rest_names = [m for m, _, _ in rest]
            launch_tables(ditems, rest_names, _lib.Fp8BlockItem, lib.ct_fp8block_dequant_plan,
                          lambda table, n, blocks, handle: lib.ct_fp8block_dequant_batch(table, n, blocks, xdt, handle), dev)
            plan, launch = table_calls(*codec.rtn_mxfp4_launch(dtype))
            launch_tables(mitems, rest_names, _lib.W4Item, plan, launch, dev)  # (the dense buffer was allocated on this stream: freed in its order)

        if not to_host:
            stream.synchronize()
            out.keep.clear()
            for name, view in dev_out.items():  # tensors of their own, as FP8BlockDequantizer hands back: a view would keep the whole buffer alive
                out[name] = view.clone()        # and alias its neighbour's storage, which a saved state dict must not
            return
        return_to_host(out, specs, dbuf, stream)
        settle(out, stream, stream_results)


class FP8BlockToMXFP4Converter(Converter):
    """Transcode a checkpoint block-quantized with the FP8 quant_method (`weight` float8_e4m3fn, `weight_scale_inv` per block) to the MXFP4 scheme in
    the compressed-tensors `mxfp4-pack-quantized` format: per targeted module `weight_packed` (uint8, (rows, cols / 2)) where the weight was and
    `weight_scale` (uint8 E8M0 exponents, (rows, cols / 32)) behind it; the `weight_scale_inv` is dropped.  The bytes are those of
    `FP8BlockDequantizer(dtype=dtype)` followed by the round-to-nearest MXFP4 compress of the dense weights.  `activations=True` writes the MXFP4
    preset (dynamic MXFP4 input activations) instead of MXFP4A16; `fused`: None follows `FP8BLOCK_MXFP4_MEASURED_FASTER`, True / False force the one
    launch / the composition."""

    format = "mxfp4-pack-quantized"

    def __init__(self, ignore: Iterable[str] = tuple(), targets: Iterable[str] = tuple(), weight_block_size=(128, 128), dtype=torch.bfloat16,
                 activations: bool = False, *, device=None, fused=None):
        if dtype not in _DENSE_DTYPES:
            raise ValueError(f"FP8BlockToMXFP4Converter: dtype must be torch.bfloat16 or torch.float16, got {dtype}")
        self.weight_block_size = _block_size("FP8BlockToMXFP4Converter", weight_block_size)
        self.ignore = ignore
        self.targets = targets
        self.dtype = dtype
        self.activations = bool(activations)
        self.device = torch.device(device) if device is not None else None
        self.fused = fused
        self.param_names = ["weight", "weight_scale_inv"]
        # as the other converters: `process` may return before its D2H copies have landed (a ReadyDict) when this is set or inside
        # `streaming_results()`; otherwise it synchronises first
        self.stream_results = False

    def _fused(self) -> bool:
        return FP8BLOCK_MXFP4_MEASURED_FASTER if self.fused is None else bool(self.fused)

    def process(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """the converted shard, in the input's order: every targeted `weight` is replaced by its `weight_packed` followed by its `weight_scale`, its
        `weight_scale_inv` is dropped, every other tensor passes through as the same object"""
        modules = [m for m, name in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=self.param_names)
                   if name.rpartition(".")[-1] == "weight"]
        for m in modules:  # everything that raises for a module raises here, before anything is staged
            if f"{m}.weight_scale_inv" not in tensors:
                raise ValueError(f"Found weight without corresponding weight_scale_inv {m}.weight")
            _check_module(m, tensors[f"{m}.weight"], tensors[f"{m}.weight_scale_inv"])
            _check_columns(m, tensors[f"{m}.weight"])
        targeted = set(modules)
        out = ReadyDict()
        for name, t in tensors.items():
            m, _, param = name.rpartition(".")
            if m in targeted and param == "weight":
                out[f"{m}.weight_packed"] = out[f"{m}.weight_scale"] = None  # their places; `transcode` fills them
            elif not (m in targeted and param == "weight_scale_inv"):
                out[name] = t
        if modules:
            transcode(out, modules, [(tensors[f"{m}.weight"], tensors[f"{m}.weight_scale_inv"]) for m in modules], self.weight_block_size,
                      self.dtype, self.device or _lib.require_device(), self._fused(), stream_results=self.stream_results)
        return out

    def validate(self, tensors: Dict[str, torch.Tensor]):
        """as FP8BlockDequantizer's: only the NAMES are inspected (`tensors` may hold meta tensors, or None)"""
        targeted_names = [name for _, name in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=self.param_names)]
        for name in targeted_names:
            module_name, _, param_name = name.rpartition(".")
            if param_name == "weight" and f"{module_name}.weight_scale_inv" not in tensors:
                raise ValueError(f"Found weight without corresponding weight_scale_inv {name}")
            if param_name == "weight_scale_inv" and f"{module_name}.weight" not in tensors:
                raise ValueError(f"Found weight_scale_inv without corresponding weight {name}")
        targeted = set(targeted_names)
        for name in tensors.keys():
            if name not in targeted and not any(match_name(name, ign) for ign in self.ignore) and name.rsplit(".", 1)[-1] == "weight_scale_inv":
                raise ValueError(f"Found unexpected non-targeted tensor {name}")

    def get_dependencies(self, weight_name: str) -> Set[str]:
        module_name, _, param_name = weight_name.rpartition(".")
        if (any(match_name(module_name, t) for t in self.targets) and not any(match_name(module_name, i) for i in self.ignore)
                and param_name == "weight"):
            return {f"{module_name}.weight_scale_inv"}
        return set()

    def _preset_args(self):
        return mxfp4_preset_args(self.activations)

    create_config = _DenseQuantizer.create_config  # the same config shape: it reads `targets`, `ignore`, `format` and `_preset_args` alone
