"""FP8 block-quantized checkpoints -> MXFP4, MXFP8 and NVFP4 checkpoints without the dense checkpoint in between: the body the three converters
share, and the two of them that are not `FP8BlockToMXFP4Converter` (fp8block_mxfp4.py, its third user).

MI355X design of `process`, whatever the target: the float8_e4m3fn `weight` and the `weight_scale_inv` of ALL targeted modules of a shard are staged to
the GPU through one pinned buffer and one copy; the target's fused launch(es) over the rows its plan admits — ONE `ct_fp8block_mxfp4_batch` /
`ct_fp8block_mxfp8_batch`, or `ct_fp8block_nvfp4_amax_batch` and `ct_fp8block_nvfp4_batch` behind one fill of the amax keys — write every output
into one buffer (the dequantized element rounded to `dtype` in registers, then the target's one-pass compress on those bits), and the results come
back through one pinned buffer.  The bytes are those of the composition — `FP8BlockDequantizer(dtype=dtype)`, then the target's one-pass compress of
the dense weights —, which is also the path of what the fused plan refuses and of `fused=False`: one `ct_fp8block_dequant_batch` launch into a dense
device buffer and the target's table over it.

A `Target` holds what differs: the column multiple and its error text, the output specs in shard order, the item type, plan and launch(es) of the
fused form, the composition's second stage, the preset and the format."""
from typing import Callable, Dict, Iterable, List, NamedTuple, Set

import torch

from ... import _lib
from .converters import Converter, match_name, match_quantizable_tensors
from .dense import _DenseQuantizer, mxfp4_preset_args, mxfp8_preset_args
from .fp8block import _block_size, _check_module
from .modelopt import _NVFP4_INPUTS, _NVFP4_WEIGHTS
from .staging import ReadyDict, device_outputs, launch_tables, return_to_host, settle, stage_inputs, table_calls

__all__ = ["FP8BlockToMXFP8Converter", "FP8BlockToNVFP4Converter", "FP8BLOCK_MXFP8_MEASURED_FASTER", "FP8BLOCK_NVFP4_MEASURED_FASTER"]

_DENSE_DTYPES = (torch.bfloat16, torch.float16)
_F8 = torch.float8_e4m3fn

# the dispatch of `fused=None`: True only when tools/fp8block_transcode_bench.py has measured the fused form's median below the composition's MINIMUM
# on both of its tables in both of its runs (the project's dispatch rule).  profiles/fp8block_transcode_bench.jsonl, µs, run 1 / run 2:
# MXFP8  DeepSeek-V3.2-shaped table fused 1050 / 1059 against the composition's minimum 1531 / 1535, Qwen3-4B-shaped one 3376 / 3367 against 5214 / 5222
# NVFP4  (a sample is the key fill and both launches) 1373 / 1374 against 2157 / 2165, and 4348 / 4416 against 7221 / 7278
FP8BLOCK_MXFP8_MEASURED_FASTER = True
FP8BLOCK_NVFP4_MEASURED_FASTER = True


class Target(NamedTuple):
    """what one target format changes of the shared body"""

    format: str
    group: int                # whole groups of this many columns: the reference's GROUP-strategy text otherwise; the fused plan asks it of block_w too
    outputs: Callable         # (rows, cols) -> [(key suffix, shape, dtype)], in the shard's order
    item: str                 # the fused table's row type, a name of `_lib`
    plan: str                 # the fused plan's symbol
    fill: Callable            # (row, views {suffix: tensor}, key address or 0): the output pointers of a fused row
    launches: Callable        # (lib, xdt, dtype, dev) -> launch(table, n, workgroups, stream handle) of `launch_tables`
    keyed: bool               # the fused rows own one zeroed 32-bit amax key each
    second_stage: Callable    # (rest [(module, dense, views)], dtype, dev): the composition behind the dequantize launch
    preset_args: Callable     # (activations) -> (weights, input_activations) of the config group


def check_columns(target: Target, module_name: str, w: torch.Tensor) -> None:
    """the reference's text for a weight whose columns are no whole groups (quantization/lifecycle/forward.py, the GROUP strategy)"""
    if w.shape[1] % target.group:
        prefix = f"{module_name}: " if module_name else ""
        raise ValueError(f"{prefix}tensor column shape must be divisble by the given group_size {target.group} but got {w.shape[1]}")


def source_fields(it, w: torch.Tensor, s: torch.Tensor, block):
    """the fields of a table row that describe the block-quantized weight (every `ct_fp8block_*item` names them alike)"""
    s2 = s.reshape((1,) * (2 - s.dim()) + tuple(s.shape))  # torch broadcasting of a 0-D / 1-D scale
    it.w, it.scale = w.data_ptr(), s2.data_ptr()
    it.rows, it.cols, it.block_h, it.block_w = w.shape[0], w.shape[1], block[0], block[1]
    it.scale_shape[0], it.scale_shape[1] = s2.shape
    it.sdt = _lib.DT[s.dtype]
    return it


def fused_admits(target: Target, w: torch.Tensor, first_output: torch.Tensor, block) -> bool:
    """what the target's fused plan asks of a row beyond the checks made before anything was staged: the plan is never handed a row it would refuse"""
    return block[1] % target.group == 0 and w.data_ptr() % 16 == 0 and first_output.data_ptr() % 16 == 0


def transcode(target: Target, out: ReadyDict, modules: List[str], pairs, block, dtype, dev, fused: bool, to_host: bool = True,
              stream_results: bool = False) -> None:
    """`out[f"{module}.{suffix}"]` of every (weight, weight_scale_inv) pair and output of the target: one staging copy, the fused launch(es) over the
    rows the plan admits (`fused`), the composition over the others, one copy back (`to_host`; else device tensors of their own)"""
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        inputs = [{"w": w, "s": s} for w, s in pairs]
        stage_inputs(out, inputs, dev)
        specs, suffixes = [], {}
        for m, sd in zip(modules, inputs):
            entries = target.outputs(*sd["w"].shape)
            suffixes[m] = [suffix for suffix, _, _ in entries]
            specs += [(f"{m}.{suffix}", shape, dt) for suffix, shape, dt in entries]
        dbuf, dev_out = device_outputs(specs, dev)

        lib, xdt = _lib.load(), _lib.DT[dtype]
        item_type = getattr(_lib, target.item)
        fused_rows, rest = [], []
        for m, sd in zip(modules, inputs):
            w, s = sd["w"], sd["s"]
            if w.numel() == 0:
                continue
            views = {suffix: dev_out[f"{m}.{suffix}"] for suffix in suffixes[m]}
            if fused and fused_admits(target, w, views[suffixes[m][0]], block):
                fused_rows.append((m, w, s, views))
            else:
                rest.append((m, w, s, views))
        keys = torch.zeros(len(fused_rows), dtype=torch.int32, device=dev) if target.keyed and fused_rows else None  # the table's one fill
        items = []
        for n, (m, w, s, views) in enumerate(fused_rows):
            it = source_fields(item_type(), w, s, block)
            target.fill(it, views, keys.data_ptr() + 4 * n if keys is not None else 0)
            items.append(it)
        launch_tables(items, [m for m, _, _, _ in fused_rows], item_type, getattr(lib, target.plan), target.launches(lib, xdt, dtype, dev), dev)

        if rest:  # the composition: the dequantize table into a dense device buffer, the target's one-pass table over it
            _, dense = device_outputs([(m, tuple(w.shape), dtype) for m, w, _, _ in rest], dev)
            ditems = []
            for m, w, s, _ in rest:
                it = source_fields(_lib.Fp8BlockItem(), w, s, block)
                it.out = dense[m].data_ptr()
                ditems.append(it)
            launch_tables(ditems, [m for m, _, _, _ in rest], _lib.Fp8BlockItem, lib.ct_fp8block_dequant_plan,
                          lambda table, n, blocks, handle: lib.ct_fp8block_dequant_batch(table, n, blocks, xdt, handle), dev)
            target.second_stage([(m, dense[m], views) for m, _, _, views in rest], dtype, dev)  # (the dense buffer was allocated on this stream: freed in its order)

        if not to_host:
            stream.synchronize()
            out.keep.clear()
            for name, view in dev_out.items():  # tensors of their own, as FP8BlockDequantizer hands back: a view would keep the whole buffer alive
                out[name] = view.clone()        # and alias its neighbour's storage, which a saved state dict must not
            return
        return_to_host(out, specs, dbuf, stream)
        settle(out, stream, stream_results)


def transcode_one(target: Target, entry: str, weight, weight_scale_inv, weight_block_size, dtype):
    """the single-tensor entries of `codec` (`fp8block_to_mxfp4` / `_mxfp8` / `_nvfp4`): the outputs of one weight in the target's order; host tensors
    in, host tensors out, device tensors stay on their device.  Everything that raises raises before a device is asked for."""
    if dtype not in _DENSE_DTYPES:
        raise ValueError(f"{entry}: dtype must be torch.bfloat16 or torch.float16, got {dtype}")
    block = _block_size(entry, weight_block_size)
    _check_module("weight", weight, weight_scale_inv)
    check_columns(target, "", weight)
    on_device = weight.device.type == "cuda"
    got = ReadyDict()
    transcode(target, got, ["w"], [(weight, weight_scale_inv)], block, dtype, weight.device if on_device else _lib.require_device(), True,
              to_host=not on_device)
    got.wait()
    return tuple(got[f"w.{suffix}"] for suffix, _, _ in target.outputs(*weight.shape))


# ----------------------------------------------------------------------------------------------------------------------- the targets
def _w4_rows(rest, group: int, dst: str, stored: str):
    """the `ct_w4_item` rows of a one-pass table over the dense weights: dst = the codes, zp_packed = the stored scales"""
    rows = []
    for _, d, views in rest:
        row = _lib.W4Item()
        row.src, row.rows, row.cols, row.group = d.data_ptr(), d.shape[0], d.shape[1], group
        row.dst, row.zp_packed = views[dst].data_ptr(), views[stored].data_ptr()
        rows.append(row)
    return rows


def _mx_fill(codes: str):
    def fill(it, views, key):
        it.packed, it.e8m0 = views[codes].data_ptr(), views["weight_scale"].data_ptr()
    return fill


def _mxfp4_second_stage(rest, dtype, dev):
    from ... import codec

    plan, launch = table_calls(*codec.rtn_mxfp4_launch(dtype))
    launch_tables(_w4_rows(rest, 32, "weight_packed", "weight_scale"), [m for m, _, _ in rest], _lib.W4Item, plan, launch, dev)


def _mxfp8_second_stage(rest, dtype, dev):
    from ... import codec

    plan, launch = table_calls(*codec.rtn_group8_launch(dtype, dev, codec._QP_MXFP8))
    launch_tables(_w4_rows(rest, 32, "weight", "weight_scale"), [m for m, _, _ in rest], _lib.W4Item, plan, launch, dev)


def _mxfp8_launches(lib, xdt, dtype, dev):
    from ... import codec

    lut = codec._mx_code_table(dtype, dev).data_ptr()  # cached per (dtype, device): outlives the launch
    return lambda table, n, blocks, handle: lib.ct_fp8block_mxfp8_batch(table, n, blocks, xdt, lut, handle)


def _nvfp4_fill(it, views, key):
    it.packed, it.scale_f8 = views["weight_packed"].data_ptr(), views["weight_scale"].data_ptr()
    it.key, it.global_scale = key, views["weight_global_scale"].data_ptr()


def _nvfp4_second_stage(rest, dtype, dev):
    """the two launches of the one-pass NVFP4 table over what it takes (cols % 32 == 0); a weight of an odd number of groups per row goes through
    `generate_gparam`, the observer and the FP4 compress, which write the same bytes"""
    from ... import codec

    table = [r for r in rest if r[1].shape[1] % 32 == 0]
    if table:
        keys = codec.rtn_nvfp4_keys(len(table), dev)
        rows = _w4_rows(table, 16, "weight_packed", "weight_scale")
        for n, (row, (_, _, views)) in enumerate(zip(rows, table)):
            row.zp, row.scale = keys.data_ptr() + 4 * n, views["weight_global_scale"].data_ptr()
        (plan, fold), (_, quantize) = (table_calls("rtn_nvfp4", d, (_lib.DT[dtype],)) for d in (0, 1))  # one plan, two launches over the same rows
        launch_tables(rows, [m for m, _, _ in table], _lib.W4Item, plan, lambda *a: fold(*a) or quantize(*a), dev)
    for _, d, views in rest:
        if d.shape[1] % 32 == 0:
            continue
        gs = codec.generate_gparam(d)
        scale = codec.minmax_qparams_float(d, kind="nvfp4", group_size=16, global_scale=gs)
        got = codec.fp4_quantize_and_pack_stored(d, scale, gs, group_size=16, scale_dtype=_F8)
        packed, stored = got if got is not None else (codec.fp4_quantize_and_pack(d, scale, gs, group_size=16), scale.to(_F8))
        views["weight_packed"].copy_(packed)
        views["weight_scale"].copy_(stored)
        views["weight_global_scale"].copy_(gs)


def _nvfp4_launches(lib, xdt, dtype, dev):
    return lambda table, n, blocks, handle: (lib.ct_fp8block_nvfp4_amax_batch(table, n, blocks, xdt, handle)
                                             or lib.ct_fp8block_nvfp4_batch(table, n, blocks, xdt, handle))


MXFP4 = Target(
    format="mxfp4-pack-quantized", group=32,
    outputs=lambda rows, cols: [("weight_packed", (rows, cols // 2), torch.uint8), ("weight_scale", (rows, cols // 32), torch.uint8)],
    item="Fp8BlockMxItem", plan="ct_fp8block_mxfp4_plan", fill=_mx_fill("weight_packed"),
    launches=lambda lib, xdt, dtype, dev: (lambda table, n, blocks, handle: lib.ct_fp8block_mxfp4_batch(table, n, blocks, xdt, handle)),
    keyed=False, second_stage=_mxfp4_second_stage, preset_args=mxfp4_preset_args)

MXFP8 = Target(
    format="mxfp8-quantized", group=32,
    outputs=lambda rows, cols: [("weight", (rows, cols), _F8), ("weight_scale", (rows, cols // 32), torch.uint8)],
    item="Fp8BlockMxItem", plan="ct_fp8block_mxfp8_plan", fill=_mx_fill("weight"), launches=_mxfp8_launches,
    keyed=False, second_stage=_mxfp8_second_stage, preset_args=lambda activations: mxfp8_preset_args())

NVFP4 = Target(
    format="nvfp4-pack-quantized", group=16,
    outputs=lambda rows, cols: [("weight_packed", (rows, cols // 2), torch.uint8), ("weight_scale", (rows, cols // 16), _F8),
                                ("weight_global_scale", (1,), torch.float32)],
    item="Fp8BlockNvItem", plan="ct_fp8block_nvfp4_plan", fill=_nvfp4_fill, launches=_nvfp4_launches,
    keyed=True, second_stage=_nvfp4_second_stage,
    preset_args=lambda activations: (dict(_NVFP4_WEIGHTS), dict(_NVFP4_INPUTS) if activations else None))


# ----------------------------------------------------------------------------------------------------------------------- the converters
class FP8BlockTranscoder(Converter):
    """The body of the converters that transcode a checkpoint block-quantized with the FP8 quant_method (`weight` float8_e4m3fn, `weight_scale_inv`
    per block): every targeted `weight` is replaced by the target's entries, its `weight_scale_inv` is dropped, every other tensor passes through as
    the same object.  A concrete class names its `target` and its measured flag (`_measured`).  `fused`: None follows that flag, True / False force
    the fused launch(es) / the composition."""

    target: Target = None
    format: str = None  # the target's

    def __init__(self, ignore: Iterable[str] = tuple(), targets: Iterable[str] = tuple(), weight_block_size=(128, 128), dtype=torch.bfloat16,
                 activations: bool = False, *, device=None, fused=None):
        if dtype not in _DENSE_DTYPES:
            raise ValueError(f"{type(self).__name__}: dtype must be torch.bfloat16 or torch.float16, got {dtype}")
        self.weight_block_size = _block_size(type(self).__name__, weight_block_size)
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

    def _measured(self) -> bool:
        raise NotImplementedError

    def _fused(self) -> bool:
        return self._measured() if self.fused is None else bool(self.fused)

    def process(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """the converted shard, in the input's order: every targeted `weight` is replaced by the target's entries in their order, its
        `weight_scale_inv` is dropped, every other tensor passes through as the same object"""
        modules = [m for m, name in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=self.param_names)
                   if name.rpartition(".")[-1] == "weight"]
        for m in modules:  # everything that raises for a module raises here, before anything is staged
            if f"{m}.weight_scale_inv" not in tensors:
                raise ValueError(f"Found weight without corresponding weight_scale_inv {m}.weight")
            _check_module(m, tensors[f"{m}.weight"], tensors[f"{m}.weight_scale_inv"])
            check_columns(self.target, m, tensors[f"{m}.weight"])
        targeted = set(modules)
        out = ReadyDict()
        for name, t in tensors.items():
            m, _, param = name.rpartition(".")
            if m in targeted and param == "weight":
                for suffix, _, _ in self.target.outputs(*t.shape):
                    out[f"{m}.{suffix}"] = None  # their places; `transcode` fills them
            elif not (m in targeted and param == "weight_scale_inv"):
                out[name] = t
        if modules:
            transcode(self.target, out, modules, [(tensors[f"{m}.weight"], tensors[f"{m}.weight_scale_inv"]) for m in modules],
                      self.weight_block_size, self.dtype, self.device or _lib.require_device(), self._fused(), stream_results=self.stream_results)
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
        return self.target.preset_args(self.activations)

    create_config = _DenseQuantizer.create_config  # the same config shape: it reads `targets`, `ignore`, `format` and `_preset_args` alone


class FP8BlockToMXFP8Converter(FP8BlockTranscoder):
    """Transcode an FP8 block-quantized checkpoint to the MXFP8 scheme in the compressed-tensors `mxfp8-quantized` format: per targeted module
    `weight` (the requantized float8_e4m3fn codes, (rows, cols)) where the weight was and `weight_scale` (uint8 E8M0 exponents, (rows, cols / 32))
    behind it; the `weight_scale_inv` is dropped.  The bytes are those of `FP8BlockDequantizer(dtype=dtype)` followed by the round-to-nearest MXFP8
    compress of the dense weights (`MXFP8Quantizer`).  The config is the reference's MXFP8 preset (`activations` changes nothing: the preset's
    activations are dynamic).  `fused`: None follows `FP8BLOCK_MXFP8_MEASURED_FASTER`."""

    target, format = MXFP8, MXFP8.format

    def _measured(self) -> bool:
        return FP8BLOCK_MXFP8_MEASURED_FASTER


class FP8BlockToNVFP4Converter(FP8BlockTranscoder):
    """Transcode an FP8 block-quantized checkpoint to the NVFP4A16 scheme in the compressed-tensors `nvfp4-pack-quantized` format: per targeted
    module `weight_packed` (uint8, (rows, cols / 2)) where the weight was, `weight_scale` (float8_e4m3fn, (rows, cols / 16)) and
    `weight_global_scale` (float32 (1,)) behind it; the `weight_scale_inv` is dropped.  The bytes are those of `FP8BlockDequantizer(dtype=dtype)`
    followed by `generate_gparam` and the round-to-nearest NVFP4 compress of the dense weights.  `activations=True` writes the NVFP4 preset (its
    input activations are dynamic per group under a global scale that is calibrated elsewhere) instead of NVFP4A16.  `fused`: None follows
    `FP8BLOCK_NVFP4_MEASURED_FASTER`."""

    target, format = NVFP4, NVFP4.format

    def _measured(self) -> bool:
        return FP8BLOCK_NVFP4_MEASURED_FASTER
