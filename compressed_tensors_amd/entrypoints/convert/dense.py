"""Dense checkpoints -> compressed-tensors checkpoints of the data-free presets (no reference counterpart: the reference produces such checkpoints
through calibration-free `compress_model`; the bits are those of calculate_qparams over each block's, group's or output channel's min / max followed by
`quantize` and the format's packing): `FP8BlockQuantizer` (FP8_BLOCK, `float-quantized`), `MXFP8Quantizer` (`mxfp8-quantized`), `MXFP4Quantizer`
(MXFP4A16 / MXFP4, `mxfp4-pack-quantized`), `FP8DynamicQuantizer` (FP8_DYNAMIC, `float-quantized`), `W8A8Quantizer` (INT8_W8A8, `int-quantized`) and
`PackQuantizedQuantizer` (W4A16, W4A16_ASYM, W2A16 ... W7A16 and their channel-wise forms, `pack-quantized`).  One body, `_DenseQuantizer`, serves all
six; `CompressedTensorsDequantizer` reads every one of them back."""
from typing import Dict, Iterable, List, Set

import torch

from ... import _lib, codec
from ...compressors.fp4.base import MXFP4PackedCompressor
from ...compressors.mxfp8.base import MXFP8QuantizationCompressor
from ...compressors.naive_quantized.base import FloatQuantizationCompressor, IntQuantizationCompressor
from ...compressors.pack_quantized.base import PackedQuantizationCompressor
from ...quantization.quant_args import QuantizationArgs, QuantizationScheme
from .converters import Converter, _ConfigDict, match_quantizable_tensors
from .fp8block import _block_size
from .staging import ReadyDict, device_outputs, launch_tables, return_to_host, settle, stage_inputs, table_calls

__all__ = ["FP8BlockQuantizer", "MXFP8Quantizer", "MXFP4Quantizer", "FP8DynamicQuantizer", "W8A8Quantizer", "PackQuantizedQuantizer"]

_DENSE_DTYPES = (torch.bfloat16, torch.float16)
_DEFAULT_IGNORE = ("lm_head", "re:.*embed_tokens$")


def _preset(**changed) -> dict:
    """a QuantizationArgs.model_dump() of the reference's presets (quantization/quant_scheme.py), written as what it changes of FP8_DYNAMIC's weights:
    static symmetric float8 codes under one min-max scale per output channel"""
    return {"num_bits": 8, "type": "float", "symmetric": True, "group_size": None, "strategy": "channel", "block_structure": None, "dynamic": False,
            "actorder": None, "scale_dtype": None, "zp_dtype": None, "observer": "memoryless_minmax", "observer_kwargs": {}, **changed}


def mxfp4_preset_args(activations: bool):
    """(weights, input_activations) of the reference's MXFP4A16 preset, or of MXFP4 with `activations` (quant_scheme.py:204-238)"""
    mx = dict(num_bits=4, strategy="group", group_size=32, scale_dtype="torch.uint8")  # (a symmetric scheme dumps no zp_dtype)
    return _preset(**mx), (_preset(dynamic=True, observer=None, **mx) if activations else None)


def mxfp8_preset_args():
    """(weights, input_activations) of the reference's MXFP8 preset (quant_scheme.py:253-274)"""
    mx = dict(strategy="group", group_size=32, scale_dtype="torch.uint8")
    return _preset(**mx), _preset(dynamic=True, observer=None, **mx)


class _DenseQuantizer(Converter):
    """The body of every dense-checkpoint quantizer: each targeted 2-D bf16 / fp16 `weight` of a shard is replaced by its entries under the scheme, in the
    input's order; every other tensor passes through as the same object.

    MI355X design of `process`: the dense weights of ALL targeted modules of a shard are staged to the GPU through one pinned buffer and one copy, and
    ONE one-pass table launch per shard and dtype (observer, scale, codes in one pass over each weight; the launch takes the weights' dtype) writes
    every entry into one output buffer; the results come back through one pinned buffer.  What the table's plan refuses (ragged columns, a group or
    block it does not serve, a misaligned device-resident weight) goes through the compressor's `compress_rtn`, one by one, into the same buffer.

    A concrete class supplies what differs: `format`, `_preset_args` (the config's `weights` and `input_activations`, as changes of `_preset`), `_scheme`,
    `_compressor` (whose `compress_rtn` serves the refused modules), `_outputs` with `entry_of` (a module's ordered entries: key suffix, shape, dtype, and the
    table row's field that points at each), `_group` (the admission test and the row's group) and `_launch` (which table, with which arguments)."""

    format: str = None
    partners = ("weight_scale", "weight_scale_inv", "weight_packed")  # the names `validate` refuses beside a targeted weight
    entry_of: dict = None  # the `ct_w4_item` field of a codec output -> the key suffix of the module's entry it becomes; no suffix: scratch behind the row

    def __init__(self, ignore: Iterable[str] = _DEFAULT_IGNORE, targets: Iterable[str] = tuple(), *, device=None):
        self.ignore = ignore
        self.targets = targets
        self.device = torch.device(device) if device is not None else None
        self.param_names = ["weight"]
        # as the other converters: `process` may return before its D2H copies have landed (a ReadyDict) when this is set or inside
        # `streaming_results()`; otherwise it synchronises first
        self.stream_results = False

    # ---- what a concrete class supplies
    def _preset_args(self):
        """(weights, input_activations) of the config group"""
        raise NotImplementedError

    def _scheme(self):
        raise NotImplementedError

    def _compressor(self):
        raise NotImplementedError

    def _outputs(self, rows: int, cols: int, dtype) -> list:
        """codec's `rtn_*_outputs` of one weight: [(row field, shape, dtype)]"""
        raise NotImplementedError

    def _group(self, shape):
        """the row's `group` when the table takes a weight of this shape, else None"""
        raise NotImplementedError

    def _launch(self, dtype, dev) -> tuple:
        """codec's `rtn_*_launch` of a table of `dtype` weights: (kind, d, scalars)"""
        raise NotImplementedError

    # ---- the steps `process` is made of; PackQuantizedQuantizer overrides some
    def _targeted(self, tensors) -> List[str]:
        return [m for m, _ in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=self.param_names)]

    def _entries(self, m: str, w: torch.Tensor) -> list:
        """the ordered entries of module `m`: [(key suffix or None, row field or None, shape, dtype)].  An entry with a suffix is an output of the shard;
        one without is scratch the row points at.  Called before anything is staged: what must raise for a weight's shape raises here."""
        return [(self.entry_of.get(field), field, shape, dtype) for field, shape, dtype in self._outputs(w.shape[0], w.shape[1], w.dtype)]

    def _place(self, out: ReadyDict, m: str, w: torch.Tensor, entries) -> None:
        """the module's keys, where its weight was"""
        for suffix, _, _, _ in entries:
            if suffix:
                out[f"{m}.{suffix}"] = None

    def _row(self, m: str, w: torch.Tensor, entries, dev_out, scratch):
        """the table row of a staged weight, or None for what goes through `compress_rtn`"""
        group = self._group(w.shape)
        at = {field: dev_out[f"{m}.{suffix}"].data_ptr() for suffix, field, _, _ in entries if field and suffix}
        # one check for every scheme: the kernels read and write 16-byte vectors.  Every output slot starts on a 256-byte boundary (`output_layout`), so
        # the destination's half never refuses; the source's does for a misaligned weight handed over on the device
        if group is None or w.data_ptr() % 16 or at["dst"] % 16:
            return None
        it = _lib.W4Item()
        it.src, it.rows, it.cols, it.group = w.data_ptr(), w.shape[0], w.shape[1], group
        for suffix, field, shape, dtype in entries:
            if field and not suffix:
                t = torch.empty(shape, dtype=dtype, device=w.device)
                scratch.append((m, field, t))
                at[field] = t.data_ptr()
        for field, address in at.items():
            setattr(it, field, address)
        return it

    def _after_tables(self, scratch, dev_out) -> None:
        """what follows the table launches on the same stream"""

    def process(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """the converted shard, in the input's order: every targeted 2-D bf16 / fp16 `weight` is replaced by its entries (`_entries`), every other tensor
        passes through as the same object"""
        def dense(t):
            return t.dim() == 2 and t.dtype in _DENSE_DTYPES and t.numel()

        weights = {m: tensors[f"{m}.weight"] for m in self._targeted(tensors) if dense(tensors[f"{m}.weight"])}
        entries = {m: self._entries(m, w) for m, w in weights.items()}
        out = ReadyDict()
        for name, t in tensors.items():  # the outputs' places: a module's entries where its weight was
            m = name[:-7] if name.endswith(".weight") else None
            if m in weights:
                self._place(out, m, t, entries[m])
            else:
                out[name] = t
        if not weights:
            return out
        dev = self.device or _lib.require_device()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            inputs = [{"w": w} for w in weights.values()]
            stage_inputs(out, inputs, dev)
            specs = [(f"{m}.{suffix}", shape, dtype) for m in weights for suffix, _, shape, dtype in entries[m] if suffix]
            dbuf, dev_out = device_outputs(specs, dev)

            tables, rest, scratch = {}, [], []  # one table per dtype: the launch takes the weights' dtype
            for m, sd in zip(weights, inputs):
                w = sd["w"]
                it = self._row(m, w, entries[m], dev_out, scratch)
                if it is None:
                    rest.append((m, w))
                    continue
                items, names = tables.setdefault(w.dtype, ([], []))
                items.append(it)
                names.append(m)
            for dtype, (items, names) in tables.items():
                plan, launch = table_calls(*self._launch(dtype, dev))
                launch_tables(items, names, _lib.W4Item, plan, launch, dev)
            self._after_tables(scratch, dev_out)
            if rest:  # what the plan refuses: `compress_rtn`, one by one
                scheme, compressor = self._scheme(), self._compressor()
                for m, w in rest:
                    got = compressor.compress_rtn(w, scheme)
                    for suffix, _, _, _ in entries[m]:
                        if suffix:
                            dev_out[f"{m}.{suffix}"].copy_(got[suffix])
            return_to_host(out, specs, dbuf, stream)
            settle(out, stream, self.stream_results)
        return out

    def validate(self, tensors: Dict[str, torch.Tensor]):
        """only the NAMES are inspected (`tensors` may hold meta tensors, or None): a targeted module must still be dense"""
        for m in self._targeted(tensors):
            for partner in self.partners:
                if f"{m}.{partner}" in tensors:
                    raise ValueError(f"Found {m}.{partner} beside the targeted {m}.weight: the module is quantized already")

    def get_dependencies(self, weight_name: str) -> Set[str]:
        """a dense weight has no partner tensors"""
        return set()

    def create_config(self) -> _ConfigDict:
        weights, inputs = self._preset_args()
        return _ConfigDict({
            "config_groups": {"config_group_0": {"targets": list(self.targets) or ["Linear"], "weights": weights, "input_activations": inputs,
                                                 "output_activations": None, "format": self.format}},
            "quant_method": "compressed-tensors",
            "kv_cache_scheme": None,
            "format": self.format,
            "quantization_status": "compressed",
            "global_compression_ratio": None,
            "ignore": list(self.ignore),
        })


class FP8BlockQuantizer(_DenseQuantizer):
    """Quantize a dense checkpoint to the FP8_BLOCK scheme (weights float8_e4m3fn in blocks of `weight_block_size`, round-to-nearest under each
    block's min-max scale; activations dynamic in groups of 128) in the compressed-tensors `float-quantized` format: per targeted module `weight`
    (float8_e4m3fn) and `weight_scale` (ceil(rows / bh), ceil(cols / bw)) in the dense weight's dtype.  The inverse of `FP8BlockDequantizer` up
    to the layout: that one reads the HF `fp8` layout (`weight_scale_inv`), `CompressedTensorsDequantizer` reads this one."""

    format = "float-quantized"
    entry_of = {"dst": "weight", "scale": "weight_scale"}

    def __init__(self, ignore: Iterable[str] = _DEFAULT_IGNORE, targets: Iterable[str] = tuple(), weight_block_size=(128, 128), *, device=None):
        _block_size("FP8BlockQuantizer", weight_block_size)
        super().__init__(ignore, targets, device=device)
        self.weight_block_size = weight_block_size

    def _preset_args(self):  # the reference's FP8_BLOCK (quant_scheme.py:385-402), under the converter's block
        return (_preset(strategy="block", block_structure=list(self.weight_block_size)),
                _preset(strategy="group", group_size=128, dynamic=True, observer=None))

    def _scheme(self):
        return QuantizationScheme(targets=["Linear"],
                                  weights=QuantizationArgs(num_bits=8, type="float", strategy="block", symmetric=True, dynamic=False,
                                                           block_structure=list(self.weight_block_size)),
                                  input_activations=QuantizationArgs(num_bits=8, type="float", strategy="group", symmetric=True, dynamic=True,
                                                                     group_size=128))

    def _compressor(self):
        return FloatQuantizationCompressor

    def _outputs(self, rows, cols, dtype):
        return codec.rtn_block8_outputs(rows, cols, dtype, self.weight_block_size)

    def _group(self, shape):
        return codec.rtn_block8_group(shape, self.weight_block_size) or None

    def _launch(self, dtype, dev):
        return codec.rtn_block8_launch(dtype, True, True)


class MXFP8Quantizer(_DenseQuantizer):
    """Quantize a dense checkpoint to the MXFP8 scheme (weights float8_e4m3fn in groups of 32, round-to-nearest under each group's E8M0
    min-max scale; activations dynamic in groups of 32) in the compressed-tensors `mxfp8-quantized` format: per targeted module `weight`
    (float8_e4m3fn) and `weight_scale` (uint8 exponents, (rows, cols / 32)).  Columns that are no whole groups of 32 raise the reference's
    ValueError."""

    format = "mxfp8-quantized"
    entry_of = {"dst": "weight", "zp_packed": "weight_scale"}  # the stored scale is the E8M0 code output

    def _preset_args(self):
        return mxfp8_preset_args()

    def _scheme(self):
        mx = dict(num_bits=8, type="float", strategy="group", symmetric=True, group_size=32, scale_dtype=torch.uint8, zp_dtype=torch.uint8)
        return QuantizationScheme(targets=["Linear"], weights=QuantizationArgs(dynamic=False, **mx), input_activations=QuantizationArgs(dynamic=True, **mx))

    def _compressor(self):
        return MXFP8QuantizationCompressor

    def _outputs(self, rows, cols, dtype):
        return codec.rtn_group8_outputs(rows, cols, dtype, 32, "float", mx=True, with_scale=False)

    def _group(self, shape):
        return codec.rtn_group8_group(shape, 32) or None

    def _launch(self, dtype, dev):
        return codec.rtn_group8_launch(dtype, dev, codec._QP_MXFP8)


class MXFP4Quantizer(_DenseQuantizer):
    """Quantize a dense checkpoint to the MXFP4A16 scheme (weights E2M1 nibbles in groups of 32, round-to-nearest under each group's E8M0 min-max
    scale; with `activations` the MXFP4 scheme: dynamic MXFP4 input activations as well) in the compressed-tensors `mxfp4-pack-quantized` format: per
    targeted module `weight_packed` (uint8, (rows, cols / 2)) where the weight was and `weight_scale` (uint8 exponents, (rows, cols / 32)).  Columns
    that are no whole groups of 32 raise the reference's ValueError."""

    format = "mxfp4-pack-quantized"
    entry_of = {"dst": "weight_packed", "zp_packed": "weight_scale"}  # the stored scale is the E8M0 code output

    def __init__(self, ignore: Iterable[str] = _DEFAULT_IGNORE, targets: Iterable[str] = tuple(), activations: bool = False, *, device=None):
        super().__init__(ignore, targets, device=device)
        self.activations = bool(activations)

    def _preset_args(self):
        return mxfp4_preset_args(self.activations)

    def _scheme(self):
        mx = dict(num_bits=4, type="float", strategy="group", symmetric=True, group_size=32, scale_dtype=torch.uint8, zp_dtype=torch.uint8)
        return QuantizationScheme(targets=["Linear"], weights=QuantizationArgs(dynamic=False, **mx),
                                  input_activations=QuantizationArgs(dynamic=True, **mx) if self.activations else None)

    def _compressor(self):
        return MXFP4PackedCompressor

    def _outputs(self, rows, cols, dtype):
        return codec.rtn_mxfp4_outputs(rows, cols)

    def _group(self, shape):
        return 32  # (`_entries` has refused every other shape)

    def _launch(self, dtype, dev):
        return codec.rtn_mxfp4_launch(dtype)

    def _entries(self, m, w):
        if w.shape[1] % 32:
            raise ValueError(f"{m}: tensor column shape must be divisble by the given group_size 32 but got {w.shape[1]}")
        return super()._entries(m, w)


class _Channel8Quantizer(_DenseQuantizer):
    """the two channel-wise 8-bit presets, data-free by construction: weights round-to-nearest under one min-max scale per row (short, workgroup and
    long rows in one table), activations dynamic per token; both are symmetric: no zero point.  A subclass names its number type and format."""

    qtype: str = None  # "float" / "int"
    entry_of = {"dst": "weight", "scale": "weight_scale"}

    def _preset_args(self):  # the reference's FP8_DYNAMIC and INT8_W8A8 (quant_scheme.py:365-380, 296-311)
        return _preset(type=self.qtype), _preset(type=self.qtype, strategy="token", dynamic=True, observer=None)

    def _scheme(self):
        return QuantizationScheme(targets=["Linear"], weights=QuantizationArgs(num_bits=8, type=self.qtype, strategy="channel", symmetric=True, dynamic=False),
                                  input_activations=QuantizationArgs(num_bits=8, type=self.qtype, strategy="token", symmetric=True, dynamic=True))

    def _compressor(self):
        return FloatQuantizationCompressor if self.qtype == "float" else IntQuantizationCompressor

    def _outputs(self, rows, cols, dtype):
        return codec.rtn_channel8_outputs(rows, cols, dtype, self.qtype == "float")

    def _group(self, shape):
        return 0 if codec.rtn_channel8_form(shape, True) else None  # (the table's rows carry no group)

    def _launch(self, dtype, dev):
        return codec.rtn_channel8_launch(dtype, self.qtype == "float", True)


class FP8DynamicQuantizer(_Channel8Quantizer):
    """Quantize a dense checkpoint to the FP8_DYNAMIC scheme (weights float8_e4m3fn, round-to-nearest under one min-max scale per output channel;
    activations dynamic per token) in the compressed-tensors `float-quantized` format: per targeted module `weight` (float8_e4m3fn) and
    `weight_scale` ((rows, 1), the dense dtype)."""

    qtype, format = "float", "float-quantized"


class W8A8Quantizer(_Channel8Quantizer):
    """Quantize a dense checkpoint to the W8A8 scheme (the reference's INT8_W8A8 preset: weights int8, round-to-nearest under one symmetric
    min-max scale per output channel; activations dynamic per token) in the compressed-tensors `int-quantized` format: per targeted module
    `weight` (int8) and `weight_scale` ((rows, 1), the dense dtype)."""

    qtype, format = "int", "int-quantized"


class PackQuantizedQuantizer(_DenseQuantizer):
    """Quantize a dense checkpoint to an integer weight-only scheme of 2..7 bits (round-to-nearest under each group's — or each output channel's —
    min-max scale, symmetric or not) in the compressed-tensors `pack-quantized` format: per targeted module `weight_packed` (int32,
    (rows, ceil(cols * num_bits / 32))) where the weight was, `weight_scale` ((rows, cols / group), the dense dtype), for an asymmetric scheme
    `weight_zero_point` in its stored form (int32, (ceil(rows * num_bits / 32), cols / group)), and `weight_shape` (int64 [rows, cols]).  The one-pass
    table is `rtn_w4` at 4 bits and `rtn_wb` at 2, 3, 5, 6 and 7; the stored zero points follow it in one `zp4_batch` launch (4 bits) or one
    `pack_to_int32` per module.  Columns that are no whole groups raise the reference's ValueError."""

    format = "pack-quantized"
    partners = _DenseQuantizer.partners + ("weight_shape", "weight_zero_point")
    entry_of = {"dst": "weight_packed", "scale": "weight_scale"}  # the launch's int8 zero points are scratch: their stored form is the entry

    def __init__(self, num_bits: int = 4, group_size: int = 128, symmetric: bool = True, strategy: str = "group",
                 ignore: Iterable[str] = _DEFAULT_IGNORE, targets: Iterable[str] = tuple(), *, device=None):
        self.num_bits = int(num_bits)
        if self.num_bits != 4 and self.num_bits not in codec.RTN_PACKW_BITS:
            raise ValueError(f"PackQuantizedQuantizer writes 2..7-bit words, got num_bits={num_bits} (8 bits: W8A8Quantizer)")
        strategy = getattr(strategy, "value", strategy)
        if strategy not in ("group", "channel"):
            raise ValueError(f"PackQuantizedQuantizer takes the strategies 'group' and 'channel', got {strategy!r}")
        if strategy == "group" and (group_size is None or int(group_size) <= 0):
            raise ValueError("the group strategy needs a positive group_size")
        super().__init__(ignore, targets, device=device)
        self.strategy = strategy
        self.group_size = int(group_size) if strategy == "group" else None
        self.symmetric = bool(symmetric)

    def _preset_args(self):  # the reference's integer weight-only presets (quant_scheme.py:104-131, _int_wnam); no activations
        return _preset(num_bits=self.num_bits, type="int", symmetric=self.symmetric, group_size=self.group_size, strategy=self.strategy,
                       zp_dtype=None if self.symmetric else "torch.int8"), None

    def _scheme(self):
        return QuantizationScheme(targets=["Linear"], weights=QuantizationArgs(num_bits=self.num_bits, type="int", strategy=self.strategy,
                                                                              group_size=self.group_size, symmetric=self.symmetric, dynamic=False))

    def _compressor(self):
        return PackedQuantizationCompressor

    def _outputs(self, rows, cols, dtype):
        return codec.rtn_wb_outputs(rows, cols, dtype, self.group_size or cols, self.num_bits, not self.symmetric)

    def _group(self, shape):
        return codec.rtn_w4_group(shape, self.group_size) or None

    def _launch(self, dtype, dev):
        return codec.rtn_w4_launch(dtype, self.symmetric) if self.num_bits == 4 else codec.rtn_wb_launch(dtype, self.num_bits, self.symmetric)

    def _entries(self, m, w):
        rows, cols = w.shape
        g = self.group_size or cols
        if cols % g:
            raise ValueError(f"{m}: tensor column shape must be divisble by the given group_size {g} but got {cols}")
        entries = super()._entries(m, w)
        if not self.symmetric:  # behind the launch's int8 zero points (scratch), their stored form
            entries.append(("weight_zero_point", None, (-(-rows * self.num_bits // 32), cols // g), torch.int32))
        return entries

    def _place(self, out, m, w, entries):
        super()._place(out, m, w, entries)
        out[f"{m}.weight_shape"] = torch.tensor(w.shape)  # int64, on the host: as the compressor writes it

    def _after_tables(self, scratch, dev_out):
        if scratch and self.num_bits == 4:  # pack_to_int32(zp, 4, packed_dim=0) of every module in one launch
            codec.zp4_batch([(zp, dev_out[f"{m}.weight_zero_point"]) for m, _, zp in scratch], "pack")
        else:
            for m, _, zp in scratch:
                dev_out[f"{m}.weight_zero_point"].copy_(codec.pack_to_int32(zp, self.num_bits, packed_dim=0))
