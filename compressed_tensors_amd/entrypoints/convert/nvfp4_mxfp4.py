"""NVFP4 checkpoints -> `mxfp4-pack-quantized` checkpoints without the dense checkpoint in between (no reference counterpart: the reference reaches
MXFP4 from such a checkpoint through `CompressedTensorsDequantizer`, a model load and `compress_model`).  gfx950's block-scaled matrix cores take
MXFP4 (groups of 32 under E8M0 scales); NVFP4 (groups of 16 under float8_e4m3fn scales and a float32 global scale) is what ModelOpt and llm-compressor
publish.

MI355X design of `NVFP4ToMXFP4Converter.process`: the `weight_packed`, `weight_scale` and `weight_global_scale` of ALL targeted modules of a shard are
staged to the GPU through one pinned buffer and one copy, ONE `ct_nvfp4_mxfp4_batch` launch per shard (csrc/ct_fp4.hip: the bfloat16 element of the
NVFP4 decompress made in registers, then the one-pass MXFP4 compress on those bits; one lane per MX group, which is exactly two NVFP4 groups) writes
every MXFP4 `weight_packed` and `weight_scale` into one output buffer, and the results come back through one pinned buffer.  The bytes are those of
the composition — `CompressedTensorsDequantizer` (bfloat16, the dtype the NVFP4 decompress always yields), then the one-pass MXFP4 compress of the
dense weights —, which is also the path of what the fused plan refuses and of `fused=False`: `NVFP4PackedCompressor.decompress_many` (the
`ct_fp4_unpack_dequant_batch` table) into dense device tensors and one `rtn_mxfp4` table launch over them."""
from typing import Dict, Iterable, List, NamedTuple, Optional, Set

import torch

from ... import _lib
from .converters import Converter, _ConfigDict, match_name, match_quantizable_tensors
from .dense import _DenseQuantizer, mxfp4_preset_args
from .fp8block_transcode import MXFP4, _mxfp4_second_stage, check_columns
from .modelopt import ModelOptNvfp4Converter, _args_dump
from .staging import ReadyDict, device_outputs, launch_tables, return_to_host, settle, stage_inputs

__all__ = ["NVFP4ToMXFP4Converter", "NVFP4_MXFP4_MEASURED_FASTER"]

_F8 = torch.float8_e4m3fn
_SOURCES = ("compressed-tensors", "modelopt")
_PARTNERS = ("weight_scale", "weight_global_scale")
_DIM_MAX = 1 << 31

# the dispatch of `fused=None`: True only when tools/nvfp4_mxfp4_bench.py has measured the fused launch's median below the composition's MINIMUM on
# both of its tables in both of its runs (the project's dispatch rule).  Not measured yet: the composition is the default and
# `fused=True` asks for the one launch
NVFP4_MXFP4_MEASURED_FASTER = False


class _Shape(NamedTuple):
    """what `check_columns` reads of a weight: the dense shape of a packed one"""

    shape: tuple


def _check_module(module_name: str, packed, scale, global_scale) -> None:
    """an NVFP4 module as the compressed-tensors format stores it, else a ValueError naming the module; then the reference's GROUP-strategy text for a
    width that is whole NVFP4 groups but no whole MX groups"""
    prefix = f"{module_name}: " if module_name else ""
    if not (isinstance(packed, torch.Tensor) and packed.dim() == 2 and packed.dtype is torch.uint8):
        raise ValueError(f"{prefix}weight_packed: expected a 2-D uint8 tensor, got {_describe(packed)}")
    rows, cols = packed.shape[0], 2 * packed.shape[1]
    if not (isinstance(scale, torch.Tensor) and scale.dim() == 2 and scale.dtype is _F8):
        raise ValueError(f"{prefix}weight_scale: expected a 2-D float8_e4m3fn tensor, got {_describe(scale)}")
    if cols % 16 or tuple(scale.shape) != (rows, cols // 16):
        raise ValueError(f"{prefix}weight_scale of shape {tuple(scale.shape)} for a weight_packed of shape {tuple(packed.shape)}: expected one scale "
                         f"per 16 columns of the ({rows}, {cols}) weight")
    if not (isinstance(global_scale, torch.Tensor) and global_scale.numel() == 1 and global_scale.is_floating_point()):
        raise ValueError(f"{prefix}weight_global_scale: expected one floating-point element, got {_describe(global_scale)}")
    check_columns(MXFP4, module_name, _Shape((rows, cols)))


def _describe(t) -> str:
    return f"{t.dtype} of shape {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__


def _fused_admits(packed: torch.Tensor, scale: torch.Tensor, global_scale: torch.Tensor, packed_out: torch.Tensor) -> bool:
    """what `ct_nvfp4_mxfp4_plan` asks of a row beyond the checks made before anything was staged: the plan is never handed a row it would refuse"""
    return (global_scale.dtype is torch.float32 and packed.shape[0] < _DIM_MAX and 2 * packed.shape[1] < _DIM_MAX and packed.data_ptr() % 16 == 0
            and packed_out.data_ptr() % 16 == 0 and scale.data_ptr() % 2 == 0 and global_scale.data_ptr() % 4 == 0)


def transcode(out: ReadyDict, modules: List[str], triples, dev, fused: bool, to_host: bool = True, stream_results: bool = False) -> None:
    """`out[f"{module}.weight_packed"]` / `out[f"{module}.weight_scale"]` (MXFP4) of every (weight_packed, weight_scale, weight_global_scale) triple
    (NVFP4): one staging copy, one fused launch over the rows its plan admits (`fused`), the composition over the others, one copy back (`to_host`;
    else device tensors of their own)"""
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        inputs = [{"p": p, "s": s, "g": g} for p, s, g in triples]
        stage_inputs(out, inputs, dev)
        specs = []
        for m, sd in zip(modules, inputs):
            rows, half = sd["p"].shape
            specs += [(f"{m}.weight_packed", (rows, half), torch.uint8), (f"{m}.weight_scale", (rows, half // 16), torch.uint8)]
        dbuf, dev_out = device_outputs(specs, dev)

        lib = _lib.load()
        fused_rows, rest = [], []
        for m, sd in zip(modules, inputs):
            p, s, g = sd["p"], sd["s"], sd["g"]
            if p.numel() == 0:
                continue
            views = {"weight_packed": dev_out[f"{m}.weight_packed"], "weight_scale": dev_out[f"{m}.weight_scale"]}
            (fused_rows if fused and _fused_admits(p, s, g, views["weight_packed"]) else rest).append((m, p, s, g, views))
        items = []
        for _, p, s, g, views in fused_rows:
            it = _lib.Nvfp4MxItem()
            it.packed_in, it.scale_f8, it.global_scale = p.data_ptr(), s.data_ptr(), g.data_ptr()
            it.packed_out, it.e8m0 = views["weight_packed"].data_ptr(), views["weight_scale"].data_ptr()
            it.rows, it.cols = p.shape[0], 2 * p.shape[1]
            items.append(it)
        launch_tables(items, [r[0] for r in fused_rows], _lib.Nvfp4MxItem, lib.ct_nvfp4_mxfp4_plan, lib.ct_nvfp4_mxfp4_batch, dev)

        if rest:  # the composition: the NVFP4 decompress table into dense bfloat16 tensors, the one-pass MXFP4 table over them
            from ...compressors.fp4.base import NVFP4PackedCompressor

            dense = NVFP4PackedCompressor.decompress_many([{"weight_packed": p, "weight_scale": s, "weight_global_scale": g} for _, p, s, g, _ in rest], None)
            _mxfp4_second_stage([(m, d["weight"], views) for (m, _, _, _, views), d in zip(rest, dense)], torch.bfloat16, dev)
            del dense  # (allocated on this stream: freed in its order)

        if not to_host:
            stream.synchronize()
            out.keep.clear()
            for name, view in dev_out.items():  # tensors of their own: a view would keep the whole buffer alive and alias its neighbour's storage
                out[name] = view.clone()
            return
        return_to_host(out, specs, dbuf, stream)
        settle(out, stream, stream_results)


def transcode_one(weight_packed, weight_scale, weight_global_scale):
    """`codec.nvfp4_to_mxfp4`: (weight_packed, weight_scale) of one weight; host tensors in, host tensors out, device tensors stay on their device.
    Everything that raises raises before a device is asked for."""
    _check_module("", weight_packed, weight_scale, weight_global_scale)
    on_device = weight_packed.device.type == "cuda"
    got = ReadyDict()
    transcode(got, ["w"], [(weight_packed, weight_scale, weight_global_scale)], weight_packed.device if on_device else _lib.require_device(), True,
              to_host=not on_device)
    got.wait()
    return got["w.weight_packed"], got["w.weight_scale"]


class NVFP4ToMXFP4Converter(Converter):
    """Transcode an NVFP4 checkpoint to the MXFP4 scheme in the compressed-tensors `mxfp4-pack-quantized` format: per targeted module the MXFP4
    `weight_packed` (uint8, (rows, cols / 2)) where the NVFP4 one was and `weight_scale` (uint8 E8M0 exponents, (rows, cols / 32)) behind it;
    `weight_global_scale` is dropped, and so is `input_global_scale` (MXFP4's activations are dynamic per group and have no global scale).  Every other
    tensor passes through as the same object.  The bytes are those of the NVFP4 decompress (bfloat16) followed by the round-to-nearest MXFP4 compress
    of the dense weights.

    `source`: "compressed-tensors" reads the format's own names; "modelopt" reads a ModelOpt NVFP4 checkpoint, whose shard first goes through
    `ModelOptNvfp4Converter(ignore, targets, kv_cache_scheme).process` (`validate` and `get_dependencies` then answer in ModelOpt's names).
    `activations=True` writes the MXFP4 preset (dynamic MXFP4 input activations) instead of MXFP4A16; `fused`: None follows
    `NVFP4_MXFP4_MEASURED_FASTER`, True / False force the one launch / the composition."""

    format = MXFP4.format

    def __init__(self, ignore: Iterable[str] = tuple(), targets: Iterable[str] = tuple(), activations: bool = False, *,
                 source: str = "compressed-tensors", kv_cache_scheme=None, device=None, fused: Optional[bool] = None):
        if source not in _SOURCES:
            raise ValueError(f"NVFP4ToMXFP4Converter: source must be one of {_SOURCES}, got {source!r}")
        self.ignore = ignore
        self.targets = targets
        self.activations = bool(activations)
        self.source = source
        self.kv_cache_scheme = kv_cache_scheme
        self.device = torch.device(device) if device is not None else None
        self.fused = fused
        self._modelopt = ModelOptNvfp4Converter(ignore, targets, kv_cache_scheme) if source == "modelopt" else None
        self.param_names = list(self._modelopt.param_names) if self._modelopt else ["weight_packed", *_PARTNERS, "input_global_scale"]
        # as the other converters: `process` may return before its D2H copies have landed (a ReadyDict) when this is set or inside
        # `streaming_results()`; otherwise it synchronises first
        self.stream_results = False

    def _fused(self) -> bool:
        return NVFP4_MXFP4_MEASURED_FASTER if self.fused is None else bool(self.fused)

    def _matched(self, tensors, param: str) -> List[str]:
        return [m for m, _ in match_quantizable_tensors(tensors, self.ignore, self.targets, param_targets=[param])]

    def process(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """the converted shard, in the order of the input (of `ModelOptNvfp4Converter.process`'s output for that source): every targeted
        `weight_packed` is replaced by the MXFP4 `weight_packed` and `weight_scale`, its NVFP4 `weight_scale`, `weight_global_scale` and
        `input_global_scale` are dropped, every other tensor passes through as the same object"""
        if self._modelopt is not None:
            tensors = self._modelopt.process(dict(tensors))
        modules = self._matched(tensors, "weight_packed")
        for m in modules:  # everything that raises for a module raises here, before anything is staged
            for partner in _PARTNERS:
                if f"{m}.{partner}" not in tensors:
                    raise ValueError(f"Found weight_packed without corresponding {partner} {m}.weight_packed")
            _check_module(m, tensors[f"{m}.weight_packed"], tensors[f"{m}.weight_scale"], tensors[f"{m}.weight_global_scale"])
        targeted, no_inputs = set(modules), set(self._matched(tensors, "input_global_scale"))
        out = ReadyDict()
        for name, t in tensors.items():
            m, _, param = name.rpartition(".")
            if m in targeted and param == "weight_packed":
                out[f"{m}.weight_packed"] = out[f"{m}.weight_scale"] = None  # their places; `transcode` fills them
            elif not ((m in targeted and param in _PARTNERS) or (m in no_inputs and param == "input_global_scale")):
                out[name] = t
        if modules:
            transcode(out, modules, [tuple(tensors[f"{m}.{p}"] for p in ("weight_packed", *_PARTNERS)) for m in modules],
                      self.device or _lib.require_device(), self._fused(), stream_results=self.stream_results)
        return out

    def validate(self, tensors: Dict[str, torch.Tensor]):
        """only the NAMES are inspected (`tensors` may hold meta tensors, or None): a targeted `weight_packed` has both partners, and no
        `weight_global_scale` sits outside the targeted modules"""
        if self._modelopt is not None:
            return self._modelopt.validate(tensors)
        targeted = set(self._matched(tensors, "weight_packed"))
        for m in targeted:
            for partner in _PARTNERS:
                if f"{m}.{partner}" not in tensors:
                    raise ValueError(f"Found weight_packed without corresponding {partner} {m}.weight_packed")
        for name in tensors.keys():
            m, _, param = name.rpartition(".")
            if param == "weight_global_scale" and m not in targeted and not any(match_name(name, ign) or match_name(m, ign) for ign in self.ignore):
                raise ValueError(f"Found unexpected non-targeted tensor {name}")

    def get_dependencies(self, weight_name: str) -> Set[str]:
        if self._modelopt is not None:
            return self._modelopt.get_dependencies(weight_name)
        module_name, _, param_name = weight_name.rpartition(".")
        if (any(match_name(module_name, t) for t in self.targets) and not any(match_name(module_name, i) for i in self.ignore)
                and param_name == "weight_packed"):
            return {f"{module_name}.{partner}" for partner in _PARTNERS}
        return set()

    def _preset_args(self):
        return mxfp4_preset_args(self.activations)

    def create_config(self) -> _ConfigDict:
        """the config shape of the dense-checkpoint quantizers under the MXFP4A16 / MXFP4 preset, with the kv_cache_scheme dumped as
        `ModelOptNvfp4Converter` dumps it"""
        cfg = _DenseQuantizer.create_config(self).model_dump()
        cfg["kv_cache_scheme"] = _args_dump(self.kv_cache_scheme)
        return _ConfigDict(cfg)
