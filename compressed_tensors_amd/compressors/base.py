"""Compressor plug-in surface, mirrored from the reference (compressors/base.py:34-219).

`BaseCompressor` subclasses are never instantiated: they are looked up by their wire-format
string (`BaseCompressor.get_value_from_registry("pack-quantized")`) and used through
classmethods on *local-name* state dicts (`weight`, `weight_scale`, ...).  Inputs are never
mutated; untouched tensors are returned by identity.
"""
from abc import ABC
from typing import Optional

import torch

from ..config import CompressionFormat
from ..quantization.quant_args import QuantizationStatus, is_scheme
from ..registry import RegistryMixin
from ..utils.module import direct_entry, get_direct_state_dict, replace_direct_state_dict, swap_direct_entries

__all__ = ["BaseCompressor", "symmetric_zp_keys", "zp_drop_mask", "rtn_windows", "run_rtn_windows", "launch_chunks", "run_planned", "compress_module", "decompress_module", "compress_modules", "decompress_modules", "COMPRESSIBLE_MODULE_TYPES"]

# reference compressors/base.py:31
COMPRESSIBLE_MODULE_TYPES = (torch.nn.Linear, torch.nn.Embedding)


_ZP_OF_ARGS = (("input_activations", "input_zero_point"), ("weights", "weight_zero_point"), ("output_activations", "output_zero_point"))


def symmetric_zp_keys(scheme) -> list:
    """the zero-point names that a symmetric scheme does not store (compressors/base.py:147-167)"""
    keys = []
    for args_name, key in _ZP_OF_ARGS:
        args = getattr(scheme, args_name, None)
        if args is not None and getattr(args, "symmetric", False):
            keys.append(key)
    return keys


def zp_drop_mask(scheme) -> int:
    """`symmetric_zp_keys` as the bit mask the C++ host loops take (csrc/host/ct_hostpath.cpp): 1 weight, 2 input, 4 output zero point"""
    drop = 0
    for key in symmetric_zp_keys(scheme):
        drop |= {"weight_zero_point": 1, "input_zero_point": 2, "output_zero_point": 4}[key]
    return drop


# modules per table of the data-free (round-to-nearest) module paths — the codecs' window hook `compress_rtn_modules`, over `run_rtn_windows` below:
# building a table costs the host ~10 us per module, during which the GPU would idle, so a long list leaves as windows — the host builds window k + 1 and rewrites the parameter dictionaries of window k under
# window k's kernel.  tools/rtn_bench.py, W4 g128, windows of 16 / 32 / 64 / one table: 3.60 / 3.63 / 3.74 / 4.66 ms on an 8B-shaped tree (the per-module
# loop: 4.53), 2.20 / 2.06 / 2.00 / 2.09 ms on a TinyLlama-shaped one (3.14)
RTN_WINDOW = 32


def rtn_windows(modules):
    modules = list(modules)
    return [modules[lo:lo + RTN_WINDOW] for lo in range(0, len(modules), RTN_WINDOW)]


def run_rtn_windows(cls, modules, item, launch, entries, state=None) -> None:
    """the driver of every data-free window hook (`compress_rtn_modules` of the codecs that have a one-pass table): `compress_rtn` + the parameter
    swap for a list of modules, in windows (`rtn_windows`).  Per window it fetches each module's `weight`, groups the modules the codec takes into
    tables, issues EVERY table's launch before any module is touched, rewrites the parameter dictionaries under the kernels — every `weight*`
    entry goes, the codec's entries come — and then runs the modules no table took through `cls.compress_rtn_module`, in module order.  Every
    module ends in exactly the state `compress_rtn_module` leaves it in.  The codec supplies what differs:

    `item(m, w, table)` -> None, or `(key, row, outs)` once it takes module `m` with weight `w`: `key` = (device, dtype, ...) names the launch the
        module joins, `row` is its `codec.item_row` and `outs` its freshly allocated outputs.  A table opens at its first item — (flat rows, jobs,
        `state(len(window), device)` or None); a codec whose rows point into that state (NVFP4: the amax keys, item n owns word n = `len(jobs)`)
        asks for it with `table(key)` before it builds the row;
    `launch(key, flat, jobs)` -> the device table: the table's launch and whatever has to follow directly behind it (W4: the stored zero
        points); the driver records the device table, then the state, on the device's current stream;
    `entries(w, outs)` -> the parameters a job adds.

    (Host-bound at 10-19 us per module: per module this adds no allocation beyond the job tuple and the returned triple.)"""
    def table(key):  # closes over `tables` and `window`, which the loop below rebinds: it always opens a table of the CURRENT window
        t = tables.get(key)
        if t is None:  # opened by its first item, its state sized by the window
            t = tables[key] = ([], [], None if state is None else state(len(window), key[0]))
        return t

    for window in rtn_windows(modules):
        tables, rest = {}, []
        for m in window:
            w = direct_entry(m, "weight")
            got = item(m, w, table) if w is not None else None
            if got is None:
                rest.append(m)
                continue
            key, row, outs = got
            t = tables.get(key) or table(key)
            t[0].extend(row)
            t[1].append((m, w, outs))  # the table holds raw pointers: the jobs keep the tensors alive
        for key, (flat, jobs, held) in tables.items():
            stream = torch.cuda.current_stream(key[0])
            launch(key, flat, jobs).record_stream(stream)
            if held is not None:
                held.record_stream(stream)
        for _, jobs, _ in tables.values():  # from here on the host works under the kernels
            for m, w, outs in jobs:
                remove = [k for k in (*m._parameters, *m._buffers) if k.startswith("weight")]
                swap_direct_entries(m, remove, entries(w, outs), status=QuantizationStatus.COMPRESSED)
        for m in rest:
            cls.compress_rtn_module(m)


def launch_chunks(n: int):
    """[lo, hi) slices of a module list for the batched launches: planning a 154-module table takes the host ~0.17 ms during which the
    GPU would idle, so a large list goes out as a short first table (the GPU starts after ~40 us) and two longer ones; a small list
    as one (every extra launch costs the host ~15 us and the device a ramp / tail of ~3 us)"""
    if n <= 64:
        return [(0, n)]
    a = 32
    b = a + (n - a) // 2
    return [(0, a), (a, b), (b, n)]


def run_planned(modules, plan, launch, finish) -> list:
    """the driver of every C++ host loop (csrc/host/ct_hostpath.cpp): per chunk of `modules` (`launch_chunks`), `plan(chunk)` -> ({(device index, code):
    (table words, n, jobs, second table's words, its n)}, the modules it does not take); `launch(device, code, words, n, aux_words, aux_n)` issues each
    group's table or tables; then `finish(jobs)` rewrites the parameter dictionaries of every group, under the kernels.  Returns the modules no plan took."""
    rest, pending = [], []
    for lo, hi in launch_chunks(len(modules)):  # the first launch leaves after a fifth of the planning, not after all of it
        planned, back = plan(modules[lo:hi])
        rest += back
        for (dev_index, code), (words, n, jobs, aux_words, aux_n) in planned.items():
            launch(torch.device("cuda", dev_index) if dev_index >= 0 else torch.device("cpu"), code, words, n, aux_words, aux_n)
            pending.append(jobs)
    for jobs in pending:
        finish(jobs)
    return rest


class BaseCompressor(RegistryMixin, ABC):
    @classmethod
    def compression_param_names(cls, scheme) -> tuple:
        raise NotImplementedError(
            f"{cls.__name__} does not implement the classmethod compression_param_names interface"
        )

    @classmethod
    def compress(cls, state_dict: dict, scheme) -> dict:
        raise NotImplementedError(f"{cls.__name__} does not implement the classmethod compress interface")

    @classmethod
    def decompress(cls, state_dict: dict, scheme) -> dict:
        raise NotImplementedError(f"{cls.__name__} does not implement the classmethod decompress interface")

    @classmethod
    def can_compress(cls, module_type: type, scheme) -> bool:
        raise NotImplementedError(f"{cls.__name__} does not implement match")

    @classmethod
    def compress_module(cls, module: torch.nn.Module) -> None:
        """compressors/base.py:95-112"""
        scheme = getattr(module, "quantization_scheme")
        state_dict = get_direct_state_dict(module)
        replace_direct_state_dict(module, cls.compress(state_dict, scheme))
        module.quantization_status = QuantizationStatus.COMPRESSED

    @classmethod
    def decompress_module(cls, module: torch.nn.Module) -> None:
        """compressors/base.py:114-131"""
        scheme = getattr(module, "quantization_scheme")
        state_dict = get_direct_state_dict(module)
        replace_direct_state_dict(module, cls.decompress(state_dict, scheme))
        module.quantization_status = QuantizationStatus.DECOMPRESSED

    @classmethod
    def compress_modules(cls, modules) -> None:
        """compress several modules of this format; codecs may override to batch their launches
        (the reference loops, model_compressor.py:167-169)"""
        for m in modules:
            cls.compress_module(m)

    @classmethod
    def decompress_modules(cls, modules) -> None:
        for m in modules:
            cls.decompress_module(m)

    @classmethod
    def compress_rtn_module(cls, module: torch.nn.Module) -> None:
        """data-free compression of one module from its dense weight (`compress_rtn` of the codecs that have one): every `weight*` entry goes,
        the codec's entries come, bias and the rest stay"""
        new = cls.compress_rtn(direct_entry(module, "weight").data, module.quantization_scheme)
        remove = [k for k in (*module._parameters, *module._buffers) if k.startswith("weight")]
        swap_direct_entries(module, remove, new, status=QuantizationStatus.COMPRESSED)

    @classmethod
    def decompress_many(cls, state_dicts, scheme) -> list:
        """decompress several local-name state dicts of one scheme (the model-free path: one safetensors
        shard, converters/ct_dequantizer.py:63-99); codecs may override to batch their launches"""
        return [cls.decompress(sd, scheme) for sd in state_dicts]

    @classmethod
    def _remove_symmetric_zp(cls, state_dict: dict, scheme) -> dict:
        """compressors/base.py:147-167: vLLM cannot load zero points of symmetric schemes"""
        for key in symmetric_zp_keys(scheme):
            state_dict.pop(key, None)
        return state_dict


def _resolve_format(module, scheme, format):
    from .format import infer_module_format

    fmt = format or getattr(scheme, "format", None) or infer_module_format(type(module), scheme)
    fmt = CompressionFormat(getattr(fmt, "value", fmt))
    try:
        scheme.format = fmt
    except Exception:  # pydantic schemes validate assignment; the string value is always accepted
        scheme.format = fmt.value
    return fmt


def compress_module(module: torch.nn.Module, format: Optional[CompressionFormat] = None):
    """compressors/base.py:170-193"""
    scheme = getattr(module, "quantization_scheme", None)
    if not is_scheme(scheme):
        return
    fmt = _resolve_format(module, scheme, format)
    BaseCompressor.get_value_from_registry(fmt.value).compress_module(module)


def _by_format(modules, format):
    """modules grouped by the wire format their scheme resolves to; the resolution (and the `scheme.format` write-back of
    compress_module, compressors/base.py:186-190) happens once per (scheme object, module type), not once per module"""
    groups, seen = {}, {}
    for m in modules:
        scheme = getattr(m, "quantization_scheme", None)
        key = (id(scheme), type(m))
        fmt = seen.get(key)
        if fmt is None:
            if not is_scheme(scheme):
                continue
            fmt = seen[key] = _resolve_format(m, scheme, format).value
        group = groups.get(fmt)
        if group is None:
            group = groups[fmt] = []
        group.append(m)
    return groups


def compress_modules(modules, format: Optional[CompressionFormat] = None):
    """compress_module over a list, grouped by format so that a codec can batch its kernel launches"""
    for fmt, ms in _by_format(modules, format).items():
        BaseCompressor.get_value_from_registry(fmt).compress_modules(ms)


def decompress_modules(modules, format: Optional[CompressionFormat] = None):
    for fmt, ms in _by_format(modules, format).items():
        BaseCompressor.get_value_from_registry(fmt).decompress_modules(ms)


def decompress_module(module: torch.nn.Module, format: Optional[CompressionFormat] = None):
    """compressors/base.py:196-219"""
    scheme = getattr(module, "quantization_scheme", None)
    if not is_scheme(scheme):
        return
    fmt = _resolve_format(module, scheme, format)
    BaseCompressor.get_value_from_registry(fmt.value).decompress_module(module)
