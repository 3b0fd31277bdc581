"""Dynamic activation quantization: `compute_dynamic_scales_and_zp` (quantization/utils/helpers.py:140-195) and
`forward_quantize` (quantization/lifecycle/forward.py:304-335) with the reference's signatures and control flow.

The dynamic branch runs the fused kernel of csrc/ct_dynamic.hip: the activation is read once, the QDQ result written once,
and the scales and zero points stay in registers unless they are asked for.  `plan_dynamic` is the host half: it maps the
reference's arguments onto the kernel's segments and kinds, and raises NotImplementedError for every case the kernel does
not compute exactly as the reference does (`install(patch_forward=True)` hands those to the reference), or the reference's
own ValueError where it raises one.

`plan_rotated_dynamic` / `rotated_fake_quantize` / `forward_rotate_quantize` are the same forward behind an online Hadamard
rotation (QuaRot, SpinQuant, a `transform_config` with `location: input`): where the plan fuses, the rotation and the QDQ are
ONE launch of csrc/ct_rotated.hip; where it does not, they are the two existing calls — the same bits either way.
"""
import math
import weakref
from typing import Optional

import torch

from .. import codec
from .forward import fake_quantize
from .quant_args import enum_value

__all__ = ["compute_dynamic_scales_and_zp", "forward_quantize", "plan_dynamic", "DynamicPlan", "plan_rotated_dynamic", "RotatedPlan",
           "rotated_fake_quantize", "forward_rotate_quantize", "MEASURED_FASTER", "ALL_FORMS", "remember_prequantized", "take_prequantized"]

_FLOATS = (torch.float32, torch.float16, torch.bfloat16)
_F8 = torch.float8_e4m3fn
_STRATEGIES = ("token", "tensor", "tensor_group", "group")
_ATTENTION_STATES = ("q", "k", "v")  # base names of modeling/attention.py and modeling/kvcache.py
_LIFECYCLE = {"initialized": 0, "calibration": 1, "frozen": 2, "compressed": 3, "decompressed": 4}  # quant_config.py:115-121


class DynamicPlan:
    """what the kernel computes for one call: `segs` segments of `seg_len` elements (one scale each), the calculate_qparams
    kind, and the shapes and dtypes of the scale and zero point the reference returns"""

    __slots__ = ("kind", "num_bits", "symmetric", "segs", "seg_len", "scale_shape", "scale_dtype", "zp_dtype", "tensor_form")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def launches(self) -> int:
        return 2 if self.segs == 1 and self.seg_len > 512 else 1  # codec.dynamic_qdq's choice of the two-launch form


def _kind(args, global_scale):
    """(kind, zp_dtype) of the arguments, or NotImplementedError: calculate_qparams' branches (helpers.py:50-137) the kernel has"""
    qt, bits = enum_value(getattr(args, "type", "int")), int(args.num_bits)
    scale_dtype, zp_dtype = getattr(args, "scale_dtype", None), getattr(args, "zp_dtype", None)
    symmetric = bool(args.symmetric)
    if qt == "int":
        kind = "int"
        ok = 1 <= bits <= 8 and scale_dtype is None and zp_dtype in (None, torch.int8)
        zp_dtype = torch.int8
    elif qt == "float" and scale_dtype is torch.uint8 and bits in (4, 8) and args.group_size == 32:  # should_generate_mx_scales
        kind = "mxfp4" if bits == 4 else "mxfp8"
        ok = symmetric and zp_dtype in (torch.uint8, torch.int8, _F8)
    elif qt == "float" and bits == 4 and scale_dtype is _F8:
        kind = "nvfp4"
        ok = symmetric and zp_dtype in (None, _F8, torch.uint8, torch.int8)
        zp_dtype = zp_dtype or _F8
    elif qt == "float" and bits == 8 and scale_dtype is None:
        kind = "fp8"
        ok = symmetric and zp_dtype in (None, _F8, torch.uint8, torch.int8)
        zp_dtype = zp_dtype or _F8
    else:
        ok = False
    if not ok:
        raise NotImplementedError(f"dynamic quantization of type {qt}, {bits} bits, scale_dtype {scale_dtype}, zp_dtype {zp_dtype}, "
                                  f"symmetric={symmetric} has no kernel")
    if global_scale is not None and kind != "nvfp4":
        raise NotImplementedError("a global scale is only applied by the NVFP4 kernel")
    return kind, zp_dtype


def plan_dynamic(shape, dtype: torch.dtype, args, global_scale: Optional[torch.Tensor] = None) -> DynamicPlan:
    """Host plan of compute_dynamic_scales_and_zp (helpers.py:140-195) for an activation of `shape` / `dtype`.  No tensor is
    touched: this is the dispatch rule, testable without a GPU."""
    st = enum_value(args.strategy)
    if st not in _STRATEGIES:
        raise ValueError(f"Dynamic quantization is only supported for {_STRATEGIES}")
    if dtype not in _FLOATS:
        raise NotImplementedError(f"activation dtype {dtype} has no dynamic kernel")
    kind, zp_dtype = _kind(args, global_scale)
    shape = tuple(int(d) for d in shape)
    numel = math.prod(shape)
    if numel == 0:
        raise NotImplementedError("dynamic quantization of an empty tensor")
    tensor_form = False
    if st == "token" and len(shape) >= 3:
        # reduce over dims >= 2 with keepdim (helpers.py:165-168)
        segs, seg_len = shape[0] * shape[1], numel // (shape[0] * shape[1])
        scale_shape = shape[:2] + (1,) * (len(shape) - 2)
    elif st in ("token", "tensor"):
        # tensor strategy, and token on a 1-D / 2-D input: the reduce-dims tuple is empty, aminmax of the whole tensor -> (1,)
        segs, seg_len, scale_shape, tensor_form = 1, numel, (1,), True
    else:
        if len(shape) == 0:
            raise NotImplementedError("group quantization of a 0-d tensor")
        gs, cols = int(args.group_size), shape[-1]
        if cols % gs:
            raise NotImplementedError(f"{cols} columns are not a whole number of groups of {gs}: the reference's unflatten raises")
        segs, seg_len, scale_shape = numel // gs, gs, shape[:-1] + (cols // gs,)
    scale_dtype = torch.float32 if (kind == "nvfp4" and global_scale is not None) else dtype
    return DynamicPlan(kind=kind, num_bits=int(args.num_bits), symmetric=bool(args.symmetric), segs=segs, seg_len=seg_len,
                       scale_shape=scale_shape, scale_dtype=scale_dtype, zp_dtype=zp_dtype, tensor_form=tensor_form)


def _run(value, plan: DynamicPlan, global_scale, want_out: bool, want_qparams: bool):
    return codec.dynamic_qdq(value, kind=plan.kind, segs=plan.segs, seg_len=plan.seg_len, num_bits=plan.num_bits, symmetric=plan.symmetric,
                             global_scale=global_scale, scale_shape=plan.scale_shape,
                             scale_dtype=plan.scale_dtype if want_qparams else None, zp_dtype=plan.zp_dtype if want_qparams else None,
                             want_out=want_out)


@torch.no_grad()
def compute_dynamic_scales_and_zp(value: torch.Tensor, args, module: Optional[torch.nn.Module] = None,
                                  global_scale: Optional[torch.Tensor] = None):
    """quantization/utils/helpers.py:140-195: (scale, zero_point) of the activation, in the reference's shapes and dtypes"""
    if value.is_cuda and not value.is_contiguous():
        return codec.attn_dynamic_qparams(value, args, global_scale)  # read through its strides, or copied first: the plan decides
    plan = plan_dynamic(value.shape, value.dtype, args, global_scale)
    _, scale, zp = _run(value, plan, global_scale, want_out=False, want_qparams=True)
    return scale, zp


def dynamic_fake_quantize(value: torch.Tensor, args, global_scale: Optional[torch.Tensor] = None, return_qparams: bool = False):
    """fake_quantize(value, *compute_dynamic_scales_and_zp(value, args, global_scale=gs), args, global_scale=gs) in one pass
    (two for the tensor form); with return_qparams, (out, scale, zero_point)"""
    plan = plan_dynamic(value.shape, value.dtype, args, global_scale)
    out, scale, zp = _run(value, plan, global_scale, want_out=True, want_qparams=return_qparams)
    return (out, scale, zp) if return_qparams else out


def _g_idx_initialised(g_idx) -> bool:
    return g_idx is not None and g_idx.device.type != "meta"


@torch.no_grad()
def forward_quantize(module: torch.nn.Module, value: torch.Tensor, base_name: str, args) -> torch.Tensor:
    """quantization/lifecycle/forward.py:304-335"""
    status = enum_value(getattr(module, "quantization_status", None))
    if base_name == "weight" and _LIFECYCLE.get(status, -1) >= _LIFECYCLE["compressed"]:
        return value
    if value.numel() == 0:
        return value
    if take_prequantized(module, value, base_name):
        return value  # transform.fuse_{input,attention}_quantization: the rotation's pre-hook quantized this very tensor in its own launch
    g_idx = getattr(module, "weight_g_idx", None)
    global_scale = getattr(module, f"{base_name}_global_scale", None)
    if enum_value(getattr(args, "dynamic", False)) in (True, "local"):
        if _g_idx_initialised(g_idx) and enum_value(args.strategy) in ("group", "tensor_group"):
            # the reference permutes the activation by the WEIGHT's g_idx in fake_quantize but observes it unpermuted
            raise NotImplementedError("group activations under an initialised weight_g_idx are left to the reference")
        if base_name in _ATTENTION_STATES:
            # query / key / value states are transposed views: read through their strides (csrc/ct_attn_dyn.hip) where the plan
            # allows it, copied once where it does not — laid out as the reference lays its result out either way
            return codec.attn_dynamic_fake_quantize(value, args, global_scale)
        return dynamic_fake_quantize(value, args, global_scale)
    scale = getattr(module, f"{base_name}_scale")
    zero_point = getattr(module, f"{base_name}_zero_point", None)
    if base_name in _ATTENTION_STATES and global_scale is None and enum_value(args.strategy) in ("tensor", "attn_head"):
        # query / key / value states are transposed views: read through their strides (csrc/ct_attn.hip), not copied first
        return codec.attn_fake_quantize(value, scale, zero_point, num_bits=int(args.num_bits), strategy=enum_value(args.strategy),
                                        qtype=enum_value(getattr(args, "type", "int")))
    return fake_quantize(x=value, scale=scale, zero_point=zero_point, args=args, g_idx=g_idx, global_scale=global_scale)


# ---- the same forward behind an online Hadamard rotation ----------------------------------------------------------------------------
_PREQUANTIZED = "_ct_prequantized_input"  # module attribute: a weak reference to the tensor the fused pre-hook returned
# one weak reference per base name: the module input (transform.fuse_input_quantization) and the query / key / value states of an
# attention module (transform.fuse_attention_quantization)
_PREQUANTIZED_ATTRS = {"input": _PREQUANTIZED, "q": "_ct_prequantized_q", "k": "_ct_prequantized_k", "v": "_ct_prequantized_v"}


def remember_prequantized(module: torch.nn.Module, value: torch.Tensor, base_name: str = "input") -> None:
    """the hand-off of transform.fuse_input_quantization (`value` is the module's input, already rotated AND quantized) and of
    transform.fuse_attention_quantization (base names "q", "k", "v": the attention module's states, already quantized)"""
    module.__dict__[_PREQUANTIZED_ATTRS[base_name]] = weakref.ref(value)


def take_prequantized(module: torch.nn.Module, value: torch.Tensor, base_name: str) -> bool:
    """True when `value` IS (object identity) the tensor the module's fused pre-hook returned for this call under `base_name`:
    forward_quantize then returns it untouched (a QDQ is not idempotent bit for bit).  The reference of that base name is cleared
    either way; any other tensor — another hook replaced it, or nobody pre-quantized — is quantized as always."""
    attr = _PREQUANTIZED_ATTRS.get(base_name)
    if attr is None:
        return False
    ref = module.__dict__.pop(attr, None)
    return ref is not None and ref() is value


class RotatedPlan:
    """what `rotated_fake_quantize` launches for one call: `fused` (one launch of ct_hadamard_dynamic_qdq) in `form`
      "in_wave"    n <= 512, segments of 8 * 2^k <= 512 elements: butterfly, reduction and QDQ inside a wave
      "block"      n = 1024 .. 8192, one workgroup per rotation block, such segments reduced inside the wave
      "block_row"  n = 1024 .. 8192 and the block IS the segment (a token row): min / max finished across the waves
      "head_row"   n <= 512 dividing a longer segment (a token row of head-dim blocks, up to 32768 elements)
    or not fused (`form` None, `reason` says why — a shape the kernels do not fuse, or a form outside MEASURED_FASTER): the two
    existing calls.  `hadamard` / `dynamic` are the parents' plans."""

    __slots__ = ("fused", "form", "reason", "hadamard", "dynamic")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def launches(self) -> int:
        return 1 if self.fused else 1 + self.dynamic.launches()


def _measure_key(form: str, n: int) -> str:
    """what one measurement of tools/rotated_bench.py speaks for: a form, and for the workgroup-block kernel its instantiation"""
    return form if form in ("in_wave", "head_row") else f"{form}_{n}"


ALL_FORMS = frozenset({"in_wave", "head_row"} | {f"{f}_{n}" for f in ("block", "block_row") for n in (1024, 2048, 4096, 8192)})
# The forms the plan dispatches to the fused launch: those `tools/rotated_bench.py` has MEASURED faster than the two launches by
# more than the spread between its runs (profiles/rotated_bench.jsonl).  A form that is not listed — not measured
# yet, or measured and not faster — is declined: rotated_fake_quantize is then the two existing calls.
MEASURED_FASTER = frozenset({"head_row", "block_1024", "block_2048", "block_4096", "block_row_1024", "block_row_2048", "block_row_4096", "block_row_8192"})


def plan_rotated_dynamic(shape, dtype: torch.dtype, size: int, args, global_scale: Optional[torch.Tensor] = None) -> RotatedPlan:
    """Host plan of `dynamic_fake_quantize(hadamard_transform(x, size), args, global_scale)` for an activation of `shape` /
    `dtype`: plan_hadamard (last dimension, float32) and plan_dynamic composed — their ValueErrors and NotImplementedErrors come
    through unchanged — the rule of csrc/ct_rotated.hip for what one launch computes, and MEASURED_FASTER for which of those forms
    are dispatched to it.  No tensor is touched."""
    hp = codec.plan_hadamard(shape, dtype, size, -1, torch.float32)
    dp = plan_dynamic(shape, dtype, args, global_scale)
    n, L = hp.size, dp.seg_len
    units = L // 8
    in_wave = L % 8 == 0 and units <= 64 and units & (units - 1) == 0  # ct_dynamic_qdq's in-wave segments
    form = reason = None
    if dp.launches() == 2:
        reason = f"one segment of {L} elements is the tensor form: its reduction is global"
    elif n <= 512 and in_wave:
        form = "in_wave"
    elif n <= 512:
        if L % 8 or L % n:
            reason = f"segments of {L} elements are not whole 16-byte units of whole blocks of {n}"
        elif L > codec.ROTATED_MAX_ROW:
            reason = f"rows of {L} elements exceed the staged form ({codec.ROTATED_MAX_ROW})"
        else:
            form = "head_row"
    elif n > codec.ROTATED_MAX_BLOCK:
        reason = f"hadamard size {n} was measured slower in one launch than in two (DESIGN 5.12)"
    elif in_wave:
        form = "block"
    elif L == n:
        form = "block_row"
    else:
        reason = f"a segment of {L} elements over workgroup-sized blocks of {n} is not fused"
    if form is not None and _measure_key(form, n) not in MEASURED_FASTER:
        form, reason = None, f"the {_measure_key(form, n)} form is not measured faster than the two launches (MEASURED_FASTER)"
    return RotatedPlan(fused=form is not None, form=form, reason=reason, hadamard=hp, dynamic=dp)


def _run_rotated(value, size, plan: RotatedPlan, global_scale, want_qparams: bool, want_rotated: bool):
    dp = plan.dynamic
    return codec.hadamard_dynamic_qdq(value, size, kind=dp.kind, seg_len=dp.seg_len, num_bits=dp.num_bits, symmetric=dp.symmetric,
                                      global_scale=global_scale, scale_shape=dp.scale_shape,
                                      scale_dtype=dp.scale_dtype if want_qparams else None, zp_dtype=dp.zp_dtype if want_qparams else None,
                                      want_out=True, want_rotated=want_rotated)


def rotated_fake_quantize(value: torch.Tensor, size: int, args, global_scale: Optional[torch.Tensor] = None, *,
                          return_qparams: bool = False, return_rotated: bool = False):
    """dynamic_fake_quantize(hadamard_transform(value, size), args, global_scale, ...): one launch where the plan fuses, the two
    existing calls where it does not — the same bits either way.  Returns out, or (out, scale, zero_point) with return_qparams,
    with the rotated tensor appended under return_rotated."""
    plan = plan_rotated_dynamic(value.shape, value.dtype, size, args, global_scale)
    if plan.fused:
        out, scale, zp, rotated = _run_rotated(value, size, plan, global_scale, return_qparams, return_rotated)
    else:
        rotated = codec.hadamard_transform(value, size)
        out, scale, zp = _run(rotated, plan.dynamic, global_scale, want_out=True, want_qparams=return_qparams)
    res = (out, scale, zp) if return_qparams else (out,)
    if return_rotated:
        res += (rotated,)
    return res if len(res) > 1 else out


@torch.no_grad()
def forward_rotate_quantize(module: torch.nn.Module, value: torch.Tensor, base_name: str, args, size: int) -> torch.Tensor:
    """forward_quantize(module, hadamard_transform(value, size), base_name, args) with the dynamic branch in one launch where
    the plan fuses.  The early returns hand back the rotated value; a static scheme rotates and calls the static fake_quantize."""
    status = enum_value(getattr(module, "quantization_status", None))
    if (base_name == "weight" and _LIFECYCLE.get(status, -1) >= _LIFECYCLE["compressed"]) or value.numel() == 0:
        return codec.hadamard_transform(value, size)
    g_idx = getattr(module, "weight_g_idx", None)
    global_scale = getattr(module, f"{base_name}_global_scale", None)
    if enum_value(getattr(args, "dynamic", False)) in (True, "local"):
        if _g_idx_initialised(g_idx) and enum_value(args.strategy) in ("group", "tensor_group"):
            raise NotImplementedError("group activations under an initialised weight_g_idx are left to the reference")
        return rotated_fake_quantize(value, size, args, global_scale)
    scale = getattr(module, f"{base_name}_scale")
    zero_point = getattr(module, f"{base_name}_zero_point", None)
    return fake_quantize(x=codec.hadamard_transform(value, size), scale=scale, zero_point=zero_point, args=args, g_idx=g_idx, global_scale=global_scale)
