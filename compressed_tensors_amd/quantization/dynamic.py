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
`plan_rotated_k_dynamic` / `random_rotated_fake_quantize` are that pair for the `random-hadamard` rotation of size K * 2^m with
K > 1 (R4 in front of down_proj): one launch of csrc/ct_rotated_k.hip where the plan fuses.  The `random-hadamard` rotation whose
size is a power of two (K = 1: signs and the butterfly) is `rotated_fake_quantize(signs=)` / `plan_rotated_dynamic(signed=True)`:
one launch of csrc/ct_rotated_signed.hip.
"""
import math
import weakref
from typing import Optional

import torch

from .. import codec
from .forward import fake_quantize
from .quant_args import enum_value

__all__ = ["compute_dynamic_scales_and_zp", "forward_quantize", "plan_dynamic", "DynamicPlan", "plan_rotated_dynamic", "RotatedPlan",
           "rotated_fake_quantize", "forward_rotate_quantize", "MEASURED_FASTER", "ALL_FORMS", "remember_prequantized", "take_prequantized",
           "plan_rotated_k_dynamic", "RotatedKPlan", "random_rotated_fake_quantize", "ROTATED_K_ALL_FORMS", "ROTATED_K_MEASURED_FASTER",
           "ROTATED_SIGNED_MEASURED_FASTER"]

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
    """what `rotated_fake_quantize` launches for one call: `fused` (one launch of ct_hadamard_dynamic_qdq, or of
    ct_hadamard_signed_dynamic_qdq for a signed plan) in `form`
      "in_wave"    n <= 512, segments of 8 * 2^k <= 512 elements: butterfly, reduction and QDQ inside a wave
      "block"      n = 1024 .. 8192, one workgroup per rotation block, such segments reduced inside the wave
      "block_row"  n = 1024 .. 8192 and the block IS the segment (a token row): min / max finished across the waves
      "head_row"   n <= 512 dividing a longer segment (a token row of head-dim blocks, up to 32768 elements)
    or not fused (`form` None, `reason` says why — a shape the kernels do not fuse, or a form outside MEASURED_FASTER): the two
    existing calls.  `key` names the measurement that speaks for the shape (`_measure_key`) wherever the kernel computes it,
    dispatched or not; None where it does not.  `hadamard` / `dynamic` are the parents' plans."""

    __slots__ = ("fused", "form", "key", "reason", "hadamard", "dynamic")

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
# The same rule for the signed rotation (csrc/ct_rotated_signed.hip, the keys of ALL_FORMS): filled only from a GPU run of
# `tools/rotated_signed_bench.py` (profiles/rotated_signed_bench.jsonl).  Not measured yet: nothing is dispatched.
ROTATED_SIGNED_MEASURED_FASTER = frozenset()


def plan_rotated_dynamic(shape, dtype: torch.dtype, size: int, args, global_scale: Optional[torch.Tensor] = None, *, signed: bool = False) -> RotatedPlan:
    """Host plan of `dynamic_fake_quantize(hadamard_transform(x, size), args, global_scale)` for an activation of `shape` /
    `dtype`: plan_hadamard (last dimension, float32) and plan_dynamic composed — their ValueErrors and NotImplementedErrors come
    through unchanged — the rule of csrc/ct_rotated.hip for what one launch computes, and MEASURED_FASTER for which of those forms
    are dispatched to it.  `signed`: the plan of `dynamic_fake_quantize(hadamard_k_transform(x, size, None, signs), ...)` instead —
    plan_hadamard_k with k = 1 behind a ValueError for a size that is not a power of two, the rule of csrc/ct_rotated_signed.hip
    (16-bit activations, 8 <= size) and ROTATED_SIGNED_MEASURED_FASTER.  No tensor is touched."""
    if signed:
        if int(size) <= 0 or int(size) & (int(size) - 1):
            raise ValueError(f"hadamard size {size} is not a power of two: the signed butterfly is the k == 1 rotation")
        hp = codec.plan_hadamard_k(shape, dtype, size, 1, -1, torch.float32)
    else:
        hp = codec.plan_hadamard(shape, dtype, size, -1, torch.float32)
    dp = plan_dynamic(shape, dtype, args, global_scale)
    n, L = hp.size, dp.seg_len
    units = L // 8
    in_wave = L % 8 == 0 and units <= 64 and units & (units - 1) == 0  # ct_dynamic_qdq's in-wave segments
    measured = ROTATED_SIGNED_MEASURED_FASTER if signed else MEASURED_FASTER
    form = reason = None
    if signed and dtype is torch.float32:
        reason = "float32 activations take the two launches: the fused sign is a flip of a 16-bit word"
    elif signed and n < 8:
        reason = f"blocks of {n} elements are not whole 16-byte units"
    elif signed and n > codec.ROTATED_MAX_BLOCK:
        reason = f"hadamard size {n} exceeds the fused maximum {codec.ROTATED_MAX_BLOCK}"
    elif dp.launches() == 2:
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
    key = None if form is None else _measure_key(form, n)
    if key is not None and key not in measured:
        form, reason = None, f"the {key} form is not measured faster than the two launches ({'ROTATED_SIGNED_' * signed}MEASURED_FASTER)"
    return RotatedPlan(fused=form is not None, form=form, key=key, reason=reason, hadamard=hp, dynamic=dp)


def _run_rotated(value, size, plan: RotatedPlan, global_scale, want_qparams: bool, want_rotated: bool, signs=None):
    dp = plan.dynamic
    kw = dict(kind=dp.kind, seg_len=dp.seg_len, num_bits=dp.num_bits, symmetric=dp.symmetric, global_scale=global_scale, scale_shape=dp.scale_shape,
              scale_dtype=dp.scale_dtype if want_qparams else None, zp_dtype=dp.zp_dtype if want_qparams else None, want_out=True, want_rotated=want_rotated)
    if signs is not None:
        return codec.hadamard_signed_dynamic_qdq(value, size, signs, **kw)
    return codec.hadamard_dynamic_qdq(value, size, **kw)


def rotated_fake_quantize(value: torch.Tensor, size: int, args, global_scale: Optional[torch.Tensor] = None, *,
                          return_qparams: bool = False, return_rotated: bool = False, signs: Optional[torch.Tensor] = None,
                          fused: Optional[bool] = None):
    """dynamic_fake_quantize(hadamard_transform(value, size), args, global_scale, ...): one launch where the plan fuses, the two
    existing calls where it does not — the same bits either way.  `signs` (int8 (size,) of +-1 on value's device): the rotation
    is hadamard_k_transform(value, size, None, signs), the `random-hadamard` rotation whose size is a power of two, and the plan
    the signed one.  `fused=None` follows the plan; `fused=True` asks for the one launch wherever the kernel computes the shape,
    measured faster or not; `fused=False` is the composition.  Returns out, or (out, scale, zero_point) with return_qparams, with
    the rotated tensor appended under return_rotated."""
    plan = plan_rotated_dynamic(value.shape, value.dtype, size, args, global_scale, signed=signs is not None)
    if plan.fused if fused is None else (bool(fused) and plan.key is not None):
        out, scale, zp, rotated = _run_rotated(value, size, plan, global_scale, return_qparams, return_rotated, signs)
    else:
        rotated = codec.hadamard_transform(value, size) if signs is None else codec.hadamard_k_transform(value, size, None, signs)
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


# ---- the same forward behind a random-hadamard rotation of size K * 2^m, K > 1 (csrc/ct_rotated_k.hip) ------------------------------
class RotatedKPlan:
    """what `random_rotated_fake_quantize` launches for one call: `fused` (one launch of ct_hadamard_k_dynamic_qdq) in `form`
      "mfma_group"  segments of 8 * 2^j <= 512 elements that divide the rotation block: reduced inside a wave on the block in LDS
      "mfma_row"    the rotation block IS the segment (a token row, M >= 32): min / max finished across the waves
    or not fused (`form` None, `reason` says why): the two existing calls.  `key` names the measurement that speaks for the shape
    (form and accumulator tiles, e.g. "mfma_row_tt2") wherever the kernel computes it, dispatched or not; None where it does not.
    `hadamard` / `dynamic` are the parents' plans."""

    __slots__ = ("fused", "form", "key", "reason", "hadamard", "dynamic")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def launches(self) -> int:
        return 1 if self.fused else (2 if self.hadamard.form == "valu" else 1) + self.dynamic.launches()


ROTATED_K_ALL_FORMS = frozenset(f"{f}_tt{tt}" for f in ("mfma_group", "mfma_row") for tt in (1, 2, 4))
# The keys the plan dispatches to the one launch: those `tools/rotated_k_bench.py` has MEASURED faster than the two launches by more
# than the spread between its runs (profiles/rotated_k_bench.jsonl).  A key that is not listed — not measured, or
# measured and not faster — is declined: random_rotated_fake_quantize is then the two existing calls.
ROTATED_K_MEASURED_FASTER = frozenset({"mfma_row_tt4"})  # 0.95-0.97 of the two launches; every other key measured 1.13-1.48 x SLOWER


def plan_rotated_k_dynamic(shape, dtype: torch.dtype, size: int, k: int, args, global_scale: Optional[torch.Tensor] = None) -> RotatedKPlan:
    """Host plan of `dynamic_fake_quantize(hadamard_k_transform(x, size, had_k, signs), args, global_scale)` for an activation of
    `shape` / `dtype` and a k x k mix: plan_hadamard_k (last dimension, float32, plain form) and plan_dynamic composed — their
    ValueErrors and NotImplementedErrors come through unchanged — the rule of csrc/ct_rotated_k.hip for what one launch computes,
    and ROTATED_K_MEASURED_FASTER for which of those keys are dispatched to it.  No tensor is touched."""
    hp = codec.plan_hadamard_k(shape, dtype, size, k, -1, torch.float32)
    dp = plan_dynamic(shape, dtype, args, global_scale)
    n, m, L = hp.size, hp.m, dp.seg_len
    units = L // 8
    in_wave = L % 8 == 0 and units <= 64 and units & (units - 1) == 0  # ct_dynamic_qdq's in-wave segments
    form = reason = None
    if hp.k == 1:
        reason = "k == 1 (signs and the butterfly) has no fused launch"
    elif dtype is torch.float32:
        reason = "float32 activations take the vector form of the mix"
    elif hp.form != "mfma":
        reason = f"runs of {m} elements take the vector form of the mix"
    elif dp.launches() == 2:
        reason = f"one segment of {L} elements is the tensor form: its reduction is global"
    elif in_wave and n % L == 0:
        form = "mfma_group"
    elif L == n:
        if m >= 32:
            form = "mfma_row"
        else:
            reason = f"a token row of {n} elements shares its workgroup with {32 // m - 1} more blocks"
    elif L % n == 0:
        reason = f"a token row of {L} elements is {L // n} rotation blocks of {n}"
    else:
        reason = f"a segment of {L} elements over rotation blocks of {n} is not fused"
    key = None if form is None else f"{form}_tt{max(m, 32) // 32}"
    if key is not None and key not in ROTATED_K_MEASURED_FASTER:
        form, reason = None, f"the {key} form is not measured faster than the two launches (ROTATED_K_MEASURED_FASTER)"
    return RotatedKPlan(fused=form is not None, form=form, key=key, reason=reason, hadamard=hp, dynamic=dp)


def random_rotated_fake_quantize(value: torch.Tensor, size: int, had_k: Optional[torch.Tensor], signs: Optional[torch.Tensor], args,
                                 global_scale: Optional[torch.Tensor] = None, *, return_qparams: bool = False, return_rotated: bool = False,
                                 fused: Optional[bool] = None):
    """dynamic_fake_quantize(hadamard_k_transform(value, size, had_k, signs), args, global_scale, ...).  `fused=None` follows the
    plan: one launch where it fuses, the two existing calls where it does not; `fused=True` asks for the one launch wherever the
    kernel computes the shape, measured faster or not; `fused=False` is the composition.  The same bits in all three.  Returns out,
    or (out, scale, zero_point) with return_qparams, with the rotated tensor appended under return_rotated."""
    k = 1 if had_k is None else int(had_k.shape[0])
    plan = plan_rotated_k_dynamic(value.shape, value.dtype, size, k, args, global_scale)
    dp = plan.dynamic
    if plan.fused if fused is None else (bool(fused) and plan.key is not None):
        out, scale, zp, rotated = codec.hadamard_k_dynamic_qdq(
            value, size, had_k, signs, kind=dp.kind, seg_len=dp.seg_len, num_bits=dp.num_bits, symmetric=dp.symmetric, global_scale=global_scale,
            scale_shape=dp.scale_shape, scale_dtype=dp.scale_dtype if return_qparams else None, zp_dtype=dp.zp_dtype if return_qparams else None,
            want_out=True, want_rotated=return_rotated)
    else:
        rotated = codec.hadamard_k_transform(value, size, had_k, signs)
        out, scale, zp = _run(rotated, dp, global_scale, want_out=True, want_qparams=return_qparams)
    res = (out, scale, zp) if return_qparams else (out,)
    if return_rotated:
        res += (rotated,)
    return res if len(res) > 1 else out
