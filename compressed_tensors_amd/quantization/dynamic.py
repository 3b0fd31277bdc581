"""Dynamic activation quantization: `compute_dynamic_scales_and_zp` (quantization/utils/helpers.py:140-195) and
`forward_quantize` (quantization/lifecycle/forward.py:304-335) with the reference's signatures and control flow.

The dynamic branch runs the fused kernel of csrc/ct_dynamic.hip: the activation is read once, the QDQ result written once,
and the scales and zero points stay in registers unless they are asked for.  `plan_dynamic` is the host half: it maps the
reference's arguments onto the kernel's segments and kinds, and raises NotImplementedError for every case the kernel does
not compute exactly as the reference does (`install(patch_forward=True)` hands those to the reference), or the reference's
own ValueError where it raises one.
"""
import math
from typing import Optional

import torch

from .. import codec
from .forward import fake_quantize
from .quant_args import enum_value

__all__ = ["compute_dynamic_scales_and_zp", "forward_quantize", "plan_dynamic", "DynamicPlan"]

_FLOATS = (torch.float32, torch.float16, torch.bfloat16)
_F8 = torch.float8_e4m3fn
_STRATEGIES = ("token", "tensor", "tensor_group", "group")
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
    g_idx = getattr(module, "weight_g_idx", None)
    global_scale = getattr(module, f"{base_name}_global_scale", None)
    if enum_value(getattr(args, "dynamic", False)) in (True, "local"):
        if _g_idx_initialised(g_idx) and enum_value(args.strategy) in ("group", "tensor_group"):
            # the reference permutes the activation by the WEIGHT's g_idx in fake_quantize but observes it unpermuted
            raise NotImplementedError("group activations under an initialised weight_g_idx are left to the reference")
        return dynamic_fake_quantize(value, args, global_scale)
    scale = getattr(module, f"{base_name}_scale")
    zero_point = getattr(module, f"{base_name}_zero_point", None)
    return fake_quantize(x=value, scale=scale, zero_point=zero_point, args=args, g_idx=g_idx, global_scale=global_scale)
