"""Tensor-level entry points of the hot path: thin wrappers that validate arguments, allocate
outputs with torch and launch the HIP kernels of libct_hip.so on the caller's current stream.

Every function mirrors a reference function (cited per function; paths relative to
/root/reference/src/compressed_tensors/).  There is no eager/CPU implementation here: CPU
tensors are staged through the GPU (H2D, kernel, D2H) so the arithmetic is always the HIP
path; without a GPU the calls raise.
"""
import array
import functools
import math
import operator
from types import SimpleNamespace
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from ._lib import DT, call, ptr, stream_of, stream_on

__all__ = [
    "pack_to_int32",
    "unpack_from_int32",
    "quantize_tensor",
    "dequantize_tensor",
    "fake_quantize_tensor",
    "quantize_and_pack",
    "unpack_and_dequantize",
    "quantize_and_pack_many",
    "unpack_and_dequantize_many",
    "minmax_qparams",
    "minmax_qparams_float",
    "dynamic_qdq",
    "hadamard_dynamic_qdq",
    "generate_gparam",
    "HadamardPlan",
    "plan_hadamard",
    "hadamard_transform",
    "HadamardKPlan",
    "plan_hadamard_k",
    "hadamard_k_transform",
    "HadamardPermTables",
    "hadamard_perm_tables",
    "HadamardPermPlan",
    "plan_hadamard_perm",
    "HADAMARD_PERM_MEASURED_FASTER",
    "HADAMARD_PERM_MAX_SIZE",
    "rtn_quantize_and_pack",
    "rtn_mxfp4_quantize_and_pack",
    "rtn_quantize_channel8",
    "rtn_quantize_channel8_many",
    "rtn_channel8_form",
    "rtn_channel8_table_item",
    "launch_rtn_channel8_words",
    "RTN_CHANNEL8_MAX_COLS",
    "rtn_nvfp4_quantize_and_pack",
    "rtn_quantize_and_pack_many",
    "rtn_mxfp4_quantize_and_pack_many",
    "rtn_nvfp4_quantize_and_pack_many",
    "rtn_quantize_block8",
    "rtn_quantize_block8_many",
    "launch_rtn_w4_words",
    "launch_rtn_mxfp4_words",
    "launch_rtn_nvfp4_words",
    "pack_bitmasks",
    "unpack_bitmasks",
    "W4Batch",
    "launch_w4_words",
    "launch_zp4_words",
    "w4_batch_eligible",
    "q8_batch_group",
    "zp4_batch",
    "cast_to_fp4",
    "pack_fp4_to_uint8",
    "unpack_fp4_from_uint8",
    "compress_mx_scale",
    "decompress_mx_scale",
    "fp4_quantize_and_pack",
    "fp4_quantize_and_pack_stored",
    "fp4_unpack_and_dequantize",
    "marlin24_quant_compress",
    "marlin24_compress_w4",
    "marlin24_compress_w4_full",
    "selftest_m24_div",
    "bitmask_compress",
    "bitmask_decompress",
    "sparse24_mask",
    "sparse24_bitmask_compress",
    "sparse24_bitmask_decompress",
    "cutlass24_from_dense",
    "cutlass24_to_dense",
    "marlin24_pack_weights",
    "marlin24_pack_scales",
    "selftest_bf16_div",
    "selftest_f16_div",
    "selftest_fp4_div",
    "QuantLayout",
    "AttnPlan",
    "plan_attn_qdq",
    "attn_fake_quantize",
    "attn_quantize",
    "attn_dequantize",
    "attn_fake_quantize_pair",
    "AttnRotPlan",
    "plan_attn_rot_qdq",
    "attn_rotated_fake_quantize",
    "attn_rotated_quantize",
    "attn_rotated_fake_quantize_pair",
    "ATTN_ROTATED_MEASURED_FASTER",
    "ATTN_ROTATED_MAX_SIZE",
    "AttnDynPlan",
    "plan_attn_dynamic",
    "attn_dynamic_fake_quantize",
    "attn_dynamic_fake_quantize_pair",
    "attn_dynamic_qparams",
    "ATTN_DYNAMIC_MEASURED_FASTER",
    "item_row",
    "rtn_w4_table_item",
    "rtn_mxfp4_table_item",
    "rtn_nvfp4_table_item",
    "rtn_block8_table_item",
    "rtn_block8_group",
    "rtn_quantize_group8",
    "rtn_quantize_group8_many",
    "rtn_group8_table_item",
    "rtn_group8_group",
    "launch_rtn_group8_words",
    "rtn_nvfp4_takes",
    "rtn_nvfp4_keys",
    "attn_observe_global_scale",
    "RTN_PACKW_BITS",
    "rtn_wb_table_item",
    "launch_rtn_wb_words",
    "rtn_wb_outputs",
    "rtn_block8_outputs",
    "rtn_group8_outputs",
    "rtn_channel8_outputs",
    "rtn_w4_launch",
    "rtn_wb_launch",
    "rtn_block8_launch",
    "rtn_group8_launch",
    "rtn_channel8_launch",
    "rtn_mxfp4_outputs",
    "rtn_mxfp4_launch",
    "fp8block_to_mxfp4",
    "fp8block_to_mxfp8",
    "fp8block_to_nvfp4",
    "nvfp4_to_mxfp4",
]

_FLOATS = (torch.float32, torch.float16, torch.bfloat16)


# --------------------------------------------------------------------------- staging helpers
def _dev(t: Optional[torch.Tensor], device: torch.device) -> Optional[torch.Tensor]:
    """contiguous, 16-byte aligned tensor on `device` (views into other storage are cloned)"""
    if t is None:
        return None
    if t.device != device:
        t = t.to(device)
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


def _compute_device(*tensors) -> torch.device:
    for t in tensors:
        if t is not None and t.is_cuda:
            return t.device
    return _lib.require_device()


def _home(out: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """results live on the device of the input they were derived from (reference behaviour)"""
    return out if out.device == like.device else out.to(like.device)


def _strategy_name(strategy) -> Optional[str]:
    if strategy is None:
        return None
    return str(getattr(strategy, "value", strategy)).lower()


# --------------------------------------------------------------------------- pack / unpack
def pack_to_int32(value: torch.Tensor, num_bits: int, packed_dim: int = 1) -> torch.Tensor:
    """compressors/pack_quantized/helpers.py:20-101 (same arguments, same errors)."""
    if value.dtype is not torch.int8:
        raise ValueError("Tensor must be quantized to torch.int8 before packing")
    if not 1 <= num_bits <= 8:
        raise ValueError(f"Packing is only supported for num_bits in [1, 8], got {num_bits}")
    if value.ndim > 2 and packed_dim == 0:
        return torch.stack([pack_to_int32(value[i], num_bits, packed_dim) for i in range(value.shape[0])])
    if value.ndim < 2:
        raise ValueError(f"pack_to_int32 expects a tensor with at least 2 dims, got {value.ndim}")
    dev = _compute_device(value)
    v = _dev(value, dev)
    if packed_dim == 0:
        rows, cols = v.shape
        out = torch.empty((math.ceil(rows * num_bits / 32), cols), dtype=torch.int32, device=dev)
        call("ct_pack_int32_dim0", ptr(v), rows, cols, num_bits, ptr(out), stream_of(v))
        return _home(out, value)
    # packing is row-wise, so N-D (MoE) tensors are a stack of rows (helpers.py:45-51)
    cols = v.shape[-1]
    rows = v.numel() // cols if cols else math.prod(v.shape[:-1])
    packed_cols = math.ceil(cols * num_bits / 32)
    out = torch.empty((*v.shape[:-1], packed_cols), dtype=torch.int32, device=dev)
    call("ct_pack_int32", ptr(v), rows, cols, num_bits, ptr(out), packed_cols, stream_of(v))
    return _home(out, value)


def unpack_from_int32(value: torch.Tensor, num_bits: int, shape: Sequence[int], packed_dim: int = 1) -> torch.Tensor:
    """compressors/pack_quantized/helpers.py:104-180 (same arguments, same errors)."""
    if value.dtype is not torch.int32:
        raise ValueError(f"Expected {torch.int32} but got {value.dtype}, Aborting unpack.")
    if not 1 <= num_bits <= 8:
        raise ValueError(f"Unpacking is only supported for num_bits in [1, 8], got {num_bits}")
    shape = tuple(int(s) for s in shape)
    if value.ndim > 2 and packed_dim == 0:
        return torch.stack(
            [unpack_from_int32(value[i], num_bits, shape[1:], packed_dim) for i in range(value.shape[0])]
        )
    dev = _compute_device(value)
    v = _dev(value, dev)
    if packed_dim == 0:
        words, cols = v.shape
        rows = shape[0]
        out = torch.empty((rows, cols), dtype=torch.int8, device=dev)
        call("ct_unpack_int32_dim0", ptr(v), words, cols, rows, num_bits, ptr(out), stream_of(v))
        return _home(out, value)
    words = v.shape[-1]
    rows = math.prod(v.shape[:-1])
    cols = shape[-1]
    out = torch.empty((*v.shape[:-1], cols), dtype=torch.int8, device=dev)
    call("ct_unpack_int32", ptr(v), rows, words, words, cols, num_bits, ptr(out), stream_of(v))
    return _home(out, value)


# --------------------------------------------------------------------------- quantization layout
def _col_group_of(g_idx: torch.Tensor, group_size: int) -> torch.Tensor:
    """activation ordering (forward_helpers.py:147-175): column c uses the group of its position in the g_idx-sorted order; a g_idx
    that still holds a -1 (not initialised) means plain column order.  The reference decides that with `-1 in g_idx`, a host read
    per call; here the choice is a device-side select — no synchronisation.  Nothing is cached: `param.data.copy_(...)` rewrites a
    g_idx in place without moving its pointer or bumping its version counter, so no key derived from the tensor is safe
    (ADVICE r03), and the two argsorts of a (cols,) vector are noise next to the weight pass."""
    flat = g_idx.detach().reshape(-1)
    if flat.is_cuda and flat.dtype is torch.int32 and flat.is_contiguous() and flat.numel() and int(group_size) > 0:
        # two small launches instead of two argsorts and five more tensor ops per call (ct_gidx_col_group: a balanced g_idx needs no sort at all) — a
        # module with activation ordering spent 86 us of host time per direction, most of it here
        out = torch.empty(flat.numel() + 1, dtype=torch.int32, device=flat.device)  # the last word: the kernel pair's mode scratch
        call("ct_gidx_col_group", ptr(flat), flat.numel(), int(group_size), ptr(out), out.data_ptr() + 4 * flat.numel(), stream_of(flat))
        return out[:-1]
    inv = torch.argsort(torch.argsort(flat))
    plain = torch.arange(flat.numel(), device=flat.device)
    return (torch.where((flat == -1).any(), plain, inv) // int(group_size)).to(torch.int32)


class QuantLayout:
    """How scale / zero-point entries map onto the elements of x:
    idx(r, c) = (r // rdiv) * scale_cols + (col_group[c] if col_group is not None else c // cdiv)
    (see include/ct_hip.h).  Built from the reference's strategy vocabulary."""

    __slots__ = ("rows", "cols", "rdiv", "cdiv", "scale_cols", "col_group", "is_group", "scale_zero_dim", "heads")

    def __init__(self, x_shape, scale: torch.Tensor, strategy, group_size=None, block_structure=None,
                 g_idx: Optional[torch.Tensor] = None):
        st = _strategy_name(strategy)
        cols = int(x_shape[-1]) if len(x_shape) else 1
        rows = math.prod(x_shape[:-1]) if len(x_shape) > 1 else 1
        self.rows, self.cols = rows, cols
        self.col_group = None
        self.heads = None
        self.is_group = st in ("group", "tensor_group")
        self.scale_zero_dim = scale.ndim == 0 and not self.is_group
        if self.is_group:
            if group_size is None:
                raise ValueError("group strategy requires group_size")
            group_size = int(group_size)
            # forward_helpers.py:141-145
            if cols >= group_size and cols % group_size != 0:
                raise ValueError(
                    "tensor column shape must be divisble "
                    f"by the given group_size {group_size} but got {cols}"
                )
            srows = math.prod(scale.shape[:-1]) if scale.ndim >= 2 else scale.numel()
            scols = scale.shape[-1] if scale.ndim >= 2 else 1
            if srows not in (1, rows):
                raise ValueError(f"scale of shape {tuple(scale.shape)} does not match {rows} rows")
            self.rdiv = 1 if srows == rows else max(rows, 1)
            self.cdiv = group_size
            self.scale_cols = scols
            if scols * group_size < cols and scols != math.ceil(cols / group_size):
                raise ValueError(f"scale of shape {tuple(scale.shape)} does not cover {cols} columns with groups of {group_size}")
            if g_idx is not None and g_idx.device.type != "meta":
                self.col_group = _col_group_of(g_idx, group_size)
        elif st == "block":
            if len(x_shape) != 2:
                raise NotImplementedError("block quantization expects a 2-D weight")
            bh, bw = (int(b) for b in block_structure)
            self.rdiv, self.cdiv, self.scale_cols = bh, bw, int(scale.shape[-1])
            if scale.shape[0] != math.ceil(rows / bh) or scale.shape[1] != math.ceil(cols / bw):
                raise ValueError(f"scale of shape {tuple(scale.shape)} does not match blocks {bh}x{bw} of {tuple(x_shape)}")
        elif st in ("channel", "token"):
            if scale.numel() != rows:
                if scale.numel() == 1:
                    self.rdiv, self.cdiv, self.scale_cols = max(rows, 1), max(cols, 1), 1
                else:
                    raise ValueError(f"scale of shape {tuple(scale.shape)} does not match {rows} channels")
            else:
                self.rdiv, self.cdiv, self.scale_cols = 1, max(cols, 1), 1
        elif st in ("tensor", None):
            if scale.numel() != 1:
                raise ValueError(f"per-tensor quantization expects a single scale, got shape {tuple(scale.shape)}")
            self.rdiv, self.cdiv, self.scale_cols = max(rows, 1), max(cols, 1), 1
        elif st == "attn_head":
            # (..., H, S, D) against a scale of (H, 1, 1): idx = (row // S) % H.  quantize_tensor / fake_quantize_tensor /
            # dequantize_tensor hand this strategy to the strided entry (plan_attn_qdq, attn_*); rdiv / cdiv express it for one batch
            if len(x_shape) < 3:
                raise ValueError("Attention quant requires at least 3 observed dimensions")  # lifecycle/initialize.py:242-247
            self.heads = int(x_shape[-3])
            if scale.numel() == 1:
                self.rdiv, self.cdiv, self.scale_cols = max(rows, 1), max(cols, 1), 1
            elif scale.numel() != self.heads:
                raise ValueError(f"scale of shape {tuple(scale.shape)} does not match {self.heads} heads")
            elif rows == self.heads * int(x_shape[-2]):
                self.rdiv, self.cdiv, self.scale_cols = max(int(x_shape[-2]), 1), max(cols, 1), 1
            else:
                self.rdiv = self.cdiv = self.scale_cols = None  # several batches: not a (row // rdiv) layout
        else:
            raise NotImplementedError(f"quantization strategy {st!r} is not supported by the MI355X path")

    def args(self, dev):
        if self.rdiv is None:
            raise NotImplementedError("attn_head over several batches has no rdiv / cdiv layout: use codec.attn_fake_quantize / attn_quantize / attn_dequantize")
        cg = _dev(self.col_group, dev) if self.col_group is not None else None
        return (self.rows, self.cols, self.rdiv, self.cdiv, self.scale_cols, ptr(cg)), cg


def infer_dequant_layout(x_shape, scale: torch.Tensor):
    """strategy inferred from the scale shape when no args are given (lifecycle/forward.py:99-130)"""
    if scale.ndim in (0, 1):
        return "tensor", None, None
    if scale.ndim == 2:
        if scale.shape[1] == 1:
            return "channel", None, None
        if scale.shape[0] == 1 or scale.shape[0] == x_shape[0]:
            return "group", int(x_shape[1] / scale.shape[1]), None
        rows, cols = x_shape[-2], x_shape[-1]
        return "block", None, [rows // scale.shape[0], cols // scale.shape[1]]
    raise ValueError(
        f"Could not infer a quantization strategy from scale with {scale.ndim} "
        "dimmensions. Expected 0 or 2 dimmensions."
    )


def _result_dtype(x: torch.Tensor, scale: torch.Tensor, zero_dim: bool) -> torch.dtype:
    """torch result dtype of `x / scale` as the reference evaluates it (a 0-dim scale does not
    promote a dimensioned x; group strategies always unsqueeze the scale first)"""
    probe = scale if zero_dim else scale.reshape(-1)[:1]
    return torch.result_type(x, probe)


def _check_float(x, what):
    if x.dtype not in _FLOATS:
        raise NotImplementedError(f"{what} dtype {x.dtype} is not supported by the MI355X path")


def _zp_arg(zp, dev):
    if zp is None:
        return None, -1
    if zp.dtype not in DT or zp.dtype in (torch.bool,):
        zp = zp.to(torch.int32)
    z = _dev(zp, dev)
    return z, DT[z.dtype]


def _check_sz(layout: QuantLayout, scale, zp):
    need = (max(layout.rows, 1) + layout.rdiv - 1) // layout.rdiv * layout.scale_cols if layout.rows else 0
    if layout.rows and scale.numel() < need:
        raise ValueError(f"scale has {scale.numel()} entries, layout needs {need}")
    if zp is not None and zp.numel() != scale.numel():
        raise ValueError(f"zero_point shape {tuple(zp.shape)} does not match scale shape {tuple(scale.shape)}")


_F8 = torch.float8_e4m3fn


def _check_qtype(qtype, num_bits):
    qtype = getattr(qtype, "value", qtype)
    if qtype not in ("int", "float"):
        raise ValueError(f"Invalid quantization type {qtype}")
    if qtype == "float" and int(num_bits) not in (4, 8):
        raise NotImplementedError("Only num_bits in (4, 8) are supported")  # quant_args.py:479
    return qtype


def _gs_arg(global_scale, dev):
    if global_scale is None:
        return None
    return _dev(global_scale, dev).to(torch.float32).reshape(-1)[:1].contiguous()


def quantize_tensor(x, scale, zero_point, *, num_bits, strategy, group_size=None, block_structure=None,
                    dtype=None, g_idx=None, qtype="int", global_scale=None) -> torch.Tensor:
    """quantization/lifecycle/forward.py:36-73: returns `dtype` (int8/int32, float8_e4m3fn for FLOAT args, or a float
    type) or, when dtype is None, x.dtype for group strategies and the promoted type otherwise.  qtype "float": 8 bits
    clamp to +-448 and round to float8_e4m3fn, 4 bits clamp to +-6 and cast_to_fp4 (values stay in a float dtype), instead
    of rint.  global_scale (FLOAT 4-bit tensor_group): the effective scale is scale / global_scale in float32."""
    if _strategy_name(strategy) == "attn_head":
        return attn_quantize(x, scale, zero_point, num_bits=num_bits, strategy=strategy, qtype=qtype, dtype=dtype, global_scale=global_scale)
    qtype = _check_qtype(qtype, num_bits)
    if global_scale is not None and not (qtype == "float" and int(num_bits) == 4):
        raise NotImplementedError("global_scale is implemented for FLOAT 4-bit quantization")
    _check_float(x, "x")
    _check_float(scale, "scale")
    layout = QuantLayout(x.shape, scale, strategy, group_size, block_structure, g_idx)
    _check_sz(layout, scale, zero_point)
    T = _result_dtype(x, scale, layout.scale_zero_dim) if global_scale is None else torch.float32
    out_dtype = dtype if dtype is not None else (x.dtype if layout.is_group else T)
    fp4 = qtype == "float" and int(num_bits) == 4
    allowed = _FLOATS if fp4 else (_F8, *_FLOATS) if qtype == "float" else (torch.int8, torch.int32, *_FLOATS)
    if out_dtype not in allowed:
        raise NotImplementedError(f"quantize ({qtype}, {num_bits} bits) to {out_dtype} is not supported by the MI355X path")
    dev = _compute_device(x, scale)
    xd, sd = _dev(x, dev), _dev(scale, dev)
    zd, zdt = _zp_arg(zero_point, dev)
    out = torch.empty(x.shape, dtype=out_dtype, device=dev)
    largs, _keep = layout.args(dev)
    if fp4:
        gs = _gs_arg(global_scale, dev)
        call("ct_quantize_fp4", ptr(xd), DT[xd.dtype], ptr(sd), DT[sd.dtype], ptr(zd), zdt, *largs, ptr(gs), DT[T],
             ptr(out), DT[out_dtype], stream_of(xd))
    elif qtype == "float":
        call("ct_quantize_fp8", ptr(xd), DT[xd.dtype], ptr(sd), DT[sd.dtype], ptr(zd), zdt, *largs, DT[T],
             ptr(out), DT[out_dtype], stream_of(xd))
    else:
        call("ct_quantize", ptr(xd), DT[xd.dtype], ptr(sd), DT[sd.dtype], ptr(zd), zdt, *largs, int(num_bits), DT[T],
             ptr(out), DT[out_dtype], stream_of(xd))
    return _home(out, x)


def fake_quantize_tensor(x, scale, zero_point, *, num_bits, strategy, group_size=None, block_structure=None,
                         g_idx=None, qtype="int", global_scale=None) -> torch.Tensor:
    """quantization/lifecycle/forward.py:148-181 (forward_helpers.py:180-215); qtype / global_scale as in quantize_tensor."""
    if _strategy_name(strategy) == "attn_head":
        return attn_fake_quantize(x, scale, zero_point, num_bits=num_bits, strategy=strategy, qtype=qtype, global_scale=global_scale)
    qtype = _check_qtype(qtype, num_bits)
    if global_scale is not None and not (qtype == "float" and int(num_bits) == 4):
        raise NotImplementedError("global_scale is implemented for FLOAT 4-bit quantization")
    _check_float(x, "x")
    _check_float(scale, "scale")
    layout = QuantLayout(x.shape, scale, strategy, group_size, block_structure, g_idx)
    _check_sz(layout, scale, zero_point)
    T = _result_dtype(x, scale, layout.scale_zero_dim) if global_scale is None else torch.float32
    out_dtype = x.dtype if layout.is_group else (scale.dtype if global_scale is None else torch.float32)
    dev = _compute_device(x, scale)
    xd, sd = _dev(x, dev), _dev(scale, dev)
    zd, zdt = _zp_arg(zero_point, dev)
    out = torch.empty(x.shape, dtype=out_dtype, device=dev)
    largs, _keep = layout.args(dev)
    if qtype == "float" and int(num_bits) == 4:
        gs = _gs_arg(global_scale, dev)
        call("ct_fake_quantize_fp4", ptr(xd), DT[xd.dtype], ptr(sd), DT[sd.dtype], ptr(zd), zdt, *largs, ptr(gs), DT[T],
             ptr(out), DT[out_dtype], stream_of(xd))
    elif qtype == "float":
        call("ct_fake_quantize_fp8", ptr(xd), DT[xd.dtype], ptr(sd), DT[sd.dtype], ptr(zd), zdt, *largs, DT[T],
             ptr(out), DT[out_dtype], stream_of(xd))
    else:
        call("ct_fake_quantize", ptr(xd), DT[xd.dtype], ptr(sd), DT[sd.dtype], ptr(zd), zdt, *largs, int(num_bits), DT[T],
             ptr(out), DT[out_dtype], stream_of(xd))
    return _home(out, x)


def dequantize_tensor(x_q, scale, zero_point=None, *, strategy=None, group_size=None, block_structure=None,
                      dtype=None, g_idx=None, global_scale=None) -> torch.Tensor:
    """quantization/lifecycle/forward.py:76-145 (forward_helpers.py:549-572)."""
    _check_float(scale, "scale")
    if x_q.dtype not in (torch.int8, torch.int32, _F8, *_FLOATS):
        raise NotImplementedError(f"dequantize from {x_q.dtype} is not supported by the MI355X path")
    if strategy is None:
        strategy, group_size, block_structure = infer_dequant_layout(x_q.shape, scale)
    if _strategy_name(strategy) == "attn_head":
        return attn_dequantize(x_q, scale, zero_point, strategy=strategy, dtype=dtype, global_scale=global_scale)
    layout = QuantLayout(x_q.shape, scale, strategy, group_size, block_structure, g_idx)
    _check_sz(layout, scale, zero_point)
    out_dtype = dtype if dtype is not None else scale.dtype
    if out_dtype not in _FLOATS:
        raise NotImplementedError(f"dequantize to {out_dtype} is not supported by the MI355X path")
    dev = _compute_device(x_q, scale)
    qd, sd = _dev(x_q, dev), _dev(scale, dev)
    zd, zdt = _zp_arg(zero_point, dev)
    out = torch.empty(x_q.shape, dtype=out_dtype, device=dev)
    largs, _keep = layout.args(dev)
    if global_scale is not None:
        gs = _gs_arg(global_scale, dev)
        call("ct_dequantize_gs", ptr(qd), DT[qd.dtype], ptr(sd), DT[sd.dtype], ptr(zd), zdt, *largs, ptr(gs), ptr(out), DT[out_dtype],
             stream_of(qd))
    else:
        call("ct_dequantize", ptr(qd), DT[qd.dtype], ptr(sd), DT[sd.dtype], ptr(zd), zdt, *largs, ptr(out), DT[out_dtype],
             stream_of(qd))
    return _home(out, x_q)


# --------------------------------------------------------------------------- attention: q / k / v states, strided
class AttnPlan(NamedTuple):
    """what the attn_* functions do with one tensor: `in_place` (ct_attn_qdq reads it through its strides; False: `.contiguous()`
    first, `reason` says why), the (B, H, S, D) view the kernel gets with the b / h / s element strides it reads, `per_head`
    (H scale entries, index h; False: one entry), and `vector` (rows of whole 8-element units, units aligned on both sides —
    16-byte units of a 16-bit dtype; False: the element form of the same entry)"""
    in_place: bool
    vector: bool
    B: int
    H: int
    S: int
    D: int
    strides: tuple
    per_head: bool
    reason: Optional[str]


def _attn_is_dense(shape, strides) -> bool:
    dims = sorted((st, sz) for sz, st in zip(shape, strides) if sz > 1)
    run = 1
    for st, sz in dims:
        if st != run:
            return False
        run *= sz
    return True


def _attn_overlaps(shape, strides) -> bool:
    """conservative: dimensions sorted by stride must each step past everything the smaller ones span (expanded dimensions, stride
    0, are not storage)"""
    span = 0
    for st, sz in sorted((st, sz) for sz, st in zip(shape, strides) if sz > 1 and st != 0):
        if st <= span:
            return True
        span += (sz - 1) * st
    return False


def _attn_fold(shape, strides):
    """(B, H, S, D), (b, h, s strides) of a tensor with a unit last stride, or None when its leading dimensions do not fold into B"""
    shape, strides = tuple(shape), tuple(strides)
    if len(shape) < 4:
        pad = 4 - len(shape)
        return (1,) * pad + shape, ((0,) * pad + strides)[:3]
    lead_shape, lead_strides = shape[:-3], strides[:-3]
    B, sb = 1, 0
    for sz, st in zip(reversed(lead_shape), reversed(lead_strides)):
        if sz == 1:
            continue
        if B == 1:
            B, sb = sz, st
        elif st == sb * B:
            B *= sz
        else:
            return None
    return (B,) + shape[-3:], (sb,) + strides[-3:-1]


def _attn_unit_aligned(offset_bytes, sizes, strides, itemsize, D) -> bool:
    a = min(16, 8 * itemsize)
    return D % 8 == 0 and offset_bytes % a == 0 and all((st * itemsize) % a == 0 for sz, st in zip(sizes, strides) if sz > 1)


@functools.lru_cache(maxsize=1024)
def _dense_strides(shape) -> tuple:
    return tuple(torch.empty(tuple(shape), device="meta").stride())


def _attn_view(shape, strides, writes: bool):
    """The rule every strided attention launch plans by: (in_place, (B, H, S, D), the b / h / s strides, reason) of a tensor of at
    least one dimension.  Read in place through its strides unless a stride is negative, the last dimension is not contiguous, the
    leading dimensions do not fold into one batch (_attn_fold) or — `writes`: the launch lays out an output like the input —
    the tensor overlaps itself in storage; otherwise `reason` says why, and the view is the dense copy's."""
    reason = None
    if any(s < 0 for s in strides):
        reason = "negative strides"
    elif shape[-1] > 1 and strides[-1] != 1:
        reason = f"the last dimension has stride {strides[-1]}"
    elif writes and _attn_overlaps(shape, strides):
        reason = "the tensor overlaps itself in storage"
    folded = None if reason else _attn_fold(shape, tuple(strides[:-1]) + (1,))
    if reason is None and folded is None:
        reason = "the leading dimensions do not fold into one batch dimension"
    if reason is not None:
        folded = _attn_fold(shape, _dense_strides(shape))
    return reason is None, folded[0], folded[1], reason


def _attn_refusals(global_scale, qtype, num_bits, quantizes: bool, what: str):
    """what no strided attention launch serves — a global scale and, where it quantizes, FLOAT 4-bit states; returns the checked qtype"""
    if global_scale is not None:
        raise NotImplementedError(f"a global scale on {what} is not implemented by the MI355X path")
    if not quantizes:
        return qtype
    qtype = _check_qtype(qtype, num_bits)
    if qtype == "float" and int(num_bits) == 4:
        raise NotImplementedError("FLOAT 4-bit attention states are not implemented by the MI355X path")
    return qtype


def _attn_describe(d, x, layout_of, rest):
    """One tensor of a strided launch -> (the tensor read, what `layout_of` gave for it).  Plans x —
    layout_of(shape, strides, dtype, offset_bytes, *rest) -> (plan, ...), one of the two functions cached per layout (_attn_layout,
    _plan_attn_observe: what depends on x comes first in both, and both return a tuple that starts with the plan) —, and where the
    plan does not read it in place copies it (`.contiguous()`) and plans the copy; then fills the geometry fields AttnTensor and
    AttnObserveTensor share.  One function for both and `rest` as a tuple: the decode-shape calls are host-bound, and a frame
    and a re-packed argument list per tensor showed in them."""
    got = layout_of(x.shape, x.stride(), x.dtype, x.data_ptr() % 16, *rest)
    if not got[0].in_place:
        x = x.contiguous()
        got = layout_of(x.shape, x.stride(), x.dtype, x.data_ptr() % 16, *rest)
    plan = got[0]
    d.x, d.B, d.H, d.S, d.D = ptr(x), plan.B, plan.H, plan.S, plan.D
    d.x_stride[:], d.per_head = plan.strides, int(plan.per_head)
    return x, got


def plan_attn_qdq(shape, strides, dtype, scale_shape, strategy, *, out_dtype=None, offset_bytes: int = 0) -> AttnPlan:
    """The host plan of the attn_* functions for a tensor of `shape` / `strides` (elements) / `dtype` whose first element sits
    `offset_bytes` past a 16-byte boundary, with a scale of `scale_shape`: no tensor is touched.  Raises what the reference raises
    — ValueError for an attn_head tensor of fewer than 3 dimensions (lifecycle/initialize.py:242-247), RuntimeError for a scale that
    does not broadcast against the heads (torch's own, from forward_helpers.py:199) — and NotImplementedError for a strategy this
    entry does not serve."""
    st = _strategy_name(strategy)
    shape, strides, scale_shape = tuple(int(d) for d in shape), tuple(int(s) for s in strides), tuple(int(d) for d in scale_shape)
    if st not in ("attn_head", "tensor"):
        raise NotImplementedError(f"ct_attn_qdq serves the tensor and attn_head strategies, not {st!r}")
    scale_numel = math.prod(scale_shape)
    if st == "attn_head":
        if len(shape) < 3:
            raise ValueError("Attention quant requires at least 3 observed dimensions")
        H = shape[-3]
        if scale_numel != 1 and not (scale_numel == H and len(scale_shape) >= 3 and scale_shape[-3:] == (H, 1, 1)):
            if len(scale_shape) >= 3 and scale_shape[-2:] == (1, 1) and scale_numel == scale_shape[-3]:
                raise RuntimeError(f"The size of tensor a ({H}) must match the size of tensor b ({scale_shape[-3]}) at non-singleton dimension {len(shape) - 3}")
            raise NotImplementedError(f"an attn_head scale has shape (H, 1, 1) or one element, got {scale_shape} for {H} heads")
    elif scale_numel != 1:
        raise ValueError(f"per-tensor quantization expects a single scale, got shape {scale_shape}")
    if len(scale_shape) > max(len(shape), 1) and scale_numel == 1:
        raise NotImplementedError(f"a scale of {len(scale_shape)} dimensions would add dimensions to a tensor of {len(shape)}")
    if len(shape) == 0:
        shape, strides = (1,), (1,)
    out_dtype = dtype if out_dtype is None else out_dtype
    in_place, (B, H, S, D), xs, reason = _attn_view(shape, strides, writes=True)
    vec = D % 8 == 0
    if in_place:
        vec = _attn_unit_aligned(offset_bytes, (B, H, S), xs, dtype.itemsize, D)
        if vec and _attn_is_dense(shape, strides):  # the output keeps these strides; otherwise it is dense in the same order: multiples of D
            vec = _attn_unit_aligned(0, (B, H, S), xs, out_dtype.itemsize, D)
    return AttnPlan(in_place, vec, B, H, S, D, xs, st == "attn_head" and scale_numel != 1, reason)


_ATTN_MODES = {"fake": 0, "quantize": 1, "dequantize": 2}


@functools.lru_cache(maxsize=1024)
def _attn_out_strides(shape, strides, dtype, scale_shape, scale_strides, scale_dtype, mode: str, rounds: bool):
    """the strides the reference's result has: those torch's elementwise ops leave behind — x's own for a dense permuted x, dense
    in x's order for a slice or an expanded x, and torch's placement of size-1 dimensions, which the same-shape torch.round of the
    INT types rewrites (`rounds`) and the float8 cast does not.  Asked of torch itself, on meta tensors (no memory, no launch),
    once per layout: the op sequence of forward_helpers.py:180-215, 525-572 and quant_args.py:460-496."""
    x = torch.empty_strided(shape, strides, dtype=dtype, device="meta")
    scale = torch.empty_strided(scale_shape, scale_strides, dtype=scale_dtype, device="meta")
    if mode == "dequantize":
        return tuple((x.to(scale_dtype) * scale).stride())
    bound = torch.empty((), dtype=torch.float32, device="meta")
    t = torch.clamp(x / scale, bound, bound)
    if rounds and t.is_contiguous():
        t = torch.empty(shape, dtype=t.dtype, device="meta")  # torch.round of a contiguous tensor allocates the plain contiguous strides
    if mode == "fake":
        t = t.to(scale_dtype) * scale
    return tuple(t.stride())


@functools.lru_cache(maxsize=4096)
def _attn_layout(shape, strides, dtype, offset_bytes, scale_shape, scale_strides, scale_dtype, strategy, out_dtype, mode, rounds):  # _attn_describe's order
    """everything one call decides from shapes alone, once per layout: (plan, the output's strides, its b / h / s strides) — or
    (plan, None, None) for a tensor that is copied first (the caller asks again for the copy)"""
    plan = plan_attn_qdq(shape, strides, dtype, scale_shape, strategy, out_dtype=out_dtype, offset_bytes=offset_bytes)
    if not plan.in_place:
        return plan, None, None
    if _attn_is_dense(shape, strides) and 1 not in shape:
        out_strides = tuple(strides)  # what torch.empty_like gives: a dense permuted x keeps its strides, as in the reference
    else:
        out_strides = _attn_out_strides(shape, strides, dtype, scale_shape, scale_strides, scale_dtype, mode, rounds)
    view = _attn_fold(shape or (1,), out_strides or (1,)) if (not shape or shape[-1] <= 1 or out_strides[-1] == 1) else None
    if view is None or view[0] != (plan.B, plan.H, plan.S, plan.D):  # an order the kernel does not write: the dense form
        out_strides = tuple(torch.empty(shape, device="meta").stride())
        view = _attn_fold(shape or (1,), out_strides or (1,))
    return plan, out_strides, view[1]


@functools.lru_cache(maxsize=None)
def _attn_result_dtype(x_dtype, x_zero_dim: bool, scale_dtype, scale_zero_dim: bool):
    """_result_dtype on stand-ins of the same dtypes and dimensionality (once per combination)"""
    x = torch.empty(() if x_zero_dim else (1,), dtype=x_dtype, device="meta")
    scale = torch.empty(() if scale_zero_dim else (1,), dtype=scale_dtype, device="meta")
    return _result_dtype(x, scale, scale_zero_dim)


def _attn_qdq(tensors, mode: str, *, num_bits, strategy, qtype="int", dtype=None, global_scale=None, rot_size=0, rot_mask=0):
    """tensors: [(x, scale, zero_point)] of one or two q / k / v states sharing dtypes and arguments -> [out]; ONE ct_attn_qdq —
    or, with `rot_mask` (bit i: tensor i is rotated over runs of `rot_size` elements first), ONE ct_attn_rot_qdq.  A rotated
    tensor (one plan_attn_rot_qdq fuses) is read through its own strides and its output laid out as the composition lays it
    out: what the QDQ gives for the contiguous rotated tensor of the same shape"""
    st = _strategy_name(strategy)
    qtype = _attn_refusals(global_scale, qtype, num_bits, mode != "dequantize", "attention states")
    x0, s0, z0 = tensors[0]
    for x, s, z in tensors:
        if mode == "dequantize":
            if x.dtype not in (torch.int8, torch.int32, _F8, *_FLOATS):
                raise NotImplementedError(f"dequantize from {x.dtype} is not supported by the MI355X path")
        else:
            _check_float(x, "x")
        _check_float(s, "scale")
        if x.dtype != x0.dtype or s.dtype != s0.dtype or (z is None) != (z0 is None) or (z is not None and z.dtype != z0.dtype) or s.ndim != s0.ndim:
            raise NotImplementedError("the two tensors of one launch share their dtypes")
    if mode == "dequantize":
        T = s0.dtype
        out_dtype = dtype if dtype is not None else s0.dtype
        if out_dtype not in _FLOATS:
            raise NotImplementedError(f"dequantize to {out_dtype} is not supported by the MI355X path")
    else:
        T = _attn_result_dtype(x0.dtype, x0.ndim == 0, s0.dtype, s0.ndim == 0)
        if mode == "fake":
            out_dtype = s0.dtype
        else:
            out_dtype = dtype if dtype is not None else T
            allowed = (_F8, *_FLOATS) if qtype == "float" else (torch.int8, torch.int32, *_FLOATS)
            if out_dtype not in allowed:
                raise NotImplementedError(f"quantize ({qtype}, {num_bits} bits) to {out_dtype} is not supported by the MI355X path")
    dev = _compute_device(x0, s0)
    descs = (_lib.AttnTensor * len(tensors))()
    outs, keep, zdt = [], [], -1
    rounds = mode != "dequantize" and qtype == "int"
    for i, (x, s, z) in enumerate(tensors):
        if z is not None and z.numel() != s.numel():
            raise ValueError(f"zero_point shape {tuple(z.shape)} does not match scale shape {tuple(s.shape)}")
        xd = x if x.device == dev else x.to(dev)
        d = descs[i]
        tail = (s.shape, s.stride(), s.dtype, st, out_dtype, mode, rounds)
        xr, (_, out_strides, out_bhs) = _attn_describe(d, xd, _attn_layout, tail)
        if (rot_mask >> i) & 1:
            # hadamard_transform(x.contiguous()) is torch.empty_like of a tensor torch calls contiguous: dense strides — or x's own
            # where x already counts as contiguous (a decode step's S = 1 view keeps its stride in the size-1 dimension)
            rot_strides = xd.stride() if xd.is_contiguous() else _dense_strides(xd.shape)
            _, out_strides, out_bhs = _attn_layout(xd.shape, rot_strides, xd.dtype, 0, *tail)
        out = torch.empty_strided(xr.shape, out_strides, dtype=out_dtype, device=xr.device)
        sd = s if (s.device == dev and s.is_contiguous()) else _dev(s, dev)  # read element by element: no alignment needed
        if z is None:
            zd = None
        elif z.device == dev and z.is_contiguous() and z.dtype in DT and z.dtype is not torch.bool:
            zd, zdt = z, DT[z.dtype]
        else:
            zd, zdt = _zp_arg(z, dev)
        d.out, d.scale, d.zp, d.out_stride[:] = ptr(out), ptr(sd), ptr(zd), out_bhs
        outs.append(_home(out, x))
        keep.append((xr, sd, zd))
    kind = 1 if (mode != "dequantize" and qtype == "float") else 0
    tail = (_ATTN_MODES[mode], kind, int(num_bits) if mode != "dequantize" else 8, DT[x0.dtype], DT[s0.dtype], zdt, DT[T], DT[out_dtype], stream_on(dev))
    if rot_mask:
        call("ct_attn_rot_qdq", descs, len(tensors), int(rot_size), int(rot_mask), *tail)
    else:
        call("ct_attn_qdq", descs, len(tensors), *tail)
    return outs


def attn_fake_quantize(x, scale, zero_point=None, *, num_bits, strategy="attn_head", qtype="int", global_scale=None) -> torch.Tensor:
    """fake_quantize (lifecycle/forward.py:148-181) of a query / key / value state (..., H, S, D) under the `attn_head` strategy
    (scale (H, 1, 1), or one element) or the `tensor` strategy, read through its strides: no `.contiguous()` copy of the
    transposed views attention modules pass.  The result is allocated like torch.empty_like(x) — the strides of a dense permuted
    input are kept, as the reference's elementwise ops keep them — in the scale's dtype."""
    return _attn_qdq([(x, scale, zero_point)], "fake", num_bits=num_bits, strategy=strategy, qtype=qtype, global_scale=global_scale)[0]


def attn_quantize(x, scale, zero_point=None, *, num_bits, strategy="attn_head", qtype="int", dtype=None, global_scale=None) -> torch.Tensor:
    """quantize (lifecycle/forward.py:36-73) of such a state: to `dtype` (float8_e4m3fn for FLOAT args — what an FP8 KV cache
    stores —, int8 / int32, or a float dtype), or the promoted dtype of x / scale"""
    return _attn_qdq([(x, scale, zero_point)], "quantize", num_bits=num_bits, strategy=strategy, qtype=qtype, dtype=dtype, global_scale=global_scale)[0]


def attn_dequantize(x_q, scale, zero_point=None, *, strategy="attn_head", dtype=None, global_scale=None) -> torch.Tensor:
    """dequantize (lifecycle/forward.py:76-145) of such codes, in the scale's dtype (or `dtype`)"""
    return _attn_qdq([(x_q, scale, zero_point)], "dequantize", num_bits=8, strategy=strategy, dtype=dtype, global_scale=global_scale)[0]


def attn_fake_quantize_pair(k, v, k_scale, v_scale, k_zero_point=None, v_zero_point=None, *, num_bits, strategy="attn_head", qtype="int",
                            global_scale=None):
    """(attn_fake_quantize(k, ...), attn_fake_quantize(v, ...)) in ONE launch: what QuantizedKVCache.forward does back to back with
    the same arguments.  K and V keep their own shapes, strides and scales (MLA: different head dims); they share dtypes."""
    out = _attn_qdq([(k, k_scale, k_zero_point), (v, v_scale, v_zero_point)], "fake", num_bits=num_bits, strategy=strategy, qtype=qtype,
                    global_scale=global_scale)
    return out[0], out[1]


# --------------------------------------------------------------------------- attention: the min-max observer of the same states
ATTN_OBSERVE_MAX_ENTRIES = 1024  # kObsMaxEntries of csrc/ct_attn_observe.hip: the LDS table of a workgroup
_OBSERVE_EMPTY = (0x7FFFFFFF, -0x80000000)  # the armed keys: the identities of integer min and max (include/ct_hip.h)

# what flatten_attention_for_quantization refuses (the reference tests' observer), in its words
_ATTN_OBSERVE_REFUSED = {
    "token": "Token quantization cannot be applied to attention",
    "channel": "Channel quantization cannot be applied to attention",
    "group": "Group quantization cannot be applied to attention",
    "tensor_group": "Group quantization cannot be applied to attention",
    "block": "Block quantization cannot be applied to attention",
}


class AttnObservePlan(NamedTuple):
    """what attn_observe does with one tensor: `in_place` (ct_attn_observe reads it through its strides; False: `.contiguous()`
    first, `reason` says why), the (B, H, S, D) view and the b / h / s element strides the kernel gets, `per_head` and `entries`
    (H scale entries, or one), and `vector` (rows of whole 8-element units whose bases and strides keep the units aligned)"""
    in_place: bool
    vector: bool
    B: int
    H: int
    S: int
    D: int
    strides: tuple
    per_head: bool
    entries: int
    reason: Optional[str]


@functools.lru_cache(maxsize=4096)
def _plan_attn_observe(shape, strides, dtype, offset_bytes, st, device_type):  # _attn_describe's order, and its 1-tuple
    return (plan_attn_observe(shape, strides, dtype, st, offset_bytes=offset_bytes, device_type=device_type),)  # once per layout


def plan_attn_observe(shape, strides, dtype, strategy, *, offset_bytes: int = 0, device_type: str = "cuda") -> AttnObservePlan:
    """The host plan of attn_observe for a tensor of `shape` / `strides` (elements) / `dtype` whose first element sits
    `offset_bytes` past a 16-byte boundary: no tensor is touched.  A read-only kernel takes expanded (stride 0) dimensions and views
    that overlap themselves as they are; only what it cannot index — a negative stride, a last dimension that is not contiguous,
    leading dimensions that do not fold into one batch — is copied first.  Raises what the reference raises (the ValueError of
    flatten_attention_for_quantization for the strategies attention states do not take, of initialize_qparams for an attn_head
    tensor of fewer than 3 dimensions), ValueError for an empty tensor, and NotImplementedError for float64, CPU tensors and more
    heads than the kernel's table holds."""
    st = _strategy_name(strategy)
    shape, strides = tuple(int(d) for d in shape), tuple(int(s) for s in strides)
    if st in _ATTN_OBSERVE_REFUSED:
        raise ValueError(_ATTN_OBSERVE_REFUSED[st])
    if st not in ("attn_head", "tensor"):
        raise NotImplementedError(f"ct_attn_observe serves the tensor and attn_head strategies, not {st!r}")
    if dtype not in _FLOATS:
        raise NotImplementedError(f"observing {dtype} is not supported by the MI355X path (float32, float16 and bfloat16 are)")
    if device_type != "cuda":
        raise NotImplementedError(f"ct_attn_observe runs on the MI355X; the tensor is on {device_type!r} (there is no CPU fallback)")
    if st == "attn_head" and len(shape) < 3:
        raise ValueError("Attention quant requires at least 3 observed dimensions")
    if math.prod(shape) == 0:
        raise ValueError(f"cannot observe an empty tensor of shape {shape}: the minimum of no elements is undefined")
    if len(shape) == 0:
        shape, strides = (1,), (1,)
    per_head = st == "attn_head"
    if per_head and shape[-3] > ATTN_OBSERVE_MAX_ENTRIES:
        raise NotImplementedError(f"{shape[-3]} heads: ct_attn_observe's table holds {ATTN_OBSERVE_MAX_ENTRIES} entries")
    in_place, (B, H, S, D), xs, reason = _attn_view(shape, strides, writes=False)
    vec = _attn_unit_aligned(offset_bytes, (B, H, S), xs, dtype.itemsize, D) if in_place else D % 8 == 0
    return AttnObservePlan(in_place, vec, B, H, S, D, xs, per_head, H if per_head else 1, reason)


def attn_observe_state(entries: int, device) -> torch.Tensor:
    """the armed running state of `entries` scale entries: int32 (2, entries) order keys, row 0 the minima, row 1 the maxima"""
    return attn_observe_arm(torch.empty((2, int(entries)), dtype=torch.int32, device=device))


def attn_observe_arm(state: torch.Tensor) -> torch.Tensor:
    """arm `state` in place: every entry forgets what it has seen (two fills, nothing waits)"""
    state[0].fill_(_OBSERVE_EMPTY[0])
    state[1].fill_(_OBSERVE_EMPTY[1])
    return state


def _observe_out(given, shape, dtype, dev, what):
    if given is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    t = given  # (a Parameter answers these itself: isinstance(x, Parameter) is a Python-level metaclass check, 0.8 us on a plain tensor)
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return given


def _attn_observe(items, *, num_bits, symmetric, qtype, strategy, zp_dtype, keep, want_minmax, global_scale=None):
    """items: [(x, state, scale or None, zero_point or None)] of one or two states sharing dtype and arguments; ONE ct_attn_observe"""
    kind = int(_attn_refusals(global_scale, qtype, num_bits, True, "observed attention states") == "float")
    if kind and not symmetric:
        raise NotImplementedError("asymmetric FLOAT 8-bit observation is not implemented by the MI355X path")
    if not kind and not 1 <= int(num_bits) <= 8:
        raise NotImplementedError(f"INT {num_bits}-bit observation is not implemented by the MI355X path (1 to 8 bits are)")
    st = _strategy_name(strategy)
    zp_dtype = zp_dtype if zp_dtype is not None else (_F8 if kind else torch.int8)
    if zp_dtype not in (torch.int8, torch.int32, _F8, *_FLOATS):
        raise NotImplementedError(f"a zero point of {zp_dtype} is not supported by the MI355X path")
    x0 = items[0][0]
    descs = (_lib.AttnObserveTensor * len(items))()
    results, alive = [], []
    for i, (x, state, scale, zero_point) in enumerate(items):
        if x.dtype != x0.dtype or x.device != x0.device:
            raise NotImplementedError("the two tensors of one launch share their dtype and device")
        d = descs[i]
        xr, (plan,) = _attn_describe(d, x, _plan_attn_observe, (st, x.device.type))
        dev = x.device
        if state.dtype != torch.int32 or tuple(state.shape) != (2, plan.entries) or state.device != dev or not state.is_contiguous():
            raise ValueError(f"the observer state of {plan.entries} entries is a contiguous int32 (2, {plan.entries}) tensor on {dev} "
                             f"(attn_observe_state), got {state.dtype} {tuple(state.shape)} on {state.device}")
        out_shape = (plan.H, 1, 1) if plan.per_head else (1,)
        scale_dtype = x.dtype if scale is None else scale.dtype  # a module's parameter may be wider than the state it scales
        if scale_dtype not in _FLOATS or (results and scale_dtype != results[0][0].dtype):
            raise NotImplementedError(f"a scale of {scale_dtype} is not supported by the MI355X path (the two tensors of one launch share it)")
        scale_out = _observe_out(scale, out_shape, scale_dtype, dev, "scale")
        zp_out = _observe_out(zero_point, out_shape, zp_dtype, dev, "zero_point")
        mn = torch.empty(out_shape, dtype=x.dtype, device=dev) if want_minmax else None
        mx = torch.empty(out_shape, dtype=x.dtype, device=dev) if want_minmax else None
        d.state, d.scale, d.zp, d.min_vals, d.max_vals = ptr(state), ptr(scale_out), ptr(zp_out), ptr(mn), ptr(mx)
        results.append((scale_out, zp_out, mn, mx) if want_minmax else (scale_out, zp_out))
        alive.append(xr)
    sdt = results[0][0].dtype
    call("ct_attn_observe", descs, len(items), kind, int(num_bits), int(bool(symmetric)), DT[x0.dtype], DT[sdt], DT[zp_dtype], int(bool(keep)),
         stream_on(x0.device))
    return results


def attn_observe(x, state, *, num_bits, symmetric=True, qtype="int", strategy="attn_head", zp_dtype=None, keep=False, scale=None, zero_point=None,
                 want_minmax=False, global_scale=None):
    """A min-max observer's forward on a query / key / value state (..., H, S, D) — or, under the `tensor` strategy, any activation
    (..., hidden) — read through its strides: torch.amin / amax per head (`attn_head`) or over the tensor, folded into `state`
    (attn_observe_state), then calculate_qparams (quantization/utils/helpers.py:50-137) of the running extremes, evaluated in
    x's dtype.  Returns (scale, zero_point) — scale in x's dtype of shape (H, 1, 1) or (1,), zero_point in `zp_dtype` (int8, or
    zeros of float8_e4m3fn for FLOAT 8-bit) — and with `want_minmax` also (min_vals, max_vals) in x's dtype.  `scale` /
    `zero_point` given (module parameters of that shape): the kernel writes them in place and they are what is returned.
    keep=False: `state` is armed again behind the call (each call stands alone); keep=True: the next call folds into it.
    Two launches, no copy of a strided view, no host synchronisation."""
    return _attn_observe([(x, state, scale, zero_point)], num_bits=num_bits, symmetric=symmetric, qtype=qtype, strategy=strategy, zp_dtype=zp_dtype,
                         keep=keep, want_minmax=want_minmax, global_scale=global_scale)[0]


def attn_observe_pair(k, v, k_state, v_state, *, num_bits, symmetric=True, qtype="int", strategy="attn_head", zp_dtype=None, keep=False,
                      k_scale=None, v_scale=None, k_zero_point=None, v_zero_point=None, want_minmax=False, global_scale=None):
    """(attn_observe(k, k_state, ...), attn_observe(v, v_state, ...)) in the SAME two launches: K and V of one cache update keep
    their own shapes, strides, states and outputs (MLA: different head dims) and share dtype and arguments"""
    out = _attn_observe([(k, k_state, k_scale, k_zero_point), (v, v_state, v_scale, v_zero_point)], num_bits=num_bits, symmetric=symmetric, qtype=qtype,
                        strategy=strategy, zp_dtype=zp_dtype, keep=keep, want_minmax=want_minmax, global_scale=global_scale)
    return out[0], out[1]


def attn_observe_global_scale(x, state, *, keep=False, global_scale=None) -> torch.Tensor:
    """An observer's `get_global_scale` — `generate_gparam` (quantization/utils/helpers.py:308-337) of the extremes of the whole tensor, the
    reference observer's `reshape((1, 1, -1))` — on any activation, read in place through its strides: folded into `state`
    (attn_observe_state(1, device)) as one entry, then 448 * 6 / amax of the running extremes evaluated in x's dtype (kind 2 of ct_attn_observe:
    the arithmetic of ct_generate_gparam).  Returns the float32 (1,) global scale; `global_scale` given (a module's `input_global_scale`): the
    kernel writes it in place and it is what is returned.  `keep` as in attn_observe.  One ct_attn_observe, no copy of a view the kernel can index,
    no host synchronisation."""
    descs = (_lib.AttnObserveTensor * 1)()
    d = descs[0]
    xr, (plan,) = _attn_describe(d, x, _plan_attn_observe, ("tensor", x.device.type))
    dev = x.device
    if state.dtype != torch.int32 or tuple(state.shape) != (2, 1) or state.device != dev or not state.is_contiguous():
        raise ValueError(f"the observer state of a global scale is a contiguous int32 (2, 1) tensor on {dev} (attn_observe_state), got {state.dtype} "
                         f"{tuple(state.shape)} on {state.device}")
    out = _observe_out(global_scale, (1,), torch.float32, dev, "global_scale")
    d.state, d.scale, d.zp, d.min_vals, d.max_vals = ptr(state), ptr(out), None, None, None
    call("ct_attn_observe", descs, 1, 2, 0, 1, DT[x.dtype], DT[torch.float32], DT[torch.int8], int(bool(keep)), stream_on(dev))
    return out


# --------------------------------------------------------------------------- attention: the head-dim rotation in the QDQ's launch
ATTN_ROTATED_MAX_SIZE = 512  # the rotation blocks csrc/ct_attn_rot.hip serves: n / 8 lanes of one wave
ATTN_ROTATED_MAX_UNITS = 256  # D / 8: a row is one pass of a workgroup's lanes

# Which calls `fused=None` dispatches to the one launch (ct_attn_rot_qdq): "single" — one rotated tensor (the query states) —
# and "pair" — K rotated and V not, one cache update.  True only where tools/attn_bench.py measured the fused launch faster than
# `.contiguous()` + hadamard_transform + attn_fake_quantize{,_pair} on the same buffers by more than the spread between its runs,
# in every row that speaks for the key (profiles/attn_rot_bench.jsonl): q (1, 32, 8192, 128) 55.6-55.8 us against
# 128.3-128.5, k+v (1, 8, 8192, 128) 26.9-28.3 against 54.0-56.1, decode k+v (64, 8, 1, 128) 18.8-20.2 against 26.3-28.0, run spreads
# 0.2, 2.1 and 1.7 us.  False would mean: the composition.
ATTN_ROTATED_MEASURED_FASTER = {"single": True, "pair": True}


class AttnRotPlan(NamedTuple):
    """what the attn_rotated_* functions do with one tensor: `fused` (ct_attn_rot_qdq rotates and quantizes it in one launch,
    reading it `in_place` through its strides) or not (`reason` says why: `.contiguous()`, hadamard_transform, then the attn_*
    call).  `out_strides`: the result's strides for a rotated tensor with dense strides (the reference's: its GEMM allocates one).
    The result follows the composition: where torch already counts x as contiguous (S = 1 views) the size-1 dimension may keep
    x's stride, which no index ever multiplies.  `hadamard` / `attn` are the parents' plans (attn: of the tensor as given)."""
    fused: bool
    in_place: bool
    reason: Optional[str]
    out_strides: tuple
    hadamard: "HadamardPlan"
    attn: AttnPlan


def plan_attn_rot_qdq(shape, strides, dtype, size: int, scale_shape, strategy, *, out_dtype=None, offset_bytes: int = 0,
                      precision=torch.float32) -> AttnRotPlan:
    """The host plan of the attn_rotated_* functions, from shapes, strides and dtypes alone.  Raises what plan_hadamard raises
    (upstream's ValueError for a size that is not a positive power of two or does not divide D) first, then what plan_attn_qdq
    raises; everything the one launch does not serve is declined with a reason, and the composition serves it."""
    hp = plan_hadamard(shape, dtype, size, -1, precision)
    ap = plan_attn_qdq(shape, strides, dtype, scale_shape, strategy, out_dtype=out_dtype, offset_bytes=offset_bytes)
    n, D = hp.size, ap.D
    reason = None
    if precision is not torch.float32:
        reason = f"the fused launch accumulates in float32, not {precision}"
    elif not 2 <= n <= ATTN_ROTATED_MAX_SIZE:
        reason = f"hadamard size {n} is outside 2 .. {ATTN_ROTATED_MAX_SIZE}"
    elif D % 8:
        reason = f"rows of {D} elements are not whole 8-element units"
    elif D // 8 > ATTN_ROTATED_MAX_UNITS:
        reason = f"rows of {D} elements exceed one pass of {ATTN_ROTATED_MAX_UNITS} units"
    elif not ap.in_place:
        reason = ap.reason
    elif not ap.vector:  # (the output side never decides: a dense tensor's strides are multiples of D, and D is whole units here)
        reason = "the storage offset or a stride breaks the alignment of the 8-element units"
    return AttnRotPlan(reason is None, ap.in_place, reason, _dense_strides(tuple(int(d) for d in shape)), hp, ap)


@functools.lru_cache(maxsize=4096)
def _attn_rot_plan_fused(shape, strides, dtype, size, scale_shape, strategy, out_dtype, offset_bytes) -> bool:
    """plan_attn_rot_qdq(...).fused, once per layout (what it raises is raised on every call)"""
    return plan_attn_rot_qdq(shape, strides, dtype, size, scale_shape, strategy, out_dtype=out_dtype, offset_bytes=offset_bytes).fused


@functools.lru_cache(maxsize=4096)
def _attn_rot_plain_ok(shape, strides, dtype, scale_shape, strategy, out_dtype, offset_bytes) -> bool:
    """the unrotated tensor of a pair: read in place, in the vector form, one pass per row"""
    p = plan_attn_qdq(shape, strides, dtype, scale_shape, strategy, out_dtype=out_dtype, offset_bytes=offset_bytes)
    return p.in_place and p.vector and p.D // 8 <= ATTN_ROTATED_MAX_UNITS


def _attn_rot_fusable(x, size, scale, strategy, out_dtype) -> bool:
    """one launch serves the rotated x: GPU tensors and a plan that fuses"""
    if not (x.is_cuda and scale.is_cuda and x.numel()):
        return False
    return _attn_rot_plan_fused(x.shape, x.stride(), x.dtype, int(size), scale.shape, _strategy_name(strategy), out_dtype, x.data_ptr() % 16)


def _attn_rot_pair_fusable(k, v, size, k_scale, v_scale, strategy) -> bool:
    """one launch serves the rotated k and the unrotated v"""
    if not (_attn_rot_fusable(k, size, k_scale, strategy, k_scale.dtype) and v.is_cuda and v_scale.is_cuda and v.numel()):
        return False
    return _attn_rot_plain_ok(v.shape, v.stride(), v.dtype, v_scale.shape, _strategy_name(strategy), v_scale.dtype, v.data_ptr() % 16)


def attn_rotated_fake_quantize(x, size: int, scale, zero_point=None, *, num_bits, strategy="attn_head", qtype="int", fused: Optional[bool] = None) -> torch.Tensor:
    """attn_fake_quantize(hadamard_transform(x.contiguous(), size), scale, zero_point, ...): a query or key state rotated over
    runs of `size` elements of its head dimension (HadamardTransform at q_attn / k_cache, float32) and quantized.  `fused`: True —
    ONE launch (ct_attn_rot_qdq) wherever plan_attn_rot_qdq allows it: the strided view is read once, neither the contiguous copy
    nor the rotated tensor exist; False — the composition; None — the fused launch where ATTN_ROTATED_MEASURED_FASTER["single"]
    says it was measured faster.  The same bits, dtype, shape and strides either way."""
    want = ATTN_ROTATED_MEASURED_FASTER["single"] if fused is None else fused
    if want and _attn_rot_fusable(x, size, scale, strategy, scale.dtype):
        return _attn_qdq([(x, scale, zero_point)], "fake", num_bits=num_bits, strategy=strategy, qtype=qtype, rot_size=size, rot_mask=1)[0]
    return attn_fake_quantize(hadamard_transform(x.contiguous(), size), scale, zero_point, num_bits=num_bits, strategy=strategy, qtype=qtype)


def attn_rotated_quantize(x, size: int, scale, zero_point=None, *, num_bits, strategy="attn_head", qtype="int", dtype=None,
                          fused: Optional[bool] = None) -> torch.Tensor:
    """attn_quantize(hadamard_transform(x.contiguous(), size), ...) — what an FP8 KV cache stores of rotated keys —, in one launch
    under the rule of attn_rotated_fake_quantize"""
    want = ATTN_ROTATED_MEASURED_FASTER["single"] if fused is None else fused
    if want and _attn_rot_fusable(x, size, scale, strategy, dtype):
        return _attn_qdq([(x, scale, zero_point)], "quantize", num_bits=num_bits, strategy=strategy, qtype=qtype, dtype=dtype, rot_size=size, rot_mask=1)[0]
    return attn_quantize(hadamard_transform(x.contiguous(), size), scale, zero_point, num_bits=num_bits, strategy=strategy, qtype=qtype, dtype=dtype)


def attn_rotated_fake_quantize_pair(k, v, size: int, k_scale, v_scale, k_zero_point=None, v_zero_point=None, *, num_bits, strategy="attn_head",
                                    qtype="int", fused: Optional[bool] = None):
    """attn_fake_quantize_pair(hadamard_transform(k.contiguous(), size), v, ...): one cache update under a k_cache rotation — K
    rotated, V not — in ONE launch where both tensors suit it (`fused` as in attn_rotated_fake_quantize, key "pair")."""
    want = ATTN_ROTATED_MEASURED_FASTER["pair"] if fused is None else fused
    if want and _attn_rot_pair_fusable(k, v, size, k_scale, v_scale, strategy):
        out = _attn_qdq([(k, k_scale, k_zero_point), (v, v_scale, v_zero_point)], "fake", num_bits=num_bits, strategy=strategy, qtype=qtype,
                        rot_size=size, rot_mask=1)
        return out[0], out[1]
    return attn_fake_quantize_pair(hadamard_transform(k.contiguous(), size), v, k_scale, v_scale, k_zero_point, v_zero_point, num_bits=num_bits,
                                   strategy=strategy, qtype=qtype)


# --------------------------------------------------------------------------- attention: dynamic group QDQ of the same states
ATTN_DYNAMIC_MAX_GROUP = 512  # the groups csrc/ct_attn_dyn.hip serves: group / 8 lanes of one wave
ATTN_DYNAMIC_MAX_UNITS = 256  # D / 8: a row is one pass of a workgroup's lanes

# Which calls `form=None` dispatches to the strided launch (ct_attn_dyn_qdq): "single" — one state read through its strides
# instead of `.contiguous()` + ct_dynamic_qdq + the copy into the reference's strides — and "pair" — K and V of one cache update in
# ONE launch instead of two.  A key is True only where tools/attn_dynamic_bench.py measured that form faster than its baseline by
# more than the spread between its runs, in every row and scheme that speaks for the key (profiles/attn_dynamic_bench.jsonl, DESIGN
# 5.20).  False means: "single" — the copy form; "pair" — two launches.
# As measured (two runs, us per call): 13 of the 15 verdicts say "faster" — q (1, 32, 8192, 128) 45.4-51.1 strided against 127.5-130.1
# copied, k+v (1, 8, 8192, 128) 26.0-27.3 paired against 29.3-31.2 in two launches — but decode k+v MXFP4 strided had medians of 35.3-36.4
# (minima 22.7-23.1) against 33.6-33.8 copied, and prefill k+v NVFP4 paired medians of 32.9-35.3 (minima 26.7-27.0) against 29.3-29.5: one
# "not faster" verdict per key, so both keys stay False until a measurement clears them.
ATTN_DYNAMIC_MEASURED_FASTER = {"single": False, "pair": False}


class AttnDynPlan(NamedTuple):
    """what the attn_dynamic_* functions do with one tensor: `form` "strided" (ct_attn_dyn_qdq reads it through its strides) or
    "copy" (`reason` says why: ct_dynamic_qdq on `.contiguous()`, then one copy into the reference's strides); the (B, H, S, D)
    view and b / h / s strides of the strided form; `group` (elements of one scale inside a row; 0 in the copy form); the strides
    of the reference's result; `dynamic`: quantization.dynamic.plan_dynamic's plan (kind, scale / zero-point shapes and dtypes)"""
    form: str
    reason: Optional[str]
    B: int
    H: int
    S: int
    D: int
    strides: tuple
    group: int
    out_strides: tuple
    dynamic: object

    @property
    def scale_shape(self):
        return self.dynamic.scale_shape

    @property
    def scale_dtype(self):
        return self.dynamic.scale_dtype

    @property
    def zp_dtype(self):
        return self.dynamic.zp_dtype


@functools.lru_cache(maxsize=1024)
def _attn_dyn_out_strides(shape, strides, dtype, group: int, scale_shape, scale_dtype, has_global: bool, kind: str):
    """the strides the reference's dynamic fake_quantize leaves: asked of torch itself on meta tensors, once per layout — the group
    chain (forward_helpers.py:118-177: unflatten, the elementwise ops against a contiguous scale, flatten(-2), .to(x.dtype)) or the
    plain chain (token / tensor: forward_helpers.py:180-215), with the rounding step of the kind (quant_args.py:460-496)"""
    x = torch.empty_strided(shape, strides, dtype=dtype, device="meta")
    scale = torch.empty(scale_shape, dtype=scale_dtype, device="meta")
    zp = torch.empty(scale_shape, dtype=torch.int8, device="meta")
    if group:
        x = x.unflatten(-1, (shape[-1] // group, group))
        scale, zp = scale.unsqueeze(-1), zp.unsqueeze(-1)
    if has_global:
        scale = scale / torch.empty((1,), dtype=torch.float32, device="meta")
    t = x / scale
    t += zp.to(x.dtype)
    bound = torch.empty((), dtype=torch.float32, device="meta")
    t = torch.clamp(t, bound, bound)
    if kind == "int":
        if t.is_contiguous():
            t = torch.empty(tuple(t.shape), dtype=t.dtype, device="meta")  # torch.round of a contiguous tensor allocates the plain strides
    elif kind in ("fp8", "mxfp8"):
        t = t.to(_F8).to(t.dtype)
    else:
        t = torch.abs(t) * torch.sign(t)  # cast_to_fp4 (fp4_utils.py:78-98)
    t = t.to(scale.dtype)
    t = (t - zp.to(scale.dtype)) * scale
    if group:
        t = t.flatten(start_dim=-2).to(dtype)
    return tuple(t.stride())


@functools.lru_cache(maxsize=4096)
def _plan_attn_dynamic(shape, strides, dtype, offset_bytes, strategy, group_size, kind_key, has_global):
    from .quantization.dynamic import plan_dynamic
    args = SimpleNamespace(strategy=strategy, group_size=group_size, **dict(kind_key))
    dp = plan_dynamic(shape, dtype, args, True if has_global else None)
    in_place, (B, H, S, D), xs, reason = _attn_view(shape, strides, writes=True)
    group = 0
    if dp.tensor_form:
        reason = "one scale for the whole tensor: its reduction crosses rows"
    elif strategy == "token":
        if S != 1 or dp.seg_len != D:
            reason = f"a token scale over {dp.seg_len} elements crosses the rows of {D}"
        else:
            group = D
    else:
        group = dp.seg_len
    if reason is None:
        units = group // 8
        if D % 8:
            reason = f"rows of {D} elements are not whole 8-element units"
        elif D // 8 > ATTN_DYNAMIC_MAX_UNITS:
            reason = f"rows of {D} elements exceed one pass of {ATTN_DYNAMIC_MAX_UNITS} units"
        elif group % 8 or group > ATTN_DYNAMIC_MAX_GROUP or units & (units - 1):
            reason = f"groups of {group} elements are not 8 * 2^k <= {ATTN_DYNAMIC_MAX_GROUP}"
        elif not _attn_unit_aligned(offset_bytes, (B, H, S), xs, dtype.itemsize, D):
            reason = "the storage offset or a stride breaks the alignment of the 8-element units"
    out_strides = _attn_dyn_out_strides(shape, strides, dtype, 0 if strategy in ("token", "tensor") else dp.seg_len, dp.scale_shape, dp.scale_dtype,
                                        bool(has_global), dp.kind)
    out_bhs = None
    if reason is None:
        view = _attn_fold(shape, out_strides) if (shape[-1] <= 1 or out_strides[-1] == 1) else None
        if view is None or view[0] != (B, H, S, D) or not _attn_unit_aligned(0, (B, H, S), view[1], dtype.itemsize, D):
            reason = "the reference's output strides are not rows the kernel writes"
        else:
            out_bhs = view[1]
    if reason is not None:
        return AttnDynPlan("copy", reason, B, H, S, D, xs, 0, out_strides, dp), None
    return AttnDynPlan("strided", None, B, H, S, D, xs, group, out_strides, dp), out_bhs


def _attn_dyn_key(args):
    """the hashable part of the arguments a plan depends on"""
    return (_strategy_name(args.strategy), getattr(args, "group_size", None),
            (("num_bits", int(args.num_bits)), ("type", _strategy_name(getattr(args, "type", "int"))), ("symmetric", bool(args.symmetric)),
             ("scale_dtype", getattr(args, "scale_dtype", None)), ("zp_dtype", getattr(args, "zp_dtype", None))))


def plan_attn_dynamic(shape, strides, dtype, args, *, offset_bytes: int = 0, global_scale: bool = False) -> AttnDynPlan:
    """The host plan of the attn_dynamic_* functions for a state of `shape` / `strides` (elements) / `dtype` whose first element
    sits `offset_bytes` past a 16-byte boundary, under the dynamic arguments `args` (and a global scale or not): no tensor is
    touched.  Raises what quantization.dynamic.plan_dynamic raises — the reference's ValueError for a strategy outside token /
    tensor / group / tensor_group, NotImplementedError for what no kernel computes.  "strided": group / tensor_group with
    D % 8 == 0, D / 8 <= 256, group = 8 * 2^k <= 512 dividing D, on a view read in place with aligned units on both sides; and
    token where S == 1 and D is such a group.  Everything else is "copy", with the reason."""
    shape, strides = tuple(int(d) for d in shape), tuple(int(s) for s in strides)
    st, gs, kind_key = _attn_dyn_key(args)
    if len(shape) == 0:
        shape, strides = (1,), (1,)
    return _plan_attn_dynamic(shape, strides, dtype, int(offset_bytes) % 16, st, gs, kind_key, bool(global_scale))[0]


def _attn_dyn_copy(x, plan: AttnDynPlan, global_scale, want_out: bool, want_qparams: bool):
    """the copy form: ct_dynamic_qdq on the contiguous copy, then one copy_ into the reference's strides"""
    dp = plan.dynamic
    out, scale, zp = dynamic_qdq(x.contiguous(), kind=dp.kind, segs=dp.segs, seg_len=dp.seg_len, num_bits=dp.num_bits, symmetric=dp.symmetric,
                                 global_scale=global_scale, scale_shape=dp.scale_shape, scale_dtype=dp.scale_dtype if want_qparams else None,
                                 zp_dtype=dp.zp_dtype if want_qparams else None, want_out=want_out)
    if want_out and tuple(out.stride()) != plan.out_strides:
        laid = torch.empty_strided(out.shape, plan.out_strides, dtype=out.dtype, device=out.device)
        laid.copy_(out)
        out = laid
    return out, scale, zp


def _attn_dynamic(tensors, args, *, want_out: bool = True, want_qparams: bool = False, form: Optional[str] = None, pair: Optional[bool] = None):
    """tensors: [(x, global_scale)] of one or two states sharing dtype and arguments -> [(out, scale, zero_point)].  `form`: "strided"
    — ct_attn_dyn_qdq wherever the plan allows it —, "copy", or None: ATTN_DYNAMIC_MEASURED_FASTER["single"] decides.  Two strided
    tensors that both take a global scale, or neither, share ONE launch (`pair`; None: ATTN_DYNAMIC_MEASURED_FASTER["pair"])."""
    st, gs, kind_key = _attn_dyn_key(args)
    want_strided = ATTN_DYNAMIC_MEASURED_FASTER["single"] if form is None else form == "strided"
    if form not in (None, "strided", "copy"):
        raise ValueError(f"form is 'strided', 'copy' or None, got {form!r}")
    plans = []
    for x, g in tensors:
        _check_float(x, "activation")
        if not x.is_cuda:
            raise NotImplementedError("the dynamic QDQ kernels take GPU activations")
        shape, strides = (tuple(x.shape), tuple(x.stride())) if x.ndim else ((1,), (1,))
        plans.append(_plan_attn_dynamic(shape, strides, x.dtype, x.data_ptr() % 16, st, gs, kind_key, g is not None))
    results = [None] * len(tensors)
    strided = [i for i, (plan, _) in enumerate(plans) if want_strided and plan.form == "strided" and tensors[i][0].numel()]
    for i, (x, g) in enumerate(tensors):
        if i not in strided:
            results[i] = _attn_dyn_copy(x, plans[i][0], g, want_out, want_qparams)
    if not strided:
        return results
    together = len(strided) == 2 and (ATTN_DYNAMIC_MEASURED_FASTER["pair"] if pair is None else pair) \
        and (tensors[0][1] is None) == (tensors[1][1] is None) and tensors[0][0].dtype == tensors[1][0].dtype \
        and tensors[0][0].device == tensors[1][0].device
    for batch in ([strided] if together else [[i] for i in strided]):
        descs = (_lib.AttnDynTensor * len(batch))()
        keep = []
        for d, i in zip(descs, batch):
            (x, g), (plan, out_bhs) = tensors[i], plans[i]
            dp, dev = plan.dynamic, x.device
            out = torch.empty_strided(x.shape, plan.out_strides, dtype=x.dtype, device=dev) if want_out else None
            scale = torch.empty(dp.scale_shape, dtype=dp.scale_dtype, device=dev) if want_qparams else None
            zp = torch.empty(dp.scale_shape, dtype=dp.zp_dtype, device=dev) if want_qparams else None
            gd = _gs_arg(g, dev)
            d.x, d.out, d.scale_out, d.zp_out, d.global_scale = ptr(x), ptr(out), ptr(scale), ptr(zp), ptr(gd)
            d.B, d.H, d.S, d.D = plan.B, plan.H, plan.S, plan.D
            d.x_stride[:] = plan.strides
            d.out_stride[:] = out_bhs
            keep.append(gd)
            results[i] = (out, scale, zp)
        x0, dp0 = tensors[batch[0]][0], plans[batch[0]][0].dynamic
        call("ct_attn_dyn_qdq", descs, len(batch), int(plans[batch[0]][0].group), DYNAMIC_KINDS[dp0.kind], int(dp0.num_bits), int(bool(dp0.symmetric)),
             DT[x0.dtype], DT[dp0.zp_dtype] if want_qparams else -1, stream_of(x0))
    return results


def attn_dynamic_fake_quantize(x, args, global_scale=None, *, return_qparams: bool = False, form: Optional[str] = None):
    """quantization.dynamic.dynamic_fake_quantize(x.contiguous(), args, global_scale) of a query / key / value state (..., H, S, D)
    — the same bits — laid out with the strides the reference's op chain leaves.  "strided" form: ONE launch reads the view through
    its strides (csrc/ct_attn_dyn.hip), no copy; "copy" form: the contiguous kernel on `.contiguous()` and one copy_ into those
    strides.  `form` None: the strided form where the plan allows it and ATTN_DYNAMIC_MEASURED_FASTER["single"] says it was
    measured faster.  With return_qparams: (out, scale, zero_point) in the reference's shapes and dtypes."""
    out, scale, zp = _attn_dynamic([(x, global_scale)], args, want_qparams=return_qparams, form=form)[0]
    return (out, scale, zp) if return_qparams else out


def attn_dynamic_qparams(x, args, global_scale=None, *, form: Optional[str] = None):
    """compute_dynamic_scales_and_zp of such a state: (scale, zero_point), nothing else written"""
    _, scale, zp = _attn_dynamic([(x, global_scale)], args, want_out=False, want_qparams=True, form=form)[0]
    return scale, zp


def attn_dynamic_fake_quantize_pair(k, v, args, k_global_scale=None, v_global_scale=None, *, return_qparams: bool = False, form: Optional[str] = None,
                                    pair: Optional[bool] = None):
    """(attn_dynamic_fake_quantize(k, ...), attn_dynamic_fake_quantize(v, ...)): in ONE launch where both take the strided form
    and both global scales are present or both absent (`pair` None: where ATTN_DYNAMIC_MEASURED_FASTER["pair"] says so).  K and V
    keep their own shapes, strides and global scales (MLA: different head dims); they share the dtype."""
    res = _attn_dynamic([(k, k_global_scale), (v, v_global_scale)], args, want_qparams=return_qparams, form=form, pair=pair)
    return (res[0], res[1]) if return_qparams else (res[0][0], res[1][0])


def quantize_and_pack(x, scale, zero_point, *, num_bits, strategy, group_size=None, block_structure=None,
                      g_idx=None) -> torch.Tensor:
    """Fused quantize(dtype=int8) + pack_to_int32 (compressors/pack_quantized/base.py:96-104):
    one pass over the weight, no int8 intermediate.  Returns int32 (*x.shape[:-1], ceil(cols*bits/32))."""
    _check_float(x, "weight")
    _check_float(scale, "scale")
    if not 1 <= num_bits <= 8:
        raise ValueError(f"Packing is only supported for num_bits in [1, 8], got {num_bits}")
    layout = QuantLayout(x.shape, scale, strategy, group_size, block_structure, g_idx)
    _check_sz(layout, scale, zero_point)
    T = _result_dtype(x, scale, layout.scale_zero_dim)
    dev = _compute_device(x, scale)
    xd, sd = _dev(x, dev), _dev(scale, dev)
    zd, zdt = _zp_arg(zero_point, dev)
    packed_cols = math.ceil(layout.cols * num_bits / 32)
    out = torch.empty((*x.shape[:-1], packed_cols), dtype=torch.int32, device=dev)
    largs, _keep = layout.args(dev)
    call("ct_quant_pack", ptr(xd), DT[xd.dtype], ptr(sd), DT[sd.dtype], ptr(zd), zdt, *largs, int(num_bits), DT[T],
         ptr(out), stream_of(xd))
    return _home(out, x)


def unpack_and_dequantize(packed, shape, scale, zero_point=None, *, num_bits, strategy=None, group_size=None,
                          block_structure=None, dtype=None, g_idx=None) -> torch.Tensor:
    """Fused unpack_from_int32 + dequantize (compressors/pack_quantized/base.py:155-161).
    `zero_point` is the UNPACKED int8 zero point (or None)."""
    if packed.dtype is not torch.int32:
        raise ValueError(f"Expected {torch.int32} but got {packed.dtype}, Aborting unpack.")
    if not 1 <= num_bits <= 8:
        raise ValueError(f"Unpacking is only supported for num_bits in [1, 8], got {num_bits}")
    _check_float(scale, "scale")
    shape = tuple(int(s) for s in shape)
    if strategy is None:
        strategy, group_size, block_structure = infer_dequant_layout(shape, scale)
    layout = QuantLayout(shape, scale, strategy, group_size, block_structure, g_idx)
    _check_sz(layout, scale, zero_point)
    out_dtype = dtype if dtype is not None else scale.dtype
    if out_dtype not in _FLOATS:
        raise NotImplementedError(f"dequantize to {out_dtype} is not supported by the MI355X path")
    dev = _compute_device(packed, scale)
    pd, sd = _dev(packed, dev), _dev(scale, dev)
    zd, zdt = _zp_arg(zero_point, dev)
    words = pd.shape[-1]
    if math.prod(pd.shape[:-1]) != layout.rows:
        raise ValueError(f"packed shape {tuple(pd.shape)} does not match weight shape {shape}")
    out = torch.empty(shape, dtype=out_dtype, device=dev)
    largs, _keep = layout.args(dev)
    rows, cols, rdiv, cdiv, scols, cg = largs
    call("ct_unpack_dequant", ptr(pd), rows, words, cols, int(num_bits), ptr(sd), DT[sd.dtype], ptr(zd), zdt, rdiv, cdiv,
         scols, cg, ptr(out), DT[out_dtype], stream_of(pd))
    return _home(out, packed)


def _w4_zp_fused_ok(x_or_packed, scale, zero_point, rows, cols, group) -> bool:
    """the layout ct_quant_pack_w4_zp / ct_unpack_dequant_w4_zp take: 2-D, 16-bit scale of shape (rows, cols / group), everything
    contiguous, 16-byte aligned and on one GPU"""
    if scale is None or scale.dtype not in (torch.bfloat16, torch.float16) or not scale.is_cuda or not x_or_packed.is_cuda:
        return False
    if cols % 32 or group % 32 or cols % group or rows <= 0:
        return False
    if tuple(scale.shape) != (rows, cols // group) or not scale.is_contiguous() or not x_or_packed.is_contiguous():
        return False
    if zero_point is None or zero_point.device != scale.device or not zero_point.is_contiguous() or x_or_packed.device != scale.device:
        return False
    return _aligned16(x_or_packed, scale, zero_point)


def quantize_and_pack_with_zp(x, scale, zero_point, *, num_bits, strategy, group_size=None):
    """PackedQuantizationCompressor.compress of an ASYMMETRIC int4 scheme in ONE launch (compressors/pack_quantized/base.py:96-110):
    returns (weight_packed int32 (R, C / 8), weight_zero_point int32 (ceil(R / 8), G) = pack_to_int32(zp, 4, packed_dim=0)), or None
    when the tensors are not the layout `ct_quant_pack_w4_zp` takes (the caller then composes quantize_and_pack + pack_to_int32)."""
    st = _strategy_name(strategy)
    if int(num_bits) != 4 or x.dim() != 2 or st not in ("group", "channel") or x.dtype not in (torch.bfloat16, torch.float16):
        return None
    rows, cols = int(x.shape[0]), int(x.shape[1])
    group = cols if st == "channel" else int(group_size or 0)
    if group <= 0 or zero_point is None or zero_point.dtype is not torch.int8 or scale is None or scale.dtype is not x.dtype:
        return None
    if not _w4_zp_fused_ok(x, scale, zero_point, rows, cols, group) or tuple(zero_point.shape) != tuple(scale.shape):
        return None
    packed = torch.empty((rows, cols // 8), dtype=torch.int32, device=x.device)
    zpp = torch.empty(((rows * 4 + 31) // 32, cols // group), dtype=torch.int32, device=x.device)
    call("ct_quant_pack_w4_zp", ptr(x), DT[x.dtype], ptr(scale), ptr(zero_point), rows, cols, group, ptr(packed), ptr(zpp), stream_of(x))
    return packed, zpp


def unpack_and_dequantize_with_zp(packed, shape, scale, zp_packed, *, num_bits, want_zero_point=True):
    """PackedQuantizationCompressor.decompress of an ASYMMETRIC int4 scheme in ONE launch (base.py:147-161): the zero points are read in
    their stored form.  Returns (weight of the scale's dtype, unpacked int8 zero point or None), or None when the tensors are not the
    layout `ct_unpack_dequant_w4_zp` takes (groups of 128, cols % 512 == 0, ...): the caller then unpacks the zero points first."""
    shape = tuple(int(v) for v in shape)
    if int(num_bits) != 4 or len(shape) != 2 or scale is None or scale.dim() != 2 or scale.shape[1] == 0 or packed.dtype is not torch.int32:
        return None
    rows, cols = shape
    if cols % scale.shape[1]:
        return None
    group = cols // scale.shape[1]
    if not w4_packed_zp_readable(cols, group) or rows * (cols // 8) >= 1 << 31 or zp_packed is None or zp_packed.dtype is not torch.int32:
        return None
    if tuple(zp_packed.shape) != ((rows * 4 + 31) // 32, scale.shape[1]) or tuple(packed.shape) != (rows, cols // 8):
        return None
    if not _w4_zp_fused_ok(packed, scale, zp_packed, rows, cols, group):
        return None
    out = torch.empty(shape, dtype=scale.dtype, device=packed.device)
    zp = torch.empty((rows, scale.shape[1]), dtype=torch.int8, device=packed.device) if want_zero_point else None
    call("ct_unpack_dequant_w4_zp", ptr(packed), ptr(scale), DT[scale.dtype], ptr(zp_packed), rows, cols, group, ptr(out), ptr(zp), stream_of(packed))
    return out, zp


def minmax_qparams(x, *, num_bits, group_size=None, symmetric=True):
    """Min-max observer + calculate_qparams (quantization/utils/helpers.py:50-137) over groups of
    `group_size` consecutive columns (None: the whole row).  Returns (scale x.dtype (R, G),
    zero_point int8 (R, G))."""
    _check_float(x, "weight")
    if x.ndim != 2:
        raise ValueError("minmax_qparams expects a 2-D weight")
    dev = _compute_device(x)
    xd = _dev(x, dev)
    rows, cols = xd.shape
    cdiv = int(group_size) if group_size else max(cols, 1)
    ng = math.ceil(cols / cdiv) if cols else 0
    scale = torch.empty((rows, ng), dtype=xd.dtype, device=dev)
    zp = torch.empty((rows, ng), dtype=torch.int8, device=dev)
    call("ct_minmax_qparams", ptr(xd), DT[xd.dtype], rows, cols, cdiv, int(num_bits), int(bool(symmetric)), ptr(scale),
         ptr(zp), stream_of(xd))
    return _home(scale, x), _home(zp, x)


# --------------------------------------------------------------------------- batched W4A16
_QP_KIND = {"fp8": 1, "nvfp4": 2, "mxfp4": 3, "mxfp8": 4}


def minmax_qparams_float(x, *, kind: str, group_size=None, global_scale=None) -> torch.Tensor:
    """Min-max observer + calculate_qparams for the symmetric FLOAT schemes (quantization/utils/helpers.py:50-137,
    mxfp_utils.py:37-143): kind "fp8" (scale in x.dtype), "nvfp4" (fp8-representable float32 scale under `global_scale`),
    "mxfp4" / "mxfp8" (power-of-two scale in x.dtype, group 32).  Returns the scale (R, G); the zero points of these schemes
    are zeros of the scheme's zp_dtype."""
    _check_float(x, "weight")
    if x.ndim != 2:
        raise ValueError("minmax_qparams_float expects a 2-D weight")
    if kind not in _QP_KIND:
        raise ValueError(f"unknown float qparams kind {kind!r}")
    if kind == "nvfp4" and global_scale is None:
        raise ValueError("nvfp4 scales need the global scale")
    dev = _compute_device(x)
    xd = _dev(x, dev)
    rows, cols = xd.shape
    cdiv = int(group_size) if group_size else max(cols, 1)
    ng = math.ceil(cols / cdiv) if cols else 0
    scale = torch.empty((rows, ng), dtype=torch.float32 if kind == "nvfp4" else xd.dtype, device=dev)
    gs = _gs_arg(global_scale, dev) if kind == "nvfp4" else None
    call("ct_minmax_qparams_float", ptr(xd), DT[xd.dtype], rows, cols, cdiv, _QP_KIND[kind], ptr(gs), ptr(scale), stream_of(xd))
    return _home(scale, x)


DYNAMIC_KINDS = {"int": 0, "fp8": 1, "nvfp4": 2, "mxfp4": 3, "mxfp8": 4}
_DYNAMIC_WORKSPACE_BYTES = 16384  # CT_DYNAMIC_WORKSPACE_BYTES of include/ct_hip.h


def dynamic_qdq(x: torch.Tensor, *, kind: str, segs: int, seg_len: int, num_bits: int = 8, symmetric: bool = True,
                global_scale: Optional[torch.Tensor] = None, scale_shape=None, scale_dtype=None, zp_dtype=None, want_out: bool = True):
    """Dynamic min-max observer + calculate_qparams + fake_quantize of a contiguous activation viewed as `segs` segments of
    `seg_len` elements, one scale each (ct_dynamic_qdq; segs == 1 with seg_len == numel is the two-launch tensor form,
    ct_dynamic_qdq_tensor).  Returns (out or None, scale or None, zero_point or None): `scale_shape` / `scale_dtype` /
    `zp_dtype` None means "not requested" (the kernel then keeps them in registers)."""
    _check_float(x, "activation")
    if not x.is_cuda or not x.is_contiguous():
        raise NotImplementedError("the dynamic QDQ kernels take contiguous GPU activations")
    dev = x.device
    out = torch.empty_like(x) if want_out else None
    scale = torch.empty(scale_shape, dtype=scale_dtype, device=dev) if scale_dtype is not None else None
    zp = torch.empty(scale_shape, dtype=zp_dtype, device=dev) if zp_dtype is not None else None
    zdt = DT[zp_dtype] if zp_dtype is not None else -1
    gs = _gs_arg(global_scale, dev)
    head = (ptr(x), DT[x.dtype])
    tail = (DYNAMIC_KINDS[kind], int(num_bits), int(bool(symmetric)), ptr(gs))
    if segs == 1 and seg_len == x.numel() and seg_len > 512:
        ws = torch.empty(_DYNAMIC_WORKSPACE_BYTES // 4, dtype=torch.int32, device=dev)
        call("ct_dynamic_qdq_tensor", *head, int(seg_len), *tail, ptr(ws), ptr(out), ptr(scale), ptr(zp), zdt, stream_of(x))
    else:
        call("ct_dynamic_qdq", *head, int(segs), int(seg_len), *tail, ptr(out), ptr(scale), ptr(zp), zdt, stream_of(x))
    return out, scale, zp


HADAMARD_MAX_SIZE = {torch.float32: 16384, torch.float64: 16384}  # kHadMaxF32 / kHadMaxF64 of csrc/ct_hadamard.h


class HadamardPlan(NamedTuple):
    """what `hadamard_transform` launches: form "rows" (ct_hadamard_rows over `numel` elements, the transformed dimension
    contiguous) or "cols" (ct_hadamard_cols along dim 0 of a rows x cols matrix), `blocks` independent blocks of `size`"""
    form: str
    size: int
    blocks: int
    acc64: bool
    rows: int
    cols: int

    @property
    def is_cols(self) -> bool:
        """the column form (HadamardKPlan answers the same question)"""
        return self.form == "cols"


def _plan_rotation_dims(what: str, shape, dtype, size: int, dim: int, precision, device_type: str, contiguous: bool):
    """What plan_hadamard and plan_hadamard_k share behind their own errors for `size`, in the order both raise: upstream's ValueError for a size that
    does not divide the dimension (transform/utils/matrix.py:41-45), then NotImplementedError for the precisions, dtypes, devices and layouts no
    rotation kernel takes.  Returns the shape as a tuple, the normalised dim, and outer, inner, numel around it."""
    shape = tuple(map(int, shape))
    if not shape:
        raise ValueError(f"{what} of a 0-dim tensor")
    if not -len(shape) <= dim < len(shape):
        raise IndexError(f"dim {dim} out of range for a {len(shape)}-dim tensor")
    dim %= len(shape)
    if shape[dim] % size != 0:
        raise ValueError(f"{size} must divide {shape[dim]} (dim {dim} of shape {shape})")
    if precision in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"precision {precision}: upstream would run its GEMM in that dtype, which no kernel here reproduces")
    if precision not in HADAMARD_MAX_SIZE:
        raise NotImplementedError(f"precision must be torch.float32 or torch.float64, got {precision}")
    if dtype not in _FLOATS:
        raise NotImplementedError(f"the hadamard kernels take bfloat16, float16 and float32 tensors, got {dtype}")
    if device_type != "cuda":
        raise NotImplementedError(f"the hadamard kernels take GPU tensors, got a {device_type} tensor")
    if not contiguous:
        raise NotImplementedError("the hadamard kernels take contiguous tensors")
    outer, inner = math.prod(shape[:dim]), math.prod(shape[dim + 1:])
    return shape, dim, outer, inner, outer * shape[dim] * inner


def _rotation_rows_or_cols(shape, dim: int, size: int, outer: int, inner: int, numel: int) -> tuple:
    """("rows" or "cols", blocks, rows, cols) of a rotation along `dim`: the row form when the transformed dimension is contiguous (a bias
    column (n, 1) included), the column form along dim 0 of one matrix"""
    if inner == 1 or size == 1:
        return "rows", numel // size, numel // max(shape[dim], 1), shape[dim]
    if outer != 1:
        raise NotImplementedError(f"the column form takes one matrix: dim {dim} of shape {shape} is neither the first nor the last dimension")
    return "cols", (shape[dim] // size) * inner, shape[dim], inner


def plan_hadamard(shape, dtype, size: int, dim: int = -1, precision=torch.float32, *, device_type: str = "cuda", contiguous: bool = True) -> HadamardPlan:
    """The host-side decision of `hadamard_transform`, from shapes and dtypes alone (no tensor data is touched): the form, the
    block count and the accumulator — or upstream's ValueError (transform/utils/hadamard.py:37-42, transform/utils/matrix.py:41-45)
    for a size that is not a positive power of two or does not divide the dimension, or NotImplementedError for what the
    kernels decline (a caller such as install() hands those to the reference)."""
    size = int(size)
    if size <= 0:
        raise ValueError("Cannot construct deterministic hadamard of size <= 0")
    if size & (size - 1):
        raise ValueError("Cannot construct deterministic hadamard of size != 2^n")
    shape, dim, outer, inner, numel = _plan_rotation_dims("hadamard_transform", shape, dtype, size, dim, precision, device_type, contiguous)
    if size > HADAMARD_MAX_SIZE[precision]:
        raise NotImplementedError(f"hadamard size {size} exceeds the supported maximum {HADAMARD_MAX_SIZE[precision]} at precision {precision}")
    form, blocks, rows, cols = _rotation_rows_or_cols(shape, dim, size, outer, inner, numel)
    return HadamardPlan(form, size, blocks, precision is torch.float64, rows, cols)


def _rotation_launch(x: torch.Tensor, had_k=None, k: int = 1, signs=None, n: int = 0, gathers=()):
    """What the three launch functions do between the plan and the call, in the order all three raise: the int8 tables `had_k` (k, k) and
    `signs` (n,) are what they must be (ValueError), a GPU is there and x is on it, the tables are on x's device (ValueError), x and the 16-bit
    `gathers` are 16-byte and signs 8-byte aligned (NotImplementedError).  Returns (out, launch): the empty output, and False for an empty x."""
    tables = () if had_k is None and signs is None else (("had_k", had_k, (k, k)), ("signs", signs, (n,)))
    for name, t, shape in tables:
        if t is not None and (t.dtype is not torch.int8 or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int8 tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
    _lib.require_device()
    if not x.is_cuda:
        raise NotImplementedError(f"the hadamard kernels take GPU tensors, got a {x.device.type} tensor")
    for name, t, _ in tables:
        if t is not None and t.device != x.device:
            raise ValueError(f"{name} is on {t.device}, the value on {x.device}")
    misaligned = x.data_ptr() % 16 or (signs is not None and signs.data_ptr() % 8)
    for g in gathers:
        misaligned = misaligned or g.data_ptr() % 16
    if misaligned:
        raise NotImplementedError("the hadamard kernels take 16-byte aligned tensors")
    return torch.empty_like(x), x.numel() != 0


def hadamard_transform(x: torch.Tensor, size: int, *, dim: int = -1, precision=torch.float32, perm: Optional["HadamardPermTables"] = None,
                       form: Optional[str] = None) -> torch.Tensor:
    """HadamardTransform.forward (transform/factory/hadamard.py:91-108) for the Sylvester matrix of
    deterministic_hadamard_matrix(size): every run of `size` elements along `dim` is multiplied by H_size / sqrt(size) (the
    block-diagonal `_multihead_matmul` of transform/utils/matrix.py:124-158 when the dimension is longer), accumulated in
    `precision` and rounded once to x's dtype.  A fast Walsh-Hadamard butterfly on the GPU: no matrix, no GEMM.  The matrix is
    symmetric, so `inverse=True` upstream is the same call.  dim == last (or any dimension followed only by 1s): one launch;
    dim == 0 of a matrix: ct_hadamard_cols.  `perm` (hadamard_perm_tables): the permuted rotation of `randomize=True`, see
    plan_hadamard_perm (`form` forces its "fused" or "composed" form)."""
    if perm is not None:
        return _hadamard_perm_transform(x, size, None, None, dim, precision, False, perm, form)
    plan = plan_hadamard(x.shape, x.dtype, size, dim, precision, contiguous=x.is_contiguous())
    out, launch = _rotation_launch(x)
    if not launch:
        return out
    if plan.form == "rows":
        call("ct_hadamard_rows", ptr(x), ptr(out), DT[x.dtype], x.numel(), plan.size, int(plan.acc64), stream_of(x))
    else:
        ws = torch.empty_like(x)
        call("ct_hadamard_cols", ptr(x), ptr(out), ptr(ws), DT[x.dtype], plan.rows, plan.cols, plan.size, int(plan.acc64), stream_of(x))
    return out


HADAMARD_K_MAX_K = 256  # kHadKMaxK of csrc/ct_hadamard_k.hip
HADAMARD_K_MAX_SIZE = 32768  # kHadKMfmaMaxN: the largest n = k * 2^m with k > 1
HADAMARD_K_MAX_RUN = 4096  # kHadKRunsMaxM: the longest run 2^m of the vector form
_HADAMARD_K_MAX_LDS = 65536  # kHadKMaxLds: the staged row of the matrix-core form


class HadamardKPlan(NamedTuple):
    """what `hadamard_k_transform` launches: `entry` "rows" (ct_hadamard_k_rows, the transformed dimension contiguous) or "cols"
    (ct_hadamard_k_cols along dim 0 of a rows x cols matrix) in `form` "butterfly" (k == 1: signs + the Walsh-Hadamard butterfly),
    "mfma" (one launch, the k x k mix on the matrix cores) or "valu" (two launches through a workspace); `workspace` in bytes"""
    entry: str
    form: str
    size: int
    k: int
    m: int
    blocks: int
    acc64: bool
    rows: int
    cols: int
    workspace: int

    @property
    def is_cols(self) -> bool:
        """the column form (HadamardPlan answers the same question)"""
        return self.entry == "cols"


def plan_hadamard_k(shape, dtype, size: int, k: int = 1, dim: int = -1, precision=torch.float32, *, device_type: str = "cuda",
                    contiguous: bool = True) -> HadamardKPlan:
    """The host-side decision of `hadamard_k_transform`, from shapes and dtypes alone: upstream's ValueErrors first (a size with
    no k * 2^m factorisation is the one `random_hadamard_matrix` raises, transform/utils/hadamard.py:127-128; a size that does not
    divide the dimension is transform/utils/matrix.py:41-45), then NotImplementedError for what the kernels of
    csrc/ct_hadamard_k.hip decline."""
    size, k = int(size), int(k)
    if size <= 0 or k <= 0 or size % k or (size // k) & (size // k - 1):
        raise ValueError(f"Cannot construct random hadamard matrix of size {size}")
    shape, dim, outer, inner, numel = _plan_rotation_dims("hadamard_k_transform", shape, dtype, size, dim, precision, device_type, contiguous)
    m, acc64 = size // k, precision is torch.float64
    if k == 1:
        form = "butterfly"
        if size > HADAMARD_MAX_SIZE[precision]:
            raise NotImplementedError(f"hadamard size {size} exceeds the supported maximum {HADAMARD_MAX_SIZE[precision]} at precision {precision}")
    else:
        if k > HADAMARD_K_MAX_K:
            raise NotImplementedError(f"the hadamard mix takes k <= {HADAMARD_K_MAX_K}, got {k}")
        if size > HADAMARD_K_MAX_SIZE:
            raise NotImplementedError(f"hadamard size {size} exceeds the supported maximum {HADAMARD_K_MAX_SIZE} of the mixed forms")
        lds = max(m, 32) * (-(-k // 16) * 16 + 8) * 2
        form = "mfma" if dtype is not torch.float32 and not acc64 and 8 <= m <= 128 and lds <= _HADAMARD_K_MAX_LDS else "valu"
        if form == "valu" and m > HADAMARD_K_MAX_RUN:
            raise NotImplementedError(f"the vector form of the hadamard mix takes runs of up to {HADAMARD_K_MAX_RUN} elements, got {m}")
    entry, blocks, rows, cols = _rotation_rows_or_cols(shape, dim, size, outer, inner, numel)
    workspace = numel * (8 if acc64 else 4) if form == "valu" else 0  # the accumulators of the vector form
    if entry == "cols":  # in front of them, the transposed tensor
        workspace += (numel * (4 if dtype is torch.float32 else 2) + 15) & ~15
    return HadamardKPlan(entry, form, size, k, m, blocks, acc64, rows, cols, workspace)


def hadamard_k_transform(x: torch.Tensor, n: int, had_k: Optional[torch.Tensor] = None, signs: Optional[torch.Tensor] = None, *, dim: int = -1,
                         precision=torch.float32, transposed: bool = False, perm: Optional["HadamardPermTables"] = None,
                         form: Optional[str] = None) -> torch.Tensor:
    """HadamardTransform.forward (transform/factory/hadamard.py:91-108) for the matrix of `random_hadamard_matrix(n)`
    (transform/utils/hadamard.py:53-151), W = diag(signs) * (had_k (x) H_M)^T with M = n / k a power of two: every run of n
    elements along `dim` becomes value @ W / sqrt(n) (`transposed=False`: the online locations, Embedding weight_output, Linear
    weight_output along dim 0) or value @ W.T / sqrt(n) (`transposed=True`), accumulated in `precision`, rounded once to x's
    dtype.  `had_k`: int8 (k, k) of +-1 on x's device, None for k == 1; `signs`: int8 (n,) of +-1, None for none.  No n x n
    matrix: signs, a Walsh-Hadamard butterfly over M and a k x k mix, which for 16-bit activations runs on the matrix cores in
    one launch (csrc/ct_hadamard_k.hip).  `perm` (hadamard_perm_tables): the weight W[p][:, p] of `randomize=True`, see
    plan_hadamard_perm (`form` forces its "fused" or "composed" form)."""
    if perm is not None:
        return _hadamard_perm_transform(x, n, had_k, signs, dim, precision, transposed, perm, form)
    k = 1 if had_k is None else int(had_k.shape[0])
    plan = plan_hadamard_k(x.shape, x.dtype, n, k, dim, precision, device_type=x.device.type, contiguous=x.is_contiguous())
    out, launch = _rotation_launch(x, had_k, k, signs, plan.size)
    if not launch:
        return out
    ws = torch.empty(plan.workspace, dtype=torch.uint8, device=x.device) if plan.workspace else None
    tail = (plan.size, plan.k, ptr(had_k), ptr(signs), int(bool(transposed)), int(plan.acc64), ptr(ws), stream_of(x))
    if plan.entry == "rows":
        call("ct_hadamard_k_rows", ptr(x), ptr(out), DT[x.dtype], x.numel(), *tail)
    else:
        call("ct_hadamard_k_cols", ptr(x), ptr(out), DT[x.dtype], plan.rows, plan.cols, *tail)
    return out


# ---- the permuted rotation of TransformScheme.randomize=True (csrc/ct_hadamard_perm.hip) ------------------------------------------------
# Upstream's permuted weight is W' = W[p][:, p] (transform/factory/hadamard.py:94-95), so for every location, module type and inverse
#     T_W'(x) = G_p(T_W(G_q(x)))   with G_i(v)[j] = v[i[j]] and q = argsort(p):
# gather every block by q, the unpermuted rotation, gather the result by p.  "fused" does that in one launch, "composed" with two
# index_select around the existing entry.
HADAMARD_PERM_MAX_SIZE = {torch.float32: 16384, torch.float64: 8192}  # kHadPMaxF32 / kHadPMaxF64 of csrc/ct_hadamard_perm.hip
_HADAMARD_PERM_MAX_TABLE = 32768  # what a non-negative 16-bit entry indexes

# Which fused forms the plan dispatches: a key is True only if every verdict of profiles/hadamard_perm_bench.jsonl that speaks for it
# says the one launch is faster than the composition by more than the spread between its runs (tools/hadamard_perm_bench.py;
# tests/test_hadamard_perm.py holds the constants to that file).  "group": n <= 512 (hadp_group_kernel), "block": n = 1024 .. 16384
# (hadp_block_kernel), each per accumulator; "cols": the column form around either — measured SLOWER than its composition, whose
# gathers along dim 0 move whole rows: it stays off.
HADAMARD_PERM_MEASURED_FASTER = {"group": True, "block": True, "group_f64": True, "block_f64": True, "cols": False}


class HadamardPermTables(NamedTuple):
    """a validated permutation p of 0 .. n - 1 on one device: `gather_out` = p and `gather_in` = q = argsort(p) as 16-bit tables
    (what ct_hadamard_perm_rows reads; None for n > 32768), `index_in` / `index_out` the same as int32 for index_select"""
    n: int
    gather_in: Optional[torch.Tensor]
    gather_out: Optional[torch.Tensor]
    index_in: torch.Tensor
    index_out: torch.Tensor


def hadamard_perm_tables(perm: torch.Tensor, device) -> HadamardPermTables:
    """The tables of one permutation for `device`.  Validates ONCE, on the host, that `perm` is a 1-D integer tensor holding every
    index 0 .. n - 1 exactly once (ValueError otherwise) and uploads q = argsort(perm) and perm; the calls that take the tables
    validate nothing and synchronise nothing."""
    if not isinstance(perm, torch.Tensor) or perm.dim() != 1 or perm.dtype.is_floating_point or perm.dtype.is_complex or perm.dtype is torch.bool:
        raise ValueError("perm must be a 1-D integer tensor")
    if perm.is_meta:
        raise ValueError("perm holds no data (a meta tensor)")
    p = perm.detach().to("cpu", torch.int64)
    n = int(p.numel())
    if n == 0:
        raise ValueError("perm is empty")
    if int(p.min()) < 0 or int(p.max()) >= n:
        raise ValueError(f"perm holds an index outside 0 .. {n - 1}")
    if not bool((torch.bincount(p, minlength=n) == 1).all()):
        raise ValueError(f"perm repeats an index: it is not a permutation of 0 .. {n - 1}")
    q = torch.empty_like(p)
    q[p] = torch.arange(n, dtype=torch.int64)
    device = torch.device(device)
    small = n <= _HADAMARD_PERM_MAX_TABLE
    return HadamardPermTables(n, q.to(torch.int16).to(device) if small else None, p.to(torch.int16).to(device) if small else None,
                              q.to(torch.int32).to(device), p.to(torch.int32).to(device))


class HadamardPermPlan(NamedTuple):
    """what a permuted rotation launches: `form` "fused" (ct_hadamard_perm_rows / ct_hadamard_perm_cols) or "composed"
    (index_select, the unpermuted entry of `base`, index_select); `key` of HADAMARD_PERM_MEASURED_FASTER that speaks for the fused
    form (None where there is none) and `reason` for a composed plan.  `launches()` counts the unpermuted entry as its own plan
    does: one call is one launch except the vector form of the mix (two) and the column forms (two transposes more)"""
    form: str
    base: tuple  # HadamardPlan (the `hadamard` type) or HadamardKPlan (`random-hadamard`)
    key: Optional[str]
    reason: Optional[str]

    def launches(self) -> int:
        if self.form == "fused":
            return 3 if self.base.is_cols else 1
        return 2 + (2 if self.base.form == "valu" else 1) + (2 if self.base.is_cols else 0)


def plan_hadamard_perm(shape, dtype, size: int, dim: int = -1, precision=torch.float32, *, k: int = 1, random: bool = False,
                       device_type: str = "cuda", contiguous: bool = True, form: Optional[str] = None) -> HadamardPermPlan:
    """The host-side decision of a permuted rotation, from shapes and dtypes alone.  First the errors and declines of the
    unpermuted plan, unchanged: plan_hadamard for the `hadamard` type, plan_hadamard_k for `random-hadamard` (`random=True`, or
    k > 1).  Then the form.  The fused launch exists for k == 1 and n up to HADAMARD_PERM_MAX_SIZE; it is dispatched where
    HADAMARD_PERM_MEASURED_FASTER says it was measured faster.  Everything else is the composition, which is available wherever the
    unpermuted plan is.  `form`: "fused" / "composed" force a form ("fused" raises NotImplementedError where no fused launch exists)."""
    if form not in (None, "fused", "composed"):
        raise ValueError(f"form must be None, 'fused' or 'composed', got {form!r}")
    k = int(k)
    if random or k != 1:
        base = plan_hadamard_k(shape, dtype, size, k, dim, precision, device_type=device_type, contiguous=contiguous)
    else:
        base = plan_hadamard(shape, dtype, size, dim, precision, device_type=device_type, contiguous=contiguous)
    key, reason = None, None
    if k != 1:
        reason = f"k = {k} > 1: the mix has no permuted launch"
    elif base.size > HADAMARD_PERM_MAX_SIZE[precision]:
        reason = f"hadamard size {base.size} exceeds the maximum {HADAMARD_PERM_MAX_SIZE[precision]} of the permuted launch at precision {precision}"
    else:
        key = "cols" if base.is_cols else ("group" if base.size <= 512 else "block") + ("_f64" if base.acc64 else "")
    if form == "fused" and key is None:
        raise NotImplementedError(f"no fused permuted launch: {reason}")
    if key is not None and form is None and not HADAMARD_PERM_MEASURED_FASTER[key]:
        reason = f"the {key} form is not measured faster than the composition (HADAMARD_PERM_MEASURED_FASTER)"
    fused = key is not None and (form == "fused" or (form is None and HADAMARD_PERM_MEASURED_FASTER[key]))
    return HadamardPermPlan("fused" if fused else "composed", base, key, None if fused else (reason or "forced"))


def _hadamard_perm_transform(x, n, had_k, signs, dim, precision, transposed, perm, form):
    """hadamard_transform / hadamard_k_transform with `perm`"""
    if not isinstance(perm, HadamardPermTables):
        raise ValueError("perm must be the HadamardPermTables of hadamard_perm_tables")
    if perm.n != int(n):
        raise ValueError(f"the permutation has {perm.n} entries, the rotation size is {int(n)}")
    k = 1 if had_k is None else int(had_k.shape[0])
    random = had_k is not None or signs is not None
    plan = plan_hadamard_perm(x.shape, x.dtype, n, dim, precision, k=k, random=random, device_type=x.device.type, contiguous=x.is_contiguous(), form=form)
    if perm.index_in.device != x.device:
        raise ValueError(f"the permutation tables are on {perm.index_in.device}, the value on {x.device}")
    d = dim % x.dim()
    if plan.form == "composed":
        g = x.unflatten(d, (-1, perm.n)).index_select(d + 1, perm.index_in).flatten(d, d + 1)
        y = hadamard_k_transform(g, n, had_k, signs, dim=dim, precision=precision, transposed=transposed) if random \
            else hadamard_transform(g, n, dim=dim, precision=precision)
        return y.unflatten(d, (-1, perm.n)).index_select(d + 1, perm.index_out).flatten(d, d + 1)
    out, launch = _rotation_launch(x, None, 1, signs, perm.n, (perm.gather_in, perm.gather_out))
    if not launch:
        return out
    base = plan.base
    tail = (base.size, int(base.acc64), ptr(perm.gather_in), ptr(perm.gather_out), ptr(signs), int(bool(transposed)), stream_of(x))
    if plan.key != "cols":
        call("ct_hadamard_perm_rows", ptr(x), ptr(out), DT[x.dtype], x.numel(), *tail)
    else:
        ws = torch.empty_like(x)
        call("ct_hadamard_perm_cols", ptr(x), ptr(out), ptr(ws), DT[x.dtype], base.rows, base.cols, *tail)
    return out


ROTATED_MAX_BLOCK = 8192  # kRotMaxBlock of csrc/ct_rotated.hip: the largest rotation block the fused launch takes (16384 measured slower)
ROTATED_MAX_ROW = 32768  # kSegMaxThreads * kSegUnits * 8 of csrc/ct_dynamic.h: the longest token row the staged form holds


def hadamard_dynamic_qdq(x: torch.Tensor, size: int, *, kind: str, seg_len: int, num_bits: int = 8, symmetric: bool = True,
                         global_scale: Optional[torch.Tensor] = None, scale_shape=None, scale_dtype=None, zp_dtype=None,
                         want_out: bool = True, want_rotated: bool = False):
    """`hadamard_transform(x, size)` (last dimension, float32 accumulation) followed by `dynamic_qdq` over segments of `seg_len`
    elements of the rotated tensor, in ONE launch (ct_hadamard_dynamic_qdq): the rotated tensor stays in registers unless
    `want_rotated` asks for it.  Returns (out or None, scale or None, zero_point or None, rotated or None), bit for bit what the two
    calls return; the library answers CT_ERR_UNSUPPORTED (NotImplementedError) for a combination it does not fuse —
    quantization.dynamic.plan_rotated_dynamic is the rule."""
    _check_float(x, "activation")
    _lib.require_device()
    if not x.is_cuda:
        raise NotImplementedError(f"the hadamard kernels take GPU tensors, got a {x.device.type} tensor")
    if not x.is_contiguous():
        raise NotImplementedError("the hadamard kernels take contiguous tensors")
    if x.data_ptr() % 16:
        raise NotImplementedError("the hadamard kernels take 16-byte aligned tensors")
    dev = x.device
    out = torch.empty_like(x) if want_out else None
    rotated = torch.empty_like(x) if want_rotated else None
    scale = torch.empty(scale_shape, dtype=scale_dtype, device=dev) if scale_dtype is not None else None
    zp = torch.empty(scale_shape, dtype=zp_dtype, device=dev) if zp_dtype is not None else None
    zdt = DT[zp_dtype] if zp_dtype is not None else -1
    gs = _gs_arg(global_scale, dev)
    call("ct_hadamard_dynamic_qdq", ptr(x), DT[x.dtype], x.numel(), int(size), int(seg_len), DYNAMIC_KINDS[kind], int(num_bits),
         int(bool(symmetric)), ptr(gs), ptr(rotated), ptr(out), ptr(scale), ptr(zp), zdt, stream_of(x))
    return out, scale, zp, rotated


def generate_gparam(x: torch.Tensor) -> torch.Tensor:
    """generate_gparam (quantization/utils/helpers.py:308-337) of a whole weight: 448 * 6 / amax evaluated in x's dtype
    exactly as the eager expression does on the CPU (`float / tensor` = reciprocal, then product: two roundings), float32
    (1,), non-finite -> 1.  The tensor-wide amax is the row-wise min-max kernel followed by a reduction of one value per row."""
    _check_float(x, "weight")
    x2 = x.reshape(-1, x.shape[-1]) if x.ndim != 2 else x
    dev = _compute_device(x2)
    xd = _dev(x2, dev)
    rows, cols = xd.shape
    if rows == 0 or cols == 0:
        raise ValueError("generate_gparam of an empty tensor")
    row_amax = torch.empty((rows, 1), dtype=xd.dtype, device=dev)
    gs = torch.empty(1, dtype=torch.float32, device=dev)
    # the row maxima, then ONE workgroup: amax -> clamp(min=tiny) -> reciprocal -> x 2688 -> non-finite = 1 (seven tiny tensor ops cost 45-65 us of launches here)
    call("ct_generate_gparam", ptr(xd), DT[xd.dtype], rows, cols, ptr(row_amax), ptr(gs), stream_of(xd))
    return _home(gs, x)


RTN_PACKW_BITS = (2, 3, 5, 6, 7)  # the widths of `ct_rtn_quant_pack_wb` and its table; 4 has `ct_rtn_quant_pack_w4`, 8 `rtn_quantize_group8(words=True)`


def _rtn_pack_bits(num_bits) -> int:
    """`num_bits` of `rtn_quantize_and_pack` / `rtn_quantize_and_pack_many`, checked before anything touches a device"""
    bits = int(num_bits)
    if bits == 4 or bits in RTN_PACKW_BITS:
        return bits
    if bits == 8:
        raise NotImplementedError("the one-pass pack-quantized compress of 8 bits is rtn_quantize_group8(words=True)")
    if bits == 1:
        raise NotImplementedError("1 bit has no one-pass compress; use minmax_qparams + quantize_and_pack")
    raise ValueError(f"num_bits must be in 1..8, got {num_bits}")


def rtn_quantize_and_pack(x: torch.Tensor, *, group_size: Optional[int] = None, symmetric: bool = True, num_bits: int = 4):
    """Round-to-nearest integer compress in ONE pass over the weight: min-max observer + calculate_qparams
    (quantization/utils/helpers.py:50-137) + quantize + pack_to_int32 (compressors/pack_quantized/base.py:96-104).
    Returns (packed int32 (R, C * num_bits / 32), scale (R, C/group) in x.dtype, zero_point int8 (R, C/group)) — bit-identical to
    `minmax_qparams` followed by `quantize_and_pack`.  group_size None = one group per row (channel).  num_bits 4 is
    `ct_rtn_quant_pack_w4`, 2 / 3 / 5 / 6 / 7 are `ct_rtn_quant_pack_wb`; 1 and 8 raise NotImplementedError naming what serves them."""
    bits = _rtn_pack_bits(num_bits)
    if x.dim() != 2:
        raise ValueError("rtn_quantize_and_pack expects a 2-D weight")
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"the one-pass compress takes 16-bit float weights, got {x.dtype}")
    rows, cols = x.shape
    group = int(group_size) if group_size else cols
    if group <= 0 or cols % group != 0:
        raise ValueError(f"tensor column shape must be divisble by the given group_size {group} but got {cols}")
    if group % 32 != 0 or group > 2048 or (group // 32) & (group // 32 - 1):
        raise NotImplementedError(f"the one-pass compress needs group sizes 32 * 2^k <= 2048, got {group}; use minmax_qparams + quantize_and_pack")
    dev = _compute_device(x)
    xd = _dev(x, dev).contiguous()
    packed = torch.empty((rows, cols * bits // 32), dtype=torch.int32, device=dev)
    scale = torch.empty((rows, cols // group), dtype=x.dtype, device=dev)
    zp = torch.empty((rows, cols // group), dtype=torch.int8, device=dev)
    if bits == 4:
        call("ct_rtn_quant_pack_w4", ptr(xd), DT[xd.dtype], rows, cols, group, int(bool(symmetric)), ptr(packed), ptr(scale), ptr(zp), stream_of(xd))
    else:
        call("ct_rtn_quant_pack_wb", ptr(xd), DT[xd.dtype], rows, cols, group, bits, int(bool(symmetric)), ptr(packed), ptr(scale), ptr(zp), stream_of(xd))
    return _home(packed, x), _home(scale, x), _home(zp, x)


def rtn_mxfp4_quantize_and_pack(x: torch.Tensor, *, return_scale: bool = False):
    """Round-to-nearest MXFP4 compress in ONE pass over the weight (group 32): min-max observer + calculate_qparams' MX
    branch + quantize + cast_to_fp4 + pack + compress_mx_scale.  Returns (packed uint8 (R, C/2), scale uint8 (R, C/32))
    [, the float scale in x.dtype] — bit-identical to minmax_qparams_float("mxfp4") -> fp4_quantize_and_pack ->
    compress_mx_scale."""
    if x.dim() != 2:
        raise ValueError("rtn_mxfp4_quantize_and_pack expects a 2-D weight")
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"the one-pass MXFP4 compress takes 16-bit float weights, got {x.dtype}")
    rows, cols = x.shape
    if cols % 32 != 0:
        raise ValueError(f"tensor column shape must be divisble by the given group_size 32 but got {cols}")
    dev = _compute_device(x)
    xd = _dev(x, dev).contiguous()
    packed = torch.empty((rows, cols // 2), dtype=torch.uint8, device=dev)
    code = torch.empty((rows, cols // 32), dtype=torch.uint8, device=dev)
    scale = torch.empty((rows, cols // 32), dtype=x.dtype, device=dev) if return_scale else None
    call("ct_rtn_mxfp4_quant_pack", ptr(xd), DT[xd.dtype], rows, cols, ptr(packed), ptr(code), ptr(scale), stream_of(xd))
    if return_scale:
        return _home(packed, x), _home(code, x), _home(scale, x)
    return _home(packed, x), _home(code, x)


def fp8block_to_mxfp4(weight: torch.Tensor, weight_scale_inv: torch.Tensor, *, weight_block_size=(128, 128), dtype: torch.dtype = torch.bfloat16):
    """An FP8 block-quantized weight (float8_e4m3fn (R, C), `weight_scale_inv` per block of `weight_block_size` or a torch broadcast of it) straight to
    MXFP4: (packed uint8 (R, C / 2), E8M0 codes uint8 (R, C / 32)), byte for byte `rtn_mxfp4_quantize_and_pack` of the weight dequantized to `dtype`
    (bfloat16 or float16), which is never materialised (`ct_fp8block_mxfp4_batch`; a block width that is no multiple of 32 takes the two launches).
    Host tensors in, host tensors out; device tensors stay on their device."""
    from .entrypoints.convert import fp8block_transcode as ft

    return ft.transcode_one(ft.MXFP4, "fp8block_to_mxfp4", weight, weight_scale_inv, weight_block_size, dtype)


def fp8block_to_mxfp8(weight: torch.Tensor, weight_scale_inv: torch.Tensor, *, weight_block_size=(128, 128), dtype: torch.dtype = torch.bfloat16):
    """`fp8block_to_mxfp4` for MXFP8: (float8_e4m3fn codes (R, C), E8M0 codes uint8 (R, C / 32)), byte for byte
    `rtn_quantize_group8(..., group_size=32, qtype="float", mx=True)` of the weight dequantized to `dtype`, which is never materialised
    (`ct_fp8block_mxfp8_batch`; a block width that is no multiple of 32 takes the two launches)."""
    from .entrypoints.convert import fp8block_transcode as ft

    return ft.transcode_one(ft.MXFP8, "fp8block_to_mxfp8", weight, weight_scale_inv, weight_block_size, dtype)


def fp8block_to_nvfp4(weight: torch.Tensor, weight_scale_inv: torch.Tensor, *, weight_block_size=(128, 128), dtype: torch.dtype = torch.bfloat16):
    """`fp8block_to_mxfp4` for NVFP4: (packed uint8 (R, C / 2), float8_e4m3fn scales (R, C / 16), float32 (1,) global scale), byte for byte
    `rtn_nvfp4_quantize_and_pack` of the weight dequantized to `dtype`, which is never materialised (`ct_fp8block_nvfp4_amax_batch` and
    `ct_fp8block_nvfp4_batch`; a block width that is no multiple of 16 takes the composition)."""
    from .entrypoints.convert import fp8block_transcode as ft

    return ft.transcode_one(ft.NVFP4, "fp8block_to_nvfp4", weight, weight_scale_inv, weight_block_size, dtype)


def nvfp4_to_mxfp4(weight_packed: torch.Tensor, weight_scale: torch.Tensor, weight_global_scale: torch.Tensor):
    """An NVFP4 weight (nibbles uint8 (R, C / 2), float8_e4m3fn scales (R, C / 16), one global scale) straight to MXFP4: (packed uint8 (R, C / 2),
    E8M0 codes uint8 (R, C / 32)), byte for byte `rtn_mxfp4_quantize_and_pack` of the bfloat16 weight the NVFP4 decompress yields, which is never
    materialised (`ct_nvfp4_mxfp4_batch`; a global scale that is not float32 or a misaligned device tensor takes the two launches).
    Host tensors in, host tensors out; device tensors stay on their device."""
    from .entrypoints.convert import nvfp4_mxfp4 as nm

    return nm.transcode_one(weight_packed, weight_scale, weight_global_scale)


def rtn_nvfp4_quantize_and_pack(x: torch.Tensor, global_scale: Optional[torch.Tensor] = None, *, return_scale: bool = False):
    """Round-to-nearest NVFP4 compress (groups of 16): generate_gparam of the weight unless `global_scale` is given, then ONE
    pass: min-max observer + calculate_qparams (float8 scales under the global scale) + quantize + cast_to_fp4 + pack.
    Returns (packed uint8 (R, C/2), scale float8_e4m3fn (R, C/16), global_scale float32 (1,)) [, the float32 scales]."""
    if x.dim() != 2:
        raise ValueError("rtn_nvfp4_quantize_and_pack expects a 2-D weight")
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"the one-pass NVFP4 compress takes 16-bit float weights, got {x.dtype}")
    rows, cols = x.shape
    if cols % 32 != 0:
        raise NotImplementedError(f"the one-pass NVFP4 compress needs cols % 32 == 0, got {cols}; use minmax_qparams_float + fp4_quantize_and_pack")
    dev = _compute_device(x)
    xd = _dev(x, dev).contiguous()
    gs = generate_gparam(xd) if global_scale is None else _gs_arg(global_scale, dev)
    packed = torch.empty((rows, cols // 2), dtype=torch.uint8, device=dev)
    s8 = torch.empty((rows, cols // 16), dtype=torch.float8_e4m3fn, device=dev)
    scale = torch.empty((rows, cols // 16), dtype=torch.float32, device=dev) if return_scale else None
    call("ct_rtn_nvfp4_quant_pack", ptr(xd), DT[xd.dtype], rows, cols, ptr(gs), ptr(packed), ptr(s8), ptr(scale), stream_of(xd))
    out = (_home(packed, x), _home(s8, x), _home(gs, x))
    return out + (_home(scale, x),) if return_scale else out


RTN_CHANNEL8_MAX_COLS = 65536  # CT_RTN_CHANNEL8_MAX_COLS of include/ct_hip.h


def rtn_channel8_form(shape, symmetric: bool = True) -> str:
    """the form `ct_rtn_quant_channel8` and its table's plan (`ct_rtn_channel8_batch_plan`) give a weight of this shape: "wave" (a wave per row: rows
    of at most 2048 columns, asymmetric ones up to 8192), "row" (a workgroup per row, up to 16384 columns) or "long" (up to
    `RTN_CHANNEL8_MAX_COLS`: the row's tail streamed twice); "" for what the plan refuses — not 2-D, empty, cols % 8, cols above the maximum"""
    if len(shape) != 2:
        return ""
    rows, cols = int(shape[0]), int(shape[1])
    if rows <= 0 or cols <= 0 or cols % 8 or cols > RTN_CHANNEL8_MAX_COLS:
        return ""
    upr = cols // 8
    if (not symmetric or upr <= 256) and upr <= 1024:
        return "wave"
    return "row" if upr <= 2048 else "long"


def rtn_quantize_channel8(x: torch.Tensor, *, qtype: str = "int", symmetric: bool = True):
    """Channel-wise 8-bit round-to-nearest in ONE pass over the weight: per-row min-max observer + calculate_qparams +
    quantize to int8 (qtype "int") or float8_e4m3fn ("float").  Returns (codes (R, C), scale (R, 1) in x.dtype, zero_point):
    the zero point is int8 (R, 1) for INT, float8 zeros for FLOAT — bit-identical to the observer kernel followed by
    quantize_tensor.  Rows of up to `RTN_CHANNEL8_MAX_COLS` columns (`rtn_channel8_form`)."""
    if x.dim() != 2:
        raise ValueError("rtn_quantize_channel8 expects a 2-D weight")
    qtype = getattr(qtype, "value", qtype)
    if x.dtype not in (torch.bfloat16, torch.float16) or x.shape[1] % 8 != 0 or x.shape[1] > RTN_CHANNEL8_MAX_COLS or (qtype == "float" and not symmetric):
        raise NotImplementedError(f"the one-pass channel-wise compress takes 16-bit weights with cols % 8 == 0 and cols <= {RTN_CHANNEL8_MAX_COLS} "
                                  "(symmetric for FLOAT)")
    rows, cols = x.shape
    dev = _compute_device(x)
    xd = _dev(x, dev).contiguous()
    fp8 = qtype == "float"
    out = torch.empty((rows, cols), dtype=_F8 if fp8 else torch.int8, device=dev)
    scale = torch.empty((rows, 1), dtype=x.dtype, device=dev)
    zp = torch.zeros((rows, 1), dtype=_F8, device=dev) if fp8 else torch.empty((rows, 1), dtype=torch.int8, device=dev)
    call("ct_rtn_quant_channel8", ptr(xd), DT[xd.dtype], rows, cols, int(fp8), int(bool(symmetric)), ptr(out), ptr(scale), None if fp8 else ptr(zp), stream_of(xd))
    return _home(out, x), _home(scale, x), _home(zp, x)


def rtn_block8_group(shape, block_structure) -> int:
    """the table's `group` — -((bh << 24) | bw), as the 8-bit tables encode blocks (`q8_batch_group`) — when `ct_rtn_quant_block8` and its table
    form take a weight of this shape under this block structure: 2-D, rows > 0, bh and bw powers of two, bw >= 16, bh * bw <= 16384,
    cols % bw == 0 (the last row of blocks may be ragged); else 0"""
    if len(shape) != 2 or block_structure is None or len(block_structure) != 2:
        return 0
    rows, cols, bh, bw = int(shape[0]), int(shape[1]), int(block_structure[0]), int(block_structure[1])
    if rows <= 0 or cols <= 0 or bh < 1 or bw < 16 or bh & (bh - 1) or bw & (bw - 1) or bh * bw > 16384 or cols % bw:
        return 0
    return -((bh << 24) | bw)


def rtn_quantize_block8(x: torch.Tensor, *, block_structure, qtype: str = "float", symmetric: bool = True, codes: bool = True):
    """Block-wise 8-bit round-to-nearest in ONE pass over the weight (FP8_BLOCK; INT8 blocks): the min-max observer over blocks of
    `block_structure` = [bh, bw] elements + calculate_qparams + quantize to float8_e4m3fn (qtype "float") or int8 ("int").  Returns (codes (R, C),
    scale (ceil(R / bh), C / bw) in x.dtype, zero_point of the scale's shape: int8 for INT, float8 zeros for FLOAT) — bit-identical to
    `calculate_qparams_from_weight`'s fallback composition followed by `quantize_tensor`.  `codes=False`: the block observer alone, (None, scale,
    zero_point).  Raises NotImplementedError for what the kernel's plan refuses (`rtn_block8_group`; float32 weights)."""
    if x.dim() != 2:
        raise ValueError("rtn_quantize_block8 expects a 2-D weight")
    qtype = getattr(qtype, "value", qtype)
    if x.dtype not in (torch.bfloat16, torch.float16) or not rtn_block8_group(x.shape, block_structure) or (qtype == "float" and not symmetric):
        raise NotImplementedError("the one-pass block-wise compress takes 16-bit weights and blocks with power-of-two sides, a width >= 16 that divides "
                                  "cols and at most 16384 elements (symmetric for FLOAT)")
    rows, cols = x.shape
    bh, bw = int(block_structure[0]), int(block_structure[1])
    dev = _compute_device(x)
    xd = _dev(x, dev).contiguous()
    fp8 = qtype == "float"
    grid = (-(-rows // bh), cols // bw)
    out = torch.empty((rows, cols), dtype=_F8 if fp8 else torch.int8, device=dev) if codes else None
    scale = torch.empty(grid, dtype=x.dtype, device=dev)
    zp = torch.zeros(grid, dtype=_F8, device=dev) if fp8 else torch.empty(grid, dtype=torch.int8, device=dev)
    call("ct_rtn_quant_block8", ptr(xd), DT[xd.dtype], rows, cols, bh, bw, int(fp8), int(bool(symmetric)), ptr(out), ptr(scale), None if fp8 else ptr(zp),
         stream_of(xd))
    return (_home(out, x) if codes else None), _home(scale, x), _home(zp, x)


_RTN_GROUP8_MAX = 1024  # one wave reduces a group: 64 lanes of 16 elements (ct_rtn_group8_batch_plan)
_QP_INT, _QP_FP8, _QP_MXFP8 = 0, 1, 4  # the observer's kinds (csrc/ct_minmax.h)


def rtn_group8_group(shape, group_size) -> int:
    """the group (elements per scale) when `ct_rtn_quant_group8` and its table form take a weight of this shape — 2-D, rows > 0, a group of
    32 * 2^k <= 1024 columns that divides the row (group_size None / 0: the whole row as one group) — else 0"""
    if len(shape) != 2 or int(shape[0]) <= 0 or int(shape[1]) <= 0:
        return 0
    cols = int(shape[1])
    g = int(group_size) if group_size else cols
    if g <= 0 or cols % g or g % 32 or g > _RTN_GROUP8_MAX or (g // 32) & (g // 32 - 1):
        return 0
    return g


def _rtn_group8_kind(qtype, symmetric: bool, mx: bool, words: bool) -> int:
    qtype = getattr(qtype, "value", qtype)
    if qtype not in ("int", "float"):
        raise ValueError(f"qtype must be 'int' or 'float', got {qtype!r}")
    if qtype == "int" and mx:
        raise ValueError("MX scales belong to the FLOAT scheme")
    if qtype == "float" and (not symmetric or words):
        raise NotImplementedError("FLOAT 8-bit round-to-nearest is symmetric and has no word form")
    return _QP_INT if qtype == "int" else _QP_MXFP8 if mx else _QP_FP8


def rtn_quantize_group8(x: torch.Tensor, *, group_size, qtype: str = "int", symmetric: bool = True, mx: bool = False, words: bool = False):
    """Group-wise 8-bit round-to-nearest in ONE pass over the weight (MXFP8, W8A16, any FLOAT / INT 8-bit group scheme): the min-max observer
    over groups of `group_size` columns (None: the row) + calculate_qparams + quantize to int8 (qtype "int") or float8_e4m3fn ("float").
    Returns (codes (R, C), scale (R, C / g) in x.dtype, zero_point) and, with `mx` (FLOAT, g == 32), the E8M0 codes uint8 (R, C / 32) as a
    fourth entry: the zero point is int8 for INT and None for FLOAT.  `words` (INT): the codes are the (code + 128) bytes of pack-quantized's
    8-bit words, as int32 (R, C / 4).  Bit-identical to `minmax_qparams` / `minmax_qparams_float` followed by `quantize_tensor` /
    `quantize_and_pack` (and `compress_mx_scale`).  Raises the reference's ValueError for cols % g != 0 and NotImplementedError for what the
    kernel's plan refuses (`rtn_group8_group`; float32 weights)."""
    if x.dim() != 2:
        raise ValueError("rtn_quantize_group8 expects a 2-D weight")
    kind = _rtn_group8_kind(qtype, symmetric, mx, words)
    rows, cols = x.shape
    g = int(group_size) if group_size else cols
    if g <= 0 or cols % g != 0:
        raise ValueError(f"tensor column shape must be divisble by the given group_size {g} but got {cols}")
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"the one-pass group-wise compress takes 16-bit float weights, got {x.dtype}")
    if rows and cols and not rtn_group8_group(x.shape, g):
        raise NotImplementedError(f"the one-pass group-wise compress needs group sizes 32 * 2^k <= {_RTN_GROUP8_MAX}, got {g}")
    if mx and g != 32:
        raise NotImplementedError(f"MXFP8 groups hold 32 elements, got {g}")
    dev = _compute_device(x)
    xd = _dev(x, dev).contiguous()
    if xd.data_ptr() % 16:
        xd = xd.clone()
    fp8 = kind != _QP_INT
    out = torch.empty((rows, cols // 4), dtype=torch.int32, device=dev) if words else torch.empty((rows, cols), dtype=_F8 if fp8 else torch.int8, device=dev)
    scale = torch.empty((rows, cols // g), dtype=x.dtype, device=dev)
    zp = None if fp8 else torch.empty((rows, cols // g), dtype=torch.int8, device=dev)
    code = torch.empty((rows, cols // g), dtype=torch.uint8, device=dev) if mx else None
    lut = _mx_code_table(x.dtype, dev) if mx else None  # read for an inf / NaN scale only: the byte `compress_mx_scale` gives it
    call("ct_rtn_quant_group8", ptr(xd), DT[xd.dtype], rows, cols, g, kind, int(bool(symmetric)), int(bool(words)), ptr(out), ptr(scale), ptr(zp), ptr(code),
         ptr(lut), stream_of(xd))
    got = (_home(out, x), _home(scale, x), None if fp8 else _home(zp, x))
    return got + (_home(code, x),) if mx else got


def _aligned16(*tensors) -> bool:
    return all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


def w4_batch_eligible(weight_shape, w_dtype, scale, zero_point, *, num_bits, strategy, group_size, g_idx=None, device=None) -> bool:
    """can this tensor join a one-launch W4 batch (`ct_quant_pack_batch` / `ct_unpack_dequant_batch`)?
    int4, 2-D 16-bit weights and scales of the same dtype on the same GPU (`device`: where the weight / packed words
    live), group or channel scales with cols % 32 == 0 and group % 32 == 0, int8 (or no) zero point, 16-byte aligned
    parameters, no activation ordering.  Anything else takes the per-module path."""
    if num_bits != 4 or g_idx is not None or len(weight_shape) != 2:
        return False
    if w_dtype not in (torch.bfloat16, torch.float16) or scale is None or scale.dtype != w_dtype or not scale.is_cuda:
        return False
    if device is not None and (scale.device != device or (zero_point is not None and zero_point.device != device)):
        return False
    if not _aligned16(scale, zero_point):
        return False
    rows, cols = int(weight_shape[0]), int(weight_shape[1])
    st = _strategy_name(strategy)
    if st == "channel":
        g = cols
    elif st == "group" and group_size:
        g = int(group_size)
    else:
        return False
    if rows <= 0 or cols % 32 or g % 32 or cols % g:
        return False
    if tuple(scale.shape) != (rows, cols // g) or not scale.is_contiguous():
        return False
    if zero_point is not None and (zero_point.dtype != torch.int8 or tuple(zero_point.shape) != tuple(scale.shape)
                                   or not zero_point.is_contiguous() or not zero_point.is_cuda):
        return False
    return True


def _upload_table(words, dev) -> torch.Tensor:
    """a host table of int64 words (an `array.array("q")` or a CPU int64 tensor) -> device bytes.  The staging buffer is pinned
    (PyTorch's caching host allocator hands the block out again only after the copy's stream event has completed), so the copy is
    asynchronous: no blocking pageable H2D (25-30 us per table before) on the path of a launch"""
    import ctypes

    if isinstance(words, torch.Tensor):
        src, nbytes = words.data_ptr(), 8 * words.numel()
    else:
        src, nbytes = words.buffer_info()[0], 8 * len(words)
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) if dev.type == "cuda" else torch.empty(nbytes, dtype=torch.uint8)
    ctypes.memmove(host.data_ptr(), src, nbytes)
    return host.to(dev, non_blocking=True)


# --------------------------------------------------------------------------- table launches
_ITEM_WORDS = _lib.ITEM_WORDS  # struct ct_w4_item of include/ct_hip.h in 64-bit words: 4 pointers, rows, cols, group, first_block, units,
#                                {upg_shift, upg}, zp_packed, main_blocks, {g_magic, g_shift}
# a row is its eight settable fields and a zero, picked into word order; the order comes from the struct itself, so the next field added to
# ct_w4_item moves words here and nowhere else
_ITEM_FIELDS = ("src", "scale", "zp", "dst", "rows", "cols", "group", "zp_packed")
_ITEM_AT = {getattr(_lib.W4Item, name).offset // 8: i for i, name in enumerate(_ITEM_FIELDS)}
_pick_row = operator.itemgetter(*(_ITEM_AT.get(word, len(_ITEM_FIELDS)) for word in range(_ITEM_WORDS)))


def _word(v) -> int:
    return 0 if v is None else v.data_ptr() if isinstance(v, torch.Tensor) else int(v)


def item_row(src=0, scale=0, zp=0, dst=0, rows=0, cols=0, group=0, zp_packed=0) -> tuple:
    """one row of a host table of `struct ct_w4_item`, as `_ITEM_WORDS` ints.  The pointer arguments are ints, tensors (their `data_ptr()`) or
    None (0); the derived words (first_block, units, {upg_shift, upg}, main_blocks, {g_magic, g_shift}) are zero: the library's plan fills them.
    (The module loops build a row per module beside ~10 us of other host work: with ints given by position this is one test and one C call.)"""
    if not (type(src) is int and type(scale) is int and type(zp) is int and type(dst) is int and type(zp_packed) is int):
        src, scale, zp, dst, zp_packed = map(_word, (src, scale, zp, dst, zp_packed))
    return _pick_row((src, scale, zp, dst, rows, cols, group, zp_packed, 0))


# table kind -> (plan symbol, the plan takes a third argument, launch symbol | the launch symbols `d` of `_run_table` picks from — (compress, decompress), or
# the (fold, quantize) passes that ONE plan of "rtn_nvfp4" serves over the same rows): every table of ct_w4_item rows.  The plan's third argument is `d`:
# the direction, or for "rtn_wb" the WIDTH of the table's words
_TABLES = {
    "w4": ("ct_w4_batch_plan", True, ("ct_quant_pack_batch", "ct_unpack_dequant_batch")),
    "q8": ("ct_q8_batch_plan", True, ("ct_q8_quant_batch", "ct_q8_dequant_batch")),
    "fp4": ("ct_fp4_batch_plan", True, ("ct_fp4_quant_pack_batch", "ct_fp4_unpack_dequant_batch")),
    "mx_scale": ("ct_mx_scale_batch_plan", False, "ct_mx_scale_batch"),
    "zp4": ("ct_zp4_batch_plan", False, "ct_zp4_pack_dim0_batch"),
    "rtn_w4": ("ct_rtn_w4_batch_plan", False, "ct_rtn_quant_pack_w4_batch"),
    "rtn_mxfp4": ("ct_rtn_mxfp4_batch_plan", False, "ct_rtn_mxfp4_quant_pack_batch"),
    "rtn_nvfp4": ("ct_rtn_nvfp4_batch_plan", False, ("ct_rtn_nvfp4_amax_batch", "ct_rtn_nvfp4_quant_pack_batch")),
    "rtn_block8": ("ct_rtn_block8_batch_plan", False, "ct_rtn_quant_block8_batch"),
    "rtn_group8": ("ct_rtn_group8_batch_plan", False, "ct_rtn_quant_group8_batch"),
    "rtn_channel8": ("ct_rtn_channel8_batch_plan", False, "ct_rtn_quant_channel8_batch"),
    "rtn_wb": ("ct_rtn_wb_batch_plan", True, "ct_rtn_quant_pack_wb_batch"),
}
_Q8_KINDS = {"int8": 0, "fp8": 1, "fp8z": 2}  # the `kind` argument of the 8-bit tables' launches; fp8z: float8 codes with float8 zero points


def _q8_scalars(dt: int, kind: int, bits: int, d: int) -> tuple:
    """the scalar arguments of the 8-bit tables' launches: only the compress takes the INT scheme's num_bits"""
    return (dt, kind, bits) if d == 0 else (dt, kind)


def _plan_table(kind: str, words, n: int, device, d: int = 0):
    """the first half of `_launch_table`: plan `words` in place and upload them -> (device table, workgroups)"""
    plan, directed, _ = _TABLES[kind]
    if isinstance(words, list):
        words = array.array("q", words)
    addr = words.data_ptr() if isinstance(words, torch.Tensor) else words.buffer_info()[0]
    fn = getattr(_lib.load(), plan)
    blocks = int(fn(addr, n, d) if directed else fn(addr, n))
    if blocks < 0:
        raise ValueError(_lib.last_error())
    return _upload_table(words, device), blocks


def _run_table(kind: str, table, n: int, blocks: int, device, d: int, scalars, stream=None) -> None:
    """the second half: ONE launch of a planned, uploaded table"""
    symbol = _TABLES[kind][2]
    call(symbol if isinstance(symbol, str) else symbol[d], table.data_ptr(), n, blocks, *scalars, _lib.stream_on(device, stream))


def _launch_table(kind: str, words, n: int, device, d: int = 0, scalars=(), stream=None):
    """plan, upload and launch one table of `struct ct_w4_item` rows (`kind`: a name of `_TABLES`): `words` is `n` rows (`item_row`) as a flat CPU int64 tensor or an
    `array.array("q")`, planned in place, or as a flat list of ints, copied into one; `d`: 0 compress / pack, 1 decompress / unpack (handed to the
    plans that take it, and picking the launch of the kinds that have two; the width of an "rtn_wb" table); `scalars`: the launch's arguments between the workgroup count and the stream; `stream`: a raw hipStream_t of `device` (default:
    the caller's current stream there).  Returns the device table, or None for an empty one, before touching the library.

    Lifetime, for every entry point built on this: the caller keeps the tensors the rows point at alive.  The device table is allocated and
    uploaded on the current stream, whatever `stream` is: a caller that launches on another stream orders that stream behind the current one first
    (`wait_stream`).  One that stays on the current stream may drop the table at once — the `launch_*_words` of the C++ host loops do, and
    return nothing.  `launch_rtn_w4_words` / `launch_rtn_mxfp4_words` / `launch_rtn_nvfp4_words` hand the table back and the caller owes it a `record_stream` when its stream
    is not the allocator's; `zp4_batch` records it itself; `W4Batch` keeps it for as long as the batch lives."""
    if not n:
        return None
    table, blocks = _plan_table(kind, words, n, device, d)
    _run_table(kind, table, n, blocks, device, d, scalars, stream)
    return table


def launch_w4_words(words: torch.Tensor, n: int, direction: str, dtype: torch.dtype, device: torch.device) -> None:
    """a W4 table that already exists as a flat CPU int64 tensor of `struct ct_w4_item` words (built by the C++ host loop,
    csrc/host/ct_hostpath.cpp) in ONE launch (`ct_quant_pack_batch` / `ct_unpack_dequant_batch`) on `device`'s current stream"""
    if n:
        _launch_table("w4", words, n, device, 0 if direction == "compress" else 1, (DT[dtype],))


def launch_q8_words(words: torch.Tensor, n: int, direction: str, dtype: torch.dtype, device: torch.device, kind: int, bits: int = 8) -> None:
    """`launch_w4_words` for a table of the 8-bit codecs (`ct_q8_quant_batch` / `ct_q8_dequant_batch`); kind 0 int8, 1 fp8, 2 fp8 with float8 zero points"""
    d = 0 if direction == "compress" else 1
    if n:
        _launch_table("q8", words, n, device, d, _q8_scalars(DT[dtype], kind, bits, d))


def launch_fp4_words(words: torch.Tensor, n: int, direction: str, device: torch.device, group: int, x_dtype=None, scale_dtype=None) -> None:
    """`launch_w4_words` for a table of FP4 tensors (`ct_fp4_quant_pack_batch` / `ct_fp4_unpack_dequant_batch`): group 16 = NVFP4 (every item carries its global
    scale), 32 = MXFP4; compress: the weights' and the float scales' dtype (one per table); decompress writes bfloat16"""
    if not n:
        return
    if direction == "compress":
        lut = _mx_code_table(scale_dtype, device) if group == 32 else None
        _launch_table("fp4", words, n, device, 0, (DT[x_dtype], DT[scale_dtype], int(group), ptr(lut)))
    else:
        _launch_table("fp4", words, n, device, 1, (int(group), DT[torch.bfloat16]))


def launch_mx_scale_words(words: torch.Tensor, n: int, direction: str, device: torch.device, scale_dtype=None) -> None:
    """a table of MX scale tensors in ONE launch (`ct_mx_scale_batch`): "compress" 16-bit scales -> E8M0 codes, "decompress" codes -> bfloat16"""
    if not n:
        return
    if direction == "compress":
        _launch_table("mx_scale", words, n, device, 0, (0, DT[scale_dtype], ptr(_mx_code_table(scale_dtype, device))))
    else:
        _launch_table("mx_scale", words, n, device, 1, (1, -1, None))


def launch_zp4_words(words: torch.Tensor, n: int, direction: str, device: torch.device) -> None:
    """`zp4_batch` for a table that already exists as a flat CPU int64 tensor (src, dst, unpacked rows, cols per item; built by the C++ host
    loop): ONE `ct_zp4_pack_dim0_batch` launch on `device`'s current stream"""
    d = 0 if direction == "pack" else 1
    _launch_table("zp4", words, n, device, d, (d,))


def w4_packed_zp_readable(cols: int, group: int) -> bool:
    """can the W4 decompress kernels take this tensor's zero points in their STORED (packed) form? (include/ct_hip.h, ct_w4_item.zp_packed:
    groups of 128, whole waves per row)"""
    return group == 128 and cols % 512 == 0


class W4Batch:
    """A table of tensors processed by ONE kernel launch per direction — the per-module loop of ModelCompressor without a
    launch (and a ~5 us host call) per module.

    entries: (src, scale, zero_point or None, dst, rows, cols, group[, zp_packed or None]) with src / dst in the order the direction needs
    ("compress": weight -> codes).  `zp_packed` ("w4" only; round 6): the int32 (ceil(rows / 8), cols / group) STORED form of an
    asymmetric scheme's zero points, written ("compress", beside the int8 `zero_point` that is quantized against) or read
    ("decompress": the kernel takes the zero points from it and fills `zero_point`, if given, with the unpacked int8) by the SAME launch.  kind "w4": W4A16 pack-quantized (`ct_quant_pack_batch` / `ct_unpack_dequant_batch`,
    dst / src = packed int32 words); kind "int8" / "fp8": the 8-bit codecs (`ct_q8_quant_batch` / `ct_q8_dequant_batch`, one
    byte per element, `bits` = the INT scheme's num_bits; group may be rows * cols for a per-tensor scale).

    The host table is one flat array of 64-bit words (`item_row` per entry, the layout of `struct ct_w4_item`) planned in place by the
    library and uploaded asynchronously from pinned memory when the batch is built; `launch` may then be called any number of times."""

    def __init__(self, entries, direction: str, dtype: torch.dtype, kind: str = "w4", bits: int = 8):
        assert direction in ("compress", "decompress") and (kind == "w4" or kind in _Q8_KINDS)
        self.direction = 0 if direction == "compress" else 1
        self.kind, self.bits = kind, int(bits)
        self.dt = DT[dtype]
        self.keep = entries if isinstance(entries, list) else list(entries)  # the table holds raw pointers: keep the tensors alive
        n = self.n = len(self.keep)
        self.blocks, self.table, self.device = 0, None, None
        if n:
            flat = []
            for e in self.keep:
                flat += item_row(*e)  # an entry is item_row's arguments, in order
            self.device = self.keep[0][0].device
            self.table, self.blocks = _plan_table("w4" if kind == "w4" else "q8", flat, n, self.device, self.direction)

    def launch(self, stream=None):
        """`stream`: a raw hipStream_t of self.device (default: the caller's current stream there)"""
        if not self.n:
            return
        if self.kind == "w4":
            _run_table("w4", self.table, self.n, self.blocks, self.device, self.direction, (self.dt,), stream)
        else:
            _run_table("q8", self.table, self.n, self.blocks, self.device, self.direction, _q8_scalars(self.dt, _Q8_KINDS[self.kind], self.bits, self.direction), stream)


def quantize_and_pack_many(items, *, num_bits, strategy, group_size=None):
    """`quantize_and_pack` for a LIST of (weight, scale, zero_point or None) on one GPU: the tensors a W4 batch takes (`w4_batch_eligible`:
    int4, 2-D 16-bit weights, group / channel scales) leave in ONE `ct_quant_pack_batch` launch — what a caller holding q / k / v or
    gate / up pairs should use instead of one call per tensor (a small tensor's single launch is bound by its ramp and its launch
    boundary: 4096 x 4096 alone reaches 58-61 % of the HBM peak, bench.py reports the pair next to it) — and the others one by one.
    Returns the packed int32 tensors in order.  Mirrors the loop body of compressors/pack_quantized/base.py:96-104 per item."""
    items = [(x, s, z) for x, s, z in items]
    out = [None] * len(items)
    entries, where = [], []
    for i, (x, s, z) in enumerate(items):
        if (x.is_cuda and x.is_contiguous() and _aligned16(x)
                and w4_batch_eligible(x.shape, x.dtype, s, z, num_bits=num_bits, strategy=strategy, group_size=group_size, device=x.device)
                and (not entries or (x.device == entries[0][0].device and x.dtype == entries[0][0].dtype))):
            rows, cols = int(x.shape[0]), int(x.shape[1])
            group = cols if _strategy_name(strategy) == "channel" else int(group_size)
            dst = torch.empty((rows, cols // 8), dtype=torch.int32, device=x.device)
            entries.append((x, s, z, dst, rows, cols, group))
            where.append(i)
        else:
            out[i] = quantize_and_pack(x, s, z, num_bits=num_bits, strategy=strategy, group_size=group_size)
    if entries:
        batch = W4Batch(entries, "compress", entries[0][0].dtype)
        batch.launch()
        batch.table.record_stream(torch.cuda.current_stream(batch.device))
        for i, e in zip(where, entries):
            out[i] = e[3]
    return out


def unpack_and_dequantize_many(items, *, num_bits, strategy, group_size=None):
    """the inverse of `quantize_and_pack_many` for a list of (packed, shape, scale, zero_point or None): ONE `ct_unpack_dequant_batch`
    launch for the eligible tensors (output dtype = the scale's), `unpack_and_dequantize` for the rest
    (compressors/pack_quantized/base.py:147-161 per item; `zero_point` is the UNPACKED int8 zero point)."""
    items = [(p, tuple(int(v) for v in shape), s, z) for p, shape, s, z in items]
    out = [None] * len(items)
    entries, where = [], []
    for i, (p, shape, s, z) in enumerate(items):
        if (p.is_cuda and p.dtype is torch.int32 and p.is_contiguous() and _aligned16(p) and len(shape) == 2
                and w4_batch_eligible(shape, s.dtype, s, z, num_bits=num_bits, strategy=strategy, group_size=group_size, device=p.device)
                and tuple(p.shape) == (shape[0], shape[1] // 8)
                and (not entries or (p.device == entries[0][0].device and s.dtype == entries[0][1].dtype))):
            group = shape[1] if _strategy_name(strategy) == "channel" else int(group_size)
            dst = torch.empty(shape, dtype=s.dtype, device=p.device)
            entries.append((p, s, z, dst, shape[0], shape[1], group))
            where.append(i)
        else:
            out[i] = unpack_and_dequantize(p, shape, s, z, num_bits=num_bits, strategy=strategy, group_size=group_size)
    if entries:
        batch = W4Batch(entries, "decompress", entries[0][1].dtype)
        batch.launch()
        batch.table.record_stream(torch.cuda.current_stream(batch.device))
        for i, e in zip(where, entries):
            out[i] = e[3]
    return out


def rtn_w4_launch(dtype: torch.dtype, symmetric: bool) -> tuple:
    """the (kind, d, scalars) of the one-pass W4 table's launch: what `_launch_table` takes behind the words.  Each one-pass table has such a function, so
    that its launch's arguments are written once: `launch_rtn_*_words` and the dense-checkpoint quantizers (entrypoints/convert/dense.py) both go through it"""
    return "rtn_w4", 0, (DT[dtype], int(bool(symmetric)))


def rtn_wb_launch(dtype: torch.dtype, num_bits: int, symmetric: bool) -> tuple:
    """`rtn_w4_launch` for the table of the widths next to 4 and 8 (`RTN_PACKW_BITS`; the plan refuses any other): `d` is the width, the plan's third argument"""
    return "rtn_wb", int(num_bits), (DT[dtype], int(num_bits), int(bool(symmetric)))


def rtn_block8_launch(dtype: torch.dtype, fp8: bool, symmetric: bool) -> tuple:
    """`rtn_w4_launch` for the one-pass block-wise 8-bit table"""
    return "rtn_block8", 0, (DT[dtype], int(bool(fp8)), int(bool(symmetric)))


def rtn_group8_launch(dtype: torch.dtype, device: torch.device, kind: int, symmetric: bool = True, as_words: bool = False) -> tuple:
    """`rtn_w4_launch` for the one-pass group-wise 8-bit table; an MXFP8 table (`kind` 4) reads `_mx_code_table` of the weights' dtype on `device`"""
    lut = _mx_code_table(dtype, device).data_ptr() if int(kind) == _QP_MXFP8 else None  # cached per (dtype, device): outlives the launch
    return "rtn_group8", 0, (DT[dtype], int(kind), int(bool(symmetric)), int(bool(as_words)), lut)


def rtn_channel8_launch(dtype: torch.dtype, fp8: bool, symmetric: bool) -> tuple:
    """`rtn_w4_launch` for the one-pass channel-wise 8-bit table"""
    return "rtn_channel8", 0, (DT[dtype], int(bool(fp8)), int(bool(symmetric)))


def rtn_mxfp4_launch(dtype: torch.dtype) -> tuple:
    """`rtn_w4_launch` for the one-pass MXFP4 table"""
    return "rtn_mxfp4", 0, (DT[dtype],)


def _launch_rtn(words, n: int, device, launch, *args):
    """one launch of a one-pass table under `launch(*args)`'s (kind, d, scalars); an empty table returns None before anything about it is looked at"""
    if not n:
        return None
    kind, d, scalars = launch(*args)
    return _launch_table(kind, words, n, device, d, scalars)


def launch_rtn_w4_words(words, n: int, dtype: torch.dtype, device: torch.device, symmetric: bool) -> torch.Tensor:
    """`launch_w4_words` for a table of the one-pass round-to-nearest W4 compress (`ct_rtn_quant_pack_w4_batch`): src = weights, dst = packed words,
    scale / zp = OUTPUTS, zp_packed = 0.  Returns the device table (the caller owes it a `record_stream` when its stream is not the allocator's) or
    None for an empty table."""
    return _launch_rtn(words, n, device, rtn_w4_launch, dtype, symmetric)


def launch_rtn_wb_words(words, n: int, dtype: torch.dtype, device: torch.device, num_bits: int, symmetric: bool) -> torch.Tensor:
    """`launch_rtn_w4_words` for a table of the one-pass compress of the widths next to 4 and 8 (`ct_rtn_quant_pack_wb_batch`, `RTN_PACKW_BITS`): the same
    rows, dst = packed int32 (R, C * num_bits / 32), ONE width per table"""
    if int(num_bits) not in RTN_PACKW_BITS:
        raise NotImplementedError(f"the one-pass table of the widths next to 4 and 8 takes num_bits in {RTN_PACKW_BITS}, got {num_bits}")
    return _launch_rtn(words, n, device, rtn_wb_launch, dtype, num_bits, symmetric)


def launch_rtn_mxfp4_words(words, n: int, dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    """`launch_rtn_w4_words` for a table of the one-pass MXFP4 compress (`ct_rtn_mxfp4_quant_pack_batch`): src = weights, dst = packed bytes,
    zp_packed = the E8M0 code output, scale = the float-scale output or 0, group = 32"""
    return _launch_table("rtn_mxfp4", words, n, device, 0, (DT[dtype],)) if n else None


def launch_rtn_nvfp4_words(words, n: int, dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    """`launch_rtn_w4_words` for a table of the one-pass NVFP4 compress, `generate_gparam` of every weight included: src = weights, dst = packed
    bytes, zp_packed = the float8 scale output, zp = the item's amax key — its own 32-bit word of a buffer the caller has ZEROED on this stream —,
    scale = its float32 (1,) global-scale output, group = 16.  One plan, one upload, TWO launches over the same rows: `ct_rtn_nvfp4_amax_batch` folds
    max |x| into the keys, `ct_rtn_nvfp4_quant_pack_batch` derives each global scale from its key, stores it and quantizes under it."""
    if not n:
        return None
    table, blocks = _plan_table("rtn_nvfp4", words, n, device)
    for launch in (0, 1):
        _run_table("rtn_nvfp4", table, n, blocks, device, launch, (DT[dtype],))
    return table


def launch_rtn_block8_words(words, n: int, dtype: torch.dtype, device: torch.device, fp8: bool, symmetric: bool) -> torch.Tensor:
    """`launch_rtn_w4_words` for a table of the one-pass block-wise 8-bit compress (`ct_rtn_quant_block8_batch`): src = weights, dst = codes,
    scale / zp = OUTPUTS (zp 0 in a FLOAT or symmetric table), group = -((bh << 24) | bw)"""
    return _launch_rtn(words, n, device, rtn_block8_launch, dtype, fp8, symmetric)


def launch_rtn_group8_words(words, n: int, dtype: torch.dtype, device: torch.device, kind: int, symmetric: bool = True, as_words: bool = False) -> torch.Tensor:
    """`launch_rtn_w4_words` for a table of the one-pass group-wise 8-bit compress (`ct_rtn_quant_group8_batch`): src = weights, dst = codes,
    scale / zp = OUTPUTS (scale may be 0 in an MXFP8 table, zp 0 in a FLOAT or symmetric one), zp_packed = the E8M0 code output of an MXFP8
    table, group = the group size; `kind` 0 INT (`as_words`: the (code + 128) bytes of pack-quantized), 1 FP8, 4 MXFP8 (with `_mx_code_table` of the
    weights' dtype behind it)"""
    return _launch_rtn(words, n, device, rtn_group8_launch, dtype, device, kind, symmetric, as_words)


def launch_rtn_channel8_words(words, n: int, dtype: torch.dtype, device: torch.device, fp8: bool, symmetric: bool) -> torch.Tensor:
    """`launch_rtn_w4_words` for a table of the one-pass channel-wise 8-bit compress (`ct_rtn_quant_channel8_batch`): src = weights, dst = codes,
    scale / zp = OUTPUTS (zp 0 in a FLOAT or symmetric table: the plan reads an item with a zero-point output as asymmetric)"""
    return _launch_rtn(words, n, device, rtn_channel8_launch, dtype, fp8, symmetric)


def rtn_w4_group(shape, group_size) -> int:
    """the group (elements per scale) when `ct_rtn_quant_pack_w4` and its table form take a weight of this shape — 2-D, rows > 0, a group of
    32 * 2^k <= 2048 columns that divides the row (group_size None / 0: the whole row) — else 0"""
    if len(shape) != 2 or int(shape[0]) <= 0 or int(shape[1]) <= 0:
        return 0
    cols = int(shape[1])
    g = int(group_size) if group_size else cols
    if g <= 0 or cols % g or g % 32 or g > 2048 or (g // 32) & (g // 32 - 1):
        return 0
    return g


def _rtn_table_tensor(x) -> bool:
    return x.is_cuda and x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16) and x.is_contiguous() and x.data_ptr() % 16 == 0


# Each scheme's outputs are written once, as a pure function (rows, cols, dtype, options) -> [(field, shape, dtype)]: `field` is the `ct_w4_item` field
# that takes the output's address.  `rtn_*_table_item` allocates from it; a dense-checkpoint quantizer (entrypoints/convert/dense.py) lays out its output
# buffer and fills its rows from it, also for a weight its table refuses — so a shape here is the reference's for EVERY weight (ceil where the table only
# admits whole words or blocks).
def rtn_wb_outputs(rows: int, cols: int, dtype, group: int, num_bits: int, with_zp: bool = True) -> list:
    """the one-pass pack-quantized tables (`rtn_w4` at 4 bits, `rtn_wb` at the widths beside it): packed int32 (R, ceil(C * num_bits / 32)), scale
    (R, C / g), int8 zero point (R, C / g) — a symmetric table needs no zero-point output, the kernel skips the store"""
    grid = (rows, cols // group)
    return [("dst", (rows, -(-cols * num_bits // 32)), torch.int32), ("scale", grid, dtype)] + ([("zp", grid, torch.int8)] if with_zp else [])


def rtn_block8_outputs(rows: int, cols: int, dtype, block_structure, fp8: bool = True, with_zp: bool = False) -> list:
    """the one-pass block-wise 8-bit table: codes float8_e4m3fn — int8 without `fp8` — (R, C), scale (ceil(R / bh), ceil(C / bw)), int8 zero point of
    that shape"""
    grid = (-(-rows // int(block_structure[0])), -(-cols // int(block_structure[1])))
    return [("dst", (rows, cols), _F8 if fp8 else torch.int8), ("scale", grid, dtype)] + ([("zp", grid, torch.int8)] if with_zp else [])


def rtn_channel8_outputs(rows: int, cols: int, dtype, fp8: bool = True, with_zp: bool = False) -> list:
    """the one-pass channel-wise 8-bit table: codes float8_e4m3fn — int8 without `fp8` — (R, C), scale (R, 1), int8 zero point (R, 1) (an asymmetric
    scheme's)"""
    return [("dst", (rows, cols), _F8 if fp8 else torch.int8), ("scale", (rows, 1), dtype)] + ([("zp", (rows, 1), torch.int8)] if with_zp else [])


def rtn_group8_outputs(rows: int, cols: int, dtype, group: int, qtype: str = "int", with_zp: bool = False, mx: bool = False, words: bool = False,
                       with_scale: bool = True) -> list:
    """the one-pass group-wise 8-bit table: codes — float8_e4m3fn for qtype "float", int8 for "int", int32 (R, C / 4) with `words` —, scale (R, C / g)
    (an MXFP8 table may leave it out: `with_scale`), int8 zero point of that shape (INT only) and, with `mx`, the E8M0 codes uint8 (R, C / 32)"""
    fp8 = getattr(qtype, "value", qtype) == "float"
    grid = (rows, cols // group)
    out = [("dst", (rows, cols // 4), torch.int32) if words else ("dst", (rows, cols), _F8 if fp8 else torch.int8)]
    if with_scale or not mx:
        out.append(("scale", grid, dtype))
    if with_zp and not fp8:
        out.append(("zp", grid, torch.int8))
    return out + [("zp_packed", grid, torch.uint8)] if mx else out


def rtn_mxfp4_outputs(rows: int, cols: int) -> list:
    """the one-pass MXFP4 table: packed nibbles uint8 (R, C / 2) and, in the row's `zp_packed`, the E8M0 codes uint8 (R, C / 32)"""
    return [("dst", (rows, cols // 2), torch.uint8), ("zp_packed", (rows, cols // 32), torch.uint8)]


def _rtn_item(x, group: int, entries, fields=("dst", "scale", "zp")) -> tuple:
    """the freshly allocated outputs of `entries` in the order of `fields` (None for one that `entries` leaves out) and, last, the table row of `x` that
    points at them"""
    outs = {field: torch.empty(shape, dtype=dtype, device=x.device) for field, shape, dtype in entries}
    at = {field: t.data_ptr() for field, t in outs.items()}
    row = item_row(x.data_ptr(), at.get("scale", 0), at.get("zp", 0), at["dst"], int(x.shape[0]), int(x.shape[1]), group, at.get("zp_packed", 0))
    return tuple(outs.get(field) for field in fields) + (row,)


def rtn_wb_table_item(x, group_size, num_bits: int, with_zp: bool = True):
    """does the one-pass table of this width (`launch_rtn_w4_words` at 4 bits, `launch_rtn_wb_words` at the widths beside it) take this weight — on a GPU,
    2-D, contiguous, 16-byte aligned, 16-bit, with a group `rtn_w4_group` accepts?  Then its freshly allocated outputs (`rtn_wb_outputs`) and its row:
    (packed, scale, zero point or None without `with_zp`, row); else None"""
    g = rtn_w4_group(x.shape, group_size) if _rtn_table_tensor(x) else 0
    return _rtn_item(x, g, rtn_wb_outputs(int(x.shape[0]), int(x.shape[1]), x.dtype, g, int(num_bits), with_zp)) if g else None


def rtn_w4_table_item(x, group_size, with_zp: bool = True):
    """`rtn_wb_table_item` at 4 bits: (packed int32 (R, C / 8), scale, zero point or None, row) or None"""
    return rtn_wb_table_item(x, group_size, 4, with_zp)


def rtn_block8_table_item(x, block_structure, fp8: bool = True, with_zp: bool = False):
    """`rtn_wb_table_item` for the one-pass block-wise 8-bit table (`launch_rtn_block8_words`; `rtn_block8_group`, `rtn_block8_outputs`): (codes, scale,
    zero point or None without `with_zp`, row) or None"""
    g = rtn_block8_group(x.shape, block_structure) if _rtn_table_tensor(x) else 0
    return _rtn_item(x, g, rtn_block8_outputs(int(x.shape[0]), int(x.shape[1]), x.dtype, block_structure, fp8, with_zp)) if g else None


def rtn_channel8_table_item(x, fp8: bool = True, with_zp: bool = False):
    """`rtn_wb_table_item` for the one-pass channel-wise 8-bit table (`launch_rtn_channel8_words`; `rtn_channel8_form`, `rtn_channel8_outputs`): (codes,
    scale, zero point or None without `with_zp`, row) or None"""
    if not _rtn_table_tensor(x) or not rtn_channel8_form(x.shape, not with_zp):
        return None
    return _rtn_item(x, 0, rtn_channel8_outputs(int(x.shape[0]), int(x.shape[1]), x.dtype, fp8, with_zp))


def rtn_group8_table_item(x, group_size, qtype: str = "int", with_zp: bool = False, mx: bool = False, words: bool = False, with_scale: bool = True):
    """`rtn_wb_table_item` for the one-pass group-wise 8-bit table (`launch_rtn_group8_words`; `rtn_group8_group`, `rtn_group8_outputs`): (codes, scale
    or None without `with_scale` (MXFP8 only), zero point or None without `with_zp`, [E8M0 codes with `mx`,] row) or None"""
    g = rtn_group8_group(x.shape, group_size) if _rtn_table_tensor(x) else 0
    if not g or (mx and g != 32):
        return None
    entries = rtn_group8_outputs(int(x.shape[0]), int(x.shape[1]), x.dtype, g, qtype, with_zp, mx, words, with_scale)
    return _rtn_item(x, g, entries, ("dst", "scale", "zp", "zp_packed") if mx else ("dst", "scale", "zp"))


def _rtn_fp4_takes(x) -> bool:
    """do the one-pass FP4 tables, MXFP4 and NVFP4, take this weight — on a GPU, 2-D, contiguous, 16-byte aligned, 16-bit, cols % 32 == 0?"""
    return _rtn_table_tensor(x) and x.shape[0] > 0 and x.shape[1] > 0 and x.shape[1] % 32 == 0


def rtn_mxfp4_table_item(x):
    """`rtn_w4_table_item` for the one-pass MXFP4 table (`launch_rtn_mxfp4_words`; cols % 32 == 0): (packed uint8 (R, C / 2), E8M0 codes uint8
    (R, C / 32), row) or None"""
    if not _rtn_fp4_takes(x):
        return None
    rows, cols = int(x.shape[0]), int(x.shape[1])
    packed = torch.empty((rows, cols // 2), dtype=torch.uint8, device=x.device)
    code = torch.empty((rows, cols // 32), dtype=torch.uint8, device=x.device)
    return packed, code, item_row(x.data_ptr(), 0, 0, packed.data_ptr(), rows, cols, 32, code.data_ptr())


rtn_nvfp4_takes = _rtn_fp4_takes  # public for NVFP4: its callers ask before they open a table's key buffer


def rtn_nvfp4_keys(n: int, device) -> torch.Tensor:
    """the amax keys of a table of up to `n` items, armed: int32 zeros, one word per item (0 is the identity of the fold) — the table's one fill"""
    return torch.zeros(int(n), dtype=torch.int32, device=device)


def rtn_nvfp4_table_item(x, key: int):
    """`rtn_w4_table_item` for the one-pass NVFP4 table (`launch_rtn_nvfp4_words`; cols % 32 == 0), `key` = the address of the item's word of
    the table's key buffer (`rtn_nvfp4_keys`): (packed uint8 (R, C / 2), float8_e4m3fn scales (R, C / 16), float32 (1,) global scale, row) or None.  The
    global scale is a tensor of its own, not a view into a buffer the items share: a saved state dict must not contain aliased tensors."""
    if not rtn_nvfp4_takes(x):
        return None
    rows, cols = int(x.shape[0]), int(x.shape[1])
    packed = torch.empty((rows, cols // 2), dtype=torch.uint8, device=x.device)
    s8 = torch.empty((rows, cols // 16), dtype=_F8, device=x.device)
    gs = torch.empty(1, dtype=torch.float32, device=x.device)
    return packed, s8, gs, item_row(x.data_ptr(), gs.data_ptr(), int(key), packed.data_ptr(), rows, cols, 16, s8.data_ptr())


def _rtn_w4_one(x, group_size, symmetric, num_bits=4):
    """one tensor outside the table: the one-pass kernel where it applies, the observer + compress composition otherwise"""
    if x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16) and rtn_w4_group((1, x.shape[1]), group_size):
        return rtn_quantize_and_pack(x, group_size=group_size, symmetric=symmetric, num_bits=num_bits)
    scale, zp = minmax_qparams(x, num_bits=num_bits, group_size=group_size, symmetric=symmetric)
    packed = quantize_and_pack(x, scale, zp, num_bits=num_bits, strategy="group" if group_size else "channel", group_size=group_size)
    return packed, scale, zp


def _rtn_many(weights, item, single, launch, held=()) -> list:
    """the list form of every one-pass round-to-nearest table.  `item(i, x, n)` -> (outputs..., row) when the table takes `weights[i]` as its n-th
    item, else None; the first tensor taken fixes the table's device and dtype, and every tensor not taken goes to `single(i, x)`.  The rows are
    gathered flat, ONE `launch(flat, n, dtype, device)` follows, and the device table it returns and then whatever `held` holds by then (a buffer the
    rows point into) are recorded on the current stream.  Returns the outputs in input order; they keep the tensors the table's raw pointers name
    alive, `weights` the inputs."""
    out = [None] * len(weights)
    first, n, flat = None, 0, []
    for i, x in enumerate(weights):
        got = item(i, x, n) if first is None or (x.device == first.device and x.dtype == first.dtype) else None
        if got is None:
            out[i] = single(i, x)
            continue
        first = x if first is None else first
        out[i] = got[:-1]
        flat += got[-1]
        n += 1
    if n:
        stream = torch.cuda.current_stream(first.device)
        for t in (launch(flat, n, first.dtype, first.device), *held):
            t.record_stream(stream)
    return out


def rtn_quantize_and_pack_many(weights, *, group_size=None, symmetric=True, num_bits=4):
    """`rtn_quantize_and_pack` for a LIST of weights: the tensors the table takes (`rtn_w4_table_item` / `rtn_wb_table_item`, of the first such
    tensor's device and dtype) leave in ONE `ct_rtn_quant_pack_w4_batch` (4 bits) or `ct_rtn_quant_pack_wb_batch` (2, 3, 5, 6, 7) launch — a
    checkpoint is a few hundred
    launch-bound tensors — and the others one by one (the one-pass kernel, or `minmax_qparams` + `quantize_and_pack` where that does not apply).
    `group_size`: one value for all, or one per weight (None = one group per row).  Returns [(packed, scale, zero_point)] in input order,
    bit-identical to the single-tensor call per item (quantization/utils/helpers.py:50-137 + compressors/pack_quantized/base.py:96-104)."""
    bits = _rtn_pack_bits(num_bits)
    weights = list(weights)
    groups = list(group_size) if isinstance(group_size, (list, tuple)) else [group_size] * len(weights)
    if len(groups) != len(weights):
        raise ValueError(f"{len(groups)} group sizes for {len(weights)} weights")
    if bits == 4:
        return _rtn_many(weights, lambda i, x, n: rtn_w4_table_item(x, groups[i]), lambda i, x: _rtn_w4_one(x, groups[i], symmetric),
                         lambda flat, n, dtype, device: launch_rtn_w4_words(flat, n, dtype, device, symmetric))
    return _rtn_many(weights, lambda i, x, n: rtn_wb_table_item(x, groups[i], bits), lambda i, x: _rtn_w4_one(x, groups[i], symmetric, bits),
                     lambda flat, n, dtype, device: launch_rtn_wb_words(flat, n, dtype, device, bits, symmetric))


def rtn_mxfp4_quantize_and_pack_many(weights):
    """`rtn_mxfp4_quantize_and_pack` for a LIST of weights: the tensors the table takes (`rtn_mxfp4_table_item`, of the first such tensor's device
    and dtype) leave in ONE `ct_rtn_mxfp4_quant_pack_batch` launch, the others one by one.  Returns
    [(packed uint8 (R, C / 2), E8M0 codes uint8 (R, C / 32))] in input order, bit-identical to the single-tensor call per item."""
    return _rtn_many(list(weights), lambda i, x, n: rtn_mxfp4_table_item(x), lambda i, x: rtn_mxfp4_quantize_and_pack(x), launch_rtn_mxfp4_words)


def rtn_nvfp4_quantize_and_pack_many(weights):
    """`rtn_nvfp4_quantize_and_pack` for a LIST of weights, each under its own `generate_gparam`: the tensors the table takes
    (`rtn_nvfp4_table_item`, of the first such tensor's device and dtype) leave in one fill of the key buffer and TWO launches
    (`launch_rtn_nvfp4_words`) instead of three launches each, the others one by one.  Returns [(packed uint8 (R, C / 2), float8_e4m3fn scales
    (R, C / 16), float32 (1,) global scale)] in input order, bit-identical to the single-tensor call per item; every global scale owns its storage."""
    weights = list(weights)
    keys = []  # the table's key buffer, from its first item on

    def item(i, x, n):
        if not rtn_nvfp4_takes(x):
            return None
        if not keys:
            keys.append(rtn_nvfp4_keys(len(weights) - i, x.device))  # the n-th item's key is word n
        return rtn_nvfp4_table_item(x, keys[0].data_ptr() + 4 * n)

    return _rtn_many(weights, item, lambda i, x: rtn_nvfp4_quantize_and_pack(x), launch_rtn_nvfp4_words, keys)


def rtn_quantize_block8_many(weights, *, block_structure, qtype: str = "float", symmetric: bool = True):
    """`rtn_quantize_block8` for a LIST of weights: the tensors the table takes (`rtn_block8_table_item`, of the first such tensor's device and
    dtype) leave in ONE `ct_rtn_quant_block8_batch` launch, the others one by one.  Returns [(codes, scale, zero_point)] in input order,
    bit-identical to the single-tensor call per item."""
    qtype = getattr(qtype, "value", qtype)
    fp8 = qtype == "float"
    if fp8 and not symmetric:
        raise NotImplementedError("FLOAT 8-bit round-to-nearest is symmetric")

    def item(i, x, n):
        got = rtn_block8_table_item(x, block_structure, fp8, not fp8)
        if got is None:
            return None
        q, scale, zp, row = got
        return q, scale, (torch.zeros(scale.shape, dtype=_F8, device=x.device) if fp8 else zp), row

    return _rtn_many(list(weights), item, lambda i, x: rtn_quantize_block8(x, block_structure=block_structure, qtype=qtype, symmetric=symmetric),
                     lambda flat, n, dtype, device: launch_rtn_block8_words(flat, n, dtype, device, fp8, symmetric))


def _rtn_channel8_one(x, qtype, symmetric):
    """one tensor outside the table: the one-pass kernel where it applies, the observer + quantize composition otherwise"""
    if x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16) and (x.numel() == 0 or rtn_channel8_form(x.shape, symmetric)):
        return rtn_quantize_channel8(x, qtype=qtype, symmetric=symmetric)
    if qtype == "float":
        scale = minmax_qparams_float(x, kind="fp8")
        zp = torch.zeros(scale.shape, dtype=_F8, device=scale.device)
    else:
        scale, zp = minmax_qparams(x, num_bits=8, symmetric=symmetric)
    q = quantize_tensor(x, scale, zp, qtype=qtype, num_bits=8, strategy="channel", dtype=_F8 if qtype == "float" else torch.int8)
    return q, scale, zp


def rtn_quantize_channel8_many(weights, *, qtype: str = "int", symmetric: bool = True):
    """`rtn_quantize_channel8` for a LIST of weights: the tensors the table takes (`rtn_channel8_table_item`, of the first such tensor's device and
    dtype) leave in ONE `ct_rtn_quant_channel8_batch` launch, the others one by one, in input order (the one-pass kernel, or the observer followed by
    `quantize_tensor` for what its plan refuses: float32, cols % 8, rows beyond `RTN_CHANNEL8_MAX_COLS`).  Returns [(codes, scale, zero_point)] in
    input order, bit-identical to the single-tensor call per item."""
    qtype = getattr(qtype, "value", qtype)
    fp8 = qtype == "float"
    symmetric = bool(symmetric)
    if fp8 and not symmetric:
        raise NotImplementedError("FLOAT 8-bit round-to-nearest is symmetric")

    def item(i, x, n):
        got = rtn_channel8_table_item(x, fp8, not symmetric)
        if got is None:
            return None
        q, scale, zp, row = got
        if zp is None:  # what the single launch returns for a symmetric scheme: zeros, float8 for FLOAT
            zp = torch.zeros(scale.shape, dtype=_F8 if fp8 else torch.int8, device=x.device)
        return q, scale, zp, row

    return _rtn_many(list(weights), item, lambda i, x: _rtn_channel8_one(x, qtype, symmetric),
                     lambda flat, n, dtype, device: launch_rtn_channel8_words(flat, n, dtype, device, fp8, symmetric))


def rtn_quantize_group8_many(weights, *, group_size, qtype: str = "int", symmetric: bool = True, mx: bool = False, words: bool = False):
    """`rtn_quantize_group8` for a LIST of weights: the tensors the table takes (`rtn_group8_table_item`, of the first such tensor's device and
    dtype) leave in ONE `ct_rtn_quant_group8_batch` launch, the others one by one.  `group_size`: one value for all, or one per weight (None = one
    group per row).  Returns the single call's tuples in input order, bit-identical to the single-tensor call per item."""
    kind = _rtn_group8_kind(qtype, symmetric, mx, words)
    weights = list(weights)
    groups = list(group_size) if isinstance(group_size, (list, tuple)) else [group_size] * len(weights)
    if len(groups) != len(weights):
        raise ValueError(f"{len(groups)} group sizes for {len(weights)} weights")
    return _rtn_many(weights, lambda i, x, n: rtn_group8_table_item(x, groups[i], qtype, kind == _QP_INT, mx, words),
                     lambda i, x: rtn_quantize_group8(x, group_size=groups[i], qtype=qtype, symmetric=symmetric, mx=mx, words=words),
                     lambda flat, n, dtype, device: launch_rtn_group8_words(flat, n, dtype, device, kind, symmetric, words))


def zp4_batch(pairs, direction: str) -> None:
    """`pack_to_int32(zp, 4, packed_dim=0)` ("pack": int8 (R, G) -> int32 (ceil(R / 8), G)) or its inverse ("unpack") for a list of
    (src, dst) tensor pairs on one GPU in ONE launch (`ct_zp4_pack_dim0_batch`); dst tensors are allocated by the caller."""
    assert direction in ("pack", "unpack")
    pairs = list(pairs)
    if not pairs:
        return
    flat = []
    for src, dst in pairs:
        unpacked = src if direction == "pack" else dst
        flat += item_row(src.data_ptr(), 0, 0, dst.data_ptr(), int(unpacked.shape[0]), int(unpacked.shape[1]))
    d = 0 if direction == "pack" else 1
    dev = pairs[0][0].device
    table = _launch_table("zp4", flat, len(pairs), dev, d, (d,))
    table.record_stream(torch.cuda.current_stream(dev))


def q8_batch_group(shape, w_dtype, scale, zero_point, *, device, strategy=None, group_size=None, g_idx=None, f8_zero_point=False, block_structure=None):
    """Elements per scale (the table's `group`) if this tensor can join a one-launch 8-bit batch, else None.  2-D, 16-bit
    float dtype equal to the scale's, tensor / channel / group scales (strategy given, or inferred from the scale's shape like
    `dequantize` does, forward.py:99-130), cols % 16 == 0, group % 16 == 0, int8 or absent zero point of the scale's shape,
    everything contiguous, 16-byte aligned and on `device`."""
    if g_idx is not None or len(shape) != 2 or w_dtype not in (torch.bfloat16, torch.float16):
        return None
    if scale is None or scale.dtype != w_dtype or scale.device != device or not scale.is_contiguous() or not _aligned16(scale):
        return None
    rows, cols = int(shape[0]), int(shape[1])
    if rows <= 0 or cols % 16:
        return None
    st = _strategy_name(strategy)
    if scale.numel() == 1 and scale.dim() <= 1 and st in (None, "tensor"):
        group = rows * cols
    elif scale.dim() == 2 and scale.shape[0] == rows and scale.shape[1] == 1 and st in (None, "channel"):
        group = cols
    elif scale.dim() == 2 and scale.shape[0] == rows and scale.shape[1] > 1 and cols % scale.shape[1] == 0 and st in (None, "group"):
        group = cols // scale.shape[1]
        if st == "group" and group_size and int(group_size) != group:
            return None
    elif scale.dim() == 2 and st in (None, "block") and scale.shape[0] >= 1 and scale.shape[1] >= 1:
        # block strategy (forward.py:198-216; inferred like `dequantize` does, forward.py:118-130, when no strategy is given): the table's group is
        # -((rows per block << 24) | columns per block), include/ct_hip.h
        if st == "block":
            if block_structure is None or len(block_structure) != 2:
                return None
            bh, bw = int(block_structure[0]), int(block_structure[1])
        else:
            if rows % scale.shape[0] or cols % scale.shape[1]:
                return None
            bh, bw = rows // scale.shape[0], cols // scale.shape[1]
        if (bh < 1 or bw < 16 or bh & (bh - 1) or bw & (bw - 1) or bh >= 1 << 24 or bw >= 1 << 24 or cols % bw or rows * cols >= 1 << 34
                or tuple(scale.shape) != (-(-rows // bh), cols // bw)):
            return None
        group = -((bh << 24) | bw)
    else:
        return None
    if group > 0 and group % 16:
        return None
    # (f8_zero_point, round 6: the float8 zero points a calibrated FLOAT scheme carries — all zeros for the symmetric schemes upstream allows, but
    # read as the float8 values they are: kind "fp8z" of W4Batch)
    if zero_point is not None and (zero_point.dtype != (_F8 if f8_zero_point else torch.int8) or zero_point.shape != scale.shape or zero_point.device != device
                                   or not zero_point.is_contiguous()):
        return None
    return group


# --------------------------------------------------------------------------- bitmask codecs
def _bits_view(t: torch.Tensor) -> torch.Tensor:
    """fp8 payloads are moved as raw bytes"""
    if t.dtype.is_floating_point and t.element_size() == 1:
        return t.view(torch.int8)
    return t


def _elem_code(t: torch.Tensor) -> int:
    if t.dtype not in DT:
        raise NotImplementedError(f"element dtype {t.dtype} is not supported by the MI355X path")
    if t.element_size() not in (1, 2, 4):
        raise NotImplementedError(f"{t.element_size()}-byte elements are not supported by the sparse codecs")
    return DT[t.dtype]


def pack_bitmasks(bytemasks: torch.Tensor) -> torch.Tensor:
    """utils/helpers.py:306-318 (numpy.packbits(..., bitorder="little") on the GPU)."""
    dev = _compute_device(bytemasks)
    m = _dev(bytemasks if bytemasks.dtype in (torch.bool, torch.uint8) else bytemasks != 0, dev)
    cols = m.shape[-1] if m.ndim else 1
    rows = math.prod(m.shape[:-1]) if m.ndim > 1 else 1
    out = torch.empty((*m.shape[:-1], math.ceil(cols / 8)), dtype=torch.uint8, device=dev)
    call("ct_pack_bitmasks", ptr(m), rows, cols, ptr(out), stream_of(m))
    return _home(out, bytemasks)


def unpack_bitmasks(packed_bitmasks: torch.Tensor, original_shape) -> torch.Tensor:
    """utils/helpers.py:321-343; returns a bool tensor of `original_shape`."""
    shape = tuple(int(s) for s in original_shape)
    dev = _compute_device(packed_bitmasks)
    p = _dev(packed_bitmasks, dev)
    cols = shape[-1]
    rows = math.prod(shape[:-1])
    out = torch.empty(shape, dtype=torch.uint8, device=dev)
    call("ct_unpack_bitmasks", ptr(p), rows, cols, ptr(out), stream_of(p))
    return _home(out.view(torch.bool), packed_bitmasks)


_WS_BYTES = {}


def _bitmask_workspace_bytes(rows: int, cols: int) -> int:
    n = _WS_BYTES.get((rows, cols))
    if n is None:
        n = _WS_BYTES[(rows, cols)] = int(_lib.load().ct_bitmask_compress_workspace_bytes(rows, cols))
    return n


def bitmask_compress(tensor: torch.Tensor, two_pass: bool = False, exact: bool = True):
    """sparse-bitmask compression: returns (values, bitmask uint8 (R, ceil(C/8)), row_offsets int64 (R,)).

    `exact` (round 6, default True): `values` owns exactly nnz elements, as `tensor[mask]` does (restated S1 over utils/helpers.py:306-343) —
    the kernel writes into a worst-case sized buffer (nnz is not known before it has run) and the kept prefix is then copied out, one
    asynchronous device copy of 2 x nnz x itemsize bytes that the caller does not wait for; the worst-case buffer goes back to the allocator.
    `exact=False`: `values` is a VIEW of the worst-case buffer — no copy, but the result pins numel x itemsize bytes however sparse the
    tensor is (a "compressed" 50 %-sparse weight then holds as much memory as the dense one): for a caller that consumes the values at
    once (serialises them, copies them elsewhere) and drops them.

    Default: the fused form (`ct_bitmask_compress`; 16- and 32-bit elements: the register-resident kernel that reads the tensor once,
    otherwise count + scatter whose prefixes are sums of the counts; no scan kernel) into a worst-case sized value buffer, then
    one host wait for nnz — as unavoidable as the reference's `tensor[mask]` — to narrow it: the kernel stores nnz into a pinned
    host word (`_lib.Mailbox`) and the host spins on that word instead of copying it back.  `two_pass=True` keeps the
    count / scan / host read / scatter form that sizes `values` exactly before writing it."""
    if tensor.ndim < 1:
        raise ValueError("bitmask compression expects at least a 1-D tensor")
    if not two_pass and tensor.is_cuda and tensor.device.index == torch.cuda.current_device():
        # the same steps without the interpreter (csrc/host/ct_hostpath.cpp:bitmask_compress): this call cannot overlap its own
        # kernel — it returns nnz — so every microsecond of host work around the launch is a microsecond of the call
        hp = _lib.hostpath()
        if hp is not None:
            x = _bits_view(tensor)
            s = stream_of(x)
            mb = _lib.mailbox(s.device_index)
            r = hp.bitmask_compress(x, _elem_code(x), mb.host, mb.dev, s, bool(exact))
            if r is not None:
                _lib.check(r[0])
                return (r[1] if x is tensor else r[1].view(tensor.dtype)), r[2], r[3]
    dev = _compute_device(tensor)
    x = _dev(_bits_view(tensor), dev)
    dt = _elem_code(x)
    cols = x.shape[-1]
    rows = math.prod(x.shape[:-1]) if x.ndim > 1 else 1
    bitmask = torch.empty((rows, math.ceil(cols / 8)), dtype=torch.uint8, device=dev)
    row_offsets = torch.empty(rows, dtype=torch.int64, device=dev)
    s = stream_of(x)
    if two_pass:
        counts = torch.empty(rows + 1, dtype=torch.int64, device=dev)
        call("ct_bitmask_count", ptr(x), dt, rows, cols, ptr(bitmask), ptr(counts), s)
        total = counts[rows:]
        call("ct_exclusive_scan_i64", ptr(counts), rows, ptr(row_offsets), total.data_ptr(), s)
        nnz = int(total.item())
        values = torch.empty(nnz, dtype=x.dtype, device=dev)
        if nnz:
            call("ct_bitmask_scatter", ptr(x), dt, rows, cols, ptr(row_offsets), ptr(values), s)
    else:
        numel = rows * cols
        ws_bytes = _bitmask_workspace_bytes(rows, cols)
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        buf = torch.empty(numel, dtype=x.dtype, device=dev)
        # nnz comes back through the thread's pinned mailbox word: the kernel's last wave stores it there (system scope) as soon
        # as the prefix is known — before the last values have left — and the host spins on the word; no D2H copy, no `.item()`
        mb = _lib.mailbox(s.device_index)
        mb.words[0] = -1
        call("ct_bitmask_compress", ptr(x), dt, rows, cols, ptr(buf), numel, ptr(bitmask), ptr(row_offsets), mb.dev, ptr(ws), ws_bytes, s)
        nnz = mb.wait_word(0, -1, s)
        if nnz < 0 or nnz > numel:  # the stream drained and the word still holds the pending mark (or junk): never slice with it
            raise RuntimeError(f"ct_bitmask_compress finished without reporting the number of non-zeros (mailbox word {nnz}, numel {numel})")
        # exact: the kept prefix leaves the worst-case buffer (an asynchronous copy; nothing waits for it) unless the buffer is full anyway
        values = buf[:nnz] if (not exact or nnz == numel) else buf[:nnz].clone()
    return _home(values.view(tensor.dtype), tensor), _home(bitmask, tensor), _home(row_offsets, tensor)


def bitmask_compress_many(tensors, exact: bool = True, arena_bytes: int = 1 << 30):
    """`bitmask_compress` for a LIST of tensors (a checkpoint's sparse weights): [(values, bitmask, row_offsets), ...] in order.  The tensors on
    the current GPU go through the C++ host loop in windows — their compress launches are queued back to back, each reporting nnz into its own
    mailbox word, and the host sizes the results afterwards: one wait per window instead of ~9 us of waiting per tensor (a single call cannot
    overlap its own kernel; a batch can).  `exact` as in `bitmask_compress`; in exact mode a window's kernels share ONE worst-case arena of at
    most `arena_bytes` (never less than one tensor) instead of a worst-case allocation per tensor, and the exact-size results are filled by
    one batched copy.  A window is ONE kernel launch (`ct_bitmask_compress_batch`): a single launch of a checkpoint-sized tensor is a latency
    chain at 2-27 % of the HBM rate, the tensors of a table run theirs side by side.  Everything the loop does not take (CPU tensors, other
    devices, views, 8-bit payloads, no host extension) is compressed one by one."""
    tensors = list(tensors)
    out = [None] * len(tensors)
    hp = _lib.hostpath()
    if hp is not None and torch.cuda.is_available():
        cur = torch.cuda.current_device()
        idx = [i for i, t in enumerate(tensors) if t.ndim >= 1 and t.is_cuda and t.device.index == cur and t.numel() > 0 and t.is_contiguous()]
        if idx:
            xs = [_bits_view(tensors[i]) for i in idx]
            dts = [DT[x.dtype] if (x.dtype in DT and x.element_size() in (1, 2, 4)) else -1 for x in xs]
            s = _lib.stream_on(xs[0].device)
            mb = _lib.mailbox(s.device_index)
            r = hp.bitmask_compress_many(xs, dts, mb.host, mb.dev, mb.BATCH_WORD0, mb.BATCH_WORDS, s, bool(exact), int(arena_bytes))
            _lib.check(r[0])
            for i, x, res in zip(idx, xs, r[1:]):
                if res is not None:
                    out[i] = (res[0] if x is tensors[i] else res[0].view(tensors[i].dtype), res[1], res[2])
    for i, t in enumerate(tensors):
        if out[i] is None:
            out[i] = bitmask_compress(t, exact=exact)
    return out


def bitmask_decompress(values: torch.Tensor, bitmask: torch.Tensor, shape, row_offsets: Optional[torch.Tensor] = None,
                       fixed_row_nnz: Optional[int] = None) -> torch.Tensor:
    """sparse-bitmask decompression: zeros(shape) with `values` written at the set bits."""
    shape = tuple(int(s) for s in shape)
    dev = _compute_device(values, bitmask)
    v = _dev(_bits_view(values).reshape(-1), dev)
    b = _dev(bitmask, dev)
    dt = _elem_code(v)
    cols = shape[-1]
    rows = math.prod(shape[:-1])
    s = stream_of(b)
    ro = None
    if fixed_row_nnz is None:
        if row_offsets is None:
            counts = torch.empty(rows, dtype=torch.int64, device=dev)
            ro = torch.empty(rows, dtype=torch.int64, device=dev)
            call("ct_bitmask_row_popcount", ptr(b), rows, cols, ptr(counts), s)
            call("ct_exclusive_scan_i64", ptr(counts), rows, ptr(ro), None, s)
        else:
            ro = _dev(row_offsets.to(torch.int64), dev)
    out = torch.empty(shape, dtype=v.dtype, device=dev)
    call("ct_bitmask_decompress", ptr(v), v.numel(), ptr(b), ptr(ro), -1 if fixed_row_nnz is None else int(fixed_row_nnz),
         dt, rows, cols, ptr(out), s)
    return _home(out.view(values.dtype), values)


def bitmask_decompress_many(items):
    """`bitmask_decompress` for a LIST of (values, bitmask, shape, row_offsets): [dense tensor, ...] in order — loading a sparse checkpoint.  The
    16- / 32-bit tensors on the current GPU that have row offsets leave in ONE launch per element size (`ct_bitmask_decompress_batch`, through the
    C++ host loop: allocation of the dense outputs, the table, the launch; nothing waits); everything else one by one."""
    items = [(v, b, tuple(int(s) for s in shape), ro) for v, b, shape, ro in items]
    out = [None] * len(items)
    hp = _lib.hostpath()
    if hp is not None and torch.cuda.is_available() and items:
        cur = torch.cuda.current_device()
        idx = [i for i, (v, b, shape, ro) in enumerate(items) if ro is not None and v.is_cuda and b.is_cuda and ro.is_cuda and v.device.index == cur and len(shape) >= 1
               and v.element_size() in (2, 4) and v.dtype in DT and ro.dtype is torch.int64]
        if idx:
            vs = [_bits_view(items[i][0]).reshape(-1) for i in idx]
            r = hp.bitmask_decompress_many(vs, [items[i][1] for i in idx], [items[i][3] for i in idx], [list(items[i][2]) for i in idx], [DT[v.dtype] for v in vs],
                                           _lib.stream_on(vs[0].device))
            _lib.check(r[0])
            for i, v, res in zip(idx, vs, r[1:]):
                if res is not None:
                    out[i] = res if v.dtype is items[i][0].dtype else res.view(items[i][0].dtype)
    for i, (v, b, shape, ro) in enumerate(items):
        if out[i] is None:
            out[i] = bitmask_decompress(v, b, shape, ro)
    return out


def sparse24_mask(tensor: torch.Tensor) -> torch.Tensor:
    """bool mask keeping the 2 largest-|x| of every 4 consecutive elements
    (mask_creator, utils/semi_structured_conversions.py:301-330; ties: lower index first)."""
    if tensor.numel() % 4 != 0:
        raise ValueError(f"Tensor of size {tensor.shape} can't be evenly divided into 4 groups")
    dev = _compute_device(tensor)
    x = _dev(_bits_view(tensor), dev)
    if x.numel() % 8 != 0:
        # the kernel works on units of 8 elements; mask_creator accepts any multiple of 4 (:301-330): one zero quad is appended
        # and its mask dropped again (a copy of the tensor — only for numel % 8 == 4, which no weight matrix of the path has)
        flat = torch.cat([x.reshape(-1), torch.zeros(4, dtype=x.dtype, device=dev)])
        mask = torch.empty(flat.shape, dtype=torch.uint8, device=dev)
        call("ct_sparse24_mask", ptr(flat), _elem_code(flat), flat.numel(), ptr(mask), stream_of(flat))
        return _home(mask[:-4].reshape(x.shape).view(torch.bool), tensor)
    mask = torch.empty(x.shape, dtype=torch.uint8, device=dev)
    call("ct_sparse24_mask", ptr(x), _elem_code(x), x.numel(), ptr(mask), stream_of(x))
    return _home(mask.view(torch.bool), tensor)


def sparse24_bitmask_compress(tensor: torch.Tensor):
    """sparse-24-bitmask compression: (values (R, C/2), bitmask uint8 (R, C/8))."""
    if tensor.ndim != 2:
        raise ValueError("2:4 bitmask compression expects a 2-D tensor")
    if tensor.numel() % 4 != 0:
        raise ValueError("Tensor size must be a multiple of 4 for TWO_FOUR sparsity")
    dev = _compute_device(tensor)
    x = _dev(_bits_view(tensor), dev)
    rows, cols = x.shape
    values = torch.empty((rows, cols // 2), dtype=x.dtype, device=dev)
    bitmask = torch.empty((rows, math.ceil(cols / 8)), dtype=torch.uint8, device=dev)
    call("ct_sparse24_compress", ptr(x), _elem_code(x), rows, cols, ptr(values), ptr(bitmask), stream_of(x))
    return _home(values.view(tensor.dtype), tensor), _home(bitmask, tensor)


def sparse24_bitmask_decompress(values: torch.Tensor, bitmask: torch.Tensor, shape) -> torch.Tensor:
    shape = tuple(int(s) for s in shape)
    return bitmask_decompress(values, bitmask, shape, fixed_row_nnz=shape[-1] // 2)


# --------------------------------------------------------------------------- 2:4 cutlass + marlin-24
def cutlass24_from_dense(dense: torch.Tensor):
    """utils/semi_structured_conversions.py:66-197 -> (sparse (m, k/2), meta_reordered)."""
    if dense.dim() != 2:
        raise RuntimeError(f"Expected 2-dimensional dense tensor, got {dense.dim()}-dimensional tensor")
    if dense.dtype not in (torch.int8, torch.float16, torch.bfloat16):
        if dense.dtype in (torch.float32, torch.int32):
            raise NotImplementedError(f"{dense.dtype} 2:4 conversion is not supported by the MI355X path")
        raise RuntimeError(f"Invalid datatype {dense.dtype} of dense matrix")
    dev = _compute_device(dense)
    d = _dev(dense, dev)
    m, k = d.shape
    meta_dtype = torch.int32 if d.dtype == torch.int8 else torch.int16
    q = meta_dtype.itemsize * 2
    if m % 64 != 0:
        raise RuntimeError(f"Number of rows of dense matrix {m} must be divisible by 64")
    if k % (4 * q) != 0:
        raise RuntimeError(f"Number of columns of dense matrix {k} must be divisible by {4 * q}")
    sparse = torch.empty((m, k // 2), dtype=d.dtype, device=dev)
    meta = torch.empty((m, k // (4 * q)), dtype=meta_dtype, device=dev)
    call("ct_cutlass24_from_dense", ptr(d), DT[d.dtype], m, k, ptr(sparse), ptr(meta), stream_of(d))
    return _home(sparse, dense), _home(meta, dense)


def cutlass24_to_dense(sparse: torch.Tensor, meta_reordered: torch.Tensor) -> torch.Tensor:
    """utils/semi_structured_conversions.py:204-298."""
    if sparse.dim() != 2:
        raise RuntimeError(f"Expected 2-dimensional sparse tensor, got {sparse.dim()}-dimensional tensor")
    if meta_reordered.dim() != 2:
        raise RuntimeError(f"Expected 2-dimensional meta tensor, got {meta_reordered.dim()}-dimensional tensor")
    if meta_reordered.dtype not in (torch.int16, torch.int32):
        raise RuntimeError(f"Invalid datatype {meta_reordered.dtype} of meta matrix")
    dev = _compute_device(sparse)
    s, mt = _dev(sparse, dev), _dev(meta_reordered, dev)
    m, k = s.shape
    if mt.shape[0] != m:
        raise RuntimeError(
            f"Number of rows of meta matrix {mt.shape[0]} must be equal to number of columns of spase matrix {m}"
        )
    dense = torch.empty((m, 2 * k), dtype=s.dtype, device=dev)
    call("ct_cutlass24_to_dense", ptr(s), DT[s.dtype], ptr(mt), mt.dtype.itemsize, m, k, ptr(dense), stream_of(s))
    return _home(dense, sparse)


def marlin24_quant_compress(weight: torch.Tensor, scale: torch.Tensor, zero_point, *, num_bits: int, group_size: Optional[int]):
    """fused marlin-24 front end: fp16 quantize + 2:4 compress of a 16-bit 2:4-sparse weight.
    Returns (codes int8 (m, k/2), meta int16 (m, k/16) reordered, violated: bool) — `violated` costs one
    host read, as the reference pipeline's structure check did."""
    dev = _compute_device(weight)
    w, s = _dev(weight, dev).contiguous(), _dev(scale, dev).contiguous()
    zp = _dev(zero_point, dev).contiguous() if zero_point is not None else None
    m, k = w.shape
    g = k if not group_size or group_size > k else int(group_size)
    comp = torch.empty((m, k // 2), dtype=torch.int8, device=dev)
    meta = torch.empty((m, k // 16), dtype=torch.int16, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    call("ct_marlin24_quant_compress", ptr(w), DT[w.dtype], ptr(s), DT[s.dtype], ptr(zp), DT[zp.dtype] if zp is not None else -1,
         m, k, g, int(num_bits), ptr(comp), ptr(meta), ptr(bad), stream_of(w))
    return _home(comp, weight), _home(meta, weight), bad


def marlin24_compress_w4(weight: torch.Tensor, scale: torch.Tensor, zero_point, *, group_size: Optional[int]):
    """fully fused int4 marlin-24 weight path (rows % 64 == 0, cols % 256 == 0): fp16 quantize + 2:4 compress
    + tile-permuted nibble packing in one launch.  Returns (weight_packed int32 (k/32, m*2), meta int16
    (m, k/16) reordered, violated flag tensor)."""
    dev = _compute_device(weight)
    w, s = _dev(weight, dev).contiguous(), _dev(scale, dev).contiguous()
    zp = _dev(zero_point, dev).contiguous() if zero_point is not None else None
    m, k = w.shape
    g = k if not group_size or group_size > k else int(group_size)
    packed = torch.empty((k // 32, m * 2), dtype=torch.int32, device=dev)
    meta = torch.empty((m, k // 16), dtype=torch.int16, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    call("ct_marlin24_compress_w4", ptr(w), DT[w.dtype], ptr(s), DT[s.dtype], ptr(zp), DT[zp.dtype] if zp is not None else -1,
         m, k, g, ptr(packed), ptr(meta), ptr(bad), stream_of(w))
    return _home(packed, weight), _home(meta, weight), bad


def marlin24_compress_w4_full(weight: torch.Tensor, scale: torch.Tensor, zero_point, *, group_size: Optional[int], group_perm: bool,
                              flag_ptr: Optional[int] = None, stream=None):
    """the whole int4 marlin-24 compress in ONE host call and (16-bit scales) ONE launch (`ct_marlin24_compress_w4_full`): the
    weight path of `marlin24_compress_w4` plus the permuted fp16 scales.  `flag_ptr`: device address of a pre-zeroed int32 the
    violation is OR-ed into (a slot of the caller's ring; nothing is cleared or read here); None allocates and clears one.
    GPU tensors only — no staging, this is the fast path, kept to three allocations and one ctypes call.  Returns
    (weight_packed, meta already in the stored (k/32, 2m) shape, scale_packed fp16 (groups, m), flag tensor or None)."""
    m, k = weight.shape
    dev = weight.device
    g = k if not group_size or group_size > k else int(group_size)
    packed = torch.empty((k // 32, m * 2), dtype=torch.int32, device=dev)
    meta = torch.empty((k // 32, m * 2), dtype=torch.int16, device=dev)  # the (m, k/16) reordered matrix, viewed as upstream stores it
    scale_packed = torch.empty((k // g, m), dtype=torch.float16, device=dev)
    flag = None
    if flag_ptr is None:
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        flag_ptr = flag.data_ptr()
    call("ct_marlin24_compress_w4_full", weight.data_ptr(), DT[weight.dtype], scale.data_ptr(), DT[scale.dtype],
         None if zero_point is None else zero_point.data_ptr(), -1 if zero_point is None else DT[zero_point.dtype], m, k, g, int(group_perm),
         packed.data_ptr(), meta.data_ptr(), scale_packed.data_ptr(), flag_ptr, int(flag is not None), stream if stream is not None else stream_of(weight))
    return packed, meta, scale_packed, flag


def selftest_m24_div(mode: int, s_lo_bits: int = 0, s_hi_bits: int = 65536) -> int:
    """mismatch count of the lean marlin-24 quotients against the IEEE divide (mode 0: fp16 / fp16 with the Newton step,
    mode 1: bf16 / bf16 by one multiply; mode 2: the kernel's reciprocal against `1.0f / s`, bit for bit)"""
    dev = _lib.require_device()
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    call("ct_selftest_m24_div", int(mode), s_lo_bits, s_hi_bits, ptr(out), stream_of(out))
    return int(out.item())


def marlin24_pack_weights(q: torch.Tensor, num_bits: int, *, transposed: bool = False, add_offset: bool = False):
    """marlin-24 weight packing.  q: (size_k, size_n) codes, or with transposed=True the
    un-transposed (size_n, size_k) 2:4-compressed matrix."""
    if num_bits not in (4, 8):
        raise ValueError("num_bits must be 4 or 8, got {}".format(num_bits))
    dev = _compute_device(q)
    qd = _dev(q, dev)
    size_k, size_n = (qd.shape[1], qd.shape[0]) if transposed else qd.shape
    out = torch.empty((size_k // 16, size_n * 16 * num_bits // 32), dtype=torch.int32, device=dev)
    call("ct_marlin24_pack_weights", ptr(qd), DT[qd.dtype], int(transposed), int(add_offset), size_k, size_n, num_bits,
         ptr(out), stream_of(qd))
    return _home(out, q)


def marlin24_pack_scales(scale: torch.Tensor, *, single: bool, to_float16: bool = False):
    """marlin-24 scale packing: (size_n, groups) -> permuted (groups, size_n); to_float16 folds the reference's
    `scale.to(torch.float16)` into the same kernel (a bfloat16 scale comes out as float16)."""
    dev = _compute_device(scale)
    s = _dev(scale, dev)
    size_n, groups = s.shape
    out = torch.empty((groups, size_n), dtype=torch.float16 if to_float16 else s.dtype, device=dev)
    call("ct_marlin24_pack_scales_f16" if to_float16 else "ct_marlin24_pack_scales", ptr(s), DT[s.dtype], size_n, groups, int(single), ptr(out), stream_of(s))
    return _home(out, scale)


# --------------------------------------------------------------------------- FP4 (E2M1) codecs
_FP4_SCALE_KIND = {"plain": 0, "f8e4m3": 1, "e8m0": 2}


def cast_to_fp4(x: torch.Tensor) -> torch.Tensor:
    """quantization/utils/fp4_utils.py:77-98: nearest E2M1 value (0, 0.5, 1, 1.5, 2, 3, 4, 6 and negatives), same dtype."""
    if x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise NotImplementedError(f"cast_to_fp4 takes float tensors, got {x.dtype}")
    dev = _compute_device(x)
    xin = _dev(x, dev).contiguous()
    out = torch.empty_like(xin)
    call("ct_fp4_cast", ptr(xin), DT[xin.dtype], ptr(out), xin.numel(), stream_of(xin))
    return _home(out, x)


def pack_fp4_to_uint8(x: torch.Tensor) -> torch.Tensor:
    """compressors/nvfp4/helpers.py:108-150 (same argument, same error): (m, n) E2M1-valued -> uint8 (m, n / 2)."""
    m, n = x.shape
    if n % 2 != 0:
        raise ValueError("tensor must have an even number of columns for nvfp4 compression")
    if x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        x = x.to(torch.bfloat16)
    dev = _compute_device(x)
    xin = _dev(x, dev).contiguous()
    out = torch.empty((m, n // 2), dtype=torch.uint8, device=dev)
    call("ct_fp4_pack", ptr(xin), DT[xin.dtype], ptr(out), xin.numel(), stream_of(xin))
    return _home(out, x)


def unpack_fp4_from_uint8(a: torch.Tensor, m: int, n: int, dtype: Optional[torch.dtype] = torch.bfloat16) -> torch.Tensor:
    """compressors/nvfp4/helpers.py:153-193 (same arguments): uint8 (m, n / 2) -> (m, n) E2M1 values of `dtype`."""
    assert a.dtype == torch.uint8
    dtype = dtype or torch.float32  # upstream's lookup table is float32
    if dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise NotImplementedError(f"unpack_fp4_from_uint8 produces float tensors, got {dtype}")
    if a.numel() * 2 != m * n:
        raise ValueError(f"{a.numel()} packed bytes do not hold a {m} x {n} tensor")
    dev = _compute_device(a)
    ain = _dev(a, dev).contiguous()
    out = torch.empty((m, n), dtype=dtype, device=dev)
    call("ct_fp4_unpack", ptr(ain), m * n, ptr(out), DT[dtype], stream_of(ain))
    return _home(out, a)


def compress_mx_scale(scale: torch.Tensor, scale_dtype: torch.dtype = torch.uint8) -> torch.Tensor:
    """compressors/mx_utils.py:18-31: E8M0 code 127 + floor(log2(scale)); log2 is evaluated in the scale's dtype, as
    upstream (a small tensor: one element per 32 weights).  16-bit scales on the GPU: ONE launch that reads the codes from the table of this very
    expression over every 16-bit pattern (`_mx_code_table`) instead of four tensor ops."""
    if scale.is_cuda and scale_dtype is torch.uint8 and scale.dtype in (torch.bfloat16, torch.float16) and scale.is_contiguous() and scale.numel():
        out = torch.empty(scale.shape, dtype=torch.uint8, device=scale.device)
        call("ct_mx_scale_compress", ptr(scale), DT[scale.dtype], scale.numel(), ptr(_mx_code_table(scale.dtype, scale.device)), ptr(out), stream_of(scale))
        return out
    return (127 + torch.floor(torch.log2(scale)).to(torch.int32)).to(scale_dtype)


def decompress_mx_scale(scale: torch.Tensor) -> torch.Tensor:
    """compressors/mx_utils.py:34-44: 2 ** (code - 127) as bfloat16 (uint8 codes on the GPU: one launch)"""
    if scale.is_cuda and scale.dtype is torch.uint8 and scale.is_contiguous() and scale.numel():
        out = torch.empty(scale.shape, dtype=torch.bfloat16, device=scale.device)
        call("ct_mx_scale_decompress", ptr(scale), scale.numel(), ptr(out), stream_of(scale))
        return out
    return 2.0 ** (scale.to(torch.int32) - 127).to(torch.bfloat16)


_MX_CODE_TABLES = {}


def _mx_code_table(dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    """compress_mx_scale(scale, uint8) (mx_utils.py:18-31) of EVERY 16-bit pattern of `dtype`, evaluated once by that very expression on the host and
    kept on `device` (64 KB): the MXFP4 compress kernel reads its groups' stored codes from it, so they are upstream's for every input"""
    key = (dtype, device)
    t = _MX_CODE_TABLES.get(key)
    if t is None:
        every = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
        t = _MX_CODE_TABLES[key] = compress_mx_scale(every, torch.uint8).contiguous().to(device)
    return t


def _gs_fast(global_scale, dev):
    """the global scale as a contiguous float32 tensor of one element on `dev` (as _gs_arg; without tensor ops when it already is one)"""
    if global_scale is None:
        return None
    if global_scale.dtype is torch.float32 and global_scale.numel() == 1 and global_scale.device == dev and global_scale.data_ptr() % 4 == 0:
        return global_scale
    return _dev(global_scale, dev).to(torch.float32).reshape(-1)[:1].contiguous()


def fp4_quantize_and_pack_stored(weight: torch.Tensor, scale: torch.Tensor, global_scale: Optional[torch.Tensor], *, group_size: int, scale_dtype: torch.dtype):
    """`fp4_quantize_and_pack` plus the scale in its STORED form from the same launch — NVFP4 (group 16): `scale.to(float8_e4m3fn)`; MXFP4 (group 32):
    `compress_mx_scale(scale, uint8)` — or None when the layout is outside that kernel (the caller then converts the scale itself).  Returns
    (packed, stored_scale)."""
    want = torch.float8_e4m3fn if group_size == 16 else torch.uint8
    if (scale_dtype is not want or weight.dim() != 2 or weight.dtype not in (torch.bfloat16, torch.float16) or not weight.is_cuda or scale.device != weight.device
            or scale.dtype not in _FLOATS or (group_size == 32 and scale.dtype is torch.float32) or (global_scale is not None) != (group_size == 16)
            or not weight.is_contiguous() or not scale.is_contiguous() or weight.data_ptr() % 16 or scale.data_ptr() % 8):
        return None
    rows, cols = weight.shape
    if cols % group_size or (rows * cols) % 32 or tuple(scale.shape) != (rows, cols // group_size) or rows == 0:
        return None
    dev = weight.device
    gs = _gs_fast(global_scale, dev)
    out = torch.empty((rows, cols // 2), dtype=torch.uint8, device=dev)
    stored = torch.empty((rows, cols // group_size), dtype=want, device=dev)
    lut = _mx_code_table(scale.dtype, dev) if group_size == 32 else None
    call("ct_fp4_quant_pack_stored", ptr(weight), DT[weight.dtype], ptr(scale), DT[scale.dtype], ptr(gs), rows, cols, int(group_size), ptr(out), ptr(stored), ptr(lut),
         stream_of(weight))
    return out, stored


def fp4_quantize_and_pack(weight: torch.Tensor, scale: torch.Tensor, global_scale: Optional[torch.Tensor], *, group_size: int) -> torch.Tensor:
    """quantize(x, scale, global_scale, FP4 args) -> cast_to_fp4 -> pack_fp4_to_uint8 in one launch
    (compressors/nvfp4/base.py:88-95): uint8 (rows, cols / 2)."""
    if weight.dim() != 2:
        raise ValueError("FP4 compression expects a 2-D weight")
    if weight.shape[1] % 2 != 0:
        raise ValueError("tensor must have an even number of columns for nvfp4 compression")
    if weight.dtype not in _FLOATS:
        raise NotImplementedError(f"the MI355X FP4 path compresses float weights, got {weight.dtype}")
    dev = _compute_device(weight)
    w, s = _dev(weight, dev).contiguous(), _dev(scale, dev).contiguous()
    rows, cols = w.shape
    if tuple(s.shape) != (rows, cols // group_size):
        raise ValueError(f"scale shape {tuple(s.shape)} does not match ({rows}, {cols // group_size}) for group size {group_size}")
    gs = _gs_fast(global_scale, dev)
    out = torch.empty((rows, cols // 2), dtype=torch.uint8, device=dev)
    call("ct_fp4_quant_pack", ptr(w), DT[w.dtype], ptr(s), DT[s.dtype], ptr(gs), rows, cols, int(group_size), ptr(out), stream_of(w))
    return _home(out, weight)


def fp4_unpack_and_dequantize(packed: torch.Tensor, scale: torch.Tensor, global_scale: Optional[torch.Tensor], *, group_size: int,
                              scale_kind: str = "plain", dtype: torch.dtype = torch.bfloat16, return_scale: bool = False):
    """unpack_fp4_from_uint8 -> dequantize(x_q, scale, global_scale) in one launch (nvfp4/base.py:118-131).  `scale` is
    the STORED scale: float8-e4m3 (scale_kind "f8e4m3"), E8M0 uint8 ("e8m0") or a float tensor ("plain").
    `return_scale`: also the decompressed scale as bfloat16 — `scale.to(bfloat16)` resp. `decompress_mx_scale(scale)` — written by the same launch:
    returns (weight, scale_bf16)."""
    if packed.dtype != torch.uint8 or packed.dim() != 2:
        raise ValueError("packed FP4 weights are 2-D uint8 tensors")
    dev = _compute_device(packed)
    p, s = _dev(packed, dev).contiguous(), _dev(scale, dev).contiguous()
    rows, cols = p.shape[0], p.shape[1] * 2
    kind = _FP4_SCALE_KIND[scale_kind]
    sview = s.view(torch.uint8) if kind == 1 else s
    sdt = DT[sview.dtype] if kind == 0 else -1
    gs = _gs_fast(global_scale, dev)
    out = torch.empty((rows, cols), dtype=dtype, device=dev)
    if return_scale:
        sout = torch.empty((rows, cols // int(group_size)), dtype=torch.bfloat16, device=dev)
        if rows and cols:
            call("ct_fp4_unpack_dequant_scale", ptr(p), rows, cols, ptr(sview), kind, sdt, ptr(gs), int(group_size), ptr(out), DT[dtype], ptr(sout), stream_of(p))
        return _home(out, packed), _home(sout, packed)
    call("ct_fp4_unpack_dequant", ptr(p), rows, cols, ptr(sview), kind, sdt, ptr(gs), int(group_size), ptr(out), DT[dtype], stream_of(p))
    return _home(out, packed)


# --------------------------------------------------------------------------- diagnostics
def selftest_bf16_div(s_lo_bits: int = 0, s_hi_bits: int = 65536) -> int:
    """number of (x, s) bf16 pairs for which the reciprocal fast path disagrees with the IEEE
    divide (must be 0; see ct_quant.hip)."""
    dev = _lib.require_device()
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    call("ct_selftest_bf16_div", s_lo_bits, s_hi_bits, ptr(out), torch.cuda.current_stream(dev).cuda_stream)
    return int(out.item())


def selftest_f16_div(s_lo_bits: int = 0, s_hi_bits: int = 65536) -> int:
    """number of (x, s) fp16 pairs for which the reciprocal + Newton quotient of the marlin-24 front end
    disagrees with the IEEE divide after rounding to fp16 (must be 0; see ct_marlin24.hip)."""
    dev = _lib.require_device()
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    call("ct_selftest_f16_div", s_lo_bits, s_hi_bits, ptr(out), torch.cuda.current_stream(dev).cuda_stream)
    return int(out.item())


def selftest_fp4_div(x_dtype: torch.dtype = torch.bfloat16, m_lo: int = 0, m_hi: int = 1 << 23) -> int:
    """number of (x mantissa, s mantissa) pairs for which the shared-reciprocal quotient of the FP4 compress kernel
    differs from the IEEE fp32 divide (must be 0; see ct_fp4.hip)."""
    dev = _lib.require_device()
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    call("ct_selftest_fp4_div", DT[x_dtype], m_lo, m_hi, ptr(out), torch.cuda.current_stream(dev).cuda_stream)
    return int(out.item())
