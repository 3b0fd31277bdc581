"""Quantization parameter generation on the GPU.

`calculate_qparams_from_weight` fuses the min-max observer with the reference's
calculate_qparams (quantization/utils/helpers.py:50-137) in one streaming pass over the weight.
"""
import torch

from .. import codec
from .quant_args import enum_value

__all__ = ["calculate_qparams_from_weight", "block_one_pass", "group_one_pass", "is_module_quantized"]


@torch.no_grad()
def _float_kind(args) -> str:
    """which calculate_qparams branch a FLOAT scheme takes (helpers.py:83-112, mxfp_utils.py:37-43)"""
    bits, gs, sdt = int(args.num_bits), getattr(args, "group_size", None), getattr(args, "scale_dtype", None)
    if bits in (4, 8) and gs == 32 and sdt == torch.uint8:
        return "mxfp4" if bits == 4 else "mxfp8"
    if bits == 4:
        return "nvfp4"
    if bits == 8 and sdt is None:
        return "fp8"
    raise NotImplementedError(f"calculate_qparams_from_weight: FLOAT scheme with num_bits={bits}, scale_dtype={sdt} is not supported")


def block_one_pass(weight: torch.Tensor, args) -> bool:
    """does the one-pass block-wise 8-bit kernel (codec.rtn_quantize_block8; its plan, ct_rtn_block8_batch_plan) take this weight under these
    block-strategy args?  8 bits, INT or symmetric FLOAT with scales in the weight's dtype, a 2-D bf16 / fp16 weight, a block the plan admits"""
    qtype = enum_value(getattr(args, "type", "int"))
    return (int(args.num_bits) == 8 and weight.dim() == 2 and weight.dtype in (torch.bfloat16, torch.float16)
            and bool(codec.rtn_block8_group(weight.shape, getattr(args, "block_structure", None)))
            and (qtype == "int" or (qtype == "float" and bool(args.symmetric) and getattr(args, "scale_dtype", None) is None)))


def group_one_pass(weight: torch.Tensor, args) -> str:
    """does the one-pass group-wise 8-bit kernel (codec.rtn_quantize_group8; its plan, ct_rtn_group8_batch_plan) take this weight under these
    args?  Then which of its forms: "mxfp8" (FLOAT, groups of 32, uint8 scales), "fp8" (symmetric FLOAT, scales in the weight's dtype), "int" or
    "int_asym"; else "".  8 bits, the group strategy (or a channel as one group), no activation ordering, a 2-D bf16 / fp16 weight — 16-byte
    aligned where it already is on a GPU — and a group the plan admits"""
    qtype, st = enum_value(getattr(args, "type", "int")), enum_value(args.strategy)
    if (int(args.num_bits) != 8 or st not in ("group", "channel") or enum_value(getattr(args, "actorder", None)) == "group" or weight.dim() != 2
            or weight.dtype not in (torch.bfloat16, torch.float16) or not weight.is_contiguous() or (weight.is_cuda and weight.data_ptr() % 16)):
        return ""
    group = getattr(args, "group_size", None) if st == "group" else None
    if st == "group" and not group:
        return ""
    if not codec.rtn_group8_group(weight.shape, group):
        return ""
    if qtype == "int":
        return "int" if args.symmetric else "int_asym"
    if qtype != "float" or not args.symmetric:
        return ""
    sdt = getattr(args, "scale_dtype", None)
    if sdt is None:
        return "fp8"
    return "mxfp8" if sdt == torch.uint8 and st == "group" and int(group) == 32 else ""


def _block_rows(weight: torch.Tensor, block_structure):
    """the blocks of a 2-D weight as rows — zero-padded to whole blocks (maybe_pad_tensor_for_block_quant, helpers.py:400-428), (row blocks, bh,
    column blocks, bw) transposed to (row blocks, column blocks, bh * bw) — and the block grid's shape"""
    if weight.dim() != 2 or block_structure is None or len(block_structure) != 2:
        raise ValueError("the block strategy needs a 2-D weight and block_structure = [rows, cols] per block")
    bh, bw = int(block_structure[0]), int(block_structure[1])
    rows, cols = weight.shape
    rb, cb = -(-rows // bh), -(-cols // bw)
    if rb * bh != rows or cb * bw != cols:
        weight = torch.nn.functional.pad(weight, (0, cb * bw - cols, 0, rb * bh - rows))
    return weight.reshape(rb, bh, cb, bw).transpose(1, 2).reshape(rb * cb, bh * bw), (rb, cb)


def calculate_qparams_from_weight(weight: torch.Tensor, args, global_scale=None):
    """scale / zero-point of a 2-D weight for tensor, channel, group or block strategies (a min-max observer followed by
    calculate_qparams, quantization/utils/helpers.py:50-137).  Shapes follow the reference's initialisation:
    tensor -> (1,), channel -> (R, 1), group / tensor_group -> (R, G), block -> (ceil(R / bh), ceil(C / bw)).  FLOAT schemes are symmetric:
    their zero point is an all-zero tensor of the scheme's zp_dtype; NVFP4 needs `global_scale` (codec.generate_gparam).
    block: the observer form of the one-pass kernel where its plan takes the weight (`block_one_pass`), else the blocks rearranged into
    rows (`_block_rows`) under the channel-wise observer — the same bits."""
    st = enum_value(args.strategy)
    if st == "block":
        fp = enum_value(getattr(args, "type", "int")) == "float"
        if fp and not args.symmetric:
            raise NotImplementedError("asymmetric FLOAT quantization parameters are not generated by the MI355X path")
        if block_one_pass(weight, args):
            _, scale, zp = codec.rtn_quantize_block8(weight, block_structure=args.block_structure, qtype="float" if fp else "int",
                                                     symmetric=bool(args.symmetric), codes=False)
        else:
            blocks, grid = _block_rows(weight, getattr(args, "block_structure", None))
            if fp:
                scale, zp = codec.minmax_qparams_float(blocks, kind=_float_kind(args)).reshape(grid), None
            else:
                scale, zp = (t.reshape(grid) for t in codec.minmax_qparams(blocks, num_bits=int(args.num_bits), symmetric=bool(args.symmetric)))
        if fp:
            zp = torch.zeros(scale.shape, dtype=getattr(args, "zp_dtype", None) or torch.float8_e4m3fn, device=scale.device)
        return scale, zp
    if enum_value(getattr(args, "type", "int")) == "float":
        if not args.symmetric:
            raise NotImplementedError("asymmetric FLOAT quantization parameters are not generated by the MI355X path")
        kind = _float_kind(args)
        if st == "tensor":
            scale = codec.minmax_qparams_float(weight.reshape(1, -1), kind=kind, global_scale=global_scale).reshape(1)
        elif st == "channel":
            scale = codec.minmax_qparams_float(weight, kind=kind, global_scale=global_scale)
        elif st in ("group", "tensor_group"):
            scale = codec.minmax_qparams_float(weight, kind=kind, group_size=int(args.group_size), global_scale=global_scale)
        else:
            raise NotImplementedError(f"calculate_qparams_from_weight: strategy {st!r} not supported")
        zp_dtype = getattr(args, "zp_dtype", None) or torch.float8_e4m3fn
        return scale, torch.zeros(scale.shape, dtype=zp_dtype, device=scale.device)
    kw = dict(num_bits=int(args.num_bits), symmetric=bool(args.symmetric))
    if st == "tensor":
        scale, zp = codec.minmax_qparams(weight.reshape(1, -1), group_size=None, **kw)
        return scale.reshape(1), zp.reshape(1)
    if st == "channel":
        return codec.minmax_qparams(weight, group_size=None, **kw)
    if st == "group":
        return codec.minmax_qparams(weight, group_size=int(args.group_size), **kw)
    raise NotImplementedError(f"calculate_qparams_from_weight: strategy {st!r} not supported")


def is_module_quantized(module) -> bool:
    """quantization/utils/helpers.py:229-250: a module is quantized when it carries a scheme
    with at least one of weights / input / output args"""
    scheme = getattr(module, "quantization_scheme", None)
    if scheme is None:
        return False
    return any(getattr(scheme, k, None) is not None for k in ("weights", "input_activations", "output_activations"))
