"""FP8 block-quantized checkpoints -> `mxfp4-pack-quantized` checkpoints without the dense checkpoint in between (no reference counterpart: the
reference reaches MXFP4 from such a checkpoint through `FP8BlockDequantizer`, a model load and `compress_model`).

MI355X design of `FP8BlockToMXFP4Converter.process`: the float8_e4m3fn `weight` and the `weight_scale_inv` of ALL targeted modules of a shard are
staged to the GPU through one pinned buffer and one copy, ONE `ct_fp8block_mxfp4_batch` launch per shard (csrc/ct_fp4.hip: the dequantized element
rounded to `dtype` in registers, then the one-pass MXFP4 compress on those bits) writes every `weight_packed` and `weight_scale` into one output
buffer, and the results come back through one pinned buffer.  The bytes are those of the composition — `FP8BlockDequantizer(dtype=dtype)`, then the
one-pass MXFP4 compress of the dense weights —, which is also the path of what the fused plan refuses and of `fused=False`: one
`ct_fp8block_dequant_batch` launch into a dense device buffer and one `rtn_mxfp4` table launch over it.

The body — staging, the admission test, the fused launch with the composition over the rest, the copies back, `validate`, `get_dependencies` — is
fp8block_transcode.py's, shared with the MXFP8 and NVFP4 converters; this module holds the MXFP4 names."""
from typing import List

import torch

from . import fp8block_transcode as _body
from .fp8block_transcode import MXFP4, FP8BlockTranscoder
from .staging import ReadyDict

__all__ = ["FP8BlockToMXFP4Converter", "FP8BLOCK_MXFP4_MEASURED_FASTER"]

# the dispatch of `fused=None`: True only when tools/fp8block_mxfp4_bench.py has measured the fused launch's median below the composition's MINIMUM
# on both of its tables in both of its runs (the project's dispatch rule).  profiles/fp8block_mxfp4_bench.jsonl, µs, run 1 / run 2:
# DeepSeek-V3.2-shaped table fused 846 / 841 against the composition's minimum 1249 / 1249, Qwen3-4B-shaped one 2658 / 2680 against 4241 / 4233
FP8BLOCK_MXFP4_MEASURED_FASTER = True


def _fused_admits(w: torch.Tensor, packed: torch.Tensor, block) -> bool:
    """what `ct_fp8block_mxfp4_plan` asks of a row beyond the checks made before anything was staged: the plan is never handed a row it would refuse"""
    return _body.fused_admits(MXFP4, w, packed, block)


def transcode(out: ReadyDict, modules: List[str], pairs, block, dtype, dev, fused: bool, to_host: bool = True, stream_results: bool = False) -> None:
    """`out[f"{module}.weight_packed"]` / `out[f"{module}.weight_scale"]` of every (weight, weight_scale_inv) pair: one staging copy, one fused launch
    over the rows its plan admits (`fused`), the composition over the others, one copy back (`to_host`; else device tensors of their own)"""
    _body.transcode(MXFP4, out, modules, pairs, block, dtype, dev, fused, to_host, stream_results)


class FP8BlockToMXFP4Converter(FP8BlockTranscoder):
    """Transcode a checkpoint block-quantized with the FP8 quant_method (`weight` float8_e4m3fn, `weight_scale_inv` per block) to the MXFP4 scheme in
    the compressed-tensors `mxfp4-pack-quantized` format: per targeted module `weight_packed` (uint8, (rows, cols / 2)) where the weight was and
    `weight_scale` (uint8 E8M0 exponents, (rows, cols / 32)) behind it; the `weight_scale_inv` is dropped.  The bytes are those of
    `FP8BlockDequantizer(dtype=dtype)` followed by the round-to-nearest MXFP4 compress of the dense weights.  `activations=True` writes the MXFP4
    preset (dynamic MXFP4 input activations) instead of MXFP4A16; `fused`: None follows `FP8BLOCK_MXFP4_MEASURED_FASTER`, True / False force the one
    launch / the composition."""

    target, format = MXFP4, MXFP4.format

    def _measured(self) -> bool:
        return FP8BLOCK_MXFP4_MEASURED_FASTER
