"""Generate the pack-quantized W2-W7 round-to-nearest fixture by running the UPSTREAM REFERENCE on the CPU over the case matrix of
tests/_packw_rtn_cases.py: torch.amin / amax over each group of columns (channel-wise: over the row), calculate_qparams, quantize, then
pack_to_int32(q, bits) and, for an asymmetric scheme, pack_to_int32(zero_point, bits, packed_dim=0) — what
PackedQuantizationCompressor.compress stores.  Everything is imported from the reference tree at generation time, never copied (needs the
reference sources; see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_packw_rtn.py [--check]

Writes tests/golden/packw_rtn.safetensors: `<key>.x` (the input) and `<key>.w<bits>[a].{scale,zero_point,packed}` plus `.zp_packed` for the
asymmetric (`a`) schemes.  The inputs are integer-synthesised: two runs write byte-identical files.  `--check` writes nothing and fails if the
committed file differs.
TEST INFRASTRUCTURE ONLY.  Nothing in the product imports this.
"""
import os
import sys

import torch
from safetensors.torch import save

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402

ref_import.import_reference()

import _packw_rtn_cases as C  # noqa: E402
from compressed_tensors.compressors.pack_quantized.helpers import pack_to_int32  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors.quantization.lifecycle.forward import quantize  # noqa: E402
from compressed_tensors.quantization.utils.helpers import calculate_qparams  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "packw_rtn.safetensors")


def reference(x, group, bits, symmetric):
    if group:
        args = QuantizationArgs(num_bits=bits, type="int", symmetric=symmetric, strategy="group", group_size=group)
        grouped = x.reshape(x.shape[0], x.shape[1] // group, group)
        mn, mx = grouped.amin(dim=-1), grouped.amax(dim=-1)
    else:
        args = QuantizationArgs(num_bits=bits, type="int", symmetric=symmetric, strategy="channel")
        mn, mx = x.amin(dim=-1, keepdim=True), x.amax(dim=-1, keepdim=True)
    scale, zp = calculate_qparams(mn, mx, args)
    q = quantize(x, scale, zp, args, dtype=torch.int8)
    out = dict(scale=scale, zero_point=zp, packed=pack_to_int32(q, bits))
    if not symmetric:
        out["zp_packed"] = pack_to_int32(zp, bits, packed_dim=0)
    return out


def build() -> bytes:
    tensors = {}
    for key, recipe in C.case_list():
        x = C.make_weight(recipe)
        tensors[f"{key}.x"] = x
        for bits in recipe["bits"]:
            for symmetric in (True, False):
                for name, t in reference(x, recipe["group"], bits, symmetric).items():
                    tensors[f"{key}.{C.tag(bits, symmetric)}.{name}"] = t.contiguous()
    return save(tensors)


def main():
    blob = build()
    if "--check" in sys.argv[1:]:
        with open(PATH, "rb") as f:
            if f.read() != blob:
                raise SystemExit(f"{PATH} differs from what the reference produces")
        print("fixture matches")
        return
    with open(PATH, "wb") as f:
        f.write(blob)
    print(f"{len(C.case_list())} cases, {len(blob)} bytes")


if __name__ == "__main__":
    main()
