"""Generate the group-wise 8-bit round-to-nearest fixture by running the UPSTREAM REFERENCE on the CPU over the case matrix of
tests/_group8_rtn_cases.py: torch.amin / amax over each group of columns, calculate_qparams (its MX branch for MXFP8), then
quantize(strategy = group) — FLOAT with the all-zero zero point of a calibrated scheme present, as the compressors call it —, then
compress_mx_scale (MXFP8) and pack_to_int32 at 8 bits (INT: the pack-quantized words).  Everything is imported from the reference tree at
generation time, never copied (needs the reference sources; see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_group8_rtn.py [--check]

Writes tests/golden/group8_rtn.safetensors: `<key>.x` (the input) and `<key>.<kind>.{scale,q}` plus `.zero_point` / `.packed` (INT) and `.e8m0`
(MXFP8); float8 tensors as bytes.  The inputs are integer-synthesised: two runs write byte-identical files.  `--check` writes nothing and fails
if the committed file differs.
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

import _group8_rtn_cases as C  # noqa: E402
from compressed_tensors.compressors.mx_utils import compress_mx_scale  # noqa: E402
from compressed_tensors.compressors.pack_quantized.helpers import pack_to_int32  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors.quantization.lifecycle.forward import quantize  # noqa: E402
from compressed_tensors.quantization.utils.helpers import calculate_qparams  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "group8_rtn.safetensors")


def reference(x, group, kind):
    args = QuantizationArgs(strategy="group", group_size=group, **C.KINDS[kind])
    grouped = x.reshape(x.shape[0], x.shape[1] // group, group)
    scale, zp = calculate_qparams(grouped.amin(dim=-1), grouped.amax(dim=-1), args)
    if args.type == "float":
        q = quantize(x, scale, torch.zeros(scale.shape, dtype=C.F8), args, dtype=args.pytorch_dtype())
        out = dict(scale=scale, q=q)
        if kind == "mxfp8":
            out["e8m0"] = compress_mx_scale(scale, torch.uint8)
        return out
    q = quantize(x, scale, zp, args, dtype=args.pytorch_dtype())
    return dict(scale=scale, zero_point=zp, q=q, packed=pack_to_int32(q, 8))


def build() -> bytes:
    tensors = {}
    for key, recipe in C.case_list():
        x = C.make_weight(recipe)
        tensors[f"{key}.x"] = x
        for kind in C.kinds_of(recipe):
            for name, t in reference(x, recipe["group"], kind).items():
                tensors[f"{key}.{kind}.{name}"] = t.contiguous().view(torch.uint8) if t.dtype == C.F8 else t.contiguous()
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
