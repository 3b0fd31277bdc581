"""Generate the attention q / k / v QDQ fixtures by running the UPSTREAM REFERENCE's fake_quantize / quantize / dequantize
(quantization/lifecycle/forward.py:36-181) on the CPU over the case matrix of tests/_attn_cases.py (needs the reference sources;
see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_attn.py

Writes tests/golden/attn.safetensors (the small bfloat16 cases: `<key>.out`) and tests/golden/attn_manifest.json (every case: its
recipe, the sha256 of the synthesised input, and the dtype, shape, strides and sha256 — NaNs canonicalised — of the reference's
output).  The inputs are integer-synthesised: two runs write byte-identical files.
TEST INFRASTRUCTURE ONLY.  Nothing in the product imports this.
"""
import json
import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402

ref_import.import_reference()

import _attn_cases as C  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors.quantization.lifecycle.forward import dequantize, fake_quantize, quantize  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def reference(recipe):
    x = C.make_input(recipe)
    scale, zp = C.make_qparams(recipe)
    args = QuantizationArgs(strategy=C.strategy_of(recipe), **C.KINDS[recipe["kind"]])
    if recipe["mode"] == "fake":
        out = fake_quantize(x=x, scale=scale, zero_point=zp, args=args)
    else:
        out = quantize(x=x, scale=scale, zero_point=zp, args=args, dtype=C.quantized_dtype(recipe))
        if recipe["mode"] == "dequantize":
            out = dequantize(x_q=out, scale=scale, zero_point=zp, args=args)
    return x, out


def main():
    tensors, manifest = {}, {"cases": {}}
    for key, recipe in C.case_list():
        x, out = reference(recipe)
        entry = dict(recipe=recipe, stored=C.stored(recipe), x_sha256=C.sha(x), x_strides=list(x.stride()),
                     out=dict(dtype=str(out.dtype).replace("torch.", ""), shape=list(out.shape), strides=list(out.stride()), sha256=C.sha(out)))
        if entry["stored"]:
            tensors[f"{key}.out"] = out.contiguous() if out.dtype != C.F8 else out.contiguous().view(torch.uint8)
        manifest["cases"][key] = entry
    save_file(tensors, os.path.join(OUT, "attn.safetensors"))
    with open(os.path.join(OUT, "attn_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(manifest['cases'])} cases, {len(tensors)} stored tensors")


if __name__ == "__main__":
    main()
