"""Generate the block-wise 8-bit round-to-nearest fixtures by running the UPSTREAM REFERENCE on the CPU over the case matrix of
tests/_block_rtn_cases.py: the weight padded to whole blocks (maybe_pad_tensor_for_block_quant), torch.amin / amax over each block,
calculate_qparams, then quantize(strategy = block) — FLOAT with the all-zero float8 zero point of a calibrated scheme present, as the
compressors call it.  Everything is imported from the reference tree at generation time, never copied (needs the reference sources; see
oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_block_rtn.py [--check]

Writes tests/golden/block_rtn.safetensors (`<key>.<kind>.{scale,zero_point,q}`; float8 tensors as bytes; the codes `q` in full for the FP8 kind
of the smaller cases, `_block_rtn_cases.stores_codes`) and tests/golden/block_rtn_manifest.json (every case: its recipe, the sha256 of the
synthesised input, dtype, shape and sha256 of every result, the codes of every kind included).  The
inputs are integer-synthesised: two runs write byte-identical files.  `--check` writes nothing and fails if the committed files differ.
TEST INFRASTRUCTURE ONLY.  Nothing in the product imports this.
"""
import json
import os
import sys

import torch
from safetensors.torch import save

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402

ref_import.import_reference()

import _block_rtn_cases as C  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors.quantization.lifecycle.forward import quantize  # noqa: E402
from compressed_tensors.quantization.utils.helpers import calculate_qparams, maybe_pad_tensor_for_block_quant  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def reference(x, block, kind):
    args = QuantizationArgs(strategy="block", block_structure=list(block), **C.KINDS[kind])
    bh, bw = block
    p = maybe_pad_tensor_for_block_quant(x, tuple(block))
    blocks = p.reshape(p.shape[0] // bh, bh, p.shape[1] // bw, bw)
    scale, zp = calculate_qparams(blocks.amin(dim=(1, 3)), blocks.amax(dim=(1, 3)), args)
    q = quantize(x, scale, zp, args, dtype=args.pytorch_dtype())
    return dict(scale=scale, zero_point=zp, q=q)


def build():
    tensors, manifest = {}, {"cases": {}}
    for key, recipe in C.case_list():
        x = C.make_weight(recipe)
        entry = dict(recipe=recipe, x_sha256=C.sha(x), out={})
        for kind in C.KINDS:
            for name, t in reference(x, recipe["block"], kind).items():
                entry["out"][f"{kind}.{name}"] = dict(dtype=str(t.dtype).replace("torch.", ""), shape=list(t.shape), sha256=C.sha(t))
                if name == "q" and not C.stores_codes(recipe, kind):
                    continue  # the manifest's sha256 stands for them
                tensors[f"{key}.{kind}.{name}"] = t.contiguous().view(torch.uint8) if t.dtype == C.F8 else t.contiguous()
        manifest["cases"][key] = entry
    return save(tensors), (json.dumps(manifest, indent=1, sort_keys=True) + "\n").encode()


def main():
    blob, text = build()
    paths = (os.path.join(OUT, "block_rtn.safetensors"), os.path.join(OUT, "block_rtn_manifest.json"))
    if "--check" in sys.argv[1:]:
        for path, want in zip(paths, (blob, text)):
            with open(path, "rb") as f:
                if f.read() != want:
                    raise SystemExit(f"{path} differs from what the reference produces")
        print("fixtures match")
        return
    for path, data in zip(paths, (blob, text)):
        with open(path, "wb") as f:
            f.write(data)
    print(f"{len(json.loads(text)['cases'])} cases, {len(blob)} + {len(text)} bytes")


if __name__ == "__main__":
    main()
