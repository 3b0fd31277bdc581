"""Generate the dynamic activation QDQ fixtures by running the UPSTREAM REFERENCE's compute_dynamic_scales_and_zp and
fake_quantize (quantization/utils/helpers.py:140-195, quantization/lifecycle/forward.py:148-181) on the CPU over the case
matrix of tests/_dynamic_cases.py (needs the reference sources; see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_dynamic.py

Writes tests/golden/dynamic.safetensors (the small bfloat16 cases: `<key>.out`, `<key>.scale`, `<key>.zp`) and
tests/golden/dynamic_manifest.json (every case: its recipe, the sha256 of the synthesised input, the dtypes and shapes of the
reference's outputs and the sha256 of each output with NaNs canonicalised, and `out_nan` / `out_distinct`: how many elements
of the reference's output are NaN and how many distinct values the others take — tests/test_dynamic_quant.py holds the finite
whole-tensor cases to them).  The inputs are integer-synthesised: two runs write byte-identical files.
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

import _dynamic_cases as C  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors.quantization.lifecycle.forward import fake_quantize  # noqa: E402
from compressed_tensors.quantization.utils import compute_dynamic_scales_and_zp  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def reference(recipe):
    x = C.make_input(recipe)
    args = QuantizationArgs(**C.PRESETS[recipe["preset"]])
    gs = C.global_scale_of(recipe["gs"]) if recipe["gs"] else None
    scale, zp = compute_dynamic_scales_and_zp(value=x, args=args, module=None, global_scale=gs)
    out = fake_quantize(x=x, scale=scale, zero_point=zp, args=args, g_idx=None, global_scale=gs)
    return x, out, scale, zp


def main():
    tensors, manifest = {}, {"cases": {}}
    for key, recipe in C.case_list():
        x, out, scale, zp = reference(recipe)
        nan = torch.isnan(out)
        entry = dict(recipe=recipe, stored=C.stored(recipe), x_sha256=C.sha(x), out_nan=int(nan.sum()),
                     out_distinct=int(torch.unique(out[~nan].float()).numel()))
        for name, t in (("out", out), ("scale", scale), ("zp", zp)):
            entry[name] = dict(dtype=str(t.dtype).replace("torch.", ""), shape=list(t.shape), sha256=C.sha(t))
        if entry["stored"]:
            for name, t in (("out", out), ("scale", scale), ("zp", zp)):
                tensors[f"{key}.{name}"] = t.contiguous() if t.dtype != C.F8 else t.contiguous().view(torch.uint8)
        manifest["cases"][key] = entry
    path = os.path.join(OUT, "dynamic.safetensors")
    save_file(tensors, path)
    os.chmod(path, 0o644)
    with open(os.path.join(OUT, "dynamic_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(manifest['cases'])} cases, {len(tensors)} stored tensors")


if __name__ == "__main__":
    main()
