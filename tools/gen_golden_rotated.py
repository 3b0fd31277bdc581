"""Generate the fused rotation + dynamic QDQ fixtures by running the UPSTREAM REFERENCE on the CPU over the case matrix of
tests/_rotated_cases.py: HadamardTransform.forward (as tools/gen_golden_hadamard.py builds it), then
compute_dynamic_scales_and_zp and fake_quantize on its result (as tools/gen_golden_dynamic.py calls them).  Needs the reference
sources; see oracle/ref_import.py.

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_rotated.py

Writes tests/golden/rotated.safetensors (the small bfloat16 cases: `<key>.rotated`, `<key>.out`, `<key>.scale`, `<key>.zp`) and
tests/golden/rotated_manifest.json (every case: its recipe, the sha256 of the synthesised input, and the dtype, shape and
by-value sha256 of the reference's rotated intermediate, output, scale and zero point).  For EVERY case it asserts that the
reference's rotated intermediate equals the float32 butterfly by value: a case that fails this makes the generator fail, none is
dropped.  The inputs are integer-synthesised: two runs write byte-identical files.
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

import _hadamard_cases as H  # noqa: E402
import _rotated_cases as C  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors.quantization.lifecycle.forward import fake_quantize  # noqa: E402
from compressed_tensors.quantization.utils import compute_dynamic_scales_and_zp  # noqa: E402
from compressed_tensors.transform import TransformArgs, TransformScheme  # noqa: E402
from compressed_tensors.transform.factory.hadamard import HadamardTransform  # noqa: E402
from compressed_tensors.transform.utils.hadamard import deterministic_hadamard_matrix  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
_H = {}


def rotate(recipe, x):
    n = recipe["size"]
    if n not in _H:
        _H.clear()  # one matrix at a time
        _H[n] = torch.nn.Parameter(deterministic_hadamard_matrix(n, torch.float32, torch.device("cpu")), requires_grad=False)
    scheme = TransformScheme(type="hadamard", precision=torch.float32)
    args = TransformArgs(targets=["Linear"], location="input")
    with torch.no_grad():
        return HadamardTransform(_H[n], None, scheme, args, torch.nn.Linear)(x)


def reference(recipe):
    x = C.synth(recipe)
    rotated = rotate(recipe, x)
    args = QuantizationArgs(**C.PRESETS[recipe["preset"]])
    gs = C.D.global_scale_of(recipe["gs"]) if recipe["gs"] else None
    scale, zp = compute_dynamic_scales_and_zp(value=rotated, args=args, module=None, global_scale=gs)
    out = fake_quantize(x=rotated, scale=scale, zero_point=zp, args=args, g_idx=None, global_scale=gs)
    return x, rotated, out, scale, zp


def main():
    tensors, manifest = {}, {"cases": {}}
    for key, recipe in sorted(C.case_list(), key=lambda kr: kr[1]["size"]):  # matrices are built once per size
        x, rotated, out, scale, zp = reference(recipe)
        assert rotated.dtype == x.dtype and rotated.shape == x.shape and out.dtype == x.dtype and out.shape == x.shape
        # the condition of the family: the float32 butterfly restatement gives the reference's rotation, in every element
        assert C.equal_by_value(H.butterfly(x, recipe["size"]), rotated), key
        entry = dict(recipe=recipe, stored=C.stored(recipe), x_sha256=C.sha(x))
        parts = (("rotated", rotated), ("out", out), ("scale", scale), ("zp", zp))
        for name, t in parts:
            entry[name] = dict(dtype=str(t.dtype).replace("torch.", ""), shape=list(t.shape), sha256=C.sha(t))
        if entry["stored"]:
            for name, t in parts:
                tensors[f"{key}.{name}"] = t.contiguous() if t.dtype != C.F8 else t.contiguous().view(torch.uint8)
        manifest["cases"][key] = entry
        print(key, flush=True)
    path = os.path.join(OUT, "rotated.safetensors")
    save_file(tensors, path)
    os.chmod(path, 0o644)
    with open(os.path.join(OUT, "rotated_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    total = os.path.getsize(path) + os.path.getsize(os.path.join(OUT, "rotated_manifest.json"))
    assert total <= C.MAX_FIXTURE_BYTES, total
    print(f"{len(manifest['cases'])} cases, {len(tensors)} stored tensors, {total} bytes")


if __name__ == "__main__":
    main()
