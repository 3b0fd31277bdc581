"""Generate the fixtures of the fused head-dim rotation + attention QDQ by running the UPSTREAM REFERENCE on the CPU over
`fixture_cases()` of tests/_attn_rotated_cases.py: HadamardTransform.forward at location `q_attn` with the deterministic float32
weight (as tools/gen_golden_rotated.py builds it), then fake_quantize / quantize (as tools/gen_golden_attn.py calls them) on its
result.  Needs the reference sources; see oracle/ref_import.py.

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_attn_rotated.py

Writes tests/golden/attn_rotated.safetensors (the small bfloat16 cases: `<key>.out`) and tests/golden/attn_rotated_manifest.json
(every case: its recipe, the sha256 and strides of the synthesised input, and the dtype, shape, strides and by-value sha256 of the
reference's rotated intermediate and of its output).  For EVERY case it asserts that the rotation with float64 sums, rounded to
x's dtype, equals the reference's float32 GEMM result: a case that fails this makes the generator fail, none is dropped.  The
inputs are integer-synthesised: two runs write byte-identical files.
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

import _attn_cases as A  # noqa: E402
import _attn_rotated_cases as C  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors.quantization.lifecycle.forward import fake_quantize, quantize  # noqa: E402
from compressed_tensors.transform import TransformArgs, TransformScheme  # noqa: E402
from compressed_tensors.transform.factory.hadamard import HadamardTransform  # noqa: E402
from compressed_tensors.transform.utils.hadamard import deterministic_hadamard_matrix  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
_H = {}


def rotate(n, x):
    if n not in _H:
        _H[n] = torch.nn.Parameter(deterministic_hadamard_matrix(n, torch.float32, torch.device("cpu")), requires_grad=False)
    scheme = TransformScheme(type="hadamard", precision=torch.float32, head_dim=n)
    args = TransformArgs(targets=["LlamaAttention"], location="q_attn")
    with torch.no_grad():
        return HadamardTransform(_H[n], None, scheme, args, torch.nn.Module)(x)


def reference(recipe):
    x = C.make_input(recipe)
    rotated = rotate(recipe["n"], x)
    scale, zp = C.make_qparams(recipe)
    args = QuantizationArgs(strategy=A.strategy_of(recipe), **C.KINDS[recipe["kind"]])
    if recipe["mode"] == "fake":
        out = fake_quantize(x=rotated, scale=scale, zero_point=zp, args=args)
    else:
        out = quantize(x=rotated, scale=scale, zero_point=zp, args=args, dtype=A.quantized_dtype(recipe))
    return x, rotated, out


def main():
    tensors, manifest = {}, {"cases": {}}
    for key, recipe in C.fixture_cases():
        x, rotated, out = reference(recipe)
        assert rotated.dtype == x.dtype and rotated.shape == x.shape and out.shape == x.shape
        # the condition of the family: float64 sums, rounded once to x's dtype, give the reference's rotation in every element
        assert C.equal_by_value(C.rotation64(x, recipe["n"]), rotated), key
        entry = dict(recipe=recipe, stored=C.stored(recipe), x_sha256=C.sha(x), x_strides=list(x.stride()))
        for name, t in (("rotated", rotated), ("out", out)):
            entry[name] = dict(dtype=str(t.dtype).replace("torch.", ""), shape=list(t.shape), strides=list(t.stride()), sha256=C.sha(t))
        if entry["stored"]:
            tensors[f"{key}.out"] = out.contiguous() if out.dtype != C.F8 else out.contiguous().view(torch.uint8)
        manifest["cases"][key] = entry
        print(key, flush=True)
    assert 20 <= len(manifest["cases"]) <= 60, len(manifest["cases"])
    path = os.path.join(OUT, "attn_rotated.safetensors")
    save_file(tensors, path)
    os.chmod(path, 0o644)
    with open(os.path.join(OUT, "attn_rotated_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    sizes = [os.path.getsize(path), os.path.getsize(os.path.join(OUT, "attn_rotated_manifest.json"))]
    assert max(sizes) < C.MAX_FIXTURE_BYTES, sizes
    print(f"{len(manifest['cases'])} cases, {len(tensors)} stored tensors, {sizes} bytes")


if __name__ == "__main__":
    main()
