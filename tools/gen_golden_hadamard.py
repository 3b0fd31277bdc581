"""Generate the Hadamard rotation fixtures by running the UPSTREAM REFERENCE's HadamardTransform.forward
(transform/factory/hadamard.py:91-108) and apply_transform_config (transform/apply.py) on the CPU over the case matrix of
tests/_hadamard_cases.py (needs the reference sources; see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_hadamard.py

Writes tests/golden/hadamard.safetensors (the reference's output of the small cases, and the fused weights / bias of the
two-layer model), tests/golden/hadamard_manifest.json (every case: recipe, sha256 of the synthesised input, and for tiers A and C
the dtype, shape and sha256 of the reference's output with zeros canonicalised to +0.0) and
tests/golden/hadamard_transform_config.json (upstream's TransformConfig.model_dump() of the two-layer model's config).
For tier B it ASSERTS that the reference itself meets the derived bound on every element; nothing of tier B is stored.
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

import _hadamard_cases as C  # noqa: E402
from compressed_tensors.transform import TransformArgs, TransformConfig, TransformScheme, apply_transform_config  # noqa: E402
from compressed_tensors.transform.factory.hadamard import HadamardTransform  # noqa: E402
from compressed_tensors.transform.utils.hadamard import deterministic_hadamard_matrix  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
_H = {}


def reference(recipe, x):
    precision = C.precision_of(recipe)
    key = (recipe["size"], precision)
    if key not in _H:
        _H.clear()  # one matrix at a time: 8192^2 float64 is 512 MiB
        _H[key] = torch.nn.Parameter(deterministic_hadamard_matrix(recipe["size"], precision, torch.device("cpu")), requires_grad=False)
    scheme = TransformScheme(type="hadamard", precision=torch.float32)
    args = TransformArgs(targets=["Linear"], location=recipe["location"], inverse=recipe["inverse"])
    module_type = getattr(torch.nn, recipe["module"])
    with torch.no_grad():
        return HadamardTransform(_H[key], None, scheme, args, module_type)(x)


def main():
    tensors, manifest = {}, {"cases": {}}
    cases = sorted(C.case_list(), key=lambda kr: (kr[1]["size"], C.precision_of(kr[1]) == C.F64))  # matrices are built once per size
    for key, recipe in cases:
        x = C.synth(recipe)
        out = reference(recipe, x)
        assert out.dtype == x.dtype and out.shape == x.shape
        entry = dict(recipe=recipe, stored=C.stored(recipe), x_sha256=C.sha(x))
        if recipe["tier"] == "B":
            exact, tol = C.bound(x, recipe["size"], C.dim_of(recipe))
            ratio = ((out.to(C.F64) - exact).abs() / tol).max().item()
            assert ratio <= 1.0, (key, ratio)  # the reference meets the derived bound on every element
        else:
            # the condition of the exact tiers: the float32 / float64 butterfly restatement gives the reference's result
            assert torch.equal(C.butterfly(x, recipe["size"], C.dim_of(recipe), C.precision_of(recipe)), out), key
            entry["out"] = dict(dtype=str(out.dtype).replace("torch.", ""), shape=list(out.shape), sha256=C.sha(out))
            if entry["stored"]:
                tensors[f"{key}.out"] = out.contiguous()
        manifest["cases"][key] = entry
        print(key, flush=True)
    # the two-layer model through upstream's apply_transform_config
    config = TransformConfig.model_validate(C.MODEL_CONFIG)
    m = C.model()
    apply_transform_config(m, config)
    tensors["model.0.weight"] = m[0].weight.data.contiguous()
    tensors["model.0.bias"] = m[0].bias.data.contiguous()
    tensors["model.1.weight"] = m[1].weight.data.contiguous()
    save_file(tensors, os.path.join(OUT, "hadamard.safetensors"))
    os.chmod(os.path.join(OUT, "hadamard.safetensors"), 0o644)
    with open(os.path.join(OUT, "hadamard_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(OUT, "hadamard_transform_config.json"), "w") as f:
        json.dump(config.model_dump(), f, indent=1, sort_keys=True, default=str)
        f.write("\n")
    print(f"{len(manifest['cases'])} cases, {len(tensors)} stored tensors")


if __name__ == "__main__":
    main()
