"""Generate the random-hadamard fixtures by running the UPSTREAM REFERENCE on the CPU over the case matrix of
tests/_random_hadamard_cases.py: `random_hadamard_matrix` (transform/utils/hadamard.py:53-151) for the weights,
HadamardTransform.forward (transform/factory/hadamard.py:91-108) for the outputs and apply_transform_config for the model
(needs the reference sources; see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist; about 40 GB of memory for the largest weight):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_random_hadamard.py

Writes tests/golden/random_hadamard.safetensors — per size n the factors of the weight (`signs.<n>`, `had_k.<n>`; the weight
itself for n <= 96), the reference's output of the small cases, the signs of the model's three weights — and
tests/golden/random_hadamard_manifest.json (every case: recipe, sha256 of the synthesised input, and for tiers A and C the dtype,
shape and sha256 of the reference's output with zeros canonicalised to +0.0; the sha256 of the model's fused tensors).
It ASSERTS: every weight factors and the factors rebuild it (checked in full for n <= 4480); the evaluation from the factors
(`structured`) gives the reference's result in every element on tiers A and C; the reference meets the derived bound on tier B.
TEST INFRASTRUCTURE ONLY.  Nothing in the product imports this.
"""
import json
import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402

ref_import.import_reference()

import _random_hadamard_cases as C  # noqa: E402
import compressed_tensors.transform.factory.random_hadamard as up_r  # noqa: E402
from compressed_tensors.transform import TransformArgs, TransformConfig, TransformScheme, apply_transform_config  # noqa: E402
from compressed_tensors.transform.factory.hadamard import HadamardTransform  # noqa: E402
from compressed_tensors.transform.utils.hadamard import random_hadamard_matrix  # noqa: E402

from compressed_tensors_amd.transform.random_hadamard import factor_hadamard_weight  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
_W = {}


def weight(n, precision):
    if (n, precision) not in _W:
        _W.clear()  # one weight at a time: 28672^2 float32 is 3.3 GB
        _W[(n, precision)] = torch.nn.Parameter(random_hadamard_matrix(n, precision, torch.device("cpu"), torch.Generator().manual_seed(n)), requires_grad=False)
    return _W[(n, precision)]


def reference(recipe, x):
    scheme = TransformScheme(type="random-hadamard", precision=torch.float32)
    args = TransformArgs(targets=["Linear"], location=recipe["location"], inverse=recipe["inverse"])
    with torch.no_grad():
        return HadamardTransform(weight(recipe["size"], C.precision_of(recipe)), None, scheme, args, getattr(torch.nn, recipe["module"]))(x)


def main():
    tensors, manifest, factors = {}, {"cases": {}, "sizes": {}, "model": {}}, {}
    cases = sorted(C.case_list(), key=lambda kr: (kr[1]["size"], C.precision_of(kr[1]) == C.F64))
    worst = {}
    for key, recipe in cases:
        n = recipe["size"]
        w = weight(n, C.precision_of(recipe))
        if n not in factors:
            f = factor_hadamard_weight(w.data)
            assert f is not None and (f.k, f.m) == C.SIZES[n], (n, f and (f.k, f.m))
            if n <= 4480:
                assert torch.equal(C.weight_from_factors(n, f.had_k, f.signs, w.dtype), w.data), n
            factors[n] = f
            tensors[f"signs.{n}"] = f.signs.contiguous()
            if f.had_k is not None:
                tensors[f"had_k.{n}"] = f.had_k.contiguous()
            if n <= C.FULL_WEIGHT_MAX:
                tensors[f"weight.{n}"] = w.data.to(torch.int8).contiguous()
            manifest["sizes"][str(n)] = dict(k=f.k, m=f.m)
        f = factors[n]
        x = C.synth(recipe)
        out = reference(recipe, x)
        assert out.dtype == x.dtype and out.shape == x.shape
        entry = dict(recipe=recipe, stored=C.stored(recipe), x_sha256=C.sha(x))
        tr, dim = C.transposed_of(recipe), C.dim_of(recipe)
        if recipe["tier"] == "B":
            exact, tol = C.bound(x, n, f.had_k, f.signs, tr, dim)
            ratio = ((out.to(C.F64) - exact).abs() / tol).max().item()
            assert ratio <= 1.0, (key, ratio)  # the reference meets the derived bound on every element
            worst[(n, recipe["dtype"])] = max(worst.get((n, recipe["dtype"]), 0.0), ratio)
        else:
            # the condition of the exact tiers: the evaluation from the factors gives the reference's result
            assert torch.equal(C.structured(x, n, f.had_k, f.signs, tr, dim, C.precision_of(recipe)) + 0.0, out + 0.0), key
            entry["out"] = dict(dtype=str(out.dtype).replace("torch.", ""), shape=list(out.shape), sha256=C.sha(out))
            if entry["stored"]:
                tensors[f"{key}.out"] = out.contiguous()
        manifest["cases"][key] = entry
        print(key, flush=True)
    print("tier B, the reference's worst ratio per (n, dtype):", {f"{n}.{dt}": round(r, 3) for (n, dt), r in sorted(worst.items())})
    # the model through upstream's apply_transform_config; the weights it draws are recorded in order (one per config group)
    drawn = []
    orig = up_r.random_hadamard_matrix

    def recording(size, dtype, device, gen):
        w = orig(size, dtype, device, gen)
        drawn.append(w)
        return w

    up_r.random_hadamard_matrix = recording
    try:
        config = TransformConfig.model_validate(C.MODEL_CONFIG)
        m = C.model()
        apply_transform_config(m, config)
    finally:
        up_r.random_hadamard_matrix = orig
    assert len(drawn) == len(C.MODEL_CONFIG["config_groups"])
    for group, w in zip(C.MODEL_CONFIG["config_groups"], drawn):
        f = factor_hadamard_weight(w)
        assert f is not None and torch.equal(f.had_k, factors[C.MODEL_SIZE].had_k)
        tensors[f"model.signs.{group}"] = f.signs.contiguous()
    x = C.synth(dict(gen="ints", dtype="bf16", shape=[2, 5, C.MODEL_SIZE], salt=77))
    seen = []
    m[1].register_forward_pre_hook(lambda _, inputs: seen.append(inputs[0]))
    m[1](x)
    for name, t in (("0.weight", m[0].weight.data), ("0.bias", m[0].bias.data), ("1.weight", m[1].weight.data), ("1.input", seen[0])):
        manifest["model"][name] = dict(shape=list(t.shape), sha256=C.sha(t))
    save_file(tensors, os.path.join(OUT, "random_hadamard.safetensors"))
    os.chmod(os.path.join(OUT, "random_hadamard.safetensors"), 0o644)
    with open(os.path.join(OUT, "random_hadamard_manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(manifest['cases'])} cases, {len(tensors)} stored tensors, {sum(t.numel() * t.element_size() for t in tensors.values())} bytes")


if __name__ == "__main__":
    main()
