"""Generate the permuted-rotation fixtures (`TransformScheme.randomize=True`) by running the UPSTREAM REFERENCE on the CPU over the
case matrix of tests/_hadamard_perm_cases.py: its own factories, `TransformFactory.from_scheme(scheme(randomize=True), name=...,
seed=S)`, draw the weight and the permutation and its HadamardTransform.forward (transform/factory/hadamard.py:91-108) computes
the outputs; apply_transform_config's loop (one seeded factory per config group) rotates the model (needs the reference sources;
see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist; about 10 GB of memory for the permuted 16384^2 float64 weight):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_hadamard_perm.py

Writes tests/golden/hadamard_perm.safetensors — the drawn permutation per (type, size) as `perm.<type>.<n>` (int16), the
reference's output of the small cases, the model's two permutations — and tests/golden/hadamard_perm_manifest.json (every case:
recipe, seed, sha256 of the synthesised input, dtype / shape / sha256 of the reference's output with zeros canonicalised to +0.0;
the sha256 of the model's fused tensors and hooked input).
It ASSERTS: a factory draws the same permutation whatever the precision of the first use; the permutation is
`torch.randperm(n, generator=g)` on the factory's generator, for random-hadamard right after the weight whose factors
tests/golden/random_hadamard.safetensors holds; G_p(T_W(G_q(x))) from this repository's restatements of T_W equals the reference in
every element of every case; the two files stay within 512 KiB.
TEST INFRASTRUCTURE ONLY.  Nothing in the product imports this.
"""
import json
import os
import sys

import torch
from safetensors.torch import load_file, save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402

ref_import.import_reference()

import _hadamard_cases as H  # noqa: E402
import _hadamard_perm_cases as C  # noqa: E402
from compressed_tensors.transform import TransformArgs, TransformConfig, TransformFactory, TransformScheme  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
_F = {}


def module_for(recipe):
    """the smallest module whose transform size at the recipe's location is n"""
    n, first = recipe["size"], recipe["location"] in ("input", "weight_input")
    with torch.no_grad():
        if recipe["module"] == "Linear":
            return torch.nn.Linear(n, 1, bias=False) if first else torch.nn.Linear(1, n, bias=False)
        return torch.nn.Embedding(n, 1) if first else torch.nn.Embedding(1, n)


def transform_for(recipe):
    """upstream's transform of a recipe.  One factory per (type, size, precision of the location), kept for one size at a time: a
    factory keys its weight by size alone, at the precision of the first use"""
    kind, n, precision = recipe["type"], recipe["size"], C.precision_of(recipe)
    if (kind, n, precision) not in _F:
        _F.clear()
        scheme = TransformScheme(type=kind, randomize=True, precision=torch.float32)
        _F[(kind, n, precision)] = TransformFactory.from_scheme(scheme, name="g", seed=C.seed_of(kind, n))
    args = TransformArgs(targets=["x"], location=recipe["location"], inverse=recipe["inverse"])
    return _F[(kind, n, precision)].create_transform(module_for(recipe), args)


def main():
    rh = load_file(os.path.join(OUT, "random_hadamard.safetensors"))
    tensors, manifest, perms = {}, {"cases": {}, "perms": {}, "model": {}}, {}
    order = {torch.float32: 0, torch.float64: 1}
    cases = sorted(C.case_list(), key=lambda kr: (kr[1]["type"], kr[1]["size"], order[C.precision_of(kr[1])]))
    for key, recipe in cases:
        kind, n = recipe["type"], recipe["size"]
        t = transform_for(recipe)
        assert t.perm is not None and t.perm.dtype == torch.int64 and t.perm.device.type == "cpu" and t.weight.dtype == C.precision_of(recipe)
        p = t.perm.data.clone()
        if (kind, n) not in perms:
            perms[(kind, n)] = p
            g = torch.Generator().manual_seed(C.seed_of(kind, n))
            if kind == "random-hadamard":  # the weight first: its draw is n values of randint
                torch.randint(low=0, high=2, size=(n,), generator=g, dtype=t.weight.dtype)
            assert torch.equal(torch.randperm(n, generator=g), p), (kind, n)
            tensors[f"perm.{kind}.{n}"] = p.to(torch.int16)
            manifest["perms"][f"{kind}.{n}"] = dict(seed=C.seed_of(kind, n), sha256=H.sha(p.to(torch.float64)))
        assert torch.equal(perms[(kind, n)], p), (key, "the permutation depends on the precision of the first use")
        x = C.synth(recipe)
        with torch.no_grad():
            out = t(x)
        assert out.dtype == x.dtype and out.shape == x.shape
        had_k, signs = (rh.get(f"had_k.{n}"), rh[f"signs.{n}"]) if kind == "random-hadamard" else (None, None)
        assert torch.equal(C.restated(recipe, x, p, had_k, signs) + 0.0, out + 0.0), key  # the identity, on the reference's own result
        manifest["cases"][key] = dict(recipe=recipe, seed=C.seed_of(kind, n), stored=C.stored(recipe), x_sha256=C.sha(x),
                                      out=dict(dtype=str(out.dtype).replace("torch.", ""), shape=list(out.shape), sha256=C.sha(out)))
        if C.stored(recipe):
            tensors[f"{key}.out"] = out.contiguous()
        print(key, flush=True)
    _F.clear()
    # the model: upstream's apply_transform_config loop with a seed (its own signature has none: TransformFactory takes it)
    config = TransformConfig.model_validate(C.model_config())
    m = H.model()
    for name, scheme in config.config_groups.items():
        factory = TransformFactory.from_scheme(scheme, name=name, seed=C.MODEL_SEED)
        factory.apply_to_model(m, use_tqdm=False)
    found = {k: v.data.clone() for k, v in m.state_dict().items() if k.endswith(".perm")}
    assert sorted(found) == ["1.v_input.perm"], sorted(found)  # the online transform is the one that stays on the model
    gu, gv = torch.Generator().manual_seed(C.MODEL_SEED), torch.Generator().manual_seed(C.MODEL_SEED)
    pu, pv = torch.randperm(128, generator=gu), torch.randperm(64, generator=gv)
    assert torch.equal(found["1.v_input.perm"], pv)
    tensors["model.perm.u.128"], tensors["model.perm.v.64"] = pu.to(torch.int16), pv.to(torch.int16)
    x = C.synth(dict(gen="ints", dtype="bf16", shape=[2, 5, 128], salt=77))
    seen = []
    m[1].register_forward_pre_hook(lambda _, inputs: seen.append(inputs[0]))
    m[1](x)
    fresh = H.model()
    ru = dict(type="hadamard", size=128, module="Linear", location="weight_output", inverse=False)
    rw = dict(type="hadamard", size=64, module="Linear", location="weight_input", inverse=True)
    ri = dict(type="hadamard", size=64, module="Linear", location="input", inverse=False)
    assert torch.equal(C.restated(ru, fresh[0].weight.data, pu), m[0].weight.data) and torch.equal(C.restated(rw, fresh[1].weight.data, pv), m[1].weight.data)
    assert torch.equal(C.restated(ru, fresh[0].bias.data.unsqueeze(-1), pu).squeeze(-1), m[0].bias.data) and torch.equal(C.restated(ri, x, pv), seen[0])
    for name, t in (("0.weight", m[0].weight.data), ("0.bias", m[0].bias.data), ("1.weight", m[1].weight.data), ("1.input", seen[0])):
        manifest["model"][name] = dict(shape=list(t.shape), sha256=C.sha(t))
    manifest["model"]["seed"] = C.MODEL_SEED
    path_t, path_m = os.path.join(OUT, "hadamard_perm.safetensors"), os.path.join(OUT, "hadamard_perm_manifest.json")
    save_file(tensors, path_t)
    os.chmod(path_t, 0o644)
    with open(path_m, "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    total = os.path.getsize(path_t) + os.path.getsize(path_m)
    assert total <= 512 * 1024, total
    print(f"{len(manifest['cases'])} cases, {len(tensors)} stored tensors, {total} bytes in the two files")


if __name__ == "__main__":
    main()
