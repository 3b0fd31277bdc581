"""Generate the attention min-max observer fixtures by running the UPSTREAM REFERENCE's test observer (tests/mock_observer.py:
flatten_for_quantization, torch.amin / amax, calculate_qparams) on the CPU over the case matrix of tests/_attn_observe_cases.py.
The observer is imported from the reference tree at generation time, never copied (needs the reference sources; see
oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_attn_observe.py

Writes tests/golden/attn_observe.safetensors (`<key>.{min_vals,max_vals,scale,zero_point}`; float8 zero points as bytes) and
tests/golden/attn_observe_manifest.json (every case: its recipe, the sha256 and strides of the synthesised input, dtype and shape
of the four results).  The inputs are integer-synthesised: two runs write byte-identical files.
TEST INFRASTRUCTURE ONLY.  Nothing in the product imports this.
"""
import importlib.util
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

import _attn_observe_cases as C  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def _mock_observer_class():
    """MockMinMaxObserver of the reference's tests/mock_observer.py, loaded from the reference tree"""
    spec = importlib.util.spec_from_file_location("ct_reference_mock_observer", os.path.join(ref_import.root(), "tests", "mock_observer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MockMinMaxObserver


def reference(observer_cls, recipe):
    x = C.make_observed(recipe)
    observer = observer_cls(recipe["base"], QuantizationArgs(**C.args_of(recipe)), torch.nn.Module())
    scale, zero_point = observer(C.reference_view(recipe, x))
    return x, dict(min_vals=observer.min_vals, max_vals=observer.max_vals, scale=scale, zero_point=zero_point)


def main():
    observer_cls = _mock_observer_class()
    tensors, manifest = {}, {"cases": {}}
    for key, recipe in C.case_list():
        x, res = reference(observer_cls, recipe)
        entry = dict(recipe=recipe, x_sha256=C.sha(x), x_strides=list(x.stride()), out={})
        for name, t in res.items():
            entry["out"][name] = dict(dtype=str(t.dtype).replace("torch.", ""), shape=list(t.shape))
            tensors[f"{key}.{name}"] = t.contiguous().view(torch.uint8) if t.dtype == C.F8 else t.contiguous()
        manifest["cases"][key] = entry
    save_file(tensors, os.path.join(OUT, "attn_observe.safetensors"))
    with open(os.path.join(OUT, "attn_observe_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(manifest['cases'])} cases, {len(tensors)} stored tensors")


if __name__ == "__main__":
    main()
