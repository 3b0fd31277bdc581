"""Generate the calibrated NVFP4 global-scale fixtures by running the UPSTREAM REFERENCE's test observer (tests/mock_observer.py:
`get_global_scale` = reshape((1, 1, -1)), torch.amin / amax, generate_gparam) on the CPU over the case matrix of tests/_nvfp4_calib_cases.py.
The observer is imported from the reference tree at generation time, never copied (needs the reference sources; see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_nvfp4_calib.py

Writes tests/golden/nvfp4_calib.safetensors (`<key>.global_scale`, float32 (1,)) and tests/golden/nvfp4_calib_manifest.json (every case: its
recipe, the sha256 and strides of the synthesised input).  The inputs are integer-synthesised: two runs write byte-identical files.
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

import _nvfp4_calib_cases as C  # noqa: E402
from _golden import GOLDEN_DIR  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs  # noqa: E402


def _mock_observer_class():
    """MockMinMaxObserver of the reference's tests/mock_observer.py, loaded from the reference tree"""
    spec = importlib.util.spec_from_file_location("ct_reference_mock_observer", os.path.join(ref_import.root(), "tests", "mock_observer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MockMinMaxObserver


def main():
    observer_cls = _mock_observer_class()
    args = QuantizationArgs(num_bits=4, type="float", symmetric=True, strategy="tensor_group", group_size=16, dynamic="local", observer="static_minmax",
            scale_dtype=torch.float8_e4m3fn, zp_dtype=torch.float8_e4m3fn)
    cases = C.case_list()
    recipes = dict(cases)
    tensors, manifest = {}, {"cases": {}}
    for key, recipe in cases:
        x = C.build(recipe, recipes)
        gs = observer_cls("input", args, torch.nn.Module()).get_global_scale(x)
        assert gs.dtype == torch.float32 and tuple(gs.shape) == (1,), (key, gs.dtype, gs.shape)
        tensors[f"{key}.global_scale"] = gs.contiguous()
        manifest["cases"][key] = dict(recipe=recipe, x_sha256=C.sha(x), x_strides=list(x.stride()))
    save_file(tensors, os.path.join(GOLDEN_DIR, "nvfp4_calib.safetensors"))
    with open(os.path.join(GOLDEN_DIR, "nvfp4_calib_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(manifest['cases'])} cases, {len(tensors)} stored tensors")


if __name__ == "__main__":
    main()
