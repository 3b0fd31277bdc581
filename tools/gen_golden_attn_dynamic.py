"""Generate the dynamic attention q / k / v QDQ fixtures by running the UPSTREAM REFERENCE's forward_quantize
(quantization/lifecycle/forward.py:292-329) and compute_dynamic_scales_and_zp (quantization/utils/helpers.py:140-195) on the CPU
over the case matrix of tests/_attn_dynamic_cases.py (needs the reference sources; see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_attn_dynamic.py

Writes tests/golden/attn_dynamic.safetensors (the small bfloat16 cases: `<key>.out`) and tests/golden/attn_dynamic_manifest.json
(every case: its recipe, the sha256 and strides of the synthesised input and, for the reference's output, scale and zero point,
dtype, shape, strides and sha256 — NaNs canonicalised).  The inputs are integer-synthesised: two runs write byte-identical files.
The values of the MX presets are those of the reference with every group reduced in the vectorised body of torch's CPU amin / amax
(`_in_the_vector_body`): its scale of a group that holds a NaN otherwise depends on where the group lies and on the CPU's vector width.
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

import _attn_dynamic_cases as C  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs, QuantizationStatus  # noqa: E402
from compressed_tensors.quantization.lifecycle.forward import forward_quantize  # noqa: E402
from compressed_tensors.quantization.utils import compute_dynamic_scales_and_zp  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def describe(t):
    return dict(dtype=str(t.dtype).replace("torch.", ""), shape=list(t.shape), strides=list(t.stride()), sha256=C.sha(t))


PAD_GROUPS = 512  # more scales than any CPU's vectorised reduction handles per step (4 vectors of 32 16-bit lanes)


def _in_the_vector_body(run, x, group):
    """`run(x)` evaluated with x followed, along dim 0, by enough zero rows that every group of x is reduced in the VECTORISED body
    of torch's CPU amin / amax, and cut back to x's extent.  Groups are independent, so this changes nothing but one thing: the scale
    of an MX group that holds a NaN.  round_to_power_2 (mxfp_utils.py:62-110) works on the bit pattern of the NaN the reduction
    returns, and that is all-ones from the vector body (scale 2^-127) and the canonical NaN from the scalar tail that handles the
    last `groups % vector width` groups (scale +inf): by the unpadded call the same row gives one or the other by where it lies in
    the tensor and by the vector width of the CPU that runs the generator.  The body's value is the one every CPU reproduces."""
    xc = x.contiguous()
    extra = -(-PAD_GROUPS * group // (xc[0].numel() or 1)) + 1
    padded = torch.cat([xc, torch.zeros((extra,) + tuple(xc.shape[1:]), dtype=xc.dtype)], dim=0)
    return tuple(t[: xc.shape[0]] for t in run(padded))


def reference(recipe):
    x = C.make_input(recipe)
    kwargs = C.preset_args(recipe)
    args = QuantizationArgs(**kwargs)
    gs = C.global_scale(recipe)
    module = torch.nn.Module()
    module.quantization_status = QuantizationStatus.FROZEN
    if gs is not None:
        module.k_global_scale = gs

    def run(t):
        return (forward_quantize(module, t, "k", args),) + tuple(compute_dynamic_scales_and_zp(value=t, args=args, module=module, global_scale=gs))

    out, scale, zp = run(x)
    # the values are those of the same call on the contiguous copy (what the kernels are pinned to)
    assert C.sha(out) == C.sha(forward_quantize(module, x.contiguous(), "k", args)), recipe
    if kwargs.get("scale_dtype") is torch.uint8:  # the MX presets: the values come from the vector body, the layouts from the call itself
        group = kwargs["group_size"]
        body = _in_the_vector_body(run, x, group)
        has_nan = torch.isnan(x.contiguous().unflatten(-1, (x.shape[-1] // group, group))).any(-1)
        for got, want in zip((out, scale, zp), body):
            assert got.shape == want.shape and got.dtype == want.dtype, recipe
            same = (got.contiguous().view(torch.uint8) == want.contiguous().view(torch.uint8)).reshape(*has_nan.shape, -1).all(-1)  # per group
            assert bool((same | has_nan).all()), ("padding changed a group without a NaN", recipe)  # groups ARE independent
            got.copy_(want)  # in place: dtype, shape and strides stay those of the reference's own call
    return x, out, scale, zp


def main():
    tensors, manifest = {}, {"cases": {}}
    for key, recipe in C.case_list():
        x, out, scale, zp = reference(recipe)
        entry = dict(recipe=recipe, stored=C.stored(recipe), x_sha256=C.sha(x), x_strides=list(x.stride()), out=describe(out), scale=describe(scale),
                     zp=describe(zp))
        if entry["stored"]:
            tensors[f"{key}.out"] = out.contiguous()
        manifest["cases"][key] = entry
    save_file(tensors, os.path.join(OUT, "attn_dynamic.safetensors"))
    with open(os.path.join(OUT, "attn_dynamic_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(manifest['cases'])} cases, {len(tensors)} stored tensors")


if __name__ == "__main__":
    main()
