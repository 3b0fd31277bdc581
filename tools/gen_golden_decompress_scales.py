"""Generate the decompress-side scale fixture by running the UPSTREAM REFERENCE on the CPU over the case matrix of tests/_decompress_scale_cases.py:
codes, stored scales and zero points — every 16-bit scale pattern, the edge scales crossed with every zero point and code, the fp32 exponent sweep,
all 256 E8M0 bytes — through `dequantize` (lifecycle/forward.py), and through `decompress` of the pack-quantized, naive-quantized and MXFP8
compressors wherever a case is something such a checkpoint can hold.  Everything is imported from the reference tree at generation time, never
copied (needs the reference sources; see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_decompress_scales.py [--check]

Writes tests/golden/decompress_scales_manifest.json — per case the sha256 of its inputs (`_decompress_scale_cases.inputs` regenerates them) and of
its output the dtype, shape, canonical sha256 (every NaN rewritten to one NaN: payload and sign are not compared; the sign of a
zero is) and the NaN, inf and subnormal counts — and tests/golden/decompress_scales.safetensors: the `cross` outputs of at most
`_decompress_scale_cases.WHOLE_MAX` bytes, canonical, whole.

The generator STOPS AS A FINDING if the pinned oracle is not the reference on any case, or a compressor's `decompress` is not `dequantize`.
The inputs are integer-synthesised: two runs write byte-identical files.  `--check` writes nothing and fails if a committed file differs.
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

import _decompress_scale_cases as C  # noqa: E402
import oracle as O  # noqa: E402
from compressed_tensors.compressors import BaseCompressor  # noqa: E402
from compressed_tensors.compressors.pack_quantized.helpers import pack_to_int32  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs, QuantizationScheme  # noqa: E402
from compressed_tensors.quantization.lifecycle.forward import dequantize  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "decompress_scales.safetensors")
MANIFEST = os.path.join(ROOT, "tests", "golden", "decompress_scales_manifest.json")
SIZE_BOUND = os.path.getsize(os.path.join(ROOT, "tests", "golden", "packw_rtn.safetensors"))  # the largest *_rtn fixture there is


def _scheme(r, **kw):
    strategy = dict(strategy="group", group_size=r["group"]) if r["group"] else dict(strategy="channel")
    return QuantizationScheme(targets=["Linear"], weights=QuantizationArgs(num_bits=r["bits"], symmetric=r["zp"] is None, **strategy, **kw))


def compressor_route(r, t):
    """(format, state dict, scheme) of the checkpoint that holds this case, or None"""
    sd = {"weight_scale": t["scale"]}
    if t["g_idx"] is not None:
        sd["weight_g_idx"] = t["g_idx"]
    if r["e8m0"]:
        return "mxfp8-quantized", dict(sd, weight=t["q"]), _scheme(r, type="float", scale_dtype=torch.uint8, zp_dtype=torch.uint8)
    if r["sdt"] == "f32" and r["bits"] != 8:
        return None
    if r["ctype"] == "fp8" or (r["bits"] == 8 and r["zp"] in (None, "i8")):
        if t["zero_point"] is not None:
            sd["weight_zero_point"] = t["zero_point"]
        return "naive-quantized", dict(sd, weight=t["q"]), _scheme(r, type="float" if r["ctype"] == "fp8" else "int")
    if r["zp"] in (None, "i4", "ib"):  # zero points a packed checkpoint can hold: the width's own range
        if t["zero_point"] is not None:
            sd["weight_zero_point"] = pack_to_int32(t["zero_point"], r["bits"], packed_dim=0).contiguous()
        return "pack-quantized", dict(sd, weight_packed=pack_to_int32(t["q"], r["bits"]), weight_shape=torch.tensor(r["shape"])), _scheme(r)
    return None


def build():
    tensors, cases = {}, {}
    for key, r in C.case_list():
        t = C.inputs(r)
        if r["e8m0"]:
            ref = None
        else:
            ref = dequantize(t["q"], t["scale"], t["zero_point"], g_idx=t["g_idx"])
        route = compressor_route(r, t)
        if route is not None:
            fmt, sd, scheme = route
            got = BaseCompressor.get_value_from_registry(fmt).decompress(sd, scheme)["weight"]
            if ref is None:
                ref = got
            elif got.dtype != ref.dtype or not torch.equal(C.canonical(got), C.canonical(ref)):
                raise SystemExit(f"FINDING: {key}: the reference's {fmt} decompress is not its dequantize")
        mine = C.oracle_output(O, r, t)
        if mine.dtype != ref.dtype or mine.shape != ref.shape or not torch.equal(C.canonical(mine), C.canonical(ref)):
            raise SystemExit(f"FINDING: {key}: the pinned oracle is not the reference")
        whole = C.stored_whole(key, r, ref)
        cases[key] = dict(recipe=r, inputs_sha256=C.input_sha(t), route=route[0] if route else None, out=dict(C.record(ref), whole=whole))
        if whole:
            tensors[key] = C.canonical(ref).view(ref.dtype)
    blob = save(tensors)
    if len(blob) >= SIZE_BOUND:
        raise SystemExit(f"the fixture would be {len(blob)} bytes, the largest *_rtn fixture has {SIZE_BOUND}: lower WHOLE_MAX")
    return blob, (json.dumps(dict(cases=cases), indent=1, sort_keys=True) + "\n").encode()


def main():
    blob, manifest = build()
    if "--check" in sys.argv[1:]:
        for path, want in ((PATH, blob), (MANIFEST, manifest)):
            with open(path, "rb") as f:
                if f.read() != want:
                    raise SystemExit(f"{path} differs from what the reference produces")
        print("fixture matches")
        return
    for path, want in ((PATH, blob), (MANIFEST, manifest)):
        with open(path, "wb") as f:
            f.write(want)
    print(f"{len(C.case_list())} cases, {len(blob)} + {len(manifest)} bytes")


if __name__ == "__main__":
    main()
