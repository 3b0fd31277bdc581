"""Generate the FP8-block -> MXFP4 fixture by running the UPSTREAM REFERENCE on the CPU over the case matrix of tests/_fp8block_mxfp4_cases.py:
`FP8BlockDequantizer(dtype=...).process`, torch.amin / amax over groups of 32, `calculate_qparams` with the MXFP4A16 preset's weight args and
`compress` of the `mxfp4-pack-quantized` compressor (the recipe of tools/gen_golden_nonfinite_rtn.py's `mxfp4` kind); for MXFP4Quantizer the same
from a synthesised dense weight.  Everything is imported from the reference tree at generation time, never copied (oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_fp8block_mxfp4.py [--check]

Writes tests/golden/fp8block_mxfp4.safetensors (`<case>.<dense dtype>.packed` / `.e8m0`, `quantizer.<name>.<dtype>.*`: the outputs of at most
`WHOLE_MAX` bytes) and tests/golden/fp8block_mxfp4_manifest.json (per output its shape, sha256 and whether it is stored; the reference's
`model_dump()` of the MXFP4A16 and MXFP4 presets).

Two things the reference leaves to the host CPU are written in their canonical form, as the sibling fixtures write them (DESIGN sections 2, 5.10, 5.19):
- E2M1 has no NaN: a NaN quotient (a NaN code, inf / inf) has the magnitude 0 and the sign bit of that NaN, which an x86 division makes negative
  and the GPU positive.  Exactly these sign bits are cleared; the three magnitude bits of the same nibbles stay.
- the reference's MX scale of a group that HOLDS A NaN depends on which part of torch's CPU reduction saw it; the weight path's rule is the
  pinned oracle's (the scale of such a group is inf, its byte 127).  Where the two differ the oracle's group is written and the manifest counts it
  (`nan_groups_from_oracle`).  A difference in a group without a NaN stops the generator as a finding.
  Only the all-codes sweeps and `NAN_CODE_CASES` of the case matrix hold NaN codes: every other case is the reference's output in every group.

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

import _fp8block_mxfp4_cases as C  # noqa: E402
import oracle as O  # noqa: E402
from compressed_tensors.compressors import BaseCompressor  # noqa: E402
from compressed_tensors.entrypoints.convert import FP8BlockDequantizer  # noqa: E402
from compressed_tensors.quantization.quant_scheme import preset_name_to_scheme  # noqa: E402
from compressed_tensors.quantization.utils.helpers import calculate_qparams  # noqa: E402

PATH = os.path.join(C.GOLDEN, "fp8block_mxfp4.safetensors")
MANIFEST = os.path.join(C.GOLDEN, "fp8block_mxfp4_manifest.json")
SIZE_BOUND = 2 * os.path.getsize(os.path.join(C.GOLDEN, "fp8block.safetensors"))


def reference_mxfp4(dense):
    """(packed, e8m0, groups taken from the oracle) of a dense weight, in the canonical form the docstring describes"""
    scheme = preset_name_to_scheme("MXFP4A16", ["Linear"])
    grouped = dense.reshape(dense.shape[0], dense.shape[1] // 32, 32)
    scale, zp = calculate_qparams(grouped.amin(dim=-1), grouped.amax(dim=-1), scheme.weights)
    c = BaseCompressor.get_value_from_registry("mxfp4-pack-quantized").compress({"weight": dense.clone(), "weight_scale": scale, "weight_zero_point": zp}, scheme)
    packed, e8m0 = c["weight_packed"].clone(), c["weight_scale"].clone()
    assert packed.dtype == torch.uint8 and e8m0.dtype == torch.uint8

    o_scale = O.calculate_qparams_float(dense, kind="mxfp4", group_size=32)
    o = O.fp4_compress(dense, o_scale, None, fmt="mxfp4-pack-quantized")
    o_packed, o_e8m0 = o["weight_packed"], O.e8m0_encode(o_scale)

    def clear_nan_signs(p, s):
        nan = torch.isnan(dense / s.repeat_interleave(32, dim=-1)).to(torch.uint8)
        return p & ~((nan[:, 0::2] << 3) | (nan[:, 1::2] << 7))

    packed, o_packed = clear_nan_signs(packed, scale), clear_nan_signs(o_packed, o_scale)
    differ = (e8m0 != o_e8m0) | (packed.reshape(*e8m0.shape, 16) != o_packed.reshape(*e8m0.shape, 16)).any(dim=-1)
    holds_nan = torch.isnan(grouped.float()).any(dim=-1)
    if bool((differ & ~holds_nan).any()):
        row, g = (differ & ~holds_nan).nonzero()[0].tolist()
        raise SystemExit(f"FINDING: row {row} group {g} holds no NaN, yet the reference and the pinned oracle differ on it")
    packed = torch.where(differ.repeat_interleave(16, dim=-1), o_packed, packed)
    e8m0 = torch.where(differ, o_e8m0, e8m0)
    return packed, e8m0, int(differ.sum())


def build():
    tensors, outputs = {}, {}

    def record(key, packed, e8m0, from_oracle):
        for name, t in (("packed", packed), ("e8m0", e8m0)):
            whole = t.numel() <= C.WHOLE_MAX
            outputs[f"{key}.{name}"] = dict(shape=list(t.shape), sha256=C.sha(t), whole=whole)
            if whole:
                tensors[f"{key}.{name}"] = t.contiguous()
        outputs[f"{key}.packed"]["nan_groups_from_oracle"] = from_oracle

    for key, c in C.CASES.items():
        w, s = C.inputs(key)
        for dtype in C.DENSE_DTYPES:
            conv = FP8BlockDequantizer(ignore=[], targets=["re:.*"], weight_block_size=tuple(c["block"]), dtype=C.DTYPES[dtype])
            dense = conv.process({"m.weight": w.clone(), "m.weight_scale_inv": s.clone()})["m.weight"]
            assert dense.dtype == C.DTYPES[dtype] and dense.shape == w.shape
            record(f"{key}.{dtype}", *reference_mxfp4(dense))
    for name in C.QUANTIZER_SHAPES:
        for dtype in C.DENSE_DTYPES:
            record(f"quantizer.{name}.{dtype}", *reference_mxfp4(C.dense_inputs(name, dtype)))
    presets = {}
    for preset in ("MXFP4A16", "MXFP4"):
        scheme = preset_name_to_scheme(preset, ["Linear"])
        presets[preset] = json.loads(json.dumps({"weights": scheme.weights.model_dump(),
                                                 "input_activations": scheme.input_activations.model_dump() if scheme.input_activations else None}, default=str))
    blob = save(tensors)
    if len(blob) >= SIZE_BOUND:
        raise SystemExit(f"the fixture would be {len(blob)} bytes, the bound is {SIZE_BOUND}: lower WHOLE_MAX or trim the matrix")
    manifest = dict(outputs=outputs, presets=presets, groups_per_block=C.GROUPS_PER_BLOCK)
    return blob, (json.dumps(manifest, indent=1, sort_keys=True) + "\n").encode()


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
    m = json.loads(manifest)
    print(f"{len(m['outputs']) // 2} records, {len(blob)} + {len(manifest)} bytes, "
          f"{sum(v.get('nan_groups_from_oracle', 0) for v in m['outputs'].values())} NaN-holding groups written from the oracle")


if __name__ == "__main__":
    main()
