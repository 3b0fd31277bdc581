"""Generate the NVFP4 -> MXFP4 fixture by running the UPSTREAM REFERENCE on the CPU over the case matrix of tests/_nvfp4_mxfp4_cases.py:
`decompress` of the `nvfp4-pack-quantized` compressor (bfloat16, `unpack_fp4_from_uint8`'s default), torch.amin / amax over groups of 32,
`calculate_qparams` with the MXFP4A16 preset's weight args and `compress` of the `mxfp4-pack-quantized` compressor — the second half is
tools/gen_golden_fp8block_mxfp4.py's `reference_mxfp4`, imported.  Everything is imported from the reference tree at generation time, never copied
(oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_nvfp4_mxfp4.py [--check]

Writes tests/golden/nvfp4_mxfp4.json: per output (`<case>.packed` / `.e8m0`) its shape, its sha256 and, up to `WHOLE_MAX` bytes, its bytes in base64;
the reference's `model_dump()` of the MXFP4A16 and MXFP4 presets; the workgroup's share of groups the shapes were chosen for.

The golden cases hold no NaN scale byte and only finite, non-zero global scales (tests/_nvfp4_mxfp4_cases.py).  A dense NaN still arises where a zero
code meets an infinite effective scale (the global scale 2^-140); for the groups that hold one, and for the sign bit of a NaN quotient, the canonical
forms of `reference_mxfp4` apply as in the sibling fixtures (DESIGN sections 2, 5.10, 5.19), and the record counts the groups written from the pinned
oracle (`nan_groups_from_oracle`).  A difference in a group without a NaN stops the generator as a finding.

The inputs are integer-synthesised: two runs write byte-identical files.  `--check` writes nothing and fails if the committed file differs.
TEST INFRASTRUCTURE ONLY.  Nothing in the product imports this.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_import  # noqa: E402

ref_import.import_reference()

import _nvfp4_mxfp4_cases as C  # noqa: E402
from compressed_tensors.compressors import BaseCompressor  # noqa: E402
from compressed_tensors.quantization.quant_scheme import preset_name_to_scheme  # noqa: E402
from gen_golden_fp8block_mxfp4 import reference_mxfp4  # noqa: E402

SIZE_BOUND = 512 << 10


def reference_dense(packed, scale, gs):
    scheme = preset_name_to_scheme("NVFP4A16", ["Linear"])
    state = {"weight_packed": packed.clone(), "weight_scale": scale.clone(), "weight_global_scale": gs.clone()}
    dense = BaseCompressor.get_value_from_registry("nvfp4-pack-quantized").decompress(state, scheme)["weight"]
    assert dense.dtype == torch.bfloat16 and tuple(dense.shape) == (packed.shape[0], 2 * packed.shape[1])
    return dense


def build():
    outputs = {}
    for key, (packed, scale, gs) in C.golden_inputs().items():
        assert not bool(((scale.view(torch.uint8) & 0x7F) == 0x7F).any()) and bool(torch.isfinite(gs).all()) and float(gs) != 0.0, key
        out_packed, e8m0, from_oracle = reference_mxfp4(reference_dense(packed, scale, gs))
        outputs[f"{key}.packed"] = dict(C.record(out_packed), nan_groups_from_oracle=from_oracle)
        outputs[f"{key}.e8m0"] = C.record(e8m0)
    presets = {}
    for preset in ("MXFP4A16", "MXFP4"):
        scheme = preset_name_to_scheme(preset, ["Linear"])
        presets[preset] = json.loads(json.dumps({"weights": scheme.weights.model_dump(),
                                                 "input_activations": scheme.input_activations.model_dump() if scheme.input_activations else None}, default=str))
    blob = (json.dumps(dict(outputs=outputs, presets=presets, groups_per_block=C.GROUPS_PER_BLOCK), indent=1, sort_keys=True) + "\n").encode()
    if len(blob) >= SIZE_BOUND:
        raise SystemExit(f"the fixture would be {len(blob)} bytes, the bound is {SIZE_BOUND}: lower WHOLE_MAX or trim the matrix")
    return blob


def main():
    blob = build()
    if "--check" in sys.argv[1:]:
        with open(C.FIXTURE, "rb") as f:
            if f.read() != blob:
                raise SystemExit(f"{C.FIXTURE} differs from what the reference produces")
        print("fixture matches")
        return
    with open(C.FIXTURE, "wb") as f:
        f.write(blob)
    m = json.loads(blob)
    print(f"{len(m['outputs']) // 2} records, {len(blob)} bytes, "
          f"{sum(v.get('nan_groups_from_oracle', 0) for v in m['outputs'].values())} NaN-holding groups written from the oracle")


if __name__ == "__main__":
    main()
