"""Generate the FP8-block -> MXFP8 / NVFP4 fixture by running the UPSTREAM REFERENCE on the CPU over the case matrix of
tests/_fp8block_transcode_cases.py: `FP8BlockDequantizer(dtype=...).process`, then
- MXFP8: torch.amin / amax over groups of 32, `calculate_qparams` with the MXFP8 preset's weight args and `compress` of the `mxfp8-quantized`
  compressor;
- NVFP4: `generate_gparam` of the tensor's min / max, `calculate_qparams` with the NVFP4A16 preset's weight args under that global scale and `compress`
  of the `nvfp4-pack-quantized` compressor.
Everything is imported from the reference tree at generation time, never copied (oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_fp8block_transcode.py [--check]

Writes tests/golden/fp8block_transcode.safetensors (`<target>.<case>.<dense dtype>.<output>`: the outputs of at most `WHOLE_MAX` bytes, float8 ones
as bytes) and tests/golden/fp8block_transcode_manifest.json (per output its shape, sha256, whether it is stored and `bytes_from_oracle`; the
reference's `model_dump()` of the MXFP8, NVFP4A16 and NVFP4 presets; the workgroup shares the matrix was derived from).

What the reference leaves to the host CPU is written in its canonical form, as the sibling fixtures write it (DESIGN sections 2, 5.10, 5.19, 5.27):
- NaN sign and payload are not compared: a float8 output's two NaN codes are written as 0x7f; E2M1 has no NaN, so a NaN quotient has the magnitude 0
  and the sign bit of that NaN, which an x86 division makes negative and the GPU positive — exactly these sign bits are cleared.
- the reference's result for a group (MXFP8) or a tensor (NVFP4: its global scale is tensor-wide) that HOLDS A NaN depends on which part of torch's
  CPU reduction saw it; the weight path's rule is the pinned oracle's.  Where the two differ the oracle's bytes are written and the manifest counts
  them per output (`bytes_from_oracle`).  A difference in a group / tensor without a NaN stops the generator as a finding, and so does any counted
  byte in a case of `finite_codes`: only the all-codes sweeps and `NAN_CODE_CASES` hold NaN codes.

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

import _fp8block_transcode_cases as C  # noqa: E402
import oracle as O  # noqa: E402
from compressed_tensors.compressors import BaseCompressor  # noqa: E402
from compressed_tensors.entrypoints.convert import FP8BlockDequantizer  # noqa: E402
from compressed_tensors.quantization.quant_scheme import preset_name_to_scheme  # noqa: E402
from compressed_tensors.quantization.utils import generate_gparam  # noqa: E402
from compressed_tensors.quantization.utils.helpers import calculate_qparams  # noqa: E402

PATH = os.path.join(C.GOLDEN, "fp8block_transcode.safetensors")
MANIFEST = os.path.join(C.GOLDEN, "fp8block_transcode_manifest.json")
SIZE_BOUND = 2 * os.path.getsize(os.path.join(C.GOLDEN, "fp8block.safetensors"))  # the size the existing golden files keep
F8 = torch.float8_e4m3fn


def _grouped_qparams(x, group, args, **kw):
    grouped = x.reshape(x.shape[0], x.shape[1] // group, group)
    return calculate_qparams(grouped.amin(dim=-1), grouped.amax(dim=-1), args, **kw)


def _merge(target, names, ref, mine, allowed, where):
    """{name: canonical bytes}, {name: bytes taken from the oracle}: the reference's canonical outputs with the oracle's where the two differ;
    `allowed` (per output, broadcastable to it) says where they may"""
    out, counts = {}, {}
    for name in names:
        a, b = C.canonical(target, name, ref[name]), C.canonical(target, name, mine[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (where, name)
        differ = a != b
        if bool((differ & ~allowed[name]).any()):
            raise SystemExit(f"FINDING: {where} {name}: the reference and the pinned oracle differ at {(differ & ~allowed[name]).nonzero()[0].tolist()}, "
                             f"where nothing holds a NaN")
        out[name], counts[name] = torch.where(differ, b, a), int(differ.sum())
    return out, counts


def reference_mxfp8(dense, where):
    scheme = preset_name_to_scheme("MXFP8", ["Linear"])
    scale, zp = _grouped_qparams(dense, 32, scheme.weights)
    c = BaseCompressor.get_value_from_registry("mxfp8-quantized").compress({"weight": dense.clone(), "weight_scale": scale, "weight_zero_point": zp}, scheme)
    ref = dict(codes=c["weight"], e8m0=c["weight_scale"])
    assert ref["codes"].dtype == F8 and ref["e8m0"].dtype == torch.uint8, (ref["codes"].dtype, ref["e8m0"].dtype)
    o_scale = O.calculate_qparams_float(dense, kind="mxfp8", group_size=32)
    o_q = O.quantize(dense, o_scale, torch.zeros(o_scale.shape, dtype=F8), num_bits=8, strategy="group", group_size=32, dtype=F8, qtype="float")
    mine = dict(codes=o_q, e8m0=O.e8m0_encode(o_scale))
    holds_nan = torch.isnan(dense.float().reshape(dense.shape[0], -1, 32)).any(dim=-1)  # per group
    return _merge("mxfp8", ("codes", "e8m0"), ref, mine, dict(codes=holds_nan.repeat_interleave(32, dim=-1), e8m0=holds_nan), where)


def _clear_nan_signs(packed, dense, scale, gs):
    """the packed nibbles without the sign bit of every element whose quotient x / (scale / global_scale) is a NaN"""
    nan = torch.isnan(dense.float() / (scale.float() / gs.float()).repeat_interleave(16, dim=-1)).to(torch.uint8)
    return packed & ~((nan[:, 0::2] << 3) | (nan[:, 1::2] << 7))


def reference_nvfp4(dense, where):
    scheme = preset_name_to_scheme("NVFP4A16", ["Linear"])
    gs = generate_gparam(dense.min().reshape(1), dense.max().reshape(1))
    scale, zp = _grouped_qparams(dense, 16, scheme.weights, global_scale=gs)
    c = BaseCompressor.get_value_from_registry("nvfp4-pack-quantized").compress(
        {"weight": dense.clone(), "weight_scale": scale, "weight_zero_point": zp, "weight_global_scale": gs}, scheme)
    ref = dict(packed=_clear_nan_signs(c["weight_packed"], dense, scale, gs), scale_f8=c["weight_scale"], global_scale=c["weight_global_scale"].reshape(1))
    assert ref["packed"].dtype == torch.uint8 and ref["scale_f8"].dtype == F8 and ref["global_scale"].dtype == torch.float32
    o_gs = O.generate_gparam(dense)
    o_scale = O.calculate_qparams_float(dense, kind="nvfp4", group_size=16, global_scale=o_gs)
    oc = O.fp4_compress(dense, o_scale, o_gs, fmt="nvfp4-pack-quantized")
    mine = dict(packed=_clear_nan_signs(oc["weight_packed"], dense, o_scale, o_gs), scale_f8=oc["weight_scale"], global_scale=o_gs.reshape(1))
    holds_nan = torch.isnan(dense.float()).any().reshape(1, 1)  # the global scale is tensor-wide
    return _merge("nvfp4", ("packed", "scale_f8", "global_scale"), ref, mine,
                  dict(packed=holds_nan, scale_f8=holds_nan, global_scale=holds_nan.reshape(1)), where)


REFERENCE = {"mxfp8": reference_mxfp8, "nvfp4": reference_nvfp4}


def build():
    tensors, outputs = {}, {}
    for key, c in C.CASES.items():
        w, s = C.inputs(key)
        for dtype in C.DENSE_DTYPES:
            conv = FP8BlockDequantizer(ignore=[], targets=["re:.*"], weight_block_size=tuple(c["block"]), dtype=C.DTYPES[dtype])
            dense = conv.process({"m.weight": w.clone(), "m.weight_scale_inv": s.clone()})["m.weight"]
            assert dense.dtype == C.DTYPES[dtype] and dense.shape == w.shape
            for target in c["targets"]:
                where = f"{target}.{key}.{dtype}"
                got, counts = REFERENCE[target](dense, where)
                for name, t in got.items():
                    if counts[name] and key not in C.HOLDS_NAN_CODES:
                        raise SystemExit(f"FINDING: {where}.{name}: {counts[name]} bytes from the oracle in a case without NaN codes")
                    whole = t.numel() * t.element_size() <= C.WHOLE_MAX
                    outputs[f"{where}.{name}"] = dict(shape=list(t.shape), sha256=C.sha(t), whole=whole, bytes_from_oracle=counts[name])
                    if whole:
                        tensors[f"{where}.{name}"] = t.contiguous()
    presets = {}
    for preset in ("MXFP8", "NVFP4A16", "NVFP4"):
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
    m = json.loads(manifest)["outputs"]
    taken = {k: v["bytes_from_oracle"] for k, v in m.items() if v["bytes_from_oracle"]}
    print(f"{len(m)} outputs, {len(blob)} + {len(manifest)} bytes, {sum(taken.values())} bytes written from the oracle in {len(taken)} outputs")
    for k, v in sorted(taken.items()):
        print(f"  {k}: {v}")


if __name__ == "__main__":
    main()
