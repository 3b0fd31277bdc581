"""Generate the non-finite round-to-nearest fixture by running the UPSTREAM REFERENCE on the CPU over the case matrix of
tests/_nonfinite_rtn_cases.py: weights with planted NaN and +-inf bit patterns through what every one-pass dense-checkpoint quantizer replaces —
torch.amin / amax over each group, row or block, calculate_qparams, quantize, then pack_to_int32 (pack-quantized), compress_mx_scale (MXFP8) or
the FP4 compressors' `compress` under generate_gparam (NVFP4) / the MX scales (MXFP4).  Everything is imported from the reference tree at
generation time, never copied (needs the reference sources; see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_nonfinite_rtn.py [--check]

Writes tests/golden/nonfinite_rtn.safetensors — `<key>.<kind>.<name>` with the names of the sibling fixtures: `scale`, `zero_point`, the codes `q` or
the words `packed`, `zp_packed`, `e8m0`, `scale_f8` and `global_scale`; float8 tensors as bytes; every NaN rewritten to the canonical one, so
the file does not depend on the payloads a CPU happens to produce — and tests/golden/nonfinite_rtn_manifest.json: per case the sha256 of its input
(`make_weight` + `plant` regenerate it) and per result its dtype, shape, canonical sha256 and NaN count; a result of more than
`_nonfinite_rtn_cases.WHOLE_MAX` bytes is kept as that sha256 alone.

`mx_exceptions` of the manifest lists every (case, kind, row, group) of the MX kinds where the reference's `scale` or `e8m0` differs from the pinned
oracle's: the reference's MX scale of a group that holds a NaN depends on which part of torch's CPU reduction saw it, the weight
path's rule is the canonical-NaN result.  The list may hold MX kinds and NaN-holding groups ONLY: anything else — a group of infinities, a finite
group, any INT, FP8 or NVFP4 mismatch — stops the generator as a finding.

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

import _nonfinite_rtn_cases as C  # noqa: E402
import oracle as O  # noqa: E402
from compressed_tensors.compressors import BaseCompressor  # noqa: E402
from compressed_tensors.compressors.mx_utils import compress_mx_scale  # noqa: E402
from compressed_tensors.compressors.pack_quantized.helpers import pack_to_int32  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors.quantization.lifecycle.forward import quantize  # noqa: E402
from compressed_tensors.quantization.quant_scheme import preset_name_to_scheme  # noqa: E402
from compressed_tensors.quantization.utils import generate_gparam  # noqa: E402
from compressed_tensors.quantization.utils.helpers import calculate_qparams, maybe_pad_tensor_for_block_quant  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "nonfinite_rtn.safetensors")
MANIFEST = os.path.join(ROOT, "tests", "golden", "nonfinite_rtn_manifest.json")
SIZE_BOUND = os.path.getsize(os.path.join(ROOT, "tests", "golden", "packw_rtn.safetensors"))  # the largest *_rtn fixture there is
MX8 = dict(num_bits=8, type="float", symmetric=True, scale_dtype=torch.uint8, zp_dtype=torch.uint8)


def _grouped_qparams(x, group, args, **kw):
    grouped = x.reshape(x.shape[0], x.shape[1] // group, group)
    return calculate_qparams(grouped.amin(dim=-1), grouped.amax(dim=-1), args, **kw)


def reference(x, r, kind):
    family, group = r["family"], r.get("group")
    if family == "pack":
        bits, symmetric = C.pack_kind(kind)
        if group:
            args = QuantizationArgs(num_bits=bits, type="int", symmetric=symmetric, strategy="group", group_size=group)
            scale, zp = _grouped_qparams(x, group, args)
        else:
            args = QuantizationArgs(num_bits=bits, type="int", symmetric=symmetric, strategy="channel")
            scale, zp = calculate_qparams(x.amin(dim=-1, keepdim=True), x.amax(dim=-1, keepdim=True), args)
        q = quantize(x, scale, zp, args, dtype=torch.int8)
        out = dict(scale=scale, zero_point=zp, packed=pack_to_int32(q, bits))
        if not symmetric:
            out["zp_packed"] = pack_to_int32(zp, bits, packed_dim=0)
        return out
    if family == "channel8":
        args = QuantizationArgs(strategy="channel", **C.KINDS8[kind])
        scale, zp = calculate_qparams(x.amin(dim=1, keepdim=True), x.amax(dim=1, keepdim=True), args)
        if args.type == "float":
            return dict(scale=scale, q=quantize(x, scale, torch.zeros(scale.shape, dtype=C.F8), args, dtype=args.pytorch_dtype()))
        return dict(scale=scale, zero_point=zp, q=quantize(x, scale, zp, args, dtype=args.pytorch_dtype()))
    if family == "block8":
        args = QuantizationArgs(strategy="block", block_structure=list(r["block"]), **C.KINDS8[kind])
        bh, bw = r["block"]
        p = maybe_pad_tensor_for_block_quant(x, tuple(r["block"]))
        blocks = p.reshape(p.shape[0] // bh, bh, p.shape[1] // bw, bw)
        scale, zp = calculate_qparams(blocks.amin(dim=(1, 3)), blocks.amax(dim=(1, 3)), args)
        return dict(scale=scale, zero_point=zp, q=quantize(x, scale, zp, args, dtype=args.pytorch_dtype()))
    if family == "group8":
        args = QuantizationArgs(strategy="group", group_size=group, **(MX8 if kind == "mxfp8" else C.KINDS8[kind]))
        scale, zp = _grouped_qparams(x, group, args)
        if args.type == "float":
            out = dict(scale=scale, q=quantize(x, scale, torch.zeros(scale.shape, dtype=C.F8), args, dtype=args.pytorch_dtype()))
            if kind == "mxfp8":
                out["e8m0"] = compress_mx_scale(scale, torch.uint8)
            return out
        q = quantize(x, scale, zp, args, dtype=args.pytorch_dtype())
        return dict(scale=scale, zero_point=zp, q=q, packed=pack_to_int32(q, 8))
    if kind == "mxfp4":
        scheme = preset_name_to_scheme("MXFP4A16", ["Linear"])
        scale, zp = _grouped_qparams(x, 32, scheme.weights)
        c = BaseCompressor.get_value_from_registry("mxfp4-pack-quantized").compress({"weight": x.clone(), "weight_scale": scale, "weight_zero_point": zp}, scheme)
        return dict(scale=scale, packed=c["weight_packed"], e8m0=c["weight_scale"])
    scheme = preset_name_to_scheme("NVFP4A16", ["Linear"])
    gs = generate_gparam(x.min().reshape(1), x.max().reshape(1)) if r["global_scale"] is None else torch.tensor([r["global_scale"]], dtype=torch.float32)
    scale, zp = _grouped_qparams(x, 16, scheme.weights, global_scale=gs)
    c = BaseCompressor.get_value_from_registry("nvfp4-pack-quantized").compress(
        {"weight": x.clone(), "weight_scale": scale, "weight_zero_point": zp, "weight_global_scale": gs}, scheme)
    return dict(scale=scale, packed=c["weight_packed"], scale_f8=c["weight_scale"], global_scale=c["weight_global_scale"])


def _as_dtype(canon, dtype):
    """the canonical bits back under the result's dtype (float8 as bytes: safetensors of this vintage has no float8)"""
    return canon if dtype == C.F8 or canon.dtype == dtype else canon.view(dtype)


def mx_exceptions(key, r, x, kind, ref):
    """[[key, kind, row, group]] where the reference's MX scale / exponent byte is not the oracle's; only a NaN-holding group may be one"""
    mine = C.oracle_outputs(O, x, r, kind)
    differ = torch.zeros(ref["scale"].shape, dtype=torch.bool)
    for name in ("scale", "e8m0"):
        assert ref[name].dtype == mine[name].dtype and ref[name].shape == mine[name].shape, (key, kind, name)
        differ |= C.canonical(ref[name]) != C.canonical(mine[name])
    out = []
    for row, g in differ.nonzero().tolist():
        if not bool(torch.isnan(x[row, 32 * g:32 * g + 32]).any()):
            raise SystemExit(f"FINDING: {key} {kind} row {row} group {g} holds no NaN, yet the reference and the oracle differ on its scale")
        out.append([key, kind, row, g])
    return out


def build():
    tensors, cases, exceptions = {}, {}, []
    for key, r in C.case_list():
        x = C.weight(r)
        entry = dict(shape=r["shape"], dtype=r["dtype"], x_sha256=C.sha(x), out={})
        for kind in C.kinds_of(r):
            ref = reference(x, r, kind)
            listed = mx_exceptions(key, r, x, kind, ref) if kind in C.MX_KINDS else []
            exceptions += listed
            # everything else must already be the oracle's, bit for bit under `comparable`
            mine = C.oracle_outputs(O, x, r, kind)
            mask = C.fp4_sign_mask(O, x, r, kind) if r["family"] == "fp4" else None
            pairs = [(row, g) for _, _, row, g in listed]
            want, got = C.comparable(ref, kind, mask, pairs), C.comparable(mine, kind, mask, pairs)
            for name in ref:
                if mine[name].dtype != ref[name].dtype or not torch.equal(want[name], got[name]):
                    raise SystemExit(f"FINDING: {key} {kind} {name}: the pinned oracle is not the reference")
            for name, t in ref.items():
                canon = C.comparable({name: t}, kind, mask)[name]  # (the listed MX groups stay as the reference gave them)
                whole = t.numel() * t.element_size() <= C.WHOLE_MAX
                if kind in C.MX_KINDS and not whole:
                    raise SystemExit(f"{key} {kind} {name}: the results of an MX kind must be stored whole (the listed groups are cut out of them)")
                entry["out"][f"{kind}.{name}"] = dict(dtype=str(t.dtype).replace("torch.", ""), shape=list(t.shape), sha256=C.sha(canon),
                                                      nans=C.nan_count(t), whole=whole)
                if whole:
                    tensors[f"{key}.{kind}.{name}"] = _as_dtype(canon, t.dtype)
        cases[key] = entry
    blob = save(tensors)
    if len(blob) >= SIZE_BOUND:
        raise SystemExit(f"the fixture would be {len(blob)} bytes, the largest *_rtn fixture has {SIZE_BOUND}: lower WHOLE_MAX or trim the matrix")
    manifest = dict(cases=cases, mx_exceptions=exceptions)
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
    print(f"{len(C.case_list())} cases, {len(blob)} + {len(manifest)} bytes, {len(json.loads(manifest)['mx_exceptions'])} listed MX groups")


if __name__ == "__main__":
    main()
