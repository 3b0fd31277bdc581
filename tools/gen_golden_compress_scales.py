"""Generate the compress-side scale fixture by running the UPSTREAM REFERENCE on the CPU over the case matrix of tests/_compress_scale_cases.py:
weights built from GIVEN scales and zero points — every 16-bit scale pattern, the edge scales crossed with every zero point, the fp32 exponent
sweep, the patterns at and next to every range guard's end points — through `quantize` and `fake_quantize` (lifecycle/forward.py), and through
`compress` of the pack-quantized and naive-quantized compressors wherever a case is something such a compressor takes.  Everything is imported from
the reference tree at generation time, never copied (needs the reference sources; see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_compress_scales.py [--check]

Writes tests/golden/compress_scales_manifest.json — per case the sha256 of its inputs (`_compress_scale_cases.inputs` regenerates them), per
recorded operation the dtype, shape, canonical sha256 (every NaN rewritten to one NaN: payload and sign are not compared; the
sign of a zero is) and the NaN / inf / zero counts, the counts of NaN and inf scales and of NaN quotients, and for the integer cases the code
histogram and the groups per number of distinct codes — and tests/golden/compress_scales.safetensors: the `cross` outputs of at most
`_compress_scale_cases.WHOLE_MAX` bytes, canonical, whole (float8 codes as their bytes).

The generator STOPS AS A FINDING if the pinned oracle is not the reference on any case, or a compressor's `compress` is not `quantize`.
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

import _compress_scale_cases as C  # noqa: E402
import oracle as O  # noqa: E402
from compressed_tensors.compressors import BaseCompressor  # noqa: E402
from compressed_tensors.compressors.pack_quantized.helpers import pack_to_int32  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs, QuantizationScheme  # noqa: E402
from compressed_tensors.quantization.lifecycle.forward import fake_quantize, quantize  # noqa: E402
from compressed_tensors.quantization.quant_scheme import preset_name_to_scheme  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "compress_scales.safetensors")
MANIFEST = os.path.join(ROOT, "tests", "golden", "compress_scales_manifest.json")
SIZE_BOUND = os.path.getsize(os.path.join(ROOT, "tests", "golden", "decompress_scales.safetensors"))  # sized like the decompress fixture


def _args(r, **kw):
    strategy = dict(strategy="group", group_size=r["group"]) if r["group"] else dict(strategy="channel")
    if r["g_idx"] is not None:
        kw["actorder"] = "group"
    return QuantizationArgs(num_bits=r["bits"], symmetric=r["zp"] is None, type="float" if r["qtype"] == "fp8" else "int", **strategy, **kw)


def attention_outputs(key, r, t) -> dict:
    """a q / k / v state of shape (1, H, S, D) under the attn_head strategy, scales (H, 1, 1); and, a head at a time under that head's scale, the
    tensor strategy — held to the same rows"""
    B, H, S, D = r["attn"]
    kind = dict(num_bits=r["bits"], type="float" if r["qtype"] == "fp8" else "int", symmetric=r["zp"] is None)
    x = t["x"].reshape(B, H, S, D)
    s = t["scale"].reshape(H, 1, 1)
    z = None if t["zero_point"] is None else t["zero_point"].reshape(H, 1, 1)
    out = {}
    for op in r["ops"]:
        def ref(xx, ss, zz, strategy):
            args = QuantizationArgs(strategy=strategy, **kind)
            if op in ("fq", "fq8"):
                return fake_quantize(x=xx, scale=ss, zero_point=zz, args=args)
            return quantize(x=xx, scale=ss, zero_point=zz, args=args, dtype=torch.int8 if op == "q" else C.F8)

        out[op] = ref(x, s, z, "attn_head").reshape(H, S * D)
        for h in range(H if H <= 17 else 0):
            one = ref(x[:, h:h + 1], s[h].reshape(1), None if z is None else z[h].reshape(1), "tensor").reshape(S * D)
            if not _same(one, out[op][h]):
                raise SystemExit(f"FINDING: {key}/{op}: head {h} under the tensor strategy is not its row under attn_head")
    return out


def fp4_outputs(key, r, t) -> dict:
    """the NVFP4 / MXFP4 compressor's `compress` of the weight under the GIVEN group scales (and global scale)"""
    fmt = C.fp4_format(r)
    scheme = preset_name_to_scheme("NVFP4A16" if r["group"] == 16 else "MXFP4A16", ["Linear"])
    assert scheme.weights.group_size == r["group"]
    sd = {"weight": t["x"].clone(), "weight_scale": t["scale"].clone()}
    if r["gs"] is not None:
        sd["weight_global_scale"] = C.global_scale(r)
    c = BaseCompressor.get_value_from_registry(fmt).compress(sd, scheme)
    return {"fp4": c["weight_packed"], "fp4s": c["weight_scale"]}


def _same(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(C.canonical(a), C.canonical(b))


def reference_outputs(key, r, t) -> dict:
    """op -> the reference's answer; the compressors' `compress` where one takes the case, held to `quantize`"""
    if r["attn"]:
        return attention_outputs(key, r, t)
    if r["qtype"] == "fp4":
        return fp4_outputs(key, r, t)
    args = _args(r)
    scheme = QuantizationScheme(targets=["Linear"], weights=args)
    x, s, z, g = t["x"], t["scale"], t["zero_point"], t["g_idx"]
    sd = {"weight": x.clone(), "weight_scale": s}
    if z is not None:
        sd["weight_zero_point"] = z
    if g is not None:
        sd["weight_g_idx"] = g
    out = {}
    for op in r["ops"]:
        if op in ("q", "pack") and "q" not in out:
            out["q"] = quantize(x, s, z, args, dtype=torch.int8, g_idx=g)
        if op == "q" and r["bits"] == 8:
            c = BaseCompressor.get_value_from_registry("int-quantized").compress(dict(sd), scheme)
            if not _same(c["weight"], out["q"]):
                raise SystemExit(f"FINDING: {key}: the reference's int-quantized compress is not its quantize")
        elif op == "pack":
            out["pack"] = pack_to_int32(out["q"], r["bits"]).contiguous()
            c = BaseCompressor.get_value_from_registry("pack-quantized").compress(dict(sd), scheme)
            if not _same(c["weight_packed"], out["pack"]):
                raise SystemExit(f"FINDING: {key}: the reference's pack-quantized compress is not pack_to_int32 of its quantize")
        elif op == "q32":
            out[op] = quantize(x, s, z, args, dtype=torch.int32, g_idx=g)
        elif op == "qx":
            out[op] = quantize(x, s, z, args, g_idx=g)
        elif op in ("fq", "fq8"):
            out[op] = fake_quantize(x, s, z, args, g_idx=g)
        elif op == "f8":
            out[op] = quantize(x, s, z, args, dtype=C.F8, g_idx=g)
            c = BaseCompressor.get_value_from_registry("float-quantized").compress(dict(sd), scheme)
            if not _same(c["weight"], out[op]):
                raise SystemExit(f"FINDING: {key}: the reference's float-quantized compress is not its quantize")
    return {op: out[op] for op in r["ops"]}


def build():
    tensors, cases = {}, {}
    for key, r in C.case_list():
        t = C.inputs(r)
        ref = reference_outputs(key, r, t)
        mine = C.oracle_outputs(O, r, t)
        outs = {}
        for op in r["ops"]:
            if op == "q32":  # the cast of a NaN to int32 (x86: INT_MIN; the oracle and the GPU: 0) is not compared
                nanq = C.nan_quotient(r, t)
                if not bool(((ref[op] == -(1 << 31)) | (ref[op] == 0))[nanq].all()) or not bool((mine[op][nanq] == 0).all()):
                    raise SystemExit(f"FINDING: {key}/{op}: a NaN quotient is cast to something other than INT_MIN (reference) / 0 (oracle)")
            if op == "fp4":  # nor is the sign bit of an FP4 code whose quotient is NaN; its magnitude is 0 on every side
                nanq = C.nan_quotient(r, t)
                for side in (ref[op], mine[op]):
                    nib = torch.stack((side & 0xF, side >> 4), dim=-1).reshape(nanq.shape)
                    if not bool(((nib & 7)[nanq] == 0).all()):
                        raise SystemExit(f"FINDING: {key}/{op}: a NaN quotient has a non-zero FP4 magnitude")
            if op in C.MASKED_OPS:
                mine[op], ref[op] = C.masked(r, t, op, mine[op]), C.masked(r, t, op, ref[op])
            if not _same(mine[op], ref[op]):
                bad = int((C.canonical(mine[op]) != C.canonical(ref[op])).sum()) if mine[op].shape == ref[op].shape and mine[op].dtype == ref[op].dtype else -1
                raise SystemExit(f"FINDING: {key}/{op}: the pinned oracle is not the reference ({bad} elements)")
            whole = C.stored_whole(r, op, ref[op])
            outs[op] = dict(C.record(ref[op]), whole=whole)
            if whole:
                c = C.canonical(ref[op])
                tensors[f"{key}/{op}"] = c if c.dtype == torch.uint8 else c.view(ref[op].dtype)
        entry = dict(recipe=r, inputs_sha256=C.input_sha(t), out=outs, scales=C.scale_stats(r, t))
        if r["qtype"] == "int":
            q = ref["q"] if "q" in ref else quantize(t["x"], t["scale"], t["zero_point"], _args(r), dtype=torch.int8, g_idx=t["g_idx"])
            entry["codes"] = C.code_stats(r, t, q)
        cases[key] = entry
    blob = save(tensors)
    if len(blob) >= SIZE_BOUND:
        raise SystemExit(f"the fixture would be {len(blob)} bytes, the decompress fixture has {SIZE_BOUND}: lower WHOLE_MAX")
    return blob, (json.dumps(dict(cases=cases), indent=None, sort_keys=True, separators=(",", ":")).replace('},"', '},\n"') + "\n").encode()


def main():
    blob, manifest = build()
    if "--check" in sys.argv[1:]:
        for path, want in ((PATH, blob), (MANIFEST, manifest)):
            with open(path, "rb") as f:
                if f.read() != want:
                    raise SystemExit(f"{path} differs from what the reference produces")
        print("fixture matches; the pinned oracle equals the reference on every case")
        return
    for path, want in ((PATH, blob), (MANIFEST, manifest)):
        with open(path, "wb") as f:
            f.write(want)
    print(f"{len(C.case_list())} cases, {len(blob)} + {len(manifest)} bytes; the pinned oracle equals the reference on every case")


if __name__ == "__main__":
    main()
