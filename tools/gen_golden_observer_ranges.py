"""Generate the observer-range fixture by running the UPSTREAM REFERENCE on the CPU over the case matrix of tests/_observer_range_cases.py: weights
whose groups hold a planted extreme and partner — every 16-bit pattern, every exponent, the edge patterns crossed with each other, the
half-integer ties of the zero point, the fp32 exponent sweep — through `torch.aminmax` of every group and `calculate_qparams`
(quantization/utils/helpers.py) under INT args of every width and both symmetries and the FP8, NVFP4, MXFP4 and MXFP8 args, and through
`generate_gparam(min, max)`.  Everything is imported from the reference tree at generation time, never copied (needs the reference sources; see
oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_observer_ranges.py [--check]

Writes tests/golden/observer_ranges_manifest.json — per case the sha256 of its input and the number of groups that hold a NaN, per recorded op
(`i<bits><s|a>`, `fp8`, `mxfp4`, `mxfp8`, `nv.<global scale>`) the scale's dtype, shape, canonical sha256 (every NaN rewritten to one NaN: payload and
sign are not compared; the sign of a zero is) and its NaN / inf / zero / eps counts, the zero points' sha256 and the number of distinct ones; per
`generate_gparam` shape the sha256 of the global scales of all its inputs — and tests/golden/observer_ranges.safetensors: the `cross` outputs, whole.

The generator STOPS AS A FINDING if the pinned oracle is not the reference on any case.  The one property it does not compare is the MX scale of a
group that holds a NaN (`_observer_range_cases.masked`): there it asserts that the oracle gives inf, the project's pinned choice.
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

import _observer_range_cases as R  # noqa: E402
import oracle as O  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors.quantization.utils import calculate_qparams, generate_gparam  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "observer_ranges.safetensors")
MANIFEST = os.path.join(ROOT, "tests", "golden", "observer_ranges_manifest.json")
SIZE_BOUND = 1 << 20

F8 = torch.float8_e4m3fn
FLOAT_ARGS = {
    "fp8": dict(num_bits=8, type="float", strategy="channel", symmetric=True),
    "nvfp4": dict(num_bits=4, type="float", strategy="tensor_group", group_size=16, symmetric=True, scale_dtype=F8, zp_dtype=F8),
    "mxfp4": dict(num_bits=4, type="float", strategy="group", group_size=32, symmetric=True, scale_dtype=torch.uint8, zp_dtype=torch.uint8),
    "mxfp8": dict(num_bits=8, type="float", strategy="group", group_size=32, symmetric=True, scale_dtype=torch.uint8, zp_dtype=torch.uint8),
}


def reference_args(op):
    p = R.parse_op(op)
    if p["kind"] == "int":
        return QuantizationArgs(num_bits=p["bits"], symmetric=p["symmetric"], strategy="channel")
    return QuantizationArgs(**FLOAT_ARGS[p["kind"]])


def reference_gparam(x):
    return generate_gparam(x.min().reshape(1), x.max().reshape(1))


def _same(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(R.canonical(a), R.canonical(b))


def build():
    tensors, cases = {}, {}
    for key, r in R.case_list():
        x = R.weight(r)
        mn, mx = R.group_minmax(r, x)
        nang = R.nan_groups(r, x)
        outs, globals_ = {}, {}
        for op in r["ops"]:
            p = R.parse_op(op)
            gs = None
            if p["kind"] == "nvfp4":
                gs = R.global_scale(O, r, x, op)
                if p["gs"] == "gen" and not _same(gs, reference_gparam(R.finite_part(x)).to(torch.float32)):
                    raise SystemExit(f"FINDING: {key}/{op}: the pinned oracle's generate_gparam is not the reference's")
                globals_[op] = int(gs.view(torch.int32))
            ref_s, ref_z = calculate_qparams(mn, mx, reference_args(op), global_scale=gs)
            ref_s = ref_s.reshape(R.grid(r))
            ref_z = ref_z.reshape(R.grid(r)) if p["kind"] == "int" else None
            mine_s, mine_z = R.oracle_output(O, r, x, op)
            if op in R.MASKED_OPS:
                if not bool(torch.isinf(mine_s[nang]).all()) or not bool((mine_s[nang] > 0).all()):
                    raise SystemExit(f"FINDING: {key}/{op}: the pinned oracle's MX scale of a group that holds a NaN is not +inf")
                mine_s, ref_s = R.masked(r, x, op, mine_s), R.masked(r, x, op, ref_s)
            if not _same(mine_s, ref_s):
                bad = int((R.canonical(mine_s) != R.canonical(ref_s)).sum()) if mine_s.shape == ref_s.shape and mine_s.dtype == ref_s.dtype else -1
                raise SystemExit(f"FINDING: {key}/{op}: the pinned oracle's scale is not the reference's ({bad} groups; {mine_s.dtype} {ref_s.dtype})")
            if ref_z is not None and not (ref_z.dtype is torch.int8 and torch.equal(ref_z, mine_z)):
                raise SystemExit(f"FINDING: {key}/{op}: the pinned oracle's zero point is not the reference's ({int((ref_z != mine_z).sum())} groups)")
            whole = R.stored_whole(r)
            outs[op] = dict(R.record(r, op, ref_s, ref_z), whole=whole)
            if whole:
                tensors[f"{key}/{op}/scale"] = R.canonical(ref_s).view(ref_s.dtype)
                if ref_z is not None:
                    tensors[f"{key}/{op}/zp"] = ref_z.contiguous()
        cases[key] = dict(recipe=r, input_sha256=R.sha(x), nan_groups=int(nang.sum()), groups=nang.numel(), out=outs, global_scales=globals_)
    gparam = {}
    for dt in ("bf16", "f16"):
        for shape in R.gparam_shapes():
            xs = R.weight(R.gparam_case(dt, shape)).reshape(-1, *shape)
            ref = torch.cat([reference_gparam(t).to(torch.float32).reshape(1) for t in xs])
            mine = torch.cat([O.generate_gparam(t).reshape(1) for t in xs])
            if not _same(ref, mine):
                raise SystemExit(f"FINDING: generate_gparam {dt} {shape}: the pinned oracle is not the reference ({int((ref != mine).sum())} inputs)")
            gparam[f"{dt}.{shape[0]}x{shape[1]}"] = dict(R.gparam_record(ref), input_sha256=R.sha(xs))
    blob = save(tensors)
    manifest = (json.dumps(dict(cases=cases, gparam=gparam), indent=None, sort_keys=True, separators=(",", ":")).replace('},"', '},\n"') + "\n").encode()
    for name, data in (("observer_ranges.safetensors", blob), ("observer_ranges_manifest.json", manifest)):
        if len(data) >= SIZE_BOUND:
            raise SystemExit(f"{name} would be {len(data)} bytes: a committed file stays under 1 MiB")
    return blob, manifest


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
    print(f"{len(R.case_list())} cases, {len(blob)} + {len(manifest)} bytes; the pinned oracle equals the reference on every case")


if __name__ == "__main__":
    main()
