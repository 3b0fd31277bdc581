"""developer script: group-wise 8-bit round-to-nearest of ONE weight in one pass (codec.rtn_quantize_group8: ct_rtn_quant_group8) against the
composition it replaces in `compress_rtn` — the group observer (codec.minmax_qparams / minmax_qparams_float), codec.quantize_tensor and, for
MXFP8, codec.compress_mx_scale — on the same GPU, and against the roofline of about 3.03 bytes per element.

    python tools/group8_rtn_bench.py [--iters 20] [--repeats 5] [--runs 2] [--out DIR]   (appends to DIR/group8_rtn_bench.jsonl; DIR defaults to profiles/)

Rows, bfloat16: 8192 x 8192, 4096 x 14336 and 14336 x 4096.  Schemes: mxfp8 (float8 in groups of 32, E8M0 scales), int8 g128 symmetric (`int`)
and asymmetric (`int_asym`), fp8 g128 — the keys of naive_quantized.base.RTN_GROUP8_MEASURED_FASTER.  Paths, alternated in the same call on the
same buffers:
  "one_pass"     rtn_quantize_group8: one launch, 2 bytes read and 1 written per element, the scales (and zero points) once;
  "composition"  the observer (2 read), the quantize (2 + 1 and the scales again), compress_mx_scale for mxfp8: two or three launches.
Protocol (as tools/block_rtn_bench.py): HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —, every path
warmed up, device events around --iters calls, --repeats regions, median and min; the whole table --runs times.  One JSON line per (scheme, row)
and run, then one "verdict" line per (scheme, row): the one pass is faster when its worst median plus the spread between the runs is below the
composition's best; a scheme is dispatched only if that holds on every row."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from attn_bench import COLD_BYTES, HBM_PEAK, region  # noqa: E402

from compressed_tensors_amd import codec  # noqa: E402

ROWS = [("8192x8192", (8192, 8192)), ("4096x14336", (4096, 14336)), ("14336x4096", (14336, 4096))]
F8 = torch.float8_e4m3fn
# scheme -> (group, rtn_quantize_group8's keywords, bytes of scales / zero points per group)
SCHEMES = {"mxfp8": (32, dict(qtype="float", mx=True), 1 + 2), "int": (128, dict(qtype="int", symmetric=True), 2 + 1),
           "int_asym": (128, dict(qtype="int", symmetric=False), 2 + 1), "fp8": (128, dict(qtype="float"), 2)}


def one_pass(w, scheme):
    group, kw, _ = SCHEMES[scheme]
    return codec.rtn_quantize_group8(w, group_size=group, **kw)


def composition(w, scheme):
    """what compress_rtn composes today: calculate_qparams_from_weight + compress"""
    group, kw, _ = SCHEMES[scheme]
    if kw["qtype"] == "float":
        scale = codec.minmax_qparams_float(w, kind="mxfp8" if scheme == "mxfp8" else "fp8", group_size=group)
        zp = torch.zeros(scale.shape, dtype=F8, device=w.device)
        q = codec.quantize_tensor(w, scale, zp, qtype="float", num_bits=8, strategy="group", group_size=group, dtype=F8)
        return (q, scale, None, codec.compress_mx_scale(scale)) if scheme == "mxfp8" else (q, scale, None)
    scale, zp = codec.minmax_qparams(w, num_bits=8, group_size=group, symmetric=kw["symmetric"])
    return codec.quantize_tensor(w, scale, zp, num_bits=8, strategy="group", group_size=group, dtype=torch.int8), scale, zp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--schemes", default=",".join(SCHEMES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of group8_rtn_bench.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group8_rtn_bench.py measures on the GPU: no device is visible")
    dev = torch.device("cuda:0")
    schemes = a.schemes.split(",")
    lines = []
    for run in range(a.runs):
        for name, shape in ROWS:
            n = shape[0] * shape[1]
            sets = [torch.randn(shape, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(max(2, -(-COLD_BYTES // (2 * n))))]
            for scheme in schemes:
                fns = {"one_pass": lambda w, s=scheme: one_pass(w, s), "composition": lambda w, s=scheme: composition(w, s)}
                got = {k: fn(sets[0]) for k, fn in fns.items()}  # warm-up of every path; the same bits
                assert all((x is None and y is None) or torch.equal(x.view(torch.uint8), y.view(torch.uint8))
                           for x, y in zip(got["one_pass"], got["composition"])), (name, scheme)
                del got
                torch.cuda.synchronize()
                samples = {k: [] for k in fns}
                for rep in range(a.repeats):  # alternated
                    for k, fn in (list(fns.items()) if rep % 2 == 0 else list(fns.items())[::-1]):
                        samples[k].append(region(fn, sets, a.iters, start_at=rep))
                group, _, per_group = SCHEMES[scheme]
                alg = 3 * n + per_group * (n // group)
                row = {"run": run, "scheme": scheme, "row": name, "shape": list(shape), "dtype": "bfloat16", "group": group,
                       "algorithmic_MB": round(alg / 1e6, 2), "buffer_sets": len(sets), "roofline_us": round(alg / HBM_PEAK * 1e6, 2)}
                for k, s in samples.items():
                    med = statistics.median(s)
                    row[f"{k}_median_us"], row[f"{k}_min_us"] = round(med * 1e3, 2), round(min(s) * 1e3, 2)
                    row[f"{k}_of_peak"] = round(alg / (med * 1e-3) / HBM_PEAK, 4)
                print(json.dumps(row), flush=True)
                lines.append(row)
            del sets
            torch.cuda.empty_cache()
    for scheme in schemes:
        for name, _ in ROWS:
            rs = [r for r in lines if r.get("row") == name and r.get("scheme") == scheme]
            p, b = [r["one_pass_median_us"] for r in rs], [r["composition_median_us"] for r in rs]
            spread = max(max(p) - min(p), max(b) - min(b)) if len(rs) > 1 else float("nan")
            v = {"verdict": name, "scheme": scheme, "path": "one_pass", "baseline": "composition", "path_worst_us": max(p), "baseline_best_us": min(b),
                 "run_spread_us": round(spread, 2), "faster": len(rs) > 1 and max(p) + spread < min(b)}
            print(json.dumps(v), flush=True)
            lines.append(v)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "group8_rtn_bench.jsonl"), "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
