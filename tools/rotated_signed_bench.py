"""developer script: the signed power-of-two Hadamard rotation fused into the dynamic QDQ launch (csrc/ct_rotated_signed.hip)
against the two launches it replaces.

    python tools/rotated_signed_bench.py [--iters 20] [--repeats 5] [--runs 2] [--out DIR]   (writes DIR/rotated_signed_bench.jsonl; DIR defaults to profiles/)

Rows (the measurement plan of DESIGN.md 5.32), all bfloat16: (1, 8192, 8192) with n = 128 (head-dim blocks) and n = 8192 (the token
row), (1, 8192, 4096) with n = 4096, each behind FP8 token, FP8 group 128 and MXFP4.  The signs are seeded.  "fused" is
quantization.dynamic.rotated_fake_quantize(..., signs=s, fused=True) — a key is measured whether or not the plan dispatches to it
today; "fused_dispatch" says whether it does —, "composed" the same call with fused=False: ct_hadamard_k_rows then ct_dynamic_qdq —
alternated in the same run, on the same buffers.
Protocol (as tools/rotated_bench.py): HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —,
every shape warmed up, device events around --iters calls, --repeats regions, median and min; the whole table --runs times.  Rates
are over the algorithmic bytes 2 * numel * itemsize as fractions of the 8 TB/s peak.  One JSON line per row and run, then one
"verdict" line per row: the worst fused median plus the spread between the runs must be below the best composed median (the rule
of DESIGN.md 5.12).  The last line names the keys that won in every row that speaks for them: what ROTATED_SIGNED_MEASURED_FASTER
may hold.  The script exits non-zero when a row the plan dispatches to the fused kernel is not faster."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _dynamic_cases as D  # noqa: E402
from compressed_tensors_amd.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors_amd.quantization import dynamic  # noqa: E402
from compressed_tensors_amd.quantization.dynamic import plan_rotated_dynamic, rotated_fake_quantize  # noqa: E402

HBM_PEAK = 8.0e12
COLD_BYTES = 2 * 256 << 20
PRESETS = ("fp8_token", "fp8_group128", "mxfp4")
SHAPES = [((1, 8192, 8192), 128), ((1, 8192, 8192), 8192), ((1, 8192, 4096), 4096)]
ROWS = [(shape, n, preset) for shape, n in SHAPES for preset in PRESETS]


def region(fn, inputs, iters, start_at=0):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(inputs[(start_at + i) % len(inputs)])
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of rotated_signed_bench.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/rotated_signed_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    dispatched = dynamic.ROTATED_SIGNED_MEASURED_FASTER  # what the plan dispatches today
    lines, slower = [], 0
    for run in range(a.runs):
        for shape, n, preset in ROWS:
            signs = (torch.randint(0, 2, (n,), generator=torch.Generator().manual_seed(n), dtype=torch.int8) * 2 - 1).to(dev)
            args = QuantizationArgs(**D.PRESETS[preset])
            plan = plan_rotated_dynamic(shape, dtype, n, args, signed=True)
            assert plan.key is not None, (shape, n, preset, plan.reason)
            nbytes = math.prod(shape) * dtype.itemsize
            inputs = [torch.randn(shape, device=dev, dtype=torch.float32).to(dtype) for _ in range(max(2, -(-COLD_BYTES // nbytes)))]
            algo = 2 * nbytes
            row = {"run": run, "row": f"{preset} {'x'.join(map(str, shape))} n={n}", "preset": preset, "shape": list(shape), "n": n, "key": plan.key,
                   "fused_dispatch": plan.key in dispatched, "MB": round(nbytes / 1e6, 2), "buffers": len(inputs)}
            fns = {"fused": lambda x: rotated_fake_quantize(x, n, args, signs=signs, fused=True),
                   "composed": lambda x: rotated_fake_quantize(x, n, args, signs=signs, fused=False)}
            for fn in fns.values():  # warm-up of every shape and path
                fn(inputs[0])
            torch.cuda.synchronize()
            samples = {k: [] for k in fns}
            for rep in range(a.repeats):  # alternated: fused, composed, fused, composed, ...
                for k, fn in fns.items():
                    samples[k].append(region(fn, inputs, a.iters, start_at=rep))
            for k, s in samples.items():
                med = statistics.median(s)
                row[f"{k}_median_us"], row[f"{k}_min_us"] = round(med * 1e3, 2), round(min(s) * 1e3, 2)
                row[f"{k}_of_peak"] = round(algo / med / 1e-3 / HBM_PEAK, 3)
            row["fused_over_composed"] = round(statistics.median(samples["fused"]) / statistics.median(samples["composed"]), 3)
            del inputs, fns
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            lines.append(row)
    if a.runs >= 2:
        for shape, n, preset in ROWS:
            rs = [r for r in lines if "run" in r and r["preset"] == preset and r["shape"] == list(shape) and r["n"] == n]
            f, c = [r["fused_median_us"] for r in rs], [r["composed_median_us"] for r in rs]
            spread = max(max(f) - min(f), max(c) - min(c))
            v = {"verdict": rs[0]["row"], "key": rs[0]["key"], "fused_dispatch": rs[0]["fused_dispatch"], "fused_worst_us": max(f), "composed_best_us": min(c),
                 "run_spread_us": round(spread, 2), "faster": max(f) + spread < min(c)}
            print(json.dumps(v), flush=True)
            lines.append(v)
            slower += v["fused_dispatch"] and not v["faster"]
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "rotated_signed_bench.jsonl"), "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    verdicts = [v for v in lines if "verdict" in v]
    wins = sorted({v["key"] for v in verdicts} - {v["key"] for v in verdicts if not v["faster"]})
    print(json.dumps({"faster_in_every_row": wins, "dispatched": sorted(dispatched)}), flush=True)  # what ROTATED_SIGNED_MEASURED_FASTER may hold
    if slower:
        sys.exit(f"{slower} fused-dispatched row(s) are not faster than the two launches: the plan must decline them")


if __name__ == "__main__":
    main()
