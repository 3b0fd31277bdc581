"""developer script: the fused rotation + dynamic QDQ launch (csrc/ct_rotated.hip) against the two launches it replaces.

    python tools/rotated_bench.py [--iters 20] [--repeats 5] [--runs 2] [--out DIR] [--kernel-only]   (writes DIR/rotated_bench.jsonl; DIR defaults to profiles/)

Rows (the measurement plan of DESIGN.md 5.12), all bfloat16:
  * (1, 8192, 8192), n = 128: FP8 group 128, MXFP4, NVFP4 under a global scale, FP8 token, INT8 token;
  * (1, 8192, 14336), n = 128 and 512: FP8 token, FP8 group 128;
  * (1, 8192, 4096), n = 4096: FP8 token, FP8 group 128, NVFP4;
  * (1, 8192, 8192), n = 8192: FP8 token;
  * (1, 32768, 1024), (1, 16384, 2048) at n = the row: FP8 token, FP8 group 128 (every workgroup-block instantiation).
"fused" is quantization.dynamic.rotated_fake_quantize with every form enabled (dynamic.MEASURED_FASTER = ALL_FORMS for the run: a form
is measured whether or not the plan dispatches to it today; "fused_dispatch" says whether it does), "composed" the parent's
dynamic_fake_quantize(hadamard_transform(x, n), ...) — alternated in the same call, on the same buffers.
Protocol (as tools/hadamard_bench.py): HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —,
every shape warmed up, device events around --iters calls, --repeats regions, median and min; the whole table --runs times.
Rates are over the algorithmic bytes 2 * numel * itemsize as fractions of the 8 TB/s peak.  One JSON line per row and run, also written to
DIR/rotated_bench.jsonl, followed by one "verdict" line per row: the fused median must be below the composed median
by more than the spread between the runs — the script exits non-zero when a row the plan
dispatches to the fused kernel is not.  --kernel-only runs the fused call alone (for a `rocprofv3 --kernel-trace --stats` run)."""
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
from compressed_tensors_amd import codec  # noqa: E402
from compressed_tensors_amd.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors_amd.quantization import dynamic  # noqa: E402
from compressed_tensors_amd.quantization.dynamic import dynamic_fake_quantize, plan_rotated_dynamic, rotated_fake_quantize  # noqa: E402

HBM_PEAK = 8.0e12
COLD_BYTES = 2 * 256 << 20

ROWS = [  # (shape, n, preset)
    *[((1, 8192, 8192), 128, p) for p in ("fp8_group128", "mxfp4", "nvfp4", "fp8_token", "int8_token")],
    *[((1, 8192, 14336), n, p) for n in (128, 512) for p in ("fp8_token", "fp8_group128")],
    *[((1, 8192, 4096), 4096, p) for p in ("fp8_token", "fp8_group128", "nvfp4")],
    ((1, 8192, 8192), 8192, "fp8_token"),
    # the other instantiations of the workgroup-block kernel: <2,1>, <4,1> (one wave, no LDS); <8,4> (n = 16384) lost and is no
    # longer built: profiles/rotated_bench_declined_n16384.jsonl
    *[((1, 32768, 1024), 1024, p) for p in ("fp8_token", "fp8_group128")],
    *[((1, 16384, 2048), 2048, p) for p in ("fp8_token", "fp8_group128")],
]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of rotated_bench.jsonl")
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    lines, slower = [], 0
    dispatched = dynamic.MEASURED_FASTER  # what the plan dispatches today
    dynamic.MEASURED_FASTER = dynamic.ALL_FORMS  # measure every form the kernels compute, dispatched today or not
    for run in range(a.runs):
        for shape, n, preset in ROWS:
            args = QuantizationArgs(**D.PRESETS[preset])
            gs = torch.tensor([37.5], device=dev) if preset == "nvfp4" else None
            plan = plan_rotated_dynamic(shape, dtype, n, args, gs)
            nbytes = math.prod(shape) * dtype.itemsize
            inputs = [torch.randn(shape, device=dev, dtype=torch.float32).to(dtype) for _ in range(max(2, -(-COLD_BYTES // nbytes)))]
            algo = 2 * nbytes
            row = {"run": run, "row": f"{preset} n={n} {'x'.join(map(str, shape))}", "preset": preset, "shape": list(shape), "n": n, "form": plan.form,
                   "key": dynamic._measure_key(plan.form, n) if plan.fused else None, "fused_dispatch": plan.fused and dynamic._measure_key(plan.form, n) in dispatched, "MB": round(nbytes / 1e6, 2), "buffers": len(inputs)}
            fns = {"fused": lambda x: rotated_fake_quantize(x, n, args, gs)}
            if not a.kernel_only:
                fns["composed"] = lambda x: dynamic_fake_quantize(codec.hadamard_transform(x, n), args, gs)
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
            if "composed" in samples:
                row["fused_over_composed"] = round(statistics.median(samples["fused"]) / statistics.median(samples["composed"]), 3)
            del inputs, fns
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            lines.append(row)
    if not a.kernel_only and a.runs >= 2:
        # the rule of DESIGN.md 5.12: in every fused-dispatched row the fused median is below the composed median by more than the
        # spread between the runs of the table (the larger of the two paths' max - min over the runs)
        for shape, n, preset in ROWS:
            rs = [r for r in lines if "run" in r and r["preset"] == preset and r["n"] == n and r["shape"] == list(shape)]
            f, c = [r["fused_median_us"] for r in rs], [r["composed_median_us"] for r in rs]
            spread = max(max(f) - min(f), max(c) - min(c))
            v = {"verdict": rs[0]["row"], "key": rs[0]["key"], "fused_dispatch": rs[0]["fused_dispatch"], "fused_worst_us": max(f), "composed_best_us": min(c),
                 "run_spread_us": round(spread, 2), "faster": max(f) + spread < min(c)}
            print(json.dumps(v), flush=True)
            lines.append(v)
            slower += v["fused_dispatch"] and not v["faster"]
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "rotated_bench.jsonl"), "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    verdicts = [v for v in lines if "verdict" in v and v["key"]]
    wins = sorted({v["key"] for v in verdicts} - {v["key"] for v in verdicts if not v["faster"]})
    print(json.dumps({"faster_in_every_row": wins, "dispatched": sorted(dispatched)}), flush=True)  # what MEASURED_FASTER may hold
    if slower:
        sys.exit(f"{slower} fused-dispatched row(s) are not faster than the two launches: the plan must decline them")


if __name__ == "__main__":
    main()
