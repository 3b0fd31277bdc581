"""developer script: the fast Walsh-Hadamard kernels (csrc/ct_hadamard.hip) against the reference's eager forward.

    python tools/hadamard_bench.py [--iters 20] [--repeats 5] [--runs 2] [--out DIR] [--only online,offline,sibling]

Rows (the measurement plan of DESIGN.md 5.11):
  * online, float32 accumulate: bfloat16 (1, 8192, H) with H = 4096 and 8192 at n = H, H = 8192 with head_dim blocks n = 128;
    float16 and float32 at (1, 8192, 4096), n = 4096;
  * offline, float64 accumulate: 4096 x 4096 and 8192 x 8192 bfloat16 weights, row form (Linear weight_input) and column form
    (Linear weight_output);
  * sibling: dyn_group_kernel's FP8 group-128 dynamic QDQ (csrc/ct_dynamic.hip) on the buffers of the n = 128 row — the same bytes
    per element, less arithmetic.
Beside each, "eager": the reference's forward restated here (the reference itself is not needed on the GPU machine),
`(x.to(precision) @ H / sqrt(n)).to(x.dtype)` with the materialised Sylvester matrix, block-diagonal through unflatten for
head_dim, `H.T @ W` for the column form — alternated with ours in the same call, on the same buffers.
Protocol: HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —, every shape warmed up,
device events around --iters launches (the float64 GEMMs of the eager side: --eager-iters), --repeats regions, median and min;
the whole table --runs times.  Rates are over the algorithmic bytes 2 * numel * itemsize, as fractions of the 8 TB/s peak and of
the 6.29 TB/s float4-copy ceiling.  One JSON line per row and run; with --out also DIR/hadamard_bench.jsonl.  --kernel-only runs
ours alone (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from compressed_tensors_amd import codec  # noqa: E402

HBM_PEAK, COPY_CEILING = 8.0e12, 6.29e12
COLD_BYTES = 2 * 256 << 20
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}

ROWS = [  # (group, name, dtype, shape, n, dim, precision)
    ("online", "online bf16 n=4096", "bf16", (1, 8192, 4096), 4096, -1, torch.float32),
    ("online", "online bf16 n=8192", "bf16", (1, 8192, 8192), 8192, -1, torch.float32),
    ("online", "online bf16 head_dim n=128", "bf16", (1, 8192, 8192), 128, -1, torch.float32),
    ("online", "online f16 n=4096", "f16", (1, 8192, 4096), 4096, -1, torch.float32),
    ("online", "online f32 n=4096", "f32", (1, 8192, 4096), 4096, -1, torch.float32),
    ("offline", "offline f64 rows 4096x4096", "bf16", (4096, 4096), 4096, -1, torch.float64),
    ("offline", "offline f64 cols 4096x4096", "bf16", (4096, 4096), 4096, 0, torch.float64),
    ("offline", "offline f64 rows 8192x8192", "bf16", (8192, 8192), 8192, -1, torch.float64),
    ("offline", "offline f64 cols 8192x8192", "bf16", (8192, 8192), 8192, 0, torch.float64),
]


def sylvester(n, dtype, device):
    H = torch.ones(1, 1, dtype=dtype, device=device)
    for _ in range(int(math.log2(n))):
        H = torch.vstack((torch.hstack((H, H)), torch.hstack((H, -H))))
    return H


def eager_fn(n, dim, precision, device):
    """HadamardTransform.forward restated: the GEMM with the materialised matrix, one division, one cast"""
    H = sylvester(n, precision, device)
    scale = torch.tensor(n, dtype=torch.float64).sqrt()

    def rows(x):
        v = x.to(precision)
        if v.shape[-1] > n:
            v = (v.unflatten(-1, (v.shape[-1] // n, n)) @ H).flatten(-2, -1)
        else:
            v = v @ H
        return (v / scale).to(x.dtype)

    def cols(x):
        return (H.T @ x.to(precision) / scale).to(x.dtype)

    return rows if dim == -1 else cols


def region(fn, inputs, iters, start_at=0):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(inputs[(start_at + i) % len(inputs)])
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--eager-iters", type=int, default=4, help="launches per region of the eager float64 GEMMs (tens of ms each)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="online,offline,sibling")
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    groups = a.only.split(",")
    lines = []

    def stats(row, name, samples, algo):
        med, mn = statistics.median(samples), min(samples)
        row[f"{name}_median_us"], row[f"{name}_min_us"] = round(med * 1e3, 2), round(mn * 1e3, 2)
        row[f"{name}_GBs"] = round(algo / med / 1e6, 1)
        row[f"{name}_of_peak"] = round(algo / med / 1e-3 / HBM_PEAK, 3)
        row[f"{name}_of_copy_ceiling"] = round(algo / med / 1e-3 / COPY_CEILING, 3)

    for run in range(a.runs):
        for group, name, dt, shape, n, dim, precision in ROWS:
            if group not in groups:
                continue
            dtype = DT[dt]
            numel = math.prod(shape)
            nbytes = numel * dtype.itemsize
            inputs = [torch.randn(shape, device=dev, dtype=torch.float32).to(dtype) for _ in range(max(2, -(-COLD_BYTES // nbytes)))]
            algo = 2 * nbytes
            row = {"run": run, "row": name, "dtype": dt, "shape": list(shape), "n": n, "dim": dim, "precision": str(precision), "MB": round(nbytes / 1e6, 2),
                   "buffers": len(inputs)}
            fns = {"ours": lambda x: codec.hadamard_transform(x, n, dim=dim, precision=precision)}
            its = {"ours": a.iters}
            if not a.kernel_only:
                fns["eager"] = eager_fn(n, dim, precision, dev)
                its["eager"] = a.eager_iters if precision is torch.float64 else a.iters
            if "sibling" in groups and n == 128 and not a.kernel_only:
                from compressed_tensors_amd.quantization import QuantizationArgs
                from compressed_tensors_amd.quantization.dynamic import dynamic_fake_quantize

                qargs = QuantizationArgs(num_bits=8, type="float", strategy="group", group_size=128, symmetric=True, dynamic=True)
                fns["sibling_fp8_group128"] = lambda x: dynamic_fake_quantize(x, qargs, None)
                its["sibling_fp8_group128"] = a.iters
            for k, fn in fns.items():  # warm-up of every shape and path
                fn(inputs[0])
            torch.cuda.synchronize()
            samples = {k: [] for k in fns}
            for rep in range(a.repeats):  # alternated: ours, eager, (sibling), ours, eager, ...
                for k, fn in fns.items():
                    samples[k].append(region(fn, inputs, its[k], start_at=rep))
            for k in fns:
                stats(row, k, samples[k], algo)
            if "eager" in fns:
                row["speedup_median"] = round(statistics.median(samples["eager"]) / statistics.median(samples["ours"]), 1)
                row["ours_slowest_us"], row["eager_fastest_us"] = round(max(samples["ours"]) * 1e3, 2), round(min(samples["eager"]) * 1e3, 2)
            del inputs, fns
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            lines.append(row)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "hadamard_bench.jsonl"), "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
