"""developer script: the random-hadamard kernels (csrc/ct_hadamard_k.hip) against the reference's eager forward.

    python tools/random_hadamard_bench.py [--iters 20] [--eager-iters 4] [--repeats 5] [--runs 2] [--out DIR] [--kernel-only]

Rows (the measurement plan of DESIGN.md 5.13), all online, float32 accumulation:
  * bfloat16 (1, 8192, 14336) and (1, 8192, 11008); (1, 4096, 28672) and (1, 4096, 18944): the matrix-core form, K = 224, 172, 224, 148;
  * bfloat16 (1, 8192, 4096) with k == 1 and signs, and beside it ct_hadamard_rows (the Sylvester rotation without signs) on the
    same buffers.
The factors are the fixtures' (tests/golden/random_hadamard.safetensors).  Beside each row "eager": the reference's forward restated
here (the reference itself is not needed on the GPU machine), `(x.to(float32) @ W / sqrt(n)).to(x.dtype)` with the materialised
n x n float32 weight — alternated with ours in the same call, on the same buffers.
Protocol: HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —, every shape warmed up, device
events around --iters launches (--eager-iters for the GEMMs), --repeats regions, median and min; the whole table --runs times.
Rates are over the algorithmic bytes 2 * numel * itemsize, as fractions of the 8 TB/s peak and of the 6.29 TB/s float4-copy
ceiling.  One JSON line per row and run; with --out also DIR/random_hadamard_bench.jsonl."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from safetensors.torch import load_file  # noqa: E402

from compressed_tensors_amd import codec  # noqa: E402

HBM_PEAK, COPY_CEILING = 8.0e12, 6.29e12
COLD_BYTES = 2 * 256 << 20

ROWS = [  # (name, shape, n)
    ("online bf16 n=14336 (224 x 64)", (1, 8192, 14336), 14336),
    ("online bf16 n=11008 (172 x 64)", (1, 8192, 11008), 11008),
    ("online bf16 n=28672 (224 x 128)", (1, 4096, 28672), 28672),
    ("online bf16 n=18944 (148 x 128)", (1, 4096, 18944), 18944),
    ("online bf16 n=4096 (signs + butterfly)", (1, 8192, 4096), 4096),
]


def weight(n, had_k, signs):
    """signs[:, None] * kron(had_k, H_M).T in float32 on the device"""
    k = 1 if had_k is None else had_k.shape[0]
    m = n // k
    i = torch.arange(m, device=signs.device)
    bits, parity = i[:, None] & i[None, :], torch.zeros(m, m, dtype=torch.int64, device=signs.device)
    while bool(bits.any()):
        parity ^= bits & 1
        bits = bits >> 1
    h = (1 - 2 * parity).float()
    hk = torch.ones(1, 1, device=signs.device) if had_k is None else had_k.float()
    return signs.float()[:, None] * torch.kron(hk, h).t()


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
    ap.add_argument("--eager-iters", type=int, default=4, help="launches per region of the eager n x n GEMMs (tens of ms each)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    golden = load_file(os.path.join(ROOT, "tests", "golden", "random_hadamard.safetensors"))
    lines = []

    def stats(row, name, samples, algo):
        med, mn = statistics.median(samples), min(samples)
        row[f"{name}_median_us"], row[f"{name}_min_us"] = round(med * 1e3, 2), round(mn * 1e3, 2)
        row[f"{name}_GBs"] = round(algo / med / 1e6, 1)
        row[f"{name}_of_peak"] = round(algo / med / 1e-3 / HBM_PEAK, 3)
        row[f"{name}_of_copy_ceiling"] = round(algo / med / 1e-3 / COPY_CEILING, 3)

    for run in range(a.runs):
        for name, shape, n in ROWS:
            had_k = golden.get(f"had_k.{n}")
            had_k, signs = (None if had_k is None else had_k.to(dev)), golden[f"signs.{n}"].to(dev)
            k = 1 if had_k is None else had_k.shape[0]
            numel = math.prod(shape)
            nbytes = numel * 2
            inputs = [torch.randn(shape, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(max(2, -(-COLD_BYTES // nbytes)))]
            algo = 2 * nbytes
            plan = codec.plan_hadamard_k(shape, torch.bfloat16, n, k)
            row = {"run": run, "row": name, "dtype": "bf16", "shape": list(shape), "n": n, "k": k, "m": n // k, "form": plan.form, "MB": round(nbytes / 1e6, 2),
                   "buffers": len(inputs)}
            fns = {"ours": lambda x: codec.hadamard_k_transform(x, n, had_k, signs)}
            its = {"ours": a.iters}
            if k == 1:
                fns["sylvester"] = lambda x: codec.hadamard_transform(x, n)
                its["sylvester"] = a.iters
            if not a.kernel_only:
                w = weight(n, had_k, signs)
                scale = torch.tensor(n, dtype=torch.float64).sqrt()
                fns["eager"] = lambda x: (x.to(torch.float32) @ w / scale).to(x.dtype)
                its["eager"] = a.eager_iters
            for fn in fns.values():  # warm-up of every shape and path
                fn(inputs[0])
            torch.cuda.synchronize()
            samples = {key: [] for key in fns}
            for rep in range(a.repeats):  # alternated: ours, (sylvester), eager, ours, ...
                for key, fn in fns.items():
                    samples[key].append(region(fn, inputs, its[key], start_at=rep))
            for key in fns:
                stats(row, key, samples[key], algo)
            row["mix_TFLOPs"] = round(2 * k * numel / statistics.median(samples["ours"]) / 1e9, 1) if k > 1 else 0.0
            if "eager" in fns:
                row["speedup_median"] = round(statistics.median(samples["eager"]) / statistics.median(samples["ours"]), 1)
                row["ours_slowest_us"], row["eager_fastest_us"] = round(max(samples["ours"]) * 1e3, 2), round(min(samples["eager"]) * 1e3, 2)
                assert max(samples["ours"]) < min(samples["eager"]), f"{name}: our slowest region is not faster than upstream's fastest"
            del inputs, fns
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            lines.append(row)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "random_hadamard_bench.jsonl"), "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
