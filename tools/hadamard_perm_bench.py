"""developer script: the permuted Hadamard rotation of `randomize=True` (csrc/ct_hadamard_perm.hip) in one launch against the
composition it replaces.

    python tools/hadamard_perm_bench.py [--iters 20] [--repeats 5] [--runs 2] [--out DIR] [--kernel-only]

Rows (bfloat16): online float32 accumulation (1, 8192, 8192) at n = 128 and n = 8192, (1, 8192, 4096) at n = 4096,
(1, 8192, 14336) at n = 128, (1, 8192, 4096) at n = 4096 with signs (random-hadamard, K = 1); offline float64 accumulation
8192 x 8192, row form (n = 8192 and head_dim blocks n = 128) and column form.  Paths, alternated in the same call on the same buffers:
  fused       codec.hadamard_transform / hadamard_k_transform(..., perm=tables, form="fused"): one launch (three in the column form)
  composed    form="composed": index_select by q, the unpermuted launch, index_select by p — THE BASELINE the dispatch is judged by
  unpermuted  the same rotation without a permutation: the floor, it says what the gathers cost
  eager       upstream's forward restated here (the reference itself is not needed on the GPU machine): the weight
              `W[perm][:, perm]` built per call as transform/factory/hadamard.py:94-95 does, the GEMM, one division, one cast
Protocol: HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —, every shape and path warmed
up, device events around --iters calls (the eager float64 GEMMs: --eager-iters), --repeats regions, median and min; the whole
table --runs times.  Rates are over the algorithmic bytes, one read and one write of the tensor plus the two tables, as fractions
of the 8 TB/s peak.  One JSON line per row and run, then one verdict per row with the rule of tools/rotated_bench.py:
    faster = fused_worst + run_spread < composed_best
(medians; the spread is the larger of the two paths' max - min over the runs), and a last line that says which keys of
codec.HADAMARD_PERM_MEASURED_FASTER may be True: those whose every verdict says faster.  Written to DIR/hadamard_perm_bench.jsonl
(default profiles/)."""
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

HBM_PEAK = 8.0e12
COLD_BYTES = 2 * 256 << 20
F32, F64 = torch.float32, torch.float64

ROWS = [  # (name, shape, n, dim, precision, signs)
    ("online n=128 8192x8192", (1, 8192, 8192), 128, -1, F32, False),
    ("online n=8192 8192x8192", (1, 8192, 8192), 8192, -1, F32, False),
    ("online n=4096 8192x4096", (1, 8192, 4096), 4096, -1, F32, False),
    ("online n=128 8192x14336", (1, 8192, 14336), 128, -1, F32, False),
    ("online n=4096 8192x4096 signs", (1, 8192, 4096), 4096, -1, F32, True),
    ("offline f64 rows 8192x8192", (8192, 8192), 8192, -1, F64, False),
    ("offline f64 rows n=128 8192x8192", (8192, 8192), 128, -1, F64, False),
    ("offline f64 cols 8192x8192", (8192, 8192), 8192, 0, F64, False),
]


def sylvester(n, dtype, device):
    H = torch.ones(1, 1, dtype=dtype, device=device)
    for _ in range(int(math.log2(n))):
        H = torch.vstack((torch.hstack((H, H)), torch.hstack((H, -H))))
    return H


def eager_fn(n, dim, precision, perm, signs, device):
    """upstream's HadamardTransform.forward with a permutation: two n x n gathers, the GEMM, one division, one cast"""
    W = sylvester(n, precision, device)
    if signs is not None:
        W = signs.to(precision)[:, None] * W  # diag(s) H: random_hadamard_matrix with K == 1
    scale = torch.tensor(n, dtype=torch.float64).sqrt()
    perm = perm.to(device)

    def rows(x):
        w = W[perm][:, perm]
        v = x.to(precision)
        if v.shape[-1] > n:
            v = (v.unflatten(-1, (v.shape[-1] // n, n)) @ w).flatten(-2, -1)
        else:
            v = v @ w
        return (v / scale).to(x.dtype)

    def cols(x):
        w = W[perm][:, perm]
        return (w.T @ x.to(precision) / scale).to(x.dtype)

    return rows if dim == -1 else cols


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
    ap.add_argument("--eager-iters", type=int, default=2, help="calls per region of the eager path (milliseconds each)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of hadamard_perm_bench.jsonl")
    ap.add_argument("--kernel-only", action="store_true", help="the fused path alone (for a kernel trace of its own)")
    a = ap.parse_args()
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    lines = []
    for run in range(a.runs):
        for name, shape, n, dim, precision, with_signs in ROWS:
            gen = torch.Generator().manual_seed(n)
            perm = torch.randperm(n, generator=gen)
            tables = codec.hadamard_perm_tables(perm, dev)
            signs = (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).to(torch.int8).to(dev) if with_signs else None
            plan = codec.plan_hadamard_perm(shape, dtype, n, dim, precision, random=with_signs, form="fused")
            nbytes = math.prod(shape) * dtype.itemsize
            inputs = [torch.randn(shape, device=dev, dtype=torch.float32).to(dtype) for _ in range(max(2, -(-COLD_BYTES // nbytes)))]
            algo = 2 * nbytes + 2 * 2 * n
            row = {"run": run, "row": name, "dtype": "bf16", "shape": list(shape), "n": n, "dim": dim, "precision": str(precision), "signs": with_signs,
                   "key": plan.key, "fused_dispatch": bool(codec.HADAMARD_PERM_MEASURED_FASTER[plan.key]), "MB": round(nbytes / 1e6, 2), "buffers": len(inputs)}
            kw = dict(dim=dim, precision=precision)

            def ours(x, **extra):
                if with_signs:
                    return codec.hadamard_k_transform(x, n, None, signs, **kw, **extra)
                return codec.hadamard_transform(x, n, **kw, **extra)

            fns = {"fused": lambda x: ours(x, perm=tables, form="fused")}
            its = {"fused": a.iters}
            if not a.kernel_only:
                fns["composed"] = lambda x: ours(x, perm=tables, form="composed")
                fns["unpermuted"] = lambda x: ours(x)
                fns["eager"] = eager_fn(n, dim, precision, perm, signs, dev)
                its.update(composed=a.iters, unpermuted=a.iters, eager=a.eager_iters)
            for fn in fns.values():  # warm-up of every shape and path
                fn(inputs[0])
            torch.cuda.synchronize()
            samples = {k: [] for k in fns}
            for rep in range(a.repeats):  # alternated: fused, composed, unpermuted, eager, fused, ...
                for k, fn in fns.items():
                    samples[k].append(region(fn, inputs, its[k], start_at=rep))
            for k, s in samples.items():
                med = statistics.median(s)
                row[f"{k}_median_us"], row[f"{k}_min_us"] = round(med * 1e3, 2), round(min(s) * 1e3, 2)
                row[f"{k}_of_peak"] = round(algo / med / 1e-3 / HBM_PEAK, 3)
            if "composed" in samples:
                row["fused_over_composed"] = round(statistics.median(samples["fused"]) / statistics.median(samples["composed"]), 3)
                row["fused_over_unpermuted"] = round(statistics.median(samples["fused"]) / statistics.median(samples["unpermuted"]), 3)
            del inputs, fns
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            lines.append(row)
    verdicts = []
    if not a.kernel_only and a.runs >= 2:
        for name, *_ in ROWS:
            rs = [r for r in lines if r.get("row") == name]
            f, c = [r["fused_median_us"] for r in rs], [r["composed_median_us"] for r in rs]
            spread = max(max(f) - min(f), max(c) - min(c))
            v = {"verdict": name, "key": rs[0]["key"], "fused_dispatch": rs[0]["fused_dispatch"], "fused_worst_us": max(f), "composed_best_us": min(c),
                 "run_spread_us": round(spread, 2), "faster": max(f) + spread < min(c)}
            print(json.dumps(v), flush=True)
            verdicts.append(v)
        lines.extend(verdicts)
        may = {k: any(v["key"] == k for v in verdicts) and all(v["faster"] for v in verdicts if v["key"] == k) for k in codec.HADAMARD_PERM_MEASURED_FASTER}
        lines.append({"HADAMARD_PERM_MEASURED_FASTER_may_be": may})
        print(json.dumps(lines[-1]), flush=True)
    if a.out and not a.kernel_only:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "hadamard_perm_bench.jsonl"), "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")
    if any(v["fused_dispatch"] and not v["faster"] for v in verdicts):
        sys.exit("a dispatched fused form is not faster than the composition: the plan must decline it")


if __name__ == "__main__":
    main()
