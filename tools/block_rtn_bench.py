"""developer script: block-wise 8-bit round-to-nearest of ONE weight in one pass (codec.rtn_quantize_block8: ct_rtn_quant_block8, FP8_BLOCK, blocks of
128 x 128) against the composition it replaces where the kernel's plan refuses a weight — the blocks rearranged into rows, the channel-wise
observer over them (codec.minmax_qparams_float) and codec.quantize_tensor under the block strategy — on the same GPU, and against the roofline
of 3 bytes per element.

    python tools/block_rtn_bench.py [--iters 20] [--repeats 5] [--runs 2] [--out DIR]   (appends to DIR/block_rtn_bench.jsonl; DIR defaults to profiles/)

Rows, bfloat16: 8192 x 8192, 4096 x 14336 and 14336 x 4096.  Paths, alternated in the same call on the same buffers:
  "one_pass"     rtn_quantize_block8: one launch, 2 bytes read and 1 written per element;
  "composition"  quantization.utils._block_rows + minmax_qparams_float + quantize_tensor: a rearranged copy (2 + 2), the observer (2), the quantize (2 + 1).
Protocol (as tools/attn_observe_bench.py): HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —, every path
warmed up, device events around --iters calls, --repeats regions, median and min; the whole table --runs times.  One JSON line per row and run,
then one "verdict" line per row: the one pass is faster when its worst median plus the spread between the runs is below the composition's best."""
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
from compressed_tensors_amd.quantization.utils import _block_rows  # noqa: E402

ROWS = [("8192x8192", (8192, 8192)), ("4096x14336", (4096, 14336)), ("14336x4096", (14336, 4096))]
BLOCK = [128, 128]
F8 = torch.float8_e4m3fn


def one_pass(w):
    return codec.rtn_quantize_block8(w, block_structure=BLOCK)


def composition(w):
    rows, grid = _block_rows(w, BLOCK)
    scale = codec.minmax_qparams_float(rows, kind="fp8").reshape(grid)
    zp = torch.zeros(grid, dtype=F8, device=w.device)
    return codec.quantize_tensor(w, scale, zp, qtype="float", num_bits=8, strategy="block", block_structure=BLOCK, dtype=F8), scale, zp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of block_rtn_bench.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("block_rtn_bench.py measures on the GPU: no device is visible")
    dev = torch.device("cuda:0")
    fns = {"one_pass": one_pass, "composition": composition}
    lines = []
    for run in range(a.runs):
        for name, shape in ROWS:
            n = shape[0] * shape[1]
            sets = [torch.randn(shape, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(max(2, -(-COLD_BYTES // (2 * n))))]
            got = {k: fn(sets[0]) for k, fn in fns.items()}  # warm-up of every path; the same bits
            assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(got["one_pass"][:2], got["composition"][:2])), name
            del got
            torch.cuda.synchronize()
            samples = {k: [] for k in fns}
            for rep in range(a.repeats):  # alternated
                for k, fn in (list(fns.items()) if rep % 2 == 0 else list(fns.items())[::-1]):
                    samples[k].append(region(fn, sets, a.iters, start_at=rep))
            alg = 3 * n + 2 * (n // (BLOCK[0] * BLOCK[1]))
            row = {"run": run, "row": name, "shape": list(shape), "dtype": "bfloat16", "block": BLOCK, "algorithmic_MB": round(alg / 1e6, 2),
                   "buffer_sets": len(sets), "roofline_us": round(alg / HBM_PEAK * 1e6, 2)}
            for k, s in samples.items():
                med = statistics.median(s)
                row[f"{k}_median_us"], row[f"{k}_min_us"] = round(med * 1e3, 2), round(min(s) * 1e3, 2)
                row[f"{k}_of_peak"] = round(alg / (med * 1e-3) / HBM_PEAK, 4)
            del sets
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            lines.append(row)
    for name, _ in ROWS:
        rs = [r for r in lines if r.get("row") == name]
        p, b = [r["one_pass_median_us"] for r in rs], [r["composition_median_us"] for r in rs]
        spread = max(max(p) - min(p), max(b) - min(b)) if len(rs) > 1 else float("nan")
        v = {"verdict": name, "path": "one_pass", "baseline": "composition", "path_worst_us": max(p), "baseline_best_us": min(b),
             "run_spread_us": round(spread, 2), "faster": len(rs) > 1 and max(p) + spread < min(b)}
        print(json.dumps(v), flush=True)
        lines.append(v)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "block_rtn_bench.jsonl"), "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
