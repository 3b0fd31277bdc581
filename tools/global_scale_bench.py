"""developer script: MinMaxObserver.get_global_scale (kind 2 of ct_attn_observe, csrc/ct_attn_observe.hip) — the calibrated global scale of NVFP4
activations — against the eager chain it replaces (the reference tests' observer: reshape, torch.amin / amax, generate_gparam) on the same GPU,
and against the read-only roofline.

    python tools/global_scale_bench.py [--iters 20] [--repeats 5] [--runs 2] [--out DIR]   (writes DIR/global_scale_bench.jsonl; DIR defaults to profiles/)

Rows, bfloat16 Linear inputs: (1, 8192, 4096) and (1, 8192, 14336).  Paths, alternated in the same call on the same buffers:
  "observe"    get_global_scale of a static_minmax observer into a preallocated float32 parameter (what modeling.calibrate_global_scales does per
               forward): two launches, read in place;
  "reference"  MockMinMaxObserver.get_global_scale of the staged reference — absent where none is staged.
Protocol (as tools/attn_observe_bench.py): HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —, every path
warmed up, device events around --iters calls, --repeats regions, median and min; the whole table --runs times.  One JSON line per row and run,
then one "verdict" line per row: the path is faster when its worst median plus the spread between the runs is below the baseline's best."""
import argparse
import importlib.util
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from attn_bench import COLD_BYTES, HBM_PEAK, region  # noqa: E402

import compressed_tensors_amd as cta  # noqa: E402

ROWS = [("hidden_4096", (1, 8192, 4096)), ("hidden_14336", (1, 8192, 14336))]
ARGS = dict(num_bits=4, type="float", symmetric=True, strategy="tensor_group", group_size=16, dynamic="local", observer="static_minmax",
            scale_dtype=torch.float8_e4m3fn, zp_dtype=torch.float8_e4m3fn)


def reference_observer():
    """the reference tests' MockMinMaxObserver for the NVFP4 preset's input arguments, or None"""
    try:
        import ref_import

        if not ref_import.available():
            return None
        ref_import.import_reference()
        from compressed_tensors.quantization import QuantizationArgs

        spec = importlib.util.spec_from_file_location("ct_reference_mock_observer", os.path.join(ref_import.root(), "tests", "mock_observer.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    except Exception as e:  # noqa: BLE001  (a developer script: say why the column is missing)
        print(json.dumps({"reference": f"unavailable: {e!r}"}), flush=True)
        return None
    return mod.MockMinMaxObserver("input", QuantizationArgs(**ARGS), torch.nn.Module())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of global_scale_bench.jsonl")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ref = reference_observer()
    lines = []
    for run in range(a.runs):
        for name, shape in ROWS:
            nbytes = math.prod(shape) * 2
            sets = [torch.randn(shape, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(max(2, -(-COLD_BYTES // nbytes)))]
            observer = cta.quantization.MinMaxObserver("input", cta.QuantizationArgs(**ARGS), None)
            param = torch.nn.Parameter(torch.empty(1, dtype=torch.float32, device=dev), requires_grad=False)
            fns = {"observe": lambda t: observer.get_global_scale(t, param)}
            if ref is not None:
                fns["reference"] = lambda t: ref.get_global_scale(t)
                assert torch.equal(fns["observe"](sets[0]).cpu().view(torch.int32), fns["reference"](sets[0]).cpu().view(torch.int32)), name  # the same bits
                observer.reset()
            for fn in fns.values():  # warm-up of every shape and path
                fn(sets[0])
            torch.cuda.synchronize()
            samples = {k: [] for k in fns}
            for rep in range(a.repeats):  # alternated
                for k, fn in fns.items():
                    samples[k].append(region(fn, sets, a.iters, start_at=rep))
            row = {"run": run, "row": name, "shape": list(shape), "dtype": "bfloat16", "MB": round(nbytes / 1e6, 2), "buffer_sets": len(sets),
                   "roofline_us": round(nbytes / HBM_PEAK * 1e6, 2)}
            for k, s in samples.items():
                med = statistics.median(s)
                row[f"{k}_median_us"], row[f"{k}_min_us"] = round(med * 1e3, 2), round(min(s) * 1e3, 2)
                row[f"{k}_of_peak"] = round(nbytes / (med * 1e-3) / HBM_PEAK, 4)
            del sets, fns
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            lines.append(row)
    for name, _ in ROWS:
        rs = [r for r in lines if r.get("row") == name]
        if "reference_median_us" not in rs[0]:
            continue
        p, b = [r["observe_median_us"] for r in rs], [r["reference_median_us"] for r in rs]
        spread = max(max(p) - min(p), max(b) - min(b)) if len(rs) > 1 else float("nan")
        v = {"verdict": name, "path": "observe", "baseline": "reference", "path_worst_us": max(p), "baseline_best_us": min(b), "run_spread_us": round(spread, 2),
             "faster": len(rs) > 1 and max(p) + spread < min(b)}
        print(json.dumps(v), flush=True)
        lines.append(v)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "global_scale_bench.jsonl"), "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
