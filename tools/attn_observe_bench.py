"""developer script: the strided min-max observer (csrc/ct_attn_observe.hip) against the eager observer it replaces and against the
read-only roofline, and its pair form against two single calls.

    python tools/attn_observe_bench.py [--iters 20] [--repeats 5] [--runs 2] [--out DIR]   (writes DIR/attn_observe_bench.jsonl; DIR defaults to profiles/)

Rows, all bfloat16, FP8, attn_head, `(B, S, H, D).transpose(1, 2)` views as a Llama passes them:
  * prefill q   (1, 32, 8192, 128): one tensor;
  * prefill k+v (1, 8, 8192, 128): two tensors;
  * decode  k+v (64, 8, 1, 128): two tensors.
Paths, alternated in the same call on the same buffers:
  "observe"    codec.attn_observe per tensor, memoryless, scale and zero point written into preallocated parameters (what
               modeling.calibrate_attention does): two launches each, read in place;
  "pair"       codec.attn_observe_pair (k+v rows): the same two launches for both tensors;
  "reference"  the reference tests' eager observer (flatten, torch.amin / amax, calculate_qparams) on the same GPU, from the
               staged reference — absent where none is staged.
"roofline_us" is the read-only floor: the bytes of every tensor, read once, over the 8 TB/s peak; "<path>_of_peak" is that floor over
the path's median.
Protocol (as tools/attn_bench.py): HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —, every path
warmed up, device events around --iters calls, --repeats regions, median and min; the whole table --runs times.  One JSON line per
row and run, then one "verdict" line per comparison: a path is faster when its worst median plus the spread between the runs is
below the baseline's best.  The last line says what modeling.calibration.OBSERVE_PAIR_MEASURED_FASTER may hold: True only if the
pair is faster at every k+v row."""
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
from attn_bench import COLD_BYTES, HBM_PEAK, make, region  # noqa: E402

from compressed_tensors_amd import codec  # noqa: E402

ROWS = [  # (name, logical (B, H, S, D), tensors per call)
    ("prefill_q", (1, 32, 8192, 128), 1),
    ("prefill_kv", (1, 8, 8192, 128), 2),
    ("decode_kv", (64, 8, 1, 128), 2),
]


def reference_observer():
    """the reference tests' MockMinMaxObserver for FP8 attn_head key states, or None"""
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
    return mod.MockMinMaxObserver("k", QuantizationArgs(num_bits=8, type="float", symmetric=True, strategy="attn_head"), torch.nn.Module())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of attn_observe_bench.jsonl")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ref = reference_observer()
    kw = dict(num_bits=8, qtype="float", strategy="attn_head")
    lines = []
    for run in range(a.runs):
        for name, shape, count in ROWS:
            H = shape[1]
            nbytes = math.prod(shape) * 2 * count
            sets = [tuple(make(shape, True, dev) for _ in range(count)) for _ in range(max(2, -(-COLD_BYTES // nbytes)))]
            states = [codec.attn_observe_state(H, dev) for _ in range(count)]
            scales = [torch.empty(H, 1, 1, dtype=torch.bfloat16, device=dev) for _ in range(count)]
            zps = [torch.zeros(H, 1, 1, dtype=torch.float8_e4m3fn, device=dev) for _ in range(count)]
            fns = {"observe": lambda ts: [codec.attn_observe(t, st, scale=s, zero_point=z, **kw) for t, st, s, z in zip(ts, states, scales, zps)]}
            if count == 2:
                fns["pair"] = lambda ts: codec.attn_observe_pair(ts[0], ts[1], states[0], states[1], k_scale=scales[0], v_scale=scales[1],
                                                                 k_zero_point=zps[0], v_zero_point=zps[1], **kw)
            if ref is not None:
                fns["reference"] = lambda ts: [ref(t) for t in ts]
            for fn in fns.values():  # warm-up of every shape and path
                fn(sets[0])
            torch.cuda.synchronize()
            samples = {k: [] for k in fns}
            for rep in range(a.repeats):  # alternated
                for k, fn in fns.items():
                    samples[k].append(region(fn, sets, a.iters, start_at=rep))
            row = {"run": run, "row": name, "shape": list(shape), "transposed_view": True, "tensors": count, "MB": round(nbytes / 1e6, 2),
                   "buffer_sets": len(sets), "roofline_us": round(nbytes / HBM_PEAK * 1e6, 2)}
            for k, s in samples.items():
                med = statistics.median(s)
                row[f"{k}_median_us"], row[f"{k}_min_us"] = round(med * 1e3, 2), round(min(s) * 1e3, 2)
                row[f"{k}_of_peak"] = round(nbytes / (med * 1e-3) / HBM_PEAK, 4)
            del sets, fns
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            lines.append(row)
    pair_wins = []
    for name, _, count in ROWS:
        rs = [r for r in lines if r.get("row") == name]
        for path, base in (("observe", "reference"),) + ((("pair", "observe"),) if count == 2 else ()):
            if f"{base}_median_us" not in rs[0]:
                continue
            p, b = [r[f"{path}_median_us"] for r in rs], [r[f"{base}_median_us"] for r in rs]
            spread = max(max(p) - min(p), max(b) - min(b)) if len(rs) > 1 else float("nan")
            v = {"verdict": name, "path": path, "baseline": base, "path_worst_us": max(p), "baseline_best_us": min(b), "run_spread_us": round(spread, 2),
                 "faster": len(rs) > 1 and max(p) + spread < min(b)}
            print(json.dumps(v), flush=True)
            lines.append(v)
            if path == "pair":
                pair_wins.append(v["faster"])
    lines.append({"OBSERVE_PAIR_MEASURED_FASTER_may_be": bool(pair_wins) and all(pair_wins)})
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "attn_observe_bench.jsonl"), "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
