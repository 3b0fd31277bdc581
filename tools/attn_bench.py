"""developer script: the strided q / k / v QDQ (csrc/ct_attn.hip) against what it replaces, and its pair form against two launches.

    python tools/attn_bench.py [--rotated] [--iters 20] [--repeats 5] [--runs 2] [--out DIR]   (writes DIR/attn_bench.jsonl; DIR defaults to profiles/)

Rows, all bfloat16, FP8, static scales:
  * prefill q   (1, 32, 8192, 128) as the (B, S, H, D).transpose(1, 2) view a Llama passes: one tensor;
  * prefill k+v (1, 8, 8192, 128), the same view: two tensors;
  * decode  k+v (64, 8, 1, 128), contiguous: two tensors.
Paths, alternated in the same call on the same buffers:
  "strided"        codec.attn_fake_quantize per tensor, attn_head (one launch each, read in place);
  "pair"           codec.attn_fake_quantize_pair (k+v rows: one launch for both);
  "strided_tensor" the same entry under the tensor strategy;
  "parent_tensor"  the parent commit's forward_quantize for the tensor strategy on the same strided input: its `.contiguous()` copy
                   plus ct_fake_quantize_fp8 (codec.fake_quantize_tensor, untouched by this work) — the baseline of "strided_tensor";
  "reference"      the reference's eager fake_quantize under attn_head on the same GPU (the staged reference) — the baseline of
                   "strided"; absent where no reference is staged.
Protocol (as tools/rotated_bench.py): HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —, every
path warmed up, device events around --iters calls, --repeats regions, median and min; the whole table --runs times.  Rates are over the
algorithmic bytes (one read plus one write of every tensor) as fractions of the 8 TB/s peak.  One JSON line per row and run, then one
"verdict" line per k+v row: the pair form is faster when its worst median is below the two launches' best by more than the spread
between the runs.  The last line says what modeling.kvcache.PAIR_MEASURED_FASTER may hold: True only if every k+v row says so.
With --rotated: the head-dim Hadamard rotation in the QDQ's launch (csrc/ct_attn_rot.hip, codec.attn_rotated_*) against the path it
replaces.  Rows, all bfloat16, FP8, attn_head, n = 128, `(B, S, H, D).transpose(1, 2)` views: q (1, 32, 8192, 128) — one tensor, key
"single" —, k+v (1, 8, 8192, 128) and decode k+v (64, 8, 1, 128) — K rotated, V not, key "pair".  Paths, alternated on the same buffers:
  "fused"     codec.attn_rotated_fake_quantize{,_pair}(fused=True): one launch;
  "composed"  the three steps it replaces: `.contiguous()`, codec.hadamard_transform, codec.attn_fake_quantize{,_pair}.
The same protocol; results are APPENDED to DIR/attn_rot_bench.jsonl: one line per row and run, one "verdict" line per row — "faster"
only if the worst fused median plus the spread between the runs is below the best composed median — and a last line that says what
modeling.ROTATED_MEASURED_FASTER may hold: a key may be True only if every row that speaks for it says "faster"."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402

from compressed_tensors_amd import codec  # noqa: E402

HBM_PEAK = 8.0e12
COLD_BYTES = 2 * 256 << 20

ROWS = [  # (name, logical (B, H, S, D), transposed view?, tensors per call)
    ("prefill_q", (1, 32, 8192, 128), True, 1),
    ("prefill_kv", (1, 8, 8192, 128), True, 2),
    ("decode_kv", (64, 8, 1, 128), False, 2),
]


def make(shape, transposed, dev):
    B, H, S, D = shape
    if transposed:
        return torch.randn((B, S, H, D), device=dev, dtype=torch.float32).to(torch.bfloat16).transpose(1, 2)
    return torch.randn(shape, device=dev, dtype=torch.float32).to(torch.bfloat16)


def region(fn, inputs, iters, start_at=0):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(inputs[(start_at + i) % len(inputs)])
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms per call


def reference_fake_quantize():
    try:
        import ref_import

        if not ref_import.available():
            return None
        ref_import.import_reference()
        from compressed_tensors.quantization import QuantizationArgs
        from compressed_tensors.quantization.lifecycle.forward import fake_quantize
    except Exception as e:  # noqa: BLE001  (a developer script: say why the column is missing)
        print(json.dumps({"reference": f"unavailable: {e!r}"}), flush=True)
        return None
    args = QuantizationArgs(num_bits=8, type="float", symmetric=True, strategy="attn_head")
    return lambda x, scale: fake_quantize(x=x, scale=scale, zero_point=None, args=args)


ROTATED_ROWS = [  # (name, logical (B, H, S, D), tensors per call, the key of modeling.ROTATED_MEASURED_FASTER it speaks for)
    ("rot_prefill_q", (1, 32, 8192, 128), 1, "single"),
    ("rot_prefill_kv", (1, 8, 8192, 128), 2, "pair"),
    ("rot_decode_kv", (64, 8, 1, 128), 2, "pair"),
]
ROTATED_SIZE = 128


def rotated_main(a):
    dev = torch.device("cuda:0")
    kw = dict(num_bits=8, qtype="float", strategy="attn_head")
    n = ROTATED_SIZE
    lines = []
    for run in range(a.runs):
        for name, shape, count, key in ROTATED_ROWS:
            H = shape[1]
            nbytes = math.prod(shape) * 2 * count
            sets = [tuple(make(shape, True, dev) for _ in range(count)) for _ in range(max(2, -(-COLD_BYTES // nbytes)))]
            head = ((torch.arange(H, dtype=torch.float32, device=dev) + 3.0) / 448.0).to(torch.bfloat16).reshape(H, 1, 1)
            if count == 1:
                fns = {"fused": lambda ts: codec.attn_rotated_fake_quantize(ts[0], n, head, None, fused=True, **kw),
                       "composed": lambda ts: codec.attn_fake_quantize(codec.hadamard_transform(ts[0].contiguous(), n), head, None, **kw)}
            else:
                fns = {"fused": lambda ts: codec.attn_rotated_fake_quantize_pair(ts[0], ts[1], n, head, head, fused=True, **kw),
                       "composed": lambda ts: codec.attn_fake_quantize_pair(codec.hadamard_transform(ts[0].contiguous(), n), ts[1], head, head, **kw)}
            for fn in fns.values():
                fn(sets[0])
            torch.cuda.synchronize()
            samples = {k: [] for k in fns}
            for rep in range(a.repeats):  # alternated
                for k, fn in fns.items():
                    samples[k].append(region(fn, sets, a.iters, start_at=rep))
            row = {"run": run, "row": name, "key": key, "shape": list(shape), "rotation": n, "transposed_view": True, "tensors": count,
                   "MB": round(nbytes / 1e6, 2), "buffer_sets": len(sets)}
            for k, s in samples.items():
                med = statistics.median(s)
                row[f"{k}_median_us"], row[f"{k}_min_us"] = round(med * 1e3, 2), round(min(s) * 1e3, 2)
                row[f"{k}_of_peak"] = round(2 * nbytes / (med * 1e-3) / HBM_PEAK, 4)
            del sets, fns
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            lines.append(row)
    may = {}
    for name, _, _, key in ROTATED_ROWS:
        rs = [r for r in lines if r.get("row") == name]
        p, b = [r["fused_median_us"] for r in rs], [r["composed_median_us"] for r in rs]
        spread = max(max(p) - min(p), max(b) - min(b)) if len(rs) > 1 else float("nan")
        v = {"verdict": name, "key": key, "path": "fused", "baseline": "composed", "path_worst_us": max(p), "baseline_best_us": min(b),
             "run_spread_us": round(spread, 2), "faster": len(rs) > 1 and max(p) + spread < min(b)}
        print(json.dumps(v), flush=True)
        lines.append(v)
        may[key] = may.get(key, True) and v["faster"]
    lines.append({"ROTATED_MEASURED_FASTER_may_be": may})
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "attn_rot_bench.jsonl"), "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of attn_bench.jsonl / attn_rot_bench.jsonl")
    ap.add_argument("--rotated", action="store_true", help="the rotated rows (fused rotation + QDQ against the three steps it replaces)")
    a = ap.parse_args()
    if a.rotated:
        return rotated_main(a)
    dev = torch.device("cuda:0")
    ref_fq = reference_fake_quantize()
    kw = dict(num_bits=8, qtype="float")
    lines = []
    for run in range(a.runs):
        for name, shape, transposed, count in ROWS:
            H = shape[1]
            nbytes = math.prod(shape) * 2 * count
            sets = [tuple(make(shape, transposed, dev) for _ in range(count)) for _ in range(max(2, -(-COLD_BYTES // nbytes)))]
            head = ((torch.arange(H, dtype=torch.float32, device=dev) + 3.0) / 448.0).to(torch.bfloat16).reshape(H, 1, 1)
            one = head.reshape(-1)[:1].clone()
            fns = {
                "strided": lambda ts: [codec.attn_fake_quantize(t, head, None, strategy="attn_head", **kw) for t in ts],
                "strided_tensor": lambda ts: [codec.attn_fake_quantize(t, one, None, strategy="tensor", **kw) for t in ts],
                "parent_tensor": lambda ts: [codec.fake_quantize_tensor(t, one, None, strategy="tensor", **kw) for t in ts],
            }
            if count == 2:
                fns["pair"] = lambda ts: codec.attn_fake_quantize_pair(ts[0], ts[1], head, head, strategy="attn_head", **kw)
            if ref_fq is not None:
                fns["reference"] = lambda ts: [ref_fq(t, head) for t in ts]
            for fn in fns.values():  # warm-up of every shape and path
                fn(sets[0])
            torch.cuda.synchronize()
            samples = {k: [] for k in fns}
            for rep in range(a.repeats):  # alternated
                for k, fn in fns.items():
                    samples[k].append(region(fn, sets, a.iters, start_at=rep))
            row = {"run": run, "row": name, "shape": list(shape), "transposed_view": transposed, "tensors": count, "MB": round(nbytes / 1e6, 2), "buffer_sets": len(sets)}
            for k, s in samples.items():
                med = statistics.median(s)
                row[f"{k}_median_us"], row[f"{k}_min_us"] = round(med * 1e3, 2), round(min(s) * 1e3, 2)
                row[f"{k}_of_peak"] = round(2 * nbytes / (med * 1e-3) / HBM_PEAK, 4)
            del sets, fns
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            lines.append(row)
    pair_wins = []
    for name, _, _, count in ROWS:
        rs = [r for r in lines if r.get("row") == name]
        for path, base in (("strided", "reference"), ("strided_tensor", "parent_tensor")) + ((("pair", "strided"),) if count == 2 else ()):
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
    lines.append({"PAIR_MEASURED_FASTER_may_be": bool(pair_wins) and all(pair_wins)})
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "attn_bench.jsonl"), "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
