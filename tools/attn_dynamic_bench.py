"""developer script: the dynamic group QDQ of strided q / k / v states (csrc/ct_attn_dyn.hip, codec.attn_dynamic_*) against what
it replaces, and its pair form against two launches.

    python tools/attn_dynamic_bench.py [--iters 20] [--repeats 5] [--runs 2] [--out DIR]   (APPENDS to DIR/attn_dynamic_bench.jsonl; DIR defaults to profiles/)

Rows, all bfloat16, `(B, S, H, D).transpose(1, 2)` views: prefill q (1, 32, 8192, 128) — one tensor, key "single" —, prefill k+v
(1, 8, 8192, 128) and decode k+v (64, 8, 1, 128) — two tensors, key "pair".  Schemes per row: FP8 group 128 (one scale per token and
head), MXFP4, NVFP4 with a global scale.  Variants, alternated in the same call on the same buffers:
  "strided"  codec.attn_dynamic_fake_quantize(form="strided") per tensor: one launch each, read in place;
  "pair"     (k+v rows) codec.attn_dynamic_fake_quantize_pair(form="strided", pair=True): one launch for both;
  "copy"     the composition the strided launch replaces, from the parent's kernels: `.contiguous()`, ct_dynamic_qdq, one copy_ into
             the reference's strides (form="copy"), per tensor;
  "eager"    the reference's op sequence (helpers.py:140-195, forward_helpers.py:118-215) restated in eager torch in this file.
Protocol (as tools/attn_bench.py): HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —, every
variant warmed up, device events around --iters calls, --repeats regions, median and min; the whole table --runs times.  Rates are
call times over the algorithmic bytes (one read plus one write of every tensor) as fractions of the 8 TB/s peak.  One JSON line per
row, scheme and run, then "verdict" lines — "faster" only if the worst median of the path plus the spread between the runs is below
the best median of its baseline: "strided" against "copy" on every row (key "single"), "pair" against "strided" on the k+v rows (key
"pair") — and a last line that says what codec.ATTN_DYNAMIC_MEASURED_FASTER may hold: a key may be True only if every verdict that
speaks for it says "faster"."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import compressed_tensors_amd as cta  # noqa: E402
from compressed_tensors_amd import codec  # noqa: E402

HBM_PEAK = 8.0e12
COLD_BYTES = 2 * 256 << 20
F8 = torch.float8_e4m3fn

ROWS = [  # (name, logical (B, H, S, D), tensors per call, the key of codec.ATTN_DYNAMIC_MEASURED_FASTER the row's own form speaks for)
    ("dyn_prefill_q", (1, 32, 8192, 128), 1, "single"),
    ("dyn_prefill_kv", (1, 8, 8192, 128), 2, "pair"),
    ("dyn_decode_kv", (64, 8, 1, 128), 2, "pair"),
]
SCHEMES = {  # name -> (arguments, global scale)
    "fp8_group128": (dict(num_bits=8, type="float", strategy="group", group_size=128, symmetric=True, dynamic=True), None),
    "mxfp4": (dict(num_bits=4, type="float", strategy="group", group_size=32, symmetric=True, dynamic=True, scale_dtype=torch.uint8, zp_dtype=torch.uint8), None),
    "nvfp4_gs": (dict(num_bits=4, type="float", strategy="tensor_group", group_size=16, symmetric=True, dynamic="local", scale_dtype=F8, zp_dtype=F8), 37.5),
}


def make(shape, dev):
    B, H, S, D = shape
    return torch.randn((B, S, H, D), device=dev, dtype=torch.float32).to(torch.bfloat16).transpose(1, 2)


def region(fn, inputs, iters, start_at=0):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(inputs[(start_at + i) % len(inputs)])
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms per call


def _cast_to_fp4(x):
    sign = torch.sign(x)
    x = torch.abs(x)
    x[(x >= 0.0) & (x <= 0.25)] = 0.0
    x[(x > 0.25) & (x < 0.75)] = 0.5
    x[(x >= 0.75) & (x <= 1.25)] = 1.0
    x[(x > 1.25) & (x < 1.75)] = 1.5
    x[(x >= 1.75) & (x <= 2.5)] = 2.0
    x[(x > 2.5) & (x < 3.5)] = 3.0
    x[(x >= 3.5) & (x <= 5.0)] = 4.0
    x[x > 5.0] = 6.0
    return x * sign


def eager(x, scheme, gs):
    """the reference's ops for a dynamic group scheme, one by one: unflatten, amin / amax, calculate_qparams, the fused
    quantize-dequantize, flatten.  (A timing stand-in: the bits are the fixtures' business, not this function's.)"""
    a = SCHEMES[scheme][0]
    g = a["group_size"]
    xg = x.unflatten(-1, (x.shape[-1] // g, g))
    mn, mx = torch.amin(xg, dim=-1), torch.amax(xg, dim=-1)
    mn, mx = torch.min(mn, torch.zeros_like(mn)), torch.max(mx, torch.zeros_like(mx))
    amax = torch.max(torch.abs(mn), torch.abs(mx))
    if scheme == "fp8_group128":
        scale, qmax = amax / 448.0, 448.0
    elif scheme == "mxfp4":
        scale, qmax = torch.exp2(torch.floor(torch.log2(amax.float())) - 2.0).to(x.dtype), 6.0
    else:
        scale, qmax = (gs * (amax / 6.0)).clamp(-448.0, 448.0).to(F8).to(torch.float32), 6.0
    scale = torch.where(scale == 0, torch.full_like(scale, torch.finfo(x.dtype).eps), scale)
    zp = torch.zeros_like(scale, dtype=torch.int8)
    scale = scale.unsqueeze(-1)
    zp = zp.unsqueeze(-1)
    if gs is not None:
        scale = scale / gs
    scaled = xg / scale
    scaled += zp.to(xg.dtype)
    q = torch.clamp(scaled, -qmax, qmax)
    q = q.to(F8).to(scaled.dtype) if qmax == 448.0 else _cast_to_fp4(q)
    d = q.to(scale.dtype) - zp.to(scale.dtype)
    return (d * scale).flatten(start_dim=-2).to(x.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of attn_dynamic_bench.jsonl")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for run in range(a.runs):
        for name, shape, count, key in ROWS:
            nbytes = math.prod(shape) * 2 * count
            sets = [tuple(make(shape, dev) for _ in range(count)) for _ in range(max(2, -(-COLD_BYTES // nbytes)))]
            for scheme, (kwargs, gsv) in SCHEMES.items():
                args = cta.QuantizationArgs(**kwargs)
                gs = None if gsv is None else torch.tensor([gsv], dtype=torch.float32, device=dev)
                fns = {
                    "strided": lambda ts: [codec.attn_dynamic_fake_quantize(t, args, gs, form="strided") for t in ts],
                    "copy": lambda ts: [codec.attn_dynamic_fake_quantize(t, args, gs, form="copy") for t in ts],
                    "eager": lambda ts: [eager(t, scheme, gs) for t in ts],
                }
                if count == 2:
                    fns["pair"] = lambda ts: codec.attn_dynamic_fake_quantize_pair(ts[0], ts[1], args, gs, gs, form="strided", pair=True)
                plan = codec.plan_attn_dynamic(sets[0][0].shape, sets[0][0].stride(), torch.bfloat16, args, global_scale=gs is not None)
                assert plan.form == "strided", plan
                for fn in fns.values():  # warm-up of every shape and variant
                    fn(sets[0])
                torch.cuda.synchronize()
                samples = {k: [] for k in fns}
                for rep in range(a.repeats):  # alternated
                    for k, fn in fns.items():
                        samples[k].append(region(fn, sets, a.iters, start_at=rep))
                row = {"run": run, "row": name, "scheme": scheme, "key": key, "shape": list(shape), "dtype": "bfloat16", "transposed_view": True,
                       "tensors": count, "MB": round(nbytes / 1e6, 2), "buffer_sets": len(sets)}
                for k, s in samples.items():
                    med = statistics.median(s)
                    row[f"{k}_median_us"], row[f"{k}_min_us"] = round(med * 1e3, 2), round(min(s) * 1e3, 2)
                    row[f"{k}_of_peak"] = round(2 * nbytes / (med * 1e-3) / HBM_PEAK, 4)
                print(json.dumps(row), flush=True)
                lines.append(row)
                del fns
            del sets
            torch.cuda.empty_cache()
    may = {}
    for name, _, count, _ in ROWS:
        for scheme in SCHEMES:
            rs = [r for r in lines if r.get("row") == name and r.get("scheme") == scheme]
            for path, base, key in (("strided", "copy", "single"),) + ((("pair", "strided", "pair"),) if count == 2 else ()):
                p, b = [r[f"{path}_median_us"] for r in rs], [r[f"{base}_median_us"] for r in rs]
                spread = max(max(p) - min(p), max(b) - min(b)) if len(rs) > 1 else float("nan")
                v = {"verdict": name, "scheme": scheme, "key": key, "path": path, "baseline": base, "path_worst_us": max(p), "baseline_best_us": min(b),
                     "run_spread_us": round(spread, 2), "faster": len(rs) > 1 and max(p) + spread < min(b)}
                print(json.dumps(v), flush=True)
                lines.append(v)
                may[key] = may.get(key, True) and v["faster"]
    lines.append({"ATTN_DYNAMIC_MEASURED_FASTER_may_be": may})
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "attn_dynamic_bench.jsonl"), "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
