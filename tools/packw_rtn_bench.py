"""developer script: round-to-nearest pack-quantized compress of ONE weight at the widths next to 4 and 8 in one pass
(codec.rtn_quantize_and_pack(num_bits=...): ct_rtn_quant_pack_wb) against the composition it replaces in `compress_rtn` — the group observer
(codec.minmax_qparams) followed by codec.quantize_and_pack — on the same GPU, and against the roofline of the algorithmic bytes
(2 + num_bits / 8 bytes per element and a scale, plus an int8 zero point, per group).

    python tools/packw_rtn_bench.py [--iters 20] [--repeats 5] [--runs 2] [--out DIR]   (appends to DIR/packw_rtn_bench.jsonl; DIR defaults to profiles/)

Rows, bfloat16: 8192 x 8192, 4096 x 14336 and 14336 x 4096; the channel-wise scheme at 4096 x 2048 (a row is one group of at most 2048 columns).
Schemes: w3 g128, w2 g128, w6 g128, w3 g128 asymmetric (`w3asym`), w3 channel-wise (`w3ch`); on request w5, w7 and w2asym, w5asym, w6asym, w7asym
(all g128).  Paths, alternated in the same call on the same buffers:
  "one_pass"     rtn_quantize_and_pack: one launch, the weight read once;
  "composition"  minmax_qparams (the weight read), quantize_and_pack (the weight and the scales read again): two launches.
Neither path includes the stored form of an asymmetric scheme's zero points (pack_to_int32 along the rows): it is the same launch behind both.
Protocol (as tools/group8_rtn_bench.py): HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —, every path
warmed up, device events around --iters calls, --repeats regions, median, min and max; the whole table --runs times.  One JSON line per (scheme,
row) and run with the composition's own min-max spread of that run, then one "verdict" line per (scheme, row): the one pass is faster when in
EVERY run its median is below the composition's median by more than the composition's spread in that run; a scheme is dispatched only if that holds
on every row."""
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

BIG = [("8192x8192", (8192, 8192)), ("4096x14336", (4096, 14336)), ("14336x4096", (14336, 4096))]
# scheme -> (num_bits, group or None for channel-wise, symmetric, rows)
SCHEMES = {"w3": (3, 128, True, BIG), "w2": (2, 128, True, BIG), "w6": (6, 128, True, BIG), "w3asym": (3, 128, False, BIG),
           "w3ch": (3, None, True, [("4096x2048", (4096, 2048))])}
DEFAULT = ",".join(SCHEMES)
# the other keys of pack_quantized.base.RTN_PACKW_MEASURED_FASTER, on request (--schemes w5,w7,w2asym,w5asym,w6asym,w7asym)
SCHEMES.update({f"w{b}": (b, 128, True, BIG) for b in (5, 7)})
SCHEMES.update({f"w{b}asym": (b, 128, False, BIG) for b in (2, 5, 6, 7)})


def one_pass(w, scheme):
    bits, group, symmetric, _ = SCHEMES[scheme]
    return codec.rtn_quantize_and_pack(w, group_size=group, symmetric=symmetric, num_bits=bits)


def composition(w, scheme):
    """what compress_rtn composes for these widths: the observer, then the compress"""
    bits, group, symmetric, _ = SCHEMES[scheme]
    scale, zp = codec.minmax_qparams(w, num_bits=bits, group_size=group, symmetric=symmetric)
    return codec.quantize_and_pack(w, scale, zp, num_bits=bits, strategy="group" if group else "channel", group_size=group), scale, zp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--schemes", default=DEFAULT)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of packw_rtn_bench.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("packw_rtn_bench.py measures on the GPU: no device is visible")
    dev = torch.device("cuda:0")
    schemes = a.schemes.split(",")
    shapes = []
    for scheme in schemes:
        shapes += [row for row in SCHEMES[scheme][3] if row not in shapes]
    lines = []
    for run in range(a.runs):
        for name, shape in shapes:
            n = shape[0] * shape[1]
            sets = [torch.randn(shape, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(max(2, -(-COLD_BYTES // (2 * n))))]
            for scheme in schemes:
                bits, group, symmetric, rows = SCHEMES[scheme]
                if (name, shape) not in rows:
                    continue
                fns = {"one_pass": lambda w, s=scheme: one_pass(w, s), "composition": lambda w, s=scheme: composition(w, s)}
                got = {k: fn(sets[0]) for k, fn in fns.items()}  # warm-up of every path; the same bits
                assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(got["one_pass"], got["composition"])), (name, scheme)
                del got
                torch.cuda.synchronize()
                samples = {k: [] for k in fns}
                for rep in range(a.repeats):  # alternated
                    for k, fn in (list(fns.items()) if rep % 2 == 0 else list(fns.items())[::-1]):
                        samples[k].append(region(fn, sets, a.iters, start_at=rep))
                g = group or shape[1]
                alg = 2 * n + n * bits // 8 + (2 + 1) * (n // g)
                row = {"run": run, "scheme": scheme, "row": name, "shape": list(shape), "dtype": "bfloat16", "num_bits": bits, "group": g,
                       "symmetric": symmetric, "algorithmic_MB": round(alg / 1e6, 2), "buffer_sets": len(sets), "roofline_us": round(alg / HBM_PEAK * 1e6, 2)}
                for k, s in samples.items():
                    med = statistics.median(s)
                    row[f"{k}_median_us"], row[f"{k}_min_us"], row[f"{k}_max_us"] = round(med * 1e3, 2), round(min(s) * 1e3, 2), round(max(s) * 1e3, 2)
                    row[f"{k}_of_peak"] = round(alg / (med * 1e-3) / HBM_PEAK, 4)
                row["composition_spread_us"] = round(row["composition_max_us"] - row["composition_min_us"], 2)
                print(json.dumps(row), flush=True)
                lines.append(row)
            del sets
            torch.cuda.empty_cache()
    for scheme in schemes:
        for name, _ in SCHEMES[scheme][3]:
            rs = [r for r in lines if r.get("row") == name and r.get("scheme") == scheme]
            v = {"verdict": name, "scheme": scheme, "path": "one_pass", "baseline": "composition", "runs": len(rs),
                 "one_pass_median_us": [r["one_pass_median_us"] for r in rs], "composition_median_us": [r["composition_median_us"] for r in rs],
                 "composition_spread_us": [r["composition_spread_us"] for r in rs],
                 "faster": len(rs) > 1 and all(r["one_pass_median_us"] + r["composition_spread_us"] < r["composition_median_us"] for r in rs)}
            print(json.dumps(v), flush=True)
            lines.append(v)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "packw_rtn_bench.jsonl"), "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
