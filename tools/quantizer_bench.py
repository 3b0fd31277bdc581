"""developer script: host-clock time of every dense-checkpoint quantizer's `process` on one seeded TinyLlama-shaped bf16 shard (six layers of
`bench.TINYLLAMA_LAYER`, on the host, as a checkpoint shard arrives).  `process` ends in a stream synchronise, so the figure is the shard's whole
round trip: staging copy, table launches, copies back.  One JSON line per row (median, min, max of `--reps` after `--warmup`); `--root DIR` times
the package of another tree with this same script (the A/B of DESIGN.md's "one dense-checkpoint quantizer body" section)."""
import argparse, json, os, statistics, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose package is timed")
ap.add_argument("--label", default="tree")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--layers", type=int, default=6)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch
import bench as B
from compressed_tensors_amd.entrypoints import convert

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(2024)
tensors = {f"model.layers.{l}.{name}.weight": torch.randn(r, c, generator=g).to(torch.bfloat16)
           for l in range(a.layers) for name, r, c in B.TINYLLAMA_LAYER}
mb = sum(t.numel() * 2 for t in tensors.values()) / 1e6
ROWS = [("fp8_block", "FP8BlockQuantizer", {}), ("mxfp8", "MXFP8Quantizer", {}), ("fp8_dynamic", "FP8DynamicQuantizer", {}), ("w8a8", "W8A8Quantizer", {}),
        ("w4_sym", "PackQuantizedQuantizer", dict(num_bits=4, symmetric=True)), ("w4_asym", "PackQuantizedQuantizer", dict(num_bits=4, symmetric=False)),
        ("w3_sym", "PackQuantizedQuantizer", dict(num_bits=3, symmetric=True))]
for row, cls, kw in ROWS:
    conv = getattr(convert, cls)(device=dev, **kw)
    ms = []
    for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        out = conv.process(dict(tensors))
        ms.append(1e3 * (time.perf_counter() - t0))
        del out
    ms = ms[a.warmup:]
    print(json.dumps({"label": a.label, "row": row, "shard_mb": round(mb, 1), "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
                      "max_ms": round(max(ms), 3), "reps": a.reps}), flush=True)
