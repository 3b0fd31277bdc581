"""developer script: channel-wise 8-bit round-to-nearest of ONE weight in one pass (codec.rtn_quantize_channel8: ct_rtn_quant_channel8) on the same GPU

  long rows   the long form (rows beyond 16384 columns) against the composition it replaces in `compress_rtn` — the per-row observer
              (codec.minmax_qparams / minmax_qparams_float) followed by codec.quantize_tensor —, and against the roofline of 3 bytes per element;
  control     the two register forms (rows of at most 16384 columns) of this tree's library against another build's (--parent-lib: the library
              of the commit this one stands on), the same entry, the same buffers.

    python tools/channel8_rtn_bench.py [--iters 20] [--repeats 5] [--runs 2] [--parent-lib FILE] [--out DIR]   (appends to DIR/channel8_rtn_bench.jsonl)

Long rows, bfloat16: 8192 x 28672 (Llama-3-70B down_proj), 8192 x 29568 (Qwen2.5-72B), 16384 x 53248 (Llama-3.1-405B), 7168 x 18432 (DeepSeek-V3's dense
MLP).  Control rows: 8192 x 8192, 4096 x 14336, 14336 x 4096, 24576 x 1536.  Kinds: fp8, int (int8 symmetric), int_asym — the keys of
naive_quantized.base.RTN_CHANNEL8_LONG_MEASURED_FASTER.
Protocol (as tools/group8_rtn_bench.py): HBM-cold — the inputs rotate over at least 2 x the 256 MiB Infinity Cache —, every path warmed
up, device events around --iters calls, --repeats regions alternated between the paths, median and min; the whole table --runs times.  One JSON line
per (kind, row) and run, then one "verdict" line per (kind, row): the long form is faster when its worst median plus the spread between the runs is
below the composition's best, and a kind is dispatched only if that holds on every row; a control row holds when in no run this tree's median is above
the parent's by more than the parent's own spread over its runs."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from attn_bench import COLD_BYTES, HBM_PEAK, region  # noqa: E402

from compressed_tensors_amd import _lib, codec  # noqa: E402

LONG_ROWS = [("8192x28672", (8192, 28672)), ("8192x29568", (8192, 29568)), ("16384x53248", (16384, 53248)), ("7168x18432", (7168, 18432))]
CONTROL_ROWS = [("8192x8192", (8192, 8192)), ("4096x14336", (4096, 14336)), ("14336x4096", (14336, 4096)), ("24576x1536", (24576, 1536))]
F8 = torch.float8_e4m3fn
KINDS = {"fp8": dict(qtype="float", symmetric=True), "int": dict(qtype="int", symmetric=True), "int_asym": dict(qtype="int", symmetric=False)}


def one_pass(w, kind):
    return codec.rtn_quantize_channel8(w, **KINDS[kind])


def composition(w, kind):
    """what compress_rtn composes for a row the one pass does not take: calculate_qparams_from_weight + compress"""
    kw = KINDS[kind]
    if kw["qtype"] == "float":
        scale = codec.minmax_qparams_float(w, kind="fp8")
        zp = torch.zeros(scale.shape, dtype=F8, device=w.device)
        return codec.quantize_tensor(w, scale, zp, qtype="float", num_bits=8, strategy="channel", dtype=F8), scale, zp
    scale, zp = codec.minmax_qparams(w, num_bits=8, symmetric=kw["symmetric"])
    return codec.quantize_tensor(w, scale, zp, num_bits=8, strategy="channel", dtype=torch.int8), scale, zp


def raw_entry(lib, kind, shape, dev):
    """ct_rtn_quant_channel8 of `lib` on preallocated outputs: what the two builds are compared on, nothing of the host path around it"""
    kw = KINDS[kind]
    fp8 = kw["qtype"] == "float"
    out = torch.empty(shape, dtype=F8 if fp8 else torch.int8, device=dev)
    scale = torch.empty((shape[0], 1), dtype=torch.bfloat16, device=dev)
    zp = torch.empty((shape[0], 1), dtype=torch.int8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fn(w):
        rc = lib.ct_rtn_quant_channel8(w.data_ptr(), _lib.BF16, shape[0], shape[1], int(fp8), int(kw["symmetric"]), out.data_ptr(), scale.data_ptr(),
                                       None if fp8 else zp.data_ptr(), stream)
        assert rc == 0, rc
        return out, scale, zp

    return fn


def measure(fns, sets, iters, repeats):
    samples = {k: [] for k in fns}
    for rep in range(repeats):  # alternated
        for k, fn in (list(fns.items()) if rep % 2 == 0 else list(fns.items())[::-1]):
            samples[k].append(region(fn, sets, iters, start_at=rep))
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--parts", default="long,control")
    ap.add_argument("--parent-lib", default=None, help="libct_hip.so of the parent commit: the control rows run only with it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of channel8_rtn_bench.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("channel8_rtn_bench.py measures on the GPU: no device is visible")
    dev = torch.device("cuda:0")
    kinds, parts = a.kinds.split(","), a.parts.split(",")
    libs = {"this": _lib.load()}
    if a.parent_lib and "control" in parts:
        parent = ctypes.CDLL(a.parent_lib)
        parent.ct_rtn_quant_channel8.argtypes, parent.ct_rtn_quant_channel8.restype = _lib._PROTOTYPES["ct_rtn_quant_channel8"]
        libs["parent"] = parent
    rows = ([("long", *r) for r in LONG_ROWS] if "long" in parts else []) + ([("control", *r) for r in CONTROL_ROWS] if len(libs) == 2 else [])
    lines = []
    for run in range(a.runs):
        for part, name, shape in rows:
            n = shape[0] * shape[1]
            sets = [torch.randn(shape, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(max(2, -(-COLD_BYTES // (2 * n))))]
            for kind in kinds:
                if part == "long":
                    fns = {"one_pass": lambda w, k=kind: one_pass(w, k), "composition": lambda w, k=kind: composition(w, k)}
                else:
                    fns = {who: raw_entry(lib, kind, shape, dev) for who, lib in libs.items()}
                got = {k: [t.clone() for t in fn(sets[0])] for k, fn in fns.items()}  # warm-up of every path; the same bits
                a_, b_ = got.values()
                assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in list(zip(a_, b_))[:2 if kind == "fp8" else 3]), (name, kind)
                del got, a_, b_
                torch.cuda.synchronize()
                samples = measure(fns, sets, a.iters, a.repeats)
                alg = 3 * n + 2 * shape[0]
                row = {"run": run, "part": part, "kind": kind, "row": name, "shape": list(shape), "dtype": "bfloat16", "form": codec.rtn_channel8_form(shape, KINDS[kind]["symmetric"]),
                       "algorithmic_MB": round(alg / 1e6, 2), "buffer_sets": len(sets), "roofline_us": round(alg / HBM_PEAK * 1e6, 2)}
                for k, s in samples.items():
                    med = statistics.median(s)
                    row[f"{k}_median_us"], row[f"{k}_min_us"] = round(med * 1e3, 2), round(min(s) * 1e3, 2)
                    row[f"{k}_of_peak"] = round(alg / (med * 1e-3) / HBM_PEAK, 4)
                print(json.dumps(row), flush=True)
                lines.append(row)
            del sets
            torch.cuda.empty_cache()
    for part, name, _ in rows:
        for kind in kinds:
            rs = [r for r in lines if r.get("row") == name and r.get("kind") == kind and r.get("part") == part]
            path, base = ("one_pass", "composition") if part == "long" else ("this", "parent")
            p, b = [r[f"{path}_median_us"] for r in rs], [r[f"{base}_median_us"] for r in rs]
            if part == "long":
                spread = max(max(p) - min(p), max(b) - min(b)) if len(rs) > 1 else float("nan")
                v = {"verdict": name, "part": part, "kind": kind, "path": path, "baseline": base, "path_worst_us": max(p), "baseline_best_us": min(b),
                     "run_spread_us": round(spread, 2), "faster": len(rs) > 1 and max(p) + spread < min(b)}
            else:
                spread = max(b) - min(b) if len(rs) > 1 else float("nan")
                v = {"verdict": name, "part": part, "kind": kind, "path": path, "baseline": base, "path_worst_us": max(p), "baseline_worst_us": max(b),
                     "baseline_spread_us": round(spread, 2), "holds": len(rs) > 1 and all(x <= y + spread for x, y in zip(p, b))}
            print(json.dumps(v), flush=True)
            lines.append(v)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "channel8_rtn_bench.jsonl"), "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
