"""ModelCompressor.compress_model_rtn wall time, table launches (batched=True) against one launch per module (batched=False, the path before the
tables existed), alternated in one process on the same trees: a Llama-3-8B-shaped tree (32 layers, 224 modules) and a TinyLlama-shaped one (22
layers, 154 modules); W4 g128 symmetric, W4 g128 asymmetric, MXFP4, NVFP4, FP8_BLOCK (`fp8block`: its table form is
`naive_quantized.base.rtn_block8_windows`, which `compress_model_rtn` does not dispatch to) and MXFP8 (`mxfp8`: the window hook of
mxfp8-quantized against its `compress_rtn` per module, as that is dispatched) and the channel-wise 8-bit presets FP8_DYNAMIC (`fp8dyn`) and W8A8 (`w8a8`:
their table form is `naive_quantized.base.rtn_channel8_windows`, likewise not dispatched to) and W3 g128 symmetric / asymmetric (`w3`, `w3asym`: the table
of the widths next to 4 and 8 with its gate forced on, against `compress_rtn` per module — `--packw-single` picks that module path).  A compress consumes the model, so the dense weights are kept and re-attached
between iterations, outside the timed region.  Prints one JSON line per (tree, scheme): the median wall time per call of both paths after warm-up,
their min / max (the spread of repeated runs), the time at which the host returns, and the fraction of the HBM peak from the algorithmic bytes.

    python tools/rtn_bench.py [--reps 7] [--warmup 2] [--trees 8b,tiny] [--schemes w4,w4asym,mxfp4,nvfp4,fp8block,mxfp8,fp8dyn,w8a8,w3,w3asym] [--packw-single shipped|one_pass|composition] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import compressed_tensors_amd as cta  # noqa: E402
from compressed_tensors_amd.compressors.naive_quantized.base import (  # noqa: E402
    FloatQuantizationCompressor,
    IntQuantizationCompressor,
    rtn_block8_windows,
    rtn_channel8_windows,
)

HBM_PEAK = 8e12  # bytes / s, the figure every table of DESIGN.md is relative to
TINY = ((2048, 2048), (256, 2048), (256, 2048), (2048, 2048), (5632, 2048), (5632, 2048), (2048, 5632))
L8B = ((4096, 4096), (1024, 4096), (1024, 4096), (4096, 4096), (14336, 4096), (14336, 4096), (4096, 14336))
TREES = {"8b": ("llama-8B-shaped", L8B, 32), "tiny": ("tinyllama-shaped", TINY, 22)}


def scheme_of(name):
    if name == "w4":
        args = cta.QuantizationArgs(num_bits=4, group_size=128, symmetric=True, strategy="group")
    elif name == "w4asym":
        args = cta.QuantizationArgs(num_bits=4, group_size=128, symmetric=False, strategy="group")
    elif name in ("w3", "w3asym"):  # the W3A16 preset and its asymmetric form: the one-pass table of the widths next to 4 and 8
        args = cta.QuantizationArgs(num_bits=3, group_size=128, symmetric=(name == "w3"), strategy="group")
    elif name == "mxfp4":
        args = cta.QuantizationArgs(num_bits=4, type="float", strategy="group", symmetric=True, group_size=32, scale_dtype=torch.uint8)
    elif name == "nvfp4":
        args = cta.QuantizationArgs(num_bits=4, type="float", strategy="tensor_group", symmetric=True, group_size=16, scale_dtype=torch.float8_e4m3fn)
    elif name == "fp8block":  # the FP8_BLOCK preset: float-quantized needs its input activations
        act = cta.QuantizationArgs(num_bits=8, type="float", strategy="group", symmetric=True, dynamic=True, group_size=128)
        return cta.QuantizationScheme(targets=["Linear"], input_activations=act,
                                      weights=cta.QuantizationArgs(num_bits=8, type="float", strategy="block", symmetric=True, block_structure=[128, 128]))
    elif name in ("fp8dyn", "w8a8"):  # the FP8_DYNAMIC / W8A8 presets: channel-wise weights, dynamic per-token activations
        qtype = "float" if name == "fp8dyn" else "int"
        return cta.QuantizationScheme(targets=["Linear"], input_activations=cta.QuantizationArgs(num_bits=8, type=qtype, strategy="token", symmetric=True, dynamic=True),
                                      weights=cta.QuantizationArgs(num_bits=8, type=qtype, strategy="channel", symmetric=True))
    elif name == "mxfp8":  # the MXFP8 preset
        mx = dict(num_bits=8, type="float", strategy="group", symmetric=True, group_size=32, scale_dtype=torch.uint8, zp_dtype=torch.uint8)
        scheme = cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(dynamic=False, **mx), input_activations=cta.QuantizationArgs(dynamic=True, **mx))
        scheme.format = "mxfp8-quantized"
        return scheme
    else:
        raise SystemExit(f"unknown scheme {name}")
    return cta.QuantizationScheme(targets=["Linear"], weights=args)


def algorithmic_bytes(name, rows, cols):
    """what one compress has to move: the weight in, the codes and the scales (and stored zero points) out"""
    n = rows * cols
    if name == "mxfp4":
        return 2 * n + n // 2 + n // 32
    if name == "mxfp8":
        return 2 * n + n + n // 32  # one byte per element and one exponent byte per group of 32
    if name in ("fp8dyn", "w8a8"):
        return 2 * n + n + 2 * rows  # one byte per element and one 16-bit scale per row
    if name == "fp8block":
        return 2 * n + n + 2 * (-(-rows // 128) * (cols // 128))  # one byte per element and one 16-bit scale per block of 128 x 128
    if name == "nvfp4":
        return 2 * 2 * n + n // 2 + n // 16 + 4  # the weight twice (the tensor-wide amax of generate_gparam is a pass of its own), the float8 scales, the global scale
    if name in ("w3", "w3asym"):
        out = 2 * n + 3 * n // 8 + 2 * (n // 128)
        if name == "w3asym":
            out += -(-rows * 3 // 32) * (cols // 128) * 4  # weight_zero_point, packed along the rows
        return out
    out = 2 * n + n // 2 + 2 * (n // 128)
    if name == "w4asym":
        out += -(-rows // 8) * (cols // 128) * 4  # weight_zero_point, packed along the rows
    return out


def build(shapes, nlayers, dev):
    """the tree on the meta device plus the pool of dense weights that is re-attached before every compress"""
    root = torch.nn.Module()
    root.layers = torch.nn.ModuleList()
    g = torch.Generator(device=dev).manual_seed(1)
    pool = []
    for _ in range(nlayers):
        blk = torch.nn.Module()
        root.layers.append(blk)
        for k, (r, c) in enumerate(shapes):
            lin = torch.nn.Linear(c, r, bias=False, device="meta")
            setattr(blk, f"proj{k}", lin)
            w = torch.randn(r, c, dtype=torch.bfloat16, device=dev, generator=g)
            pool.append((lin, torch.nn.Parameter(w, requires_grad=False)))
    return root, pool


def attach(model, pool, scheme, mc):
    mc.remove_decompression_hook(model)
    for lin, w in pool:
        lin._parameters.clear()
        lin._parameters["weight"] = w
        lin.__dict__.pop("quantization_status", None)
        lin.quantization_scheme = scheme


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=7, help="alternations of the two paths (the median is reported; at least 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trees", default="8b,tiny")
    ap.add_argument("--schemes", default="w4,w4asym,mxfp4,nvfp4")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--packw-single", default="shipped", choices=("shipped", "one_pass", "composition"),
                    help="schemes w3 / w3asym: what batched=False runs per module (default: what compress_rtn dispatches)")
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("rtn_bench.py measures on the GPU: no device is visible")
    dev = torch.device("cuda:0")
    cta.NVFP4PackedCompressor.RTN_TABLE_MEASURED_FASTER = True  # batched=True measures the NVFP4 table whatever the dispatch constant holds: this is its input
    cta.BaseCompressor.get_value_from_registry("mxfp8-quantized").RTN_TABLE_MEASURED_FASTER = True  # likewise MXFP8's
    # likewise the table of the widths next to 4 and 8 (schemes w3, w3asym); batched=False stays what `compress_rtn` dispatches per module, or what
    # --packw-single asks for: "one_pass" = one launch per module, "composition" = the observer and the compress
    from compressed_tensors_amd.compressors.pack_quantized import base as packq

    packq.RTN_PACKW_TABLE_MEASURED_FASTER.update(dict.fromkeys(packq.RTN_PACKW_TABLE_MEASURED_FASTER, True))
    if a.packw_single != "shipped":
        packq.RTN_PACKW_MEASURED_FASTER.update(dict.fromkeys(packq.RTN_PACKW_MEASURED_FASTER, a.packw_single == "one_pass"))
    for tree in a.trees.split(","):
        label, shapes, nlayers = TREES[tree]
        model, pool = build(shapes, nlayers, dev)
        for name in a.schemes.split(","):
            scheme = scheme_of(name)
            mc = cta.ModelCompressor()
            alg = sum(algorithmic_bytes(name, *w.shape) for _, w in pool)
            wall, host = {True: [], False: []}, {True: [], False: []}
            for rep in range(a.warmup + a.reps):
                for batched in (True, False) if rep % 2 == 0 else (False, True):
                    attach(model, pool, scheme, mc)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if name == "fp8block" and batched:  # the 8-bit codecs have no window hook: their table form is the block-wise window driver
                        for lin, _ in pool:
                            lin.quantization_scheme.format = "float-quantized"
                        rtn_block8_windows(FloatQuantizationCompressor, [lin for lin, _ in pool])
                    elif name in ("fp8dyn", "w8a8") and batched:  # likewise: the channel-wise window driver
                        for lin, _ in pool:
                            lin.quantization_scheme.format = "float-quantized" if name == "fp8dyn" else "int-quantized"
                        rtn_channel8_windows(FloatQuantizationCompressor if name == "fp8dyn" else IntQuantizationCompressor, [lin for lin, _ in pool])
                    else:
                        mc.compress_model_rtn(model, batched=batched)
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if rep >= a.warmup:
                        wall[batched].append(t2 - t0)
                        host[batched].append(t1 - t0)
            line = {"tree": label, "modules": len(pool), "scheme": name, "reps": a.reps, "algorithmic_bytes": alg}
            if name in ("w3", "w3asym"):
                line["per_module_path"] = a.packw_single
            for batched, key in ((True, "table"), (False, "per_module")):
                med = statistics.median(wall[batched])
                line[key] = {"wall_ms_median": round(med * 1e3, 4), "wall_ms_min": round(min(wall[batched]) * 1e3, 4),
                             "wall_ms_max": round(max(wall[batched]) * 1e3, 4), "host_ms_median": round(statistics.median(host[batched]) * 1e3, 4),
                             "host_us_per_module": round(statistics.median(host[batched]) * 1e6 / len(pool), 2),
                             "hbm_peak_fraction": round(alg / med / HBM_PEAK, 4)}
            line["speedup"] = round(line["per_module"]["wall_ms_median"] / line["table"]["wall_ms_median"], 3)
            text = json.dumps(line)
            print(text, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(text + "\n")
        del model, pool
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
