"""developer script: NVFP4 weights to MXFP4, the fused launch (ct_nvfp4_mxfp4_batch) against the composition it replaces (one
ct_fp4_unpack_dequant_batch launch into dense bfloat16 buffers, one ct_rtn_mxfp4_quant_pack_batch launch over them), on two whole tables: a
Llama-3-8B-shaped tree (tools/rtn_bench.py: 32 layers, 224 modules) and a Qwen3-4B-shaped model (tools/fp8block_bench.py: 36 layers, 252 modules).

    python tools/nvfp4_mxfp4_bench.py [--steps 10] [--warmup 2] [--run N] [--out FILE.jsonl]

Per table, event times (profiler off) of the two forms ALTERNATED on the same buffers, launch by launch: medians, minima and maxima.  HBM-cold by
construction: one launch of either form streams the whole table (the script refuses a table of less than 512 MiB of nibbles, twice the 256 MiB
Infinity Cache), so nothing a launch reads or writes is left in a cache when the next one starts.  Rates are over the algorithmic bytes of the
fused form, 0.5 + 1/16 in and 0.5 + 1/32 out per element, against the 8 TB/s HBM peak.  The outputs of the two forms are compared byte for byte first.
Also the end-to-end convert_checkpoint time on tmpfs over a few Qwen3-4B-shaped layers, max_workers 1 and 4: NVFP4ToMXFP4Converter (fused and
composed) against the two-step conversion (CompressedTensorsDequantizer to a dense checkpoint, then MXFP4Quantizer over it).
Prints one JSON line and, with --out, appends it to FILE.  `--run` tags the line: the dispatch rule reads two separate runs."""
import argparse
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from fp8block_bench import HBM_PEAK, QWEN3_4B_LAYER  # noqa: E402
from fp8block_mxfp4_bench import COLD_BYTES, _upload, alternated  # noqa: E402
from rtn_bench import L8B  # noqa: E402

TABLES = {"llama_8b": [(f"l{layer}.m{i}", R, C) for layer in range(32) for i, (R, C) in enumerate(L8B)],
          "qwen3_4b": [(f"l{layer}.{name}", R, C) for layer in range(36) for name, R, C in QWEN3_4B_LAYER]}
F8 = torch.float8_e4m3fn


def fused_bytes(shp):
    return sum(R * C // 2 + R * C // 16 + 4 + R * C // 2 + R * C // 32 for _, R, C in shp)


def composed_bytes(shp):
    return sum(R * C // 2 + R * C // 16 + 4 + 2 * R * C + R * C // 8 + 2 * R * C + R * C // 2 + R * C // 32 for _, R, C in shp)


def random_nvfp4(R, C, gen, dev="cpu"):
    """(weight_packed, weight_scale, weight_global_scale) of random nibbles under positive finite scales"""
    packed = torch.randint(0, 256, (R, C // 2), generator=gen, dtype=torch.int32, device=dev).to(torch.uint8)
    scale = torch.randint(0x08, 0x7F, (R, C // 16), generator=gen, dtype=torch.int32, device=dev).to(torch.uint8).view(F8)
    return packed, scale, torch.full((1,), 2688.0 * (1.0 + (R * 31 + C) % 7 / 8.0), dtype=torch.float32, device=dev)


def tables(shp, dev):
    """device tensors of every module and the three uploaded tables over them: fused, NVFP4 decompress, one-pass MXFP4"""
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    keep, outs, fused, deq, mx = [], [], [], [], []
    for _, R, C in shp:
        p, s, g = random_nvfp4(R, C, gen, dev)
        dense, scale_bf16 = torch.empty(R, C, dtype=torch.bfloat16, device=dev), torch.empty(R, C // 16, dtype=torch.bfloat16, device=dev)
        pair = [(torch.empty(R, C // 2, dtype=torch.uint8, device=dev), torch.empty(R, C // 32, dtype=torch.uint8, device=dev)) for _ in range(2)]
        keep += [p, s, g, dense, scale_bf16]
        outs.append(pair)
        it = _lib.Nvfp4MxItem()
        it.packed_in, it.scale_f8, it.global_scale, it.rows, it.cols = p.data_ptr(), s.data_ptr(), g.data_ptr(), R, C
        it.packed_out, it.e8m0 = pair[0][0].data_ptr(), pair[0][1].data_ptr()
        fused.append(it)
        row = _lib.W4Item()
        row.src, row.scale, row.zp, row.dst, row.zp_packed = p.data_ptr(), s.data_ptr(), g.data_ptr(), dense.data_ptr(), scale_bf16.data_ptr()
        row.rows, row.cols, row.group = R, C, 16
        deq.append(row)
        row = _lib.W4Item()
        row.src, row.rows, row.cols, row.group = dense.data_ptr(), R, C, 32
        row.dst, row.zp_packed = pair[1][0].data_ptr(), pair[1][1].data_ptr()
        mx.append(row)
    up = [_upload(fused, _lib.Nvfp4MxItem, lib.ct_nvfp4_mxfp4_plan, dev), _upload(deq, _lib.W4Item, lambda t, n: lib.ct_fp4_batch_plan(t, n, 1), dev),
          _upload(mx, _lib.W4Item, lib.ct_rtn_mxfp4_batch_plan, dev)]
    torch.cuda.synchronize(dev)
    return keep, outs, up, len(shp)


def launches(name, args):
    from compressed_tensors_amd import _lib

    dev = torch.device("cuda:0")
    shp = TABLES[name]
    elements = sum(R * C for _, R, C in shp)
    if elements // 2 < COLD_BYTES:
        raise SystemExit(f"{name}: {elements // 2} bytes of nibbles are less than twice the Infinity Cache; the launches would not be HBM-cold")
    keep, outs, ((ft, fb), (dt, db), (mt, mb)), n = tables(shp, dev)
    lib, s = _lib.load(), _lib.stream_on(dev)

    def fused():
        _lib.check(lib.ct_nvfp4_mxfp4_batch(ft.data_ptr(), n, fb, s))

    def composed():
        _lib.check(lib.ct_fp4_unpack_dequant_batch(dt.data_ptr(), n, db, 16, _lib.BF16, s))
        _lib.check(lib.ct_rtn_mxfp4_quant_pack_batch(mt.data_ptr(), n, mb, _lib.BF16, s))

    fused()
    composed()
    torch.cuda.synchronize(dev)
    for i, ((p0, e0), (p1, e1)) in enumerate(outs):  # faster and different is not faster
        if not (torch.equal(p0, p1) and torch.equal(e0, e1)):
            raise SystemExit(f"{name}: module {i} of the fused launch differs from the composition")
    ts = alternated({"fused": fused, "composed": composed}, args.steps, args.warmup, dev)
    del keep, outs
    torch.cuda.empty_cache()
    f, c = ts["fused"], ts["composed"]
    nbytes = fused_bytes(shp)
    med = f[len(f) // 2]
    return {"modules": n, "elements": elements, "fused_algorithmic_bytes": nbytes, "composed_algorithmic_bytes": composed_bytes(shp), "samples": len(f),
            "fused_s_median": med, "fused_s_min": f[0], "fused_s_max": f[-1],
            "composed_s_median": c[len(c) // 2], "composed_s_min": c[0], "composed_s_max": c[-1],
            "fused_TB_per_s": nbytes / med / 1e12, "fused_share_of_hbm_peak": nbytes / med / HBM_PEAK,
            "composed_over_fused_medians": c[len(c) // 2] / med, "fused_median_below_composed_min": med < c[0]}


def convert_times(layers, workers):
    """convert_checkpoint on tmpfs over `layers` Qwen3-4B-shaped layers, one shard per layer: the fused converter, the composed one, the two steps"""
    import tempfile

    from safetensors.torch import save_file

    from compressed_tensors_amd.entrypoints.convert import (CompressedTensorsDequantizer, ModelOptNvfp4Converter, MXFP4Quantizer, NVFP4ToMXFP4Converter,
                                                            convert_checkpoint)

    targets = ["re:.*proj$"]
    root = tempfile.mkdtemp(prefix="ct_nvfp4_mxfp4_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    src = os.path.join(root, "src")
    os.makedirs(src)
    with open(os.path.join(src, "config.json"), "w") as f:
        json.dump({"quantization_config": ModelOptNvfp4Converter(targets=targets).create_config().model_dump()}, f)
    gen = torch.Generator().manual_seed(1)
    wm, in_bytes = {}, 0
    for layer in range(layers):
        fn = f"model-{layer + 1:05d}-of-{layers:05d}.safetensors"
        t = {}
        for name, R, C in QWEN3_4B_LAYER:
            m = f"model.layers.{layer}.{name}"
            t[f"{m}.weight_packed"], t[f"{m}.weight_scale"], t[f"{m}.weight_global_scale"] = random_nvfp4(R, C, gen)
        save_file(t, os.path.join(src, fn))
        wm.update(dict.fromkeys(t, fn))
        in_bytes += sum(v.numel() * v.element_size() for v in t.values())
    with open(os.path.join(src, "model.safetensors.index.json"), "w") as f:
        json.dump({"metadata": {"total_size": in_bytes}, "weight_map": wm}, f)

    def one(fused, w, dst):
        convert_checkpoint(src, dst, NVFP4ToMXFP4Converter(targets=targets, fused=fused), max_workers=w)

    def two_steps(w, dst):
        convert_checkpoint(src, dst + "_dense", CompressedTensorsDequantizer(src), max_workers=w)
        convert_checkpoint(dst + "_dense", dst, MXFP4Quantizer(targets=targets), max_workers=w)

    forms = {"fused": lambda w, dst: one(True, w, dst), "composed": lambda w, dst: one(False, w, dst), "two_steps": two_steps}
    res = {}
    for w in workers:
        best = {}
        for rep in range(3):  # the forms take turns
            for name, go in forms.items():
                dst = os.path.join(root, f"dst_{name}_{w}_{rep}")
                t0 = time.perf_counter()
                go(w, dst)
                dt = time.perf_counter() - t0
                shutil.rmtree(dst)
                shutil.rmtree(dst + "_dense", ignore_errors=True)
                best[name] = min(best.get(name, dt), dt)
        res[f"workers_{w}"] = {f"{name}_s_best_of_3": t for name, t in best.items()} | {f"{name}_input_GB_per_s": in_bytes / t / 1e9 for name, t in best.items()}
    shutil.rmtree(root, ignore_errors=True)
    return in_bytes, res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--convert-layers", type=int, default=4)
    p.add_argument("--run", type=int, default=1, help="tag of this run in its JSON line")
    p.add_argument("--out", default=None, help="a .jsonl file the line is appended to")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nvfp4_mxfp4_bench needs an MI355X: nothing here is measured on a CPU")
    res = {"bench": "nvfp4_mxfp4", "run": args.run, "steps": args.steps, "warmup": args.warmup}
    for name in TABLES:
        res[name] = launches(name, args)
    in_bytes, conv = convert_times(args.convert_layers, (1, 4))
    res["convert_checkpoint_tmpfs_end_to_end"] = {"layers": args.convert_layers, "input_bytes": in_bytes, **conv}
    res["fused_median_below_composed_min_on_both_tables"] = all(res[t]["fused_median_below_composed_min"] for t in TABLES)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
