"""developer script: FP8 block-quantized weights to MXFP4, the fused launch (ct_fp8block_mxfp4_batch) against the composition it replaces (one
ct_fp8block_dequant_batch launch into a dense bfloat16 buffer, one ct_rtn_mxfp4_quant_pack_batch launch over it), on the two whole tables of
tools/fp8block_bench.py: DeepSeek-V3.2-shaped layers (62 modules) and a Qwen3-4B-shaped model (252 modules); 128 x 128 blocks, float32 scales.

    python tools/fp8block_mxfp4_bench.py [--steps 10] [--warmup 2] [--run N] [--out FILE.jsonl]

Per table, event times (profiler off) of the two forms ALTERNATED on the same buffers, launch by launch: medians, minima and maxima.  HBM-cold by
construction: one launch of either form streams the whole table (the script refuses a table of less than 512 MiB of codes, twice the 256 MiB
Infinity Cache), so nothing a launch reads or writes is left in a cache when the next one starts.  Rates are over the algorithmic bytes of the
fused form, 1 + 0.5 + 1/32 per element plus 4 per scale, against the 8 TB/s HBM peak.  The outputs of the two forms are compared byte for byte first.
Also the end-to-end convert_checkpoint time on tmpfs over a few Qwen3-4B-shaped layers, max_workers 1 and 4: FP8BlockToMXFP4Converter (fused and
composed) against the two-step conversion (FP8BlockDequantizer to a dense checkpoint, then MXFP4Quantizer over it).
Prints one JSON line and, with --out, appends it to FILE.  `--run` tags the line: the dispatch rule reads two separate runs."""
import argparse
import array
import ctypes
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from fp8block_bench import BLOCK, HBM_PEAK, QWEN3_4B_LAYER, nblocks, shapes  # noqa: E402

COLD_BYTES = 2 * (256 << 20)


def fused_bytes(shp):
    return sum(R * C + R * C // 2 + R * C // 32 + nblocks(R) * nblocks(C) * 4 for _, R, C in shp)


def composed_bytes(shp):
    return sum(R * C * 3 + nblocks(R) * nblocks(C) * 4 + R * C * 2 + R * C // 2 + R * C // 32 for _, R, C in shp)


def _upload(items, item_type, plan, dev):
    from compressed_tensors_amd import _lib
    from compressed_tensors_amd.codec import _upload_table

    host = (item_type * len(items))(*items)
    blocks = int(plan(ctypes.cast(host, ctypes.c_void_p), len(items)))
    if blocks < 0:
        raise RuntimeError(_lib.last_error())
    return _upload_table(array.array("q", bytes(host)), dev), blocks


def tables(shp, dev):
    """device tensors of every module and the three uploaded tables over them: fused, dequantize, one-pass MXFP4"""
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    keep, fused, deq, mx = [], [], [], []
    for _, R, C in shp:
        w = torch.randint(0, 256, (R, C), generator=gen, dtype=torch.int32, device=dev).to(torch.uint8)
        s = torch.rand(nblocks(R), nblocks(C), generator=gen, device=dev) * 1e-3 + 1e-5
        dense = torch.empty(R, C, dtype=torch.bfloat16, device=dev)
        outs = [(torch.empty(R, C // 2, dtype=torch.uint8, device=dev), torch.empty(R, C // 32, dtype=torch.uint8, device=dev)) for _ in range(2)]
        keep += [w, s, dense, outs]
        for it in (_lib.Fp8BlockMxItem(), _lib.Fp8BlockItem()):
            it.w, it.scale = w.data_ptr(), s.data_ptr()
            it.rows, it.cols, it.block_h, it.block_w = R, C, BLOCK, BLOCK
            it.scale_shape[0], it.scale_shape[1] = s.shape
            it.sdt = _lib.F32
            (fused if isinstance(it, _lib.Fp8BlockMxItem) else deq).append(it)
        fused[-1].packed, fused[-1].e8m0 = outs[0][0].data_ptr(), outs[0][1].data_ptr()
        deq[-1].out = dense.data_ptr()
        row = _lib.W4Item()
        row.src, row.rows, row.cols, row.group = dense.data_ptr(), R, C, 32
        row.dst, row.zp_packed = outs[1][0].data_ptr(), outs[1][1].data_ptr()
        mx.append(row)
    up = [_upload(fused, _lib.Fp8BlockMxItem, lib.ct_fp8block_mxfp4_plan, dev), _upload(deq, _lib.Fp8BlockItem, lib.ct_fp8block_dequant_plan, dev),
          _upload(mx, _lib.W4Item, lib.ct_rtn_mxfp4_batch_plan, dev)]
    torch.cuda.synchronize(dev)
    return keep, up, len(shp)


def alternated(forms, steps, warmup, dev):
    """{name: sorted event times}: the forms take turns, launch by launch"""
    for _ in range(warmup):
        for go in forms.values():
            go()
    torch.cuda.synchronize(dev)
    ts = {name: [] for name in forms}
    for _ in range(steps):
        for name, go in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            go()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b) * 1e-3)
    return {name: sorted(v) for name, v in ts.items()}


def launches(name, args):
    from compressed_tensors_amd import _lib

    dev = torch.device("cuda:0")
    shp = shapes(name, args)
    codes = sum(R * C for _, R, C in shp)
    if codes < COLD_BYTES:
        raise SystemExit(f"{name}: {codes} bytes of codes are less than twice the Infinity Cache; the launches would not be HBM-cold")
    keep, ((ft, fb), (dt, db), (mt, mb)), n = tables(shp, dev)
    lib, s = _lib.load(), _lib.stream_on(dev)

    def fused():
        _lib.check(lib.ct_fp8block_mxfp4_batch(ft.data_ptr(), n, fb, _lib.BF16, s))

    def composed():
        _lib.check(lib.ct_fp8block_dequant_batch(dt.data_ptr(), n, db, _lib.BF16, s))
        _lib.check(lib.ct_rtn_mxfp4_quant_pack_batch(mt.data_ptr(), n, mb, _lib.BF16, s))

    fused()
    composed()
    torch.cuda.synchronize(dev)
    for i in range(n):  # faster and different is not faster
        (p0, e0), (p1, e1) = keep[4 * i + 3]
        if not (torch.equal(p0, p1) and torch.equal(e0, e1)):
            raise SystemExit(f"{name}: module {i} of the fused launch differs from the composition")
    ts = alternated({"fused": fused, "composed": composed}, args.steps, args.warmup, dev)
    del keep
    torch.cuda.empty_cache()
    f, c = ts["fused"], ts["composed"]
    nbytes = fused_bytes(shp)
    med = f[len(f) // 2]
    return {"modules": n, "elements": codes, "fused_algorithmic_bytes": nbytes, "composed_algorithmic_bytes": composed_bytes(shp), "samples": len(f),
            "fused_s_median": med, "fused_s_min": f[0], "fused_s_max": f[-1],
            "composed_s_median": c[len(c) // 2], "composed_s_min": c[0], "composed_s_max": c[-1],
            "fused_TB_per_s": nbytes / med / 1e12, "fused_share_of_hbm_peak": nbytes / med / HBM_PEAK,
            "composed_over_fused_medians": c[len(c) // 2] / med, "fused_median_below_composed_min": med < c[0]}


def convert_times(layers, workers):
    """convert_checkpoint on tmpfs over `layers` Qwen3-4B-shaped layers, one shard per layer: the fused converter, the composed one, the two steps"""
    import tempfile

    from safetensors.torch import save_file

    from compressed_tensors_amd.entrypoints.convert import FP8BlockDequantizer, FP8BlockToMXFP4Converter, MXFP4Quantizer, convert_checkpoint

    root = tempfile.mkdtemp(prefix="ct_fp8block_mxfp4_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    src = os.path.join(root, "src")
    os.makedirs(src)
    with open(os.path.join(src, "config.json"), "w") as f:
        json.dump({"quantization_config": {"quant_method": "fp8", "weight_block_size": [BLOCK, BLOCK]}}, f)
    gen = torch.Generator().manual_seed(1)
    wm, in_bytes = {}, 0
    for layer in range(layers):
        fn = f"model-{layer + 1:05d}-of-{layers:05d}.safetensors"
        t = {}
        for name, R, C in QWEN3_4B_LAYER:
            m = f"model.layers.{layer}.{name}"
            t[f"{m}.weight"] = torch.randint(0, 256, (R, C), generator=gen, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn)
            t[f"{m}.weight_scale_inv"] = torch.rand(nblocks(R), nblocks(C), generator=gen) * 1e-3
        save_file(t, os.path.join(src, fn))
        wm.update(dict.fromkeys(t, fn))
        in_bytes += sum(v.numel() * v.element_size() for v in t.values())
    with open(os.path.join(src, "model.safetensors.index.json"), "w") as f:
        json.dump({"metadata": {"total_size": in_bytes}, "weight_map": wm}, f)
    targets = ["re:.*proj$"]

    def one(fused, w, dst):
        convert_checkpoint(src, dst, FP8BlockToMXFP4Converter(targets=targets, fused=fused), max_workers=w)

    def two_steps(w, dst):
        convert_checkpoint(src, dst + "_dense", FP8BlockDequantizer(targets=targets), max_workers=w)
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
    p.add_argument("--layers", type=int, default=2, help="DeepSeek-shaped layers")
    p.add_argument("--experts", type=int, default=8, help="routed experts per DeepSeek-shaped layer")
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--convert-layers", type=int, default=4)
    p.add_argument("--run", type=int, default=1, help="tag of this run in its JSON line")
    p.add_argument("--out", default=None, help="a .jsonl file the line is appended to")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fp8block_mxfp4_bench needs an MI355X: nothing here is measured on a CPU")
    res = {"bench": "fp8block_mxfp4", "run": args.run, "steps": args.steps, "warmup": args.warmup}
    for name in ("deepseek", "qwen3_4b"):
        res[name] = launches(name, args)
    in_bytes, conv = convert_times(args.convert_layers, (1, 4))
    res["convert_checkpoint_tmpfs_end_to_end"] = {"layers": args.convert_layers, "input_bytes": in_bytes, **conv}
    res["fused_median_below_composed_min_on_both_tables"] = all(res[t]["fused_median_below_composed_min"] for t in ("deepseek", "qwen3_4b"))
    line = json.dumps(res)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
