"""developer script: the FP8 block dequantize (ct_fp8block_dequant_batch) on two whole tables, 128 x 128 blocks, float32
weight_scale_inv, bfloat16 out.

    python tools/fp8block_bench.py [--steps 10] [--warmup 2] [--out DIR]

Tables:
  * deepseek: DeepSeek-V3.2-shaped layers (MLA attention, the indexer's wq_b / wk, `--experts` routed experts of 2048 x 7168 /
    7168 x 2048 per layer), `--layers` of them: several GB per launch, far beyond the 256 MiB Infinity Cache;
  * qwen3_4b: a Qwen3-4B-shaped whole model (36 layers: q 4096 x 2560, k / v 1024 x 2560, o 2560 x 4096, gate / up 9728 x 2560,
    down 2560 x 9728).
Prints one JSON line (and, with --out, writes it to DIR/fp8block_bench.json; the profiler's trace goes under DIR, else a temporary
directory).  Per table:
  * kernel time of one launch over the whole table, from a `rocprofv3 --kernel-trace --stats` run of its own (this script re-run
    as a child under the profiler with --kernel-only), and the rate over the algorithmic bytes: 1 + 2 per element (code in,
    bfloat16 out) plus 4 per scale;
  * event time of the same launch (profiler off);
  * the nearest existing path: the same table through `ct_q8_dequant_batch`, the 8-bit tables' block strategy.  It only writes
    16-bit weights with the scale's own dtype, so it runs with bfloat16 scales: same traffic, but NOT the reference's result
    (the scale is rounded to bfloat16 first).  There is no batched float32 output to cast from.
Also the end-to-end convert_checkpoint rate on tmpfs (/dev/shm) over a few Qwen3-4B-shaped layers, max_workers 1 and 4, in GB/s of
input: host-bound (safetensors reads and writes), not a kernel figure."""
import argparse
import array
import csv
import ctypes
import glob
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12
BLOCK = 128


def deepseek_layer(experts):
    mods = [("self_attn.q_a_proj", 1536, 7168), ("self_attn.q_b_proj", 24576, 1536), ("self_attn.kv_a_proj_with_mqa", 576, 7168),
            ("self_attn.kv_b_proj", 32768, 512), ("self_attn.o_proj", 7168, 16384), ("self_attn.indexer.wq_b", 8192, 1536),
            ("self_attn.indexer.wk", 128, 7168)]
    for e in range(experts):
        mods += [(f"mlp.experts.{e}.gate_proj", 2048, 7168), (f"mlp.experts.{e}.up_proj", 2048, 7168), (f"mlp.experts.{e}.down_proj", 7168, 2048)]
    return mods


QWEN3_4B_LAYER = [("self_attn.q_proj", 4096, 2560), ("self_attn.k_proj", 1024, 2560), ("self_attn.v_proj", 1024, 2560),
                  ("self_attn.o_proj", 2560, 4096), ("mlp.gate_proj", 9728, 2560), ("mlp.up_proj", 9728, 2560), ("mlp.down_proj", 2560, 9728)]


def shapes(name, args):
    if name == "deepseek":
        return [s for _ in range(args.layers) for s in deepseek_layer(args.experts)]
    return [s for _ in range(36) for s in QWEN3_4B_LAYER]


def nblocks(n):
    return -(-n // BLOCK)


def algorithmic_bytes(shp):
    return sum(R * C * 3 + nblocks(R) * nblocks(C) * 4 for _, R, C in shp)


def tables(shp, dev):
    """device tensors of every module, the uploaded ct_fp8block_item table over them, and a ct_q8_dequant_batch table (W4Batch) over
    the same codes with bfloat16 scales"""
    from compressed_tensors_amd import _lib
    from compressed_tensors_amd.codec import W4Batch, _upload_table

    gen = torch.Generator(device=dev).manual_seed(0)
    keep, items, q8 = [], [], []
    for _, R, C in shp:
        w = torch.randint(0, 256, (R, C), generator=gen, dtype=torch.int32, device=dev).to(torch.uint8)
        s = torch.rand(nblocks(R), nblocks(C), generator=gen, device=dev) * 1e-3 + 1e-5
        out = torch.empty(R, C, dtype=torch.bfloat16, device=dev)
        s16 = s.to(torch.bfloat16)
        keep += [w, s, out, s16]
        it = _lib.Fp8BlockItem()
        it.w, it.scale, it.out = w.data_ptr(), s.data_ptr(), out.data_ptr()
        it.rows, it.cols, it.block_h, it.block_w = R, C, BLOCK, BLOCK
        it.scale_shape[0], it.scale_shape[1] = s.shape
        it.sdt = _lib.F32
        items.append(it)
        q8.append((w.view(torch.float8_e4m3fn), s16, None, out, R, C, -((BLOCK << 24) | BLOCK)))
    host = (_lib.Fp8BlockItem * len(items))(*items)
    blocks = int(_lib.load().ct_fp8block_dequant_plan(ctypes.cast(host, ctypes.c_void_p), len(items)))
    if blocks < 0:
        raise RuntimeError(_lib.last_error())
    dtable = _upload_table(array.array("q", bytes(host)), dev)
    base = W4Batch(q8, "decompress", torch.bfloat16, kind="fp8")
    torch.cuda.synchronize(dev)
    return keep + [dtable], dtable, len(items), blocks, base


def timed(go, steps, warmup, dev):
    for _ in range(warmup):
        go()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        go()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return sorted(ts)


def launches(name, args):
    """event times of the new launch and of the q8 baseline (both run once per step; the profiler child records both kernels)"""
    from compressed_tensors_amd import _lib

    dev = torch.device("cuda:0")
    keep, dtable, n, blocks, base = tables(shapes(name, args), dev)
    lib = _lib.load()
    s = _lib.stream_on(dev)

    def go():
        _lib.check(lib.ct_fp8block_dequant_batch(dtable.data_ptr(), n, blocks, _lib.BF16, s))

    ev = timed(go, args.steps, args.warmup, dev)
    ev_base = timed(base.launch, args.steps, args.warmup, dev)
    del keep, base
    torch.cuda.empty_cache()
    return ev, ev_base, n, blocks


def kernel_times(name, args, out_dir):
    """durations of fp8block_dequant_kernel and q8_dequant_batch_kernel under rocprofv3 --kernel-trace --stats (a child process)"""
    out = os.path.join(out_dir, f"rocprof_fp8block_{name}")
    shutil.rmtree(out, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "fp8block", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--kernel-only", name, "--layers", str(args.layers), "--experts", str(args.experts),
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"rocprofv3 failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        raise RuntimeError(f"no kernel trace under {out}")
    durs = {"fp8block": [], "q8": []}
    with open(traces[0]) as f:
        for row in csv.DictReader(f):
            k = row.get("Kernel_Name", "")
            key = "fp8block" if "fp8block_dequant_kernel" in k else "q8" if "q8_dequant_batch_kernel" in k else None
            if key:
                durs[key].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9)
    return {k: sorted(v[args.warmup:]) for k, v in durs.items()}


def convert_rate(layers, workers):
    """convert_checkpoint on tmpfs: an FP8-block checkpoint of `layers` Qwen3-4B-shaped layers, one shard per layer"""
    import tempfile

    from safetensors.torch import save_file

    from compressed_tensors_amd.entrypoints.convert import FP8BlockDequantizer, convert_checkpoint

    root = tempfile.mkdtemp(prefix="ct_fp8block_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
    res = {}
    for w in workers:
        best = None
        for rep in range(3):
            dst = os.path.join(root, f"dst{w}_{rep}")
            t0 = time.perf_counter()
            convert_checkpoint(src, dst, FP8BlockDequantizer(targets=["re:.*proj$"]), max_workers=w)
            dt = time.perf_counter() - t0
            shutil.rmtree(dst)
            best = dt if best is None else min(best, dt)
        res[f"workers_{w}"] = {"seconds_best_of_3": best, "input_GB_per_s": in_bytes / best / 1e9}
    shutil.rmtree(root, ignore_errors=True)
    return in_bytes, res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layers", type=int, default=2, help="DeepSeek-shaped layers")
    p.add_argument("--experts", type=int, default=8, help="routed experts per DeepSeek-shaped layer")
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--convert-layers", type=int, default=4)
    p.add_argument("--out", default=None, help="directory for fp8block_bench.json and the profiler's traces")
    p.add_argument("--kernel-only", default=None, help="launches of one table only (the child run under rocprofv3)")
    args = p.parse_args()
    if args.kernel_only:
        launches(args.kernel_only, args)
        return
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    import tempfile

    prof_dir = args.out or tempfile.mkdtemp(prefix="fp8block_bench_")
    res = {}
    for name in ("deepseek", "qwen3_4b"):
        shp = shapes(name, args)
        nbytes = algorithmic_bytes(shp)
        ev, ev_base, n, blocks = launches(name, args)
        kt = kernel_times(name, args, prof_dir)
        k, q = kt["fp8block"], kt["q8"]
        med = k[len(k) // 2]
        res[name] = {"modules": n, "workgroups": blocks, "algorithmic_bytes": nbytes,
                     "kernel_s_median": med, "kernel_s_min": k[0], "kernel_s_max": k[-1], "kernel_samples": len(k),
                     "kernel_TB_per_s": nbytes / med / 1e12, "share_of_hbm_peak": nbytes / med / HBM_PEAK,
                     "event_s_median": ev[len(ev) // 2],
                     "q8_bf16_scale_baseline": {"kernel_s_median": q[len(q) // 2] if q else None,
                                                "share_of_hbm_peak": (nbytes / q[len(q) // 2] / HBM_PEAK) if q else None,
                                                "event_s_median": ev_base[len(ev_base) // 2]}}
    if not args.out:
        shutil.rmtree(prof_dir, ignore_errors=True)
    in_bytes, conv = convert_rate(args.convert_layers, (1, 4))
    res["convert_checkpoint_tmpfs_end_to_end"] = {"layers": args.convert_layers, "input_bytes": in_bytes, **conv}
    line = json.dumps(res)
    if args.out:
        with open(os.path.join(args.out, "fp8block_bench.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
