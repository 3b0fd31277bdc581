"""developer script: the AutoAWQ -> pack-quantized repack (ct_awq_repack_batch) on a Llama-3-8B-shaped table, g128, asymmetric.

    python tools/awq_bench.py [--layers 32] [--steps 20] [--warmup 3] [--out DIR]

Prints one JSON line (and, with --out, writes it to DIR/awq_bench.json; the profiler's trace goes under DIR, else a temporary directory):
  * kernel time of one launch over the whole table, from a `rocprofv3 --kernel-trace --stats` run of its own (this script
    re-run as a child under the profiler with --kernel-only), and the rate over the algorithmic bytes
    2 * (K*N/2 + G*N*(2 + 1/2)) per module;
  * event time of the same launch (profiler off);
  * the end-to-end convert_checkpoint rate on tmpfs (/dev/shm) over a few layers, max_workers 1 and 4;
  * where the reference sources import, the reference converter's host time on 16 threads for one layer (the CPU baseline).
The table of all 32 layers moves 7.2 GB per launch, 28x the 256 MiB Infinity Cache: every launch streams from HBM."""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402

LAYER = [("self_attn.q_proj", 4096, 4096), ("self_attn.k_proj", 4096, 1024), ("self_attn.v_proj", 4096, 1024),
         ("self_attn.o_proj", 4096, 4096), ("mlp.gate_proj", 4096, 14336), ("mlp.up_proj", 4096, 14336), ("mlp.down_proj", 14336, 4096)]
GROUP = 128
HBM_PEAK = 8.0e12


def algorithmic_bytes(layers):
    return layers * sum(2 * (K * N // 2 + (K // GROUP) * N * 2.5) for _, K, N in LAYER)


def table(layers, dev):
    """device tensors of every module and the uploaded ct_awq_item table over them"""
    from compressed_tensors_amd import _lib
    from compressed_tensors_amd.codec import _upload_table
    import array

    gen = torch.Generator(device=dev).manual_seed(0)
    keep, items = [], []
    for _ in range(layers):
        for _, K, N in LAYER:
            G = K // GROUP
            qw = torch.randint(-2 ** 31, 2 ** 31 - 1, (K, N // 8), generator=gen, dtype=torch.int32, device=dev)
            qz = torch.randint(-2 ** 31, 2 ** 31 - 1, (G, N // 8), generator=gen, dtype=torch.int32, device=dev)
            sc = torch.rand(G, N, generator=gen, device=dev).to(torch.float16)
            wp = torch.empty(N, K // 8, dtype=torch.int32, device=dev)
            zp = torch.empty(N // 8, G, dtype=torch.int32, device=dev)
            st = torch.empty(N, G, dtype=torch.float16, device=dev)
            keep += [qw, qz, sc, wp, zp, st]
            it = _lib.AwqItem()
            it.qweight, it.qzeros, it.scales = qw.data_ptr(), qz.data_ptr(), sc.data_ptr()
            it.weight_packed, it.zp_packed, it.scale_t = wp.data_ptr(), zp.data_ptr(), st.data_ptr()
            it.K, it.N, it.G, it.scale_dt = K, N, G, _lib.F16
            it.scale_shape[0], it.scale_shape[1] = G, N
            it.zp_shape[0], it.zp_shape[1] = G, N // 8
            items.append(it)
    host = (_lib.AwqItem * len(items))(*items)
    blocks = int(_lib.load().ct_awq_repack_plan(ctypes.cast(host, ctypes.c_void_p), len(items)))
    if blocks < 0:
        raise RuntimeError(_lib.last_error())
    dtable = _upload_table(array.array("q", bytes(host)), dev)
    torch.cuda.synchronize(dev)
    return keep + [dtable], dtable, len(items), blocks


def launches(layers, steps, warmup):
    from compressed_tensors_amd import _lib

    dev = torch.device("cuda:0")
    keep, dtable, n, blocks = table(layers, dev)
    lib = _lib.load()
    s = _lib.stream_on(dev)

    def go():
        _lib.check(lib.ct_awq_repack_batch(dtable.data_ptr(), n, blocks, s))

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
    del keep
    return sorted(ts), n, blocks


def kernel_time(args, out_dir):
    """median duration of awq_repack_batch_kernel under rocprofv3 --kernel-trace --stats (a child process of its own)"""
    out = os.path.join(out_dir, "rocprof_awq")
    shutil.rmtree(out, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "awq", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--kernel-only", "--layers", str(args.layers), "--steps", str(args.steps),
           "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"rocprofv3 failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        raise RuntimeError(f"no kernel trace under {out}")
    durs = []
    with open(traces[0]) as f:
        for row in csv.DictReader(f):
            if "awq_repack_batch_kernel" in row.get("Kernel_Name", ""):
                durs.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9)
    durs = sorted(durs[args.warmup:])
    return durs


def convert_rate(layers, workers):
    """convert_checkpoint on tmpfs: an AutoAWQ checkpoint of `layers` layers, one shard per layer"""
    from safetensors.torch import save_file

    from compressed_tensors_amd.entrypoints.convert import AutoAWQConverter, convert_checkpoint

    import tempfile

    root = tempfile.mkdtemp(prefix="ct_awq_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    src = os.path.join(root, "src")
    os.makedirs(src)
    with open(os.path.join(src, "config.json"), "w") as f:
        json.dump({"quantization_config": {"quant_method": "awq", "bits": 4, "group_size": GROUP, "zero_point": True, "version": "gemm"}}, f)
    gen = torch.Generator().manual_seed(1)
    wm, in_bytes = {}, 0
    for layer in range(layers):
        fn = f"model-{layer + 1:05d}-of-{layers:05d}.safetensors"
        t = {}
        for name, K, N in LAYER:
            m = f"model.layers.{layer}.{name}"
            t[f"{m}.qweight"] = torch.randint(-2 ** 31, 2 ** 31 - 1, (K, N // 8), generator=gen, dtype=torch.int32)
            t[f"{m}.qzeros"] = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // GROUP, N // 8), generator=gen, dtype=torch.int32)
            t[f"{m}.scales"] = torch.rand(K // GROUP, N, generator=gen).to(torch.float16)
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
            convert_checkpoint(src, dst, AutoAWQConverter.from_pretrained(src), max_workers=w)
            dt = time.perf_counter() - t0
            shutil.rmtree(dst)
            best = dt if best is None else min(best, dt)
        res[f"workers_{w}"] = {"seconds_best_of_3": best, "input_GB_per_s": in_bytes / best / 1e9}
    shutil.rmtree(root, ignore_errors=True)
    return in_bytes, res


def reference_cpu(threads=16):
    import ref_import

    if not ref_import.available():
        return {"skipped": "no reference sources"}
    try:
        ref_import.import_reference()
        from compressed_tensors.entrypoints.convert import AutoAWQConverter as Ref
    except ImportError as e:
        return {"skipped": f"the reference converter does not import: {e}"}
    torch.set_num_threads(threads)
    gen = torch.Generator().manual_seed(2)
    t = {}
    for name, K, N in LAYER:
        m = f"model.layers.0.{name}"
        t[f"{m}.qweight"] = torch.randint(-2 ** 31, 2 ** 31 - 1, (K, N // 8), generator=gen, dtype=torch.int32)
        t[f"{m}.qzeros"] = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // GROUP, N // 8), generator=gen, dtype=torch.int32)
        t[f"{m}.scales"] = torch.rand(K // GROUP, N, generator=gen).to(torch.float16)
    t0 = time.perf_counter()
    Ref().process(t)
    dt = time.perf_counter() - t0
    return {"threads": threads, "one_layer_seconds": dt, "algorithmic_GB_per_s": algorithmic_bytes(1) / dt / 1e9}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layers", type=int, default=32)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--convert-layers", type=int, default=4)
    p.add_argument("--out", default=None, help="directory for awq_bench.json and the profiler's trace")
    p.add_argument("--kernel-only", action="store_true", help="launches only (the child run under rocprofv3)")
    args = p.parse_args()
    if args.kernel_only:
        launches(args.layers, args.steps, args.warmup)
        return
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    nbytes = algorithmic_bytes(args.layers)
    ev, n, blocks = launches(args.layers, args.steps, args.warmup)
    torch.cuda.empty_cache()
    if args.out:
        kt = kernel_time(args, args.out)
    else:
        import tempfile

        with tempfile.TemporaryDirectory(prefix="awq_bench_") as tmp:
            kt = kernel_time(args, tmp)
    med = kt[len(kt) // 2]
    in_bytes, conv = convert_rate(args.convert_layers, (1, 4))
    res = {"layers": args.layers, "modules": n, "workgroups": blocks, "algorithmic_bytes": nbytes,
           "kernel_s_median": med, "kernel_s_min": kt[0], "kernel_s_max": kt[-1], "kernel_samples": len(kt),
           "kernel_TB_per_s": nbytes / med / 1e12, "share_of_hbm_peak": nbytes / med / HBM_PEAK,
           "event_s_median": ev[len(ev) // 2], "convert_checkpoint_tmpfs": {"layers": args.convert_layers, "input_bytes": in_bytes, **conv},
           "reference_cpu": reference_cpu()}
    line = json.dumps(res)
    if args.out:
        with open(os.path.join(args.out, "awq_bench.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
