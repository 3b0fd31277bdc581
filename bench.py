#!/usr/bin/env python3
"""bench.py — throughput of the compress/decompress hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A "step" is one pass of the hot path over one batch of synthetic input: W4A16 pack-quantized
(int4, group 128, symmetric) COMPRESS of one 8192x8192 bf16 weight plus DECOMPRESS of one
8192x8192 packed weight (BASELINE.json configs[1]), through the C ABI of libct_hip.so with all
inputs resident in HBM.  Buffers rotate over 16 disjoint sets (4.8 GiB; even the smallest stream,
the packed words, is 537 MB across the sets) so the 256 MiB Infinity Cache cannot serve re-reads:
numbers are HBM-cold.  The timed loop issues the step's two independent launches on two HIP streams
(`value`); with --full the same loop on one stream is reported as `value_one_stream`, and the per-kernel
roofline figures are single-stream HIP-event timings of back-to-back launches.

Protocol (round 3): 250 ms of the real launches before any timed region (independent of
--warmup: a fresh lease measures ~5 % low for its first milliseconds), then --warmup steps, then ONE timed region of
EXACTLY --steps steps, bracketed by barrier + torch.cuda.synchronize() and max-reduced over the ranks;
`ms_per_step` is that region's wall time / --steps.

A plain run does only that: it sets up, warms up, times the steps, writes --dump-outputs and prints the result line.
--full runs everything else too.  Before the headline's region: the same region on one stream, and once more without the
device warm-up (roofline.step).  After it: the per-kernel roofline timings, the parity gate, the extra legs (other sizes,
dtypes, formats and checkpoints; every leg's kernel row is appended to roofline.kernels[]), the multi-rank legs, the CPU
baseline and the oracle slice check.  The full result goes to bench_details.json and to stderr.
--no-extra, --no-cpu-baseline and --shard rows take effect under --full only.

--dump-outputs DIR: after the timed steps, what the last timed step computed (the packed words of its compress and the bf16
weight of its decompress) is written to DIR as .npy files, a fixed sample of rows (see dump_outputs); the inputs are
seeded, so two builds given the same arguments can be compared output for output.

value = algorithmic bytes of all ranks / max-over-ranks wall time, in GB/s; algorithmic bytes
per step = 2 x (2 N^2 + 2 N^2/128 + N^2/2) = 337,641,472 B at N = 8192.
Multi-GPU (--gpus N): under torch.distributed.run one process per GPU, as the driver launches it; without a launcher
(`python bench.py --gpus N`) the script starts its N ranks itself.  Every rank processes its own weight shard, no collective
on the data path (weak scaling); only the timing uses a barrier and a MAX.  `config.ranks_seen` is the process group's size
and `config.per_rank_GBps` what each rank did on its own.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

N = 8192
GROUP = 128
BITS = 4
NSETS = 16  # read footprint per direction >= 2x the 256 MiB Infinity Cache (packed: 16 x 33.5 MB)
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)


def alg_bytes_one_direction(n=N, gs=GROUP, bits=BITS):
    return 2 * n * n + 2 * n * (n // gs) + n * n * bits // 8


def make_sets(dev, rank):
    from compressed_tensors_amd import codec

    g = torch.Generator(device=dev).manual_seed(1000 + rank)
    sets = []
    for _ in range(NSETS):
        w = torch.randn(N, N, dtype=torch.bfloat16, device=dev, generator=g)
        scale, zp = codec.minmax_qparams(w, num_bits=BITS, group_size=GROUP, symmetric=True)
        packed = torch.empty(N, N // 8, dtype=torch.int32, device=dev)
        out = torch.empty(N, N, dtype=torch.bfloat16, device=dev)
        sets.append(dict(w=w, scale=scale, zp=zp, packed=packed, out=out))
    return sets


def make_launchers(sets, stream, stream_d=None):
    """direct C-ABI launches with precomputed arguments (what a C host would do); compress goes to
    `stream`, decompress to `stream_d` (default: the same stream)"""
    stream_d = stream if stream_d is None else stream_d
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    BF16 = _lib.BF16
    comp_args, decomp_args = [], []
    for s in sets:
        # symmetric scheme: the (all-zero) zero point is still added by the reference when present;
        # pass it like PackedQuantizationCompressor.compress does
        comp_args.append((s["w"].data_ptr(), BF16, s["scale"].data_ptr(), BF16, s["zp"].data_ptr(), _lib.I8,
                          N, N, 1, GROUP, N // GROUP, None, BITS, BF16, s["packed"].data_ptr(), stream))
        decomp_args.append((s["packed"].data_ptr(), N, N // 8, N, BITS, s["scale"].data_ptr(), BF16, None, -1,
                            1, GROUP, N // GROUP, None, s["out"].data_ptr(), BF16, stream_d))

    def compress(i):
        rc = lib.ct_quant_pack(*comp_args[i % NSETS])
        if rc:
            _lib.check(rc)

    def decompress(i):
        rc = lib.ct_unpack_dequant(*decomp_args[i % NSETS])
        if rc:
            _lib.check(rc)

    return compress, decompress


# CT_BENCH_WARM_SCALE (profiling runs only: tools/profile_round.sh sets 0.1 for the counter passes, whose per-kernel counters do not
# depend on clocks, so that rocprofv3 does not serialise ten thousand warm-up launches)
_WARM_SCALE = float(os.environ.get("CT_BENCH_WARM_SCALE", "1"))
WARM_MS = 250.0 * _WARM_SCALE   # fixed-DURATION device warm-up before the first timed region (independent of --warmup)
KERNEL_WARM_MS = 40.0 * _WARM_SCALE  # ... and before every per-kernel event timing
BLOCKS = 5        # timed regions are repeated BLOCKS times; the MEDIAN block is the one reported
MIN_LAUNCHES_PER_BLOCK = 60  # every per-kernel / per-call timing block holds at least this many back-to-back launches (VERDICT r03 hygiene)


def device_warmup(fns, min_ms):
    """run the REAL launches until `min_ms` of wall time has passed (clocks / power state / TLBs settle on a fresh lease:
    round 2's driver run, 5 warm-up steps = 0.3 ms of GPU activity before the timed region, measured 5-8 % below steady state)"""
    t0, i = time.perf_counter(), 0
    while True:
        for _ in range(32):
            for f in fns:
                f(i)
            i += 1
        torch.cuda.synchronize()
        if (time.perf_counter() - t0) * 1e3 >= min_ms:
            return i


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def time_kernel(fn, iters, offset=0, spread=None):
    """average launch duration (us) with HIP events on the launch stream: >= KERNEL_WARM_MS of the same launches first, then
    BLOCKS blocks of `iters` back-to-back launches; the median block is returned (min / max go to `spread` if given)"""
    iters = max(int(iters), MIN_LAUNCHES_PER_BLOCK)
    device_warmup([lambda i: fn(offset + i)], KERNEL_WARM_MS)
    per = []
    for _ in range(BLOCKS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(iters):
            fn(offset + i)
        stop.record()
        torch.cuda.synchronize()
        per.append(start.elapsed_time(stop) * 1000.0 / iters)
    if spread is not None:
        spread["min_us"], spread["max_us"], spread["blocks"], spread["launches_per_block"] = round(min(per), 2), round(max(per), 2), BLOCKS, iters
    return median(per)


def time_calls(fn, iters=MIN_LAUNCHES_PER_BLOCK, offset=0):
    """per-call WALL time (us) of a plug-in call that may wait on the device itself (e.g. BitmaskTensor.from_dense needs nnz on the
    host before it can return): KERNEL_WARM_MS of the same calls, then BLOCKS blocks of `iters` back-to-back calls between two
    synchronisations; the median block and the (min, max) are returned.  HIP events cannot time these: the host is part of the path."""
    iters = max(int(iters), MIN_LAUNCHES_PER_BLOCK)
    device_warmup([lambda i: fn(offset + i)], KERNEL_WARM_MS)
    per = []
    for _ in range(BLOCKS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(iters):
            fn(offset + i)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / iters * 1e6)
    return median(per), min(per), max(per)


def w4_kernel_point(dev, n, dtype=torch.bfloat16, symmetric=True, iters=60, actorder=False, cols=None):
    """HBM-cold per-kernel timing of the fused W4A16 g128 compress / decompress at another size, weight dtype, with an
    asymmetric scheme (int8 zero points) or with activation ordering (`weight_g_idx`: a random assignment of the columns to
    the groups; `cols`: a row length other than n, e.g. 28672 = 224 groups per row): enough rotating sets that the smallest read stream
    (the packed words) is >= 2x the 256 MiB Infinity Cache.
    Parity: decompress(compress(W)) == fake_quantize(W) on one set (for actorder: fake_quantize with the same g_idx)."""
    from compressed_tensors_amd import _lib, codec

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    dt = _lib.DT[dtype]
    c = n if cols is None else cols
    nsets = max(4, -(-(2 * 256 * 2 ** 20) // (n * c // 2)))
    g = torch.Generator(device=dev).manual_seed(31 + n)
    g_idx = cg = None
    if actorder:
        g_idx = (torch.randperm(c, device=dev, generator=g) // GROUP).to(torch.int32)
        cg = codec.QuantLayout((n, c), torch.empty(n, c // GROUP, dtype=dtype, device=dev), "group", GROUP, None, g_idx).col_group
        order = torch.argsort(g_idx)
    sets = []
    for _ in range(nsets):
        w = torch.randn(n, c, dtype=torch.float32, device=dev, generator=g).to(dtype)
        scale, zp = codec.minmax_qparams(w[:, order].contiguous() if actorder else w, num_bits=BITS, group_size=GROUP, symmetric=symmetric)
        sets.append((w, scale, zp, torch.empty(n, c // 8, dtype=torch.int32, device=dev), torch.empty(n, c, dtype=dtype, device=dev)))
    cgp = None if cg is None else cg.data_ptr()
    ca = [(w.data_ptr(), dt, sc.data_ptr(), dt, zp.data_ptr(), _lib.I8, n, c, 1, GROUP, c // GROUP, cgp, BITS, dt, pk.data_ptr(), stream)
          for (w, sc, zp, pk, out) in sets]
    da = [(pk.data_ptr(), n, c // 8, c, BITS, sc.data_ptr(), dt, None if symmetric else zp.data_ptr(), -1 if symmetric else _lib.I8,
           1, GROUP, c // GROUP, cgp, out.data_ptr(), dt, stream) for (w, sc, zp, pk, out) in sets]

    def compress(i):
        rc = lib.ct_quant_pack(*ca[i % nsets])
        if rc:
            _lib.check(rc)

    def decompress(i):
        rc = lib.ct_unpack_dequant(*da[i % nsets])
        if rc:
            _lib.check(rc)

    for i in range(nsets):
        compress(i)
    one = (2 * n * c + 2 * n * (c // GROUP) + n * c * BITS // 8) + (0 if symmetric else n * (c // GROUP)) + (4 * c if actorder else 0)  # + int8 zero points, + the group table
    us_c, us_d = time_kernel(compress, iters), time_kernel(decompress, iters, offset=nsets // 2)
    # the same launches on ONE buffer set (Infinity-Cache-warm; reported beside the cold figure, never instead of it)
    warm_c, warm_d = time_kernel(lambda i: compress(0), iters), time_kernel(lambda i: decompress(0), iters)
    w, sc, zp, pk, out = sets[0]
    ok = torch.equal(out, codec.fake_quantize_tensor(w, sc, zp, num_bits=BITS, strategy="group", group_size=GROUP, g_idx=g_idx))
    if actorder:  # the CPU oracle on a 64-row slice of set 0: packed words and decompressed rows, bit for bit
        O = _oracle()
        sl = slice(0, 64)
        sd = {"weight": w[sl].cpu(), "weight_scale": sc[sl].cpu(), "weight_zero_point": zp[sl].cpu(), "weight_g_idx": g_idx.cpu()}
        oc = O.pack_quantized_compress(sd, num_bits=BITS, strategy="group", group_size=GROUP, symmetric=symmetric)
        od = O.pack_quantized_decompress(oc, num_bits=BITS, strategy="group", symmetric=symmetric)
        ok = ok and torch.equal(pk[sl].cpu(), oc["weight_packed"]) and torch.equal(out[sl].cpu().view(torch.int16), od["weight"].view(torch.int16))
    pair = {}
    if n <= 4096 and c == n and symmetric and not actorder and nsets >= 4:
        # what a caller with q / k or gate / up PAIRS of this size has — `ct_quant_pack_batch` / `ct_unpack_dequant_batch`
        # with n = 2 (codec.quantize_and_pack_many): two tensors per launch, tables prebuilt, HBM-cold rotation over the same sets
        tabs_c, tabs_d = [], []
        for j in range(0, nsets - 1, 2):
            (w0, s0, _, p0, o0), (w1, s1, _, p1, o1) = sets[j], sets[j + 1]
            tabs_c.append(codec.W4Batch([(w0, s0, None, p0, n, n, GROUP), (w1, s1, None, p1, n, n, GROUP)], "compress", dtype))
            tabs_d.append(codec.W4Batch([(p0, s0, None, o0, n, n, GROUP), (p1, s1, None, o1, n, n, GROUP)], "decompress", dtype))
        npair = len(tabs_c)
        us_pc = time_kernel(lambda i: tabs_c[i % npair].launch(stream), iters)
        us_pd = time_kernel(lambda i: tabs_d[i % npair].launch(stream), iters, offset=npair // 2)
        ok = ok and torch.equal(sets[1][4], codec.fake_quantize_tensor(sets[1][0], sets[1][1], sets[1][2], num_bits=BITS, strategy="group", group_size=GROUP))
        pair = {"pair_batch": {"entry": "ct_quant_pack_batch / ct_unpack_dequant_batch with n = 2 (codec.quantize_and_pack_many)", "alg_bytes_per_direction": 2 * one,
                               "compress_us": round(us_pc, 2), "compress_frac_hbm": round(2 * one / us_pc / 1e3 / HBM_PEAK_GBPS, 4),
                               "decompress_us": round(us_pd, 2), "decompress_frac_hbm": round(2 * one / us_pd / 1e3 / HBM_PEAK_GBPS, 4)}}
    return {"alg_bytes_per_direction": one, "sets": nsets, **pair,
            "compress_us": round(us_c, 2), "compress_GBps": round(one / us_c / 1e3, 1), "compress_frac_hbm": round(one / us_c / 1e3 / HBM_PEAK_GBPS, 4),
            "decompress_us": round(us_d, 2), "decompress_GBps": round(one / us_d / 1e3, 1), "decompress_frac_hbm": round(one / us_d / 1e3 / HBM_PEAK_GBPS, 4),
            "compress_us_cache_warm": round(warm_c, 2), "decompress_us_cache_warm": round(warm_d, 2),
            "round_trip_equals_fake_quantize": bool(ok)}


def w4_variants_leg(dev):
    """north_star's second size (4096x4096) and the other weight dtypes / schemes of the same two kernels at 8192x8192"""
    out = {"workload": "W4A16 g128 fused compress / decompress kernels through the C ABI, HBM-cold rotation"}
    for key, kw in (("bf16_4096", dict(n=4096)), ("fp16_8192", dict(n=N, dtype=torch.float16)),
                    ("bf16_8192_asymmetric", dict(n=N, symmetric=False)), ("fp16_8192_asymmetric", dict(n=N, dtype=torch.float16, symmetric=False)),
                    ("bf16_8192_actorder", dict(n=N, actorder=True)),
                    ("bf16_4096x28672_actorder", dict(n=4096, cols=28672, actorder=True, iters=36))):  # 224 groups per row (a 70B down_proj): the 256-group tables
        out[key] = w4_kernel_point(dev, **kw)
        torch.cuda.empty_cache()
    return out


def other_widths_leg(dev):
    """The bit widths next to 4 and 8 (the contract is 1 <= num_bits <= 8, pack_quantized/helpers.py:39-42): W3 / W2 / W6 g128 compress and
    decompress at 8192x8192 bf16 through the C ABI (ct_quant_pack / ct_unpack_dequant take the lean kernels of ct_quant_wb.hip), HBM-cold
    (packed words of the rotating sets >= 2x the Infinity Cache).  Gate per width: compress == quantize -> pack_to_int32, round trip ==
    fake_quantize on set 0, and a 64-row slice against the CPU oracle."""
    from compressed_tensors_amd import _lib, codec

    lib = _lib.load()
    BF16 = _lib.BF16
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {"workload": f"W{{3,2,6}}A16 g128 compress / decompress, {N}x{N} bf16, C ABI, HBM-cold rotation"}
    O = _oracle()
    for bits in (3, 2, 6):
        words = N * bits // 32
        nsets = max(4, -(-2 * IC_BYTES // (N * words * 4)))
        g = torch.Generator(device=dev).manual_seed(300 + bits)
        sets = []
        for _ in range(nsets):
            w = torch.randn(N, N, dtype=torch.float32, device=dev, generator=g).to(torch.bfloat16)
            sc, zp = codec.minmax_qparams(w, num_bits=bits, group_size=GROUP, symmetric=True)
            sets.append((w, sc, zp, torch.empty(N, words, dtype=torch.int32, device=dev)))
        outs = [torch.empty(N, N, dtype=torch.bfloat16, device=dev) for _ in range(4)]
        ca = [(w.data_ptr(), BF16, sc.data_ptr(), BF16, zp.data_ptr(), _lib.I8, N, N, 1, GROUP, N // GROUP, None, bits, BF16, pk.data_ptr(), stream) for (w, sc, zp, pk) in sets]
        da = [(pk.data_ptr(), N, words, N, bits, sc.data_ptr(), BF16, None, -1, 1, GROUP, N // GROUP, None, outs[i % 4].data_ptr(), BF16, stream)
              for i, (w, sc, zp, pk) in enumerate(sets)]

        def compress(i):
            rc = lib.ct_quant_pack(*ca[i % nsets])
            if rc:
                _lib.check(rc)

        def decompress(i):
            rc = lib.ct_unpack_dequant(*da[i % nsets])
            if rc:
                _lib.check(rc)

        for i in range(nsets):
            compress(i)
        one = 2 * N * N + 2 * N * (N // GROUP) + N * N * bits // 8
        us_c = time_kernel(compress, 60)
        us_d = time_kernel(decompress, 60, offset=nsets // 2)
        w, sc, zp, pk = sets[0]
        decompress(0)
        kw = dict(num_bits=bits, strategy="group", group_size=GROUP)
        ok = torch.equal(pk, codec.pack_to_int32(codec.quantize_tensor(w, sc, zp, dtype=torch.int8, **kw), bits)) and torch.equal(outs[0], codec.fake_quantize_tensor(w, sc, zp, **kw))
        sl = slice(0, 64)
        oc = O.pack_quantized_compress({"weight": w[sl].cpu(), "weight_scale": sc[sl].cpu(), "weight_zero_point": zp[sl].cpu()}, symmetric=True, **kw)
        od = O.pack_quantized_decompress(oc, num_bits=bits, strategy="group", symmetric=True)
        ok = ok and torch.equal(pk[sl].cpu(), oc["weight_packed"]) and torch.equal(outs[0][sl].cpu().view(torch.int16), od["weight"].view(torch.int16))
        out[f"w{bits}"] = {"alg_bytes_per_direction": one, "sets": nsets, "compress_us": round(us_c, 2), "compress_frac_hbm": round(one / us_c / 1e3 / HBM_PEAK_GBPS, 4),
                           "decompress_us": round(us_d, 2), "decompress_frac_hbm": round(one / us_d / 1e3 / HBM_PEAK_GBPS, 4), "bit_exact_vs_oracle_slice": bool(ok)}
        del sets, outs, ca, da
        torch.cuda.empty_cache()
    return out


def parity_gate(sets):
    """every benchmark run re-checks the timed kernels against INDEPENDENT kernels of the same library on the full
    8192 x 8192 tensor: fused compress == quantize(int8) -> pack_to_int32, and decompress(compress(W)) ==
    fake_quantize(W) (the reference's round-trip identity).  The comparison with the CPU oracle is part of
    the cpu_baseline leg, which runs the oracle anyway."""
    from compressed_tensors_amd import codec

    s = sets[0]
    kw = dict(num_bits=BITS, strategy="group", group_size=GROUP)
    q = codec.quantize_tensor(s["w"], s["scale"], s["zp"], dtype=torch.int8, **kw)
    ok_c = torch.equal(s["packed"], codec.pack_to_int32(q, BITS))
    dec = codec.unpack_and_dequantize(s["packed"], (N, N), s["scale"], None, **kw)
    fq = codec.fake_quantize_tensor(s["w"], s["scale"], s["zp"], **kw)
    ok_d = torch.equal(dec, fq)  # value equality, as the reference's round-trip test
    return bool(ok_c and ok_d)


def lib_srchash():
    try:
        return open(os.path.join(ROOT, "compressed_tensors_amd", "libct_hip.so.srchash")).read().strip()
    except OSError:
        return None


def committed_traffic(kernel):
    """roofline.traffic comes from a committed PMC pass (profiles/pmc_traffic.json: separate FETCH_SIZE / WRITE_SIZE runs under rocprofv3,
    which cannot run inside the timed region).  The file records the source hash of the library it was collected on; if the library
    has changed since, the figure is reported as STALE instead of silently."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        d = json.load(open(path))
    except Exception:
        return None, "profiles/pmc_traffic.json missing"
    rec, cur = d.get("_srchash"), lib_srchash()
    state = "current library" if rec and rec == cur else ("STALE: kernels changed since the PMC pass" if rec else "no library hash recorded with the pass")
    return d.get(kernel), f"profiles/pmc_traffic.json ({d.get('_tag', 'committed PMC pass')}; {state})"


def valu_busy_from_profile(path=None):
    """{kernel: {"valu_busy_frac": f, ...}} from the committed SQ counter pass (profiles/<tag>_headline_sq.txt, newest tag): SQ_INSTS_VALU counts
    wave64 VALU instructions (4 cycles each on a SIMD), the chip has 1024 SIMDs; busy = instructions * 4 / (kernel time * clock * 1024) at the
    2.4 GHz peak clock (a lower bound on the utilisation if the clock was lower).  Marked stale when the library changed since the pass."""
    import glob
    import re

    if path is None:
        cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_headline_sq.txt")))
        if not cands:
            return {}
        path = cands[-1]
    alias = {"ct::w4_quant_pack_lean_kernel<2, true>": "w4_quant_pack_lean_kernel<bf16>",
             "ct::w4_unpack_dequant_kernel<2, 2, false, false>": "w4_unpack_dequant_kernel<bf16>",   # until round 5 (bool ROWLEAD)
             "ct::w4_unpack_dequant_kernel<2, 2, false, 2>": "w4_unpack_dequant_kernel<bf16>"}       # scale mode 2: scalar loads
    out = {}
    try:
        txt = open(path).read().splitlines()
    except OSError:
        return out
    rec = next((l.split()[-1] for l in txt if l.startswith("# srchash")), None)
    state = "current library" if rec and rec == lib_srchash() else ("STALE: kernels changed since the pass" if rec else "no library hash recorded with the pass")
    us, valu = {}, {}
    for line in txt:
        m = re.match(r"^(ct::.*?)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)\s+\d+\s+\d+", line)
        if m and m.group(1).strip() in alias:
            us[m.group(1).strip()] = float(m.group(3))
        m = re.match(r"^(ct::.*?)\s+SQ_INSTS_VALU\s+\d+\s+([\d.]+)", line)
        if m and m.group(1).strip() in alias:
            valu[m.group(1).strip()] = float(m.group(2))
    rel = os.path.relpath(path, ROOT)
    for k in alias:
        if k in us and k in valu:
            out[alias[k]] = {"valu_busy_frac": round(valu[k] * 4 / (us[k] * 1e-6 * 2.4e9 * 1024), 3),
                             # gfx950's SIMDs are 32 lanes wide (MI355X_MICROARCH.md: a wave64 VALU instruction issues over 2 cycles); packed-fp32 / dot
                             # instructions take two passes, so the truth lies between the two figures
                             "valu_busy_frac_at_2_cycles": round(valu[k] * 2 / (us[k] * 1e-6 * 2.4e9 * 1024), 3), "valu_insts_per_launch": int(valu[k]),
                             "valu_source": f"{rel} (SQ_INSTS_VALU x 4 cycles / (avg kernel time x 2.4 GHz x 1024 SIMDs)); committed profile, not live; {state}"}
    return out


def _oracle():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O

    return O


def oracle_slice_check(dev, rows=512):
    """the real checker on a bounded slice (runs in every configuration, also with --no-cpu-baseline): the GPU path's packed
    words, decompressed weight and observer outputs of `rows` x 8192 against the CPU oracle, bit for bit"""
    O = _oracle()
    from compressed_tensors_amd import codec

    torch.manual_seed(1)
    w = torch.randn(rows, N, dtype=torch.bfloat16)
    scale, zp = O.calculate_qparams_minmax(w, num_bits=BITS, group_size=GROUP, symmetric=True)
    c = O.pack_quantized_compress({"weight": w, "weight_scale": scale, "weight_zero_point": zp}, num_bits=BITS, strategy="group", group_size=GROUP, symmetric=True)
    d = O.pack_quantized_decompress(c, num_bits=BITS, strategy="group", symmetric=True)
    kw = dict(num_bits=BITS, strategy="group", group_size=GROUP)
    g_packed = codec.quantize_and_pack(w.to(dev), scale.to(dev), zp.to(dev), **kw)
    g_dec = codec.unpack_and_dequantize(g_packed, (rows, N), scale.to(dev), None, **kw)
    g_scale, g_zp = codec.minmax_qparams(w.to(dev), num_bits=BITS, group_size=GROUP, symmetric=True)
    return bool(torch.equal(g_packed.cpu(), c["weight_packed"]) and torch.equal(g_dec.cpu().view(torch.int16), d["weight"].view(torch.int16))
                and torch.equal(g_scale.cpu().view(torch.int16), scale.view(torch.int16)) and torch.equal(g_zp.cpu(), zp))


def staged_reference():
    """the reference itself, when it can be imported on this machine (build container: /root/reference; GPU box: the archive
    oracle/stage_ref.py packed into oracle/_ref).  cpu_baseline leg only."""
    try:
        import ref_import

        if not ref_import.available():
            return None
        ref_import.import_reference()
        from compressed_tensors.compressors import BaseCompressor
        from compressed_tensors.quantization import QuantizationArgs, QuantizationScheme

        args = QuantizationArgs(num_bits=BITS, group_size=GROUP, symmetric=True, strategy="group")
        return {"cls": BaseCompressor.get_value_from_registry("pack-quantized"), "scheme": QuantizationScheme(targets=["Linear"], weights=args)}
    except Exception:
        return None


def cpu_baseline(dev):
    """The reference's CPU path on this box's host cores, next to the GPU number (baseline, not the target).

    When the reference is importable — /root/reference in the build container, the archive oracle/stage_ref.py staged under
    oracle/_ref on the GPU box — the reference's OWN PackedQuantizationCompressor.compress / .decompress is timed on CPU tensors and
    reported (`kind: "reference"`).  Beside it (and alone, `kind: "port"`, when no reference is present): oracle/eager_ref.py, the
    reference's eager torch op sequence restated (quantize: divide / add / clamp / round / cast passes in bf16; pack: int32 upcast,
    shifts, scatter_add_; unpack: gather of a (rows x groups, 32) int32 matrix; dequantize), pinned bit-for-bit against the reference.
    torch.set_num_threads(os.cpu_count()); 1 warm-up + min AND median of 3.  Its outputs check the GPU path on the same tensor.
    The C/OpenMP oracle (a stronger baseline than the reference) is reported as `cpu_baseline_port`."""
    O = _oracle()
    import eager_ref as E

    from compressed_tensors_amd import codec

    cores = os.cpu_count() or 1
    torch.set_num_threads(cores)
    kw = dict(num_bits=BITS, strategy="group", group_size=GROUP)

    medians = {}

    def best_of(fn, n=3, label=None):
        """1 warm-up, then min (returned) and median (kept under `label`) of n >= 3 runs: SURVEY 8d / BASELINE.md 4"""
        fn()
        ts, res = [], None
        for _ in range(max(n, 3)):
            t0 = time.perf_counter()
            res = fn()
            ts.append(time.perf_counter() - t0)
        if label:
            medians[label] = round(median(ts), 4)
        return min(ts), res

    points = {}
    by_threads = {}
    ref = staged_reference()
    for n in (N, 4096):
        torch.manual_seed(0)
        w = torch.randn(n, n, dtype=torch.bfloat16)
        scale, zp = O.calculate_qparams_minmax(w, num_bits=BITS, group_size=GROUP, symmetric=True)
        sd = {"weight": w, "weight_scale": scale, "weight_zero_point": zp}
        # torch.set_num_threads(os.cpu_count()) is what SURVEY 8d prescribes; on a many-core host eager torch is FASTER with fewer
        # threads (256 threads: 2.7 s, mostly fork / join), so the same sample is also timed at 64 / 32 / 16 threads and the best
        # configuration is the one reported (with its thread count) — the baseline is never handicapped
        t_c = t_d = None
        for th in sorted({cores, 64, 32, 16} & set(range(1, cores + 1)), reverse=True):
            torch.set_num_threads(th)
            tc, c = best_of(lambda: E.pack_quantized_compress(sd, symmetric=True, **kw), 3, f"restatement_compress_s_{n}_{th}thr")
            td, d = best_of(lambda: E.pack_quantized_decompress(c, num_bits=BITS, strategy="group", symmetric=True), 3, f"restatement_decompress_s_{n}_{th}thr")
            if n == N:
                by_threads[str(th)] = round(tc + td, 4)
            if t_c is None or tc + td < t_c + t_d:
                t_c, t_d, best_th = tc, td, th
        ref_pt = None
        if ref is not None and n == N:  # the reference's OWN classes on the same tensor, at the thread count that was best for the op sequence
            torch.set_num_threads(best_th)
            rc_t, rc = best_of(lambda: ref["cls"].compress(dict(sd), ref["scheme"]), 3, "reference_compress_s")
            rd_t, rd = best_of(lambda: ref["cls"].decompress(dict(rc), ref["scheme"]), 3, "reference_decompress_s")
            ref_pt = dict(t_c=rc_t, t_d=rd_t, threads=best_th,
                          same_as_restatement=bool(torch.equal(rc["weight_packed"], c["weight_packed"]) and torch.equal(rd["weight"].view(torch.int16), d["weight"].view(torch.int16))))
        torch.set_num_threads(cores)
        t_pc, pc = best_of(lambda: O.pack_quantized_compress(sd, symmetric=True, **kw), 3)
        t_pd, pd = best_of(lambda: O.pack_quantized_decompress(pc, num_bits=BITS, strategy="group", symmetric=True), 3)
        g_packed = codec.quantize_and_pack(w.to(dev), scale.to(dev), zp.to(dev), **kw)
        g_dec = codec.unpack_and_dequantize(g_packed, (n, n), scale.to(dev), None, **kw)
        g_scale, g_zp = codec.minmax_qparams(w.to(dev), num_bits=BITS, group_size=GROUP, symmetric=True)
        same = (torch.equal(c["weight_packed"], pc["weight_packed"]) and torch.equal(d["weight"].view(torch.int16), pd["weight"].view(torch.int16)))
        matches = (torch.equal(g_packed.cpu(), c["weight_packed"]) and torch.equal(g_dec.cpu().view(torch.int16), d["weight"].view(torch.int16))
                   and torch.equal(g_scale.cpu().view(torch.int16), scale.view(torch.int16)) and torch.equal(g_zp.cpu(), zp))
        points[n] = dict(t_c=t_c, t_d=t_d, t_pc=t_pc, t_pd=t_pd, same=bool(same), matches=bool(matches), threads=best_th, ref=ref_pt)
    # BASELINE config 1, the reference's own CPU-runnable case: int8 per-tensor symmetric IntQuantizationCompressor round trip
    torch.manual_seed(0)
    w = torch.randn(4096, 4096, dtype=torch.bfloat16)
    s1 = (w.abs().max().float() / 127.0).to(torch.bfloat16).reshape(1)
    sd8 = {"weight": w, "weight_scale": s1, "weight_zero_point": torch.zeros(1, dtype=torch.int8)}
    torch.set_num_threads(points[4096]["threads"])
    t_c8, c8 = best_of(lambda: E.int_quantized_compress(sd8))
    t_d8, d8 = best_of(lambda: E.int_quantized_decompress(c8))
    torch.set_num_threads(cores)
    g_q8 = codec.quantize_tensor(w.to(dev), s1.to(dev), sd8["weight_zero_point"].to(dev), num_bits=8, strategy="tensor", dtype=torch.int8)
    g_d8 = codec.dequantize_tensor(g_q8, s1.to(dev), None)
    ok8 = bool(torch.equal(g_q8.cpu(), c8["weight"]) and torch.equal(g_d8.cpu().view(torch.int16), d8["weight"].view(torch.int16)))

    def gbps(n, t):
        return round(2 * alg_bytes_one_direction(n) / t / 1e9, 3)

    # the same op sequence through PyTorch-ROCm's eager kernels on this GPU: what the reference itself does with CUDA tensors here
    torch.manual_seed(0)
    wg = torch.randn(N, N, dtype=torch.bfloat16, device=dev)
    sg, zg = codec.minmax_qparams(wg, num_bits=BITS, group_size=GROUP, symmetric=True)
    sdg = {"weight": wg, "weight_scale": sg, "weight_zero_point": zg}

    def gpu_best(fn, n=5):
        fn(); torch.cuda.synchronize()
        best, res = None, None
        for _ in range(n):
            t0 = time.perf_counter(); res = fn(); torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, res

    tg_c, cg = gpu_best(lambda: E.pack_quantized_compress(sdg, symmetric=True, **kw))
    tg_d, dg = gpu_best(lambda: E.pack_quantized_decompress(cg, num_bits=BITS, strategy="group", symmetric=True))
    eager_gpu_same = bool(torch.equal(cg["weight_packed"].contiguous(), codec.quantize_and_pack(wg, sg, zg, **kw))
                          and torch.equal(dg["weight"], codec.unpack_and_dequantize(cg["weight_packed"].contiguous(), (N, N), sg, None, **kw)))
    del wg, sdg, cg, dg
    torch.cuda.empty_cache()

    p = points[N]
    eager = {
        "value": gbps(N, p["t_c"] + p["t_d"]),
        "unit": "GB/s",
        "cores": p["threads"],
        "host_cores": cores,
        "seconds_by_torch_threads": by_threads,
        "kind": "port",
        "impl": "torch-eager: oracle/eager_ref.py restates the reference's op sequence (pack_quantized/base.py:62-163, helpers.py:20-180, "
                "forward_helpers.py:118-177,523-572) on CPU tensors; torch.set_num_threads swept over {os.cpu_count(), 64, 32, 16}, best reported; "
                "bit-identical to the reference in the build container",
        "sample": f"PackedQuantizationCompressor-shaped compress + decompress of ONE W4A16 g128 {N}x{N} bf16 weight, 1 warm-up + min of 3 per thread count "
                  f"(compress {p['t_c']:.3f} s, decompress {p['t_d']:.3f} s); medians in `median_s`",
        "median_s": medians,
        "compress_s": round(p["t_c"], 4), "decompress_s": round(p["t_d"], 4),
        "at_4096": {"value": gbps(4096, points[4096]["t_c"] + points[4096]["t_d"]), "compress_s": round(points[4096]["t_c"], 4),
                    "decompress_s": round(points[4096]["t_d"], 4)},
        "config1_int8_per_tensor_4096": {"compress_s": round(t_c8, 4), "decompress_s": round(t_d8, 4),
                                         "GBps": round(2 * 3 * 4096 * 4096 / (t_c8 + t_d8) / 1e9, 3), "gpu_bit_exact": ok8},
        "gpu_bit_exact_vs_oracle": bool(all(q["matches"] and q["same"] for q in points.values()) and ok8),
        "reference_eager_ops_on_this_gpu": {"value": gbps(N, tg_c + tg_d), "unit": "GB/s", "compress_ms": round(tg_c * 1e3, 3), "decompress_ms": round(tg_d * 1e3, 3),
                                            "bit_identical_to_the_hip_kernels": eager_gpu_same,
                                            "note": "the reference's op sequence on CUDA tensors through PyTorch-ROCm (not the CPU baseline the metric names)"},
    }
    rp = p.get("ref")
    if rp:  # the staged reference was importable: ITS time is the baseline, the restatement moves to a sub-entry
        eager["restatement"] = {"value": eager["value"], "cores": eager["cores"], "compress_s": eager["compress_s"], "decompress_s": eager["decompress_s"],
                                "impl": "oracle/eager_ref.py (the same op sequence restated)"}
        eager.update({"value": gbps(N, rp["t_c"] + rp["t_d"]), "cores": rp["threads"], "kind": "reference",
                      "impl": "the reference's own PackedQuantizationCompressor.compress / .decompress (compressors/pack_quantized/base.py:62-163) on CPU tensors, imported from the "
                              "archive oracle/stage_ref.py staged (oracle/_ref); torch threads = the best of the sweep in seconds_by_torch_threads",
                      "sample": f"compress + decompress of ONE W4A16 g128 {N}x{N} bf16 weight, 1 warm-up + min of 3 (compress {rp['t_c']:.3f} s, decompress {rp['t_d']:.3f} s; "
                                f"medians {medians.get('reference_compress_s')} / {medians.get('reference_decompress_s')} s)",
                      "value_from_medians": gbps(N, medians.get("reference_compress_s", rp["t_c"]) + medians.get("reference_decompress_s", rp["t_d"])),
                      "compress_s": round(rp["t_c"], 4), "decompress_s": round(rp["t_d"], 4), "bit_identical_to_restatement_and_gpu": bool(rp["same_as_restatement"] and p["matches"])})
        eager["gpu_bit_exact_vs_oracle"] = bool(eager["gpu_bit_exact_vs_oracle"] and rp["same_as_restatement"])
    port = {
        "value": gbps(N, p["t_pc"] + p["t_pd"]), "unit": "GB/s", "cores": O.num_threads(), "kind": "port",
        "impl": "C restatement with OpenMP over rows (oracle/ct_oracle.c), unfused quantize->pack / unpack->dequantize",
        "sample": f"the same {N}x{N} weight, best of 3 ({p['t_pc'] + p['t_pd']:.3f} s)",
        "at_4096": {"value": gbps(4096, points[4096]["t_pc"] + points[4096]["t_pd"])},
    }
    return eager, port


def bitmask_leg(dev):
    """BASELINE config 3 (sparse-bitmask, 50 % unstructured, 8192x8192 bf16): decompress and
    compress rates, reported as extra fields"""
    from compressed_tensors_amd import _lib, codec

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(7)
    items = []
    NB = 8  # 8 x (67 MB values + 8 MB bitmask) of reads: 2.3x the Infinity Cache
    for _ in range(NB):
        w = torch.randn(N, N, dtype=torch.bfloat16, device=dev, generator=g)
        w = w.masked_fill(torch.rand(N, N, device=dev, generator=g) < 0.5, 0)
        values, bitmask, row_offsets = codec.bitmask_compress(w)
        items.append(dict(w=w, values=values, bitmask=bitmask, ro=row_offsets, out=torch.empty_like(w),
                          counts=torch.empty(N + 1, dtype=torch.int64, device=dev), ro2=torch.empty(N, dtype=torch.int64, device=dev),
                          bm2=torch.empty_like(bitmask), v2=torch.empty_like(values)))
    BF16 = _lib.BF16

    def decompress(i):
        it = items[i % NB]
        lib.ct_bitmask_decompress(it["values"].data_ptr(), it["values"].numel(), it["bitmask"].data_ptr(), it["ro"].data_ptr(), -1, BF16,
                                  N, N, it["out"].data_ptr(), stream)

    def compress(i):
        it = items[i % NB]
        lib.ct_bitmask_count(it["w"].data_ptr(), BF16, N, N, it["bm2"].data_ptr(), it["counts"].data_ptr(), stream)
        lib.ct_exclusive_scan_i64(it["counts"].data_ptr(), N, it["ro2"].data_ptr(), it["counts"][N:].data_ptr(), stream)
        lib.ct_bitmask_scatter(it["w"].data_ptr(), BF16, N, N, it["ro2"].data_ptr(), it["v2"].data_ptr(), stream)

    ws_bytes = int(lib.ct_bitmask_compress_workspace_bytes(N, N))
    for it in items:
        it["ws"] = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=dev)

    def compress1(i):
        it = items[i % NB]
        lib.ct_bitmask_compress(it["w"].data_ptr(), BF16, N, N, it["v2"].data_ptr(), it["v2"].numel(), it["bm2"].data_ptr(), it["ro2"].data_ptr(),
                                it["ws"][-1:].data_ptr(), it["ws"].data_ptr(), ws_bytes, stream)

    nnz = items[0]["values"].numel()
    nnz_of = lambda it: it["values"].numel()
    alg = 2 * N * N + 2 * nnz + N * N // 8 + 8 * N
    us_d = time_kernel(decompress, 24)
    us_c = time_kernel(compress, 24)
    ok = torch.equal(items[0]["out"].view(torch.int16), items[0]["w"].view(torch.int16)) and \
        torch.equal(items[0]["v2"].view(torch.int16), items[0]["values"].view(torch.int16))
    for it in items:
        it["v2"].zero_(); it["bm2"].zero_(); it["ro2"].zero_()
    us_c1 = time_kernel(compress1, 24)
    ok1 = all(torch.equal(it["v2"].view(torch.int16), it["values"].view(torch.int16)) and torch.equal(it["bm2"], it["bitmask"])
              and torch.equal(it["ro2"], it["ro"]) and int(it["ws"][-1].item()) == it["values"].numel() for it in items)
    # the drop-in class (VERDICT r03 weak #2c): BitmaskTensor.from_dense allocates its own worst-case value buffer, bitmask, row
    # offsets and workspace and must have nnz on the host before it returns; .decompress() allocates the dense output
    api = {}
    try:
        from compressed_tensors_amd.compressors.sparse.sparse_bitmask import BitmaskTensor

        bts = [BitmaskTensor(shape=(N, N), compressed=it["values"], bitmask=it["bitmask"], row_offsets=it["ro"]) for it in items]
        last = {}

        def api_compress(i):  # the default: `compressed` owns exactly nnz elements (tensor[mask]'s size) — the kept prefix is copied out of the worst-case buffer
            last["bt"] = BitmaskTensor.from_dense(items[i % NB]["w"])

        def api_compress_view(i):  # exact=False: no copy, `compressed` is a view of a dense-sized buffer (the result pins numel x 2 bytes)
            last["btv"] = BitmaskTensor.from_dense(items[i % NB]["w"], exact=False)

        def api_decompress(i):
            last["dense"] = bts[i % NB].decompress()

        c_us, c_min, c_max = time_calls(api_compress)
        v_us, v_min, v_max = time_calls(api_compress_view)
        bt, btv = last["bt"], last["btv"]
        j = (MIN_LAUNCHES_PER_BLOCK - 1) % NB
        api_ok = (torch.equal(bt.compressed.view(torch.int16), items[j]["values"].view(torch.int16)) and torch.equal(bt.bitmask, items[j]["bitmask"])
                  and torch.equal(bt.row_offsets, items[j]["ro"]) and torch.equal(btv.compressed.view(torch.int16), items[j]["values"].view(torch.int16)))
        storage_exact, storage_view = bt.compressed.untyped_storage().nbytes(), btv.compressed.untyped_storage().nbytes()
        d_us, d_min, d_max = time_calls(api_decompress)
        api_ok = api_ok and torch.equal(last["dense"].view(torch.int16), items[j]["w"].view(torch.int16))
        last.clear()
        api = {"api_compress_us": round(c_us, 2), "api_compress_us_min_max": [round(c_min, 2), round(c_max, 2)],
               "api_compress_frac_hbm": round(alg / c_us / 1e3 / HBM_PEAK_GBPS, 4),
               "api_compress_mode": "exact (default): values own nnz elements; + one asynchronous device copy of the kept prefix",
               "api_compress_values_storage_bytes": storage_exact,
               "api_compress_view_us": round(v_us, 2), "api_compress_view_us_min_max": [round(v_min, 2), round(v_max, 2)],
               "api_compress_view_frac_hbm": round(alg / v_us / 1e3 / HBM_PEAK_GBPS, 4),
               "api_compress_view_values_storage_bytes": storage_view, "api_compress_nnz_bytes": 2 * nnz_of(items[j]),
               "api_decompress_us": round(d_us, 2), "api_decompress_us_min_max": [round(d_min, 2), round(d_max, 2)],
               "api_decompress_frac_hbm": round(alg / d_us / 1e3 / HBM_PEAK_GBPS, 4), "api_bit_exact": bool(api_ok),
               "api": "BitmaskTensor.from_dense(w) / .decompress(): per-call wall time incl. the class's own allocations and the host wait for nnz "
                      "(pinned mailbox word, no D2H copy)"}
    except Exception as e:
        api = {"api_error": repr(e)}
    # sparse-24-bitmask (S2) on the same tensors pruned 2:4: compress = top-2 of every quad + bitmask, decompress = the 2:4-regular row path
    s24 = {}
    try:
        O = _oracle()
        for it in items:
            it["w"].masked_fill_(~codec.sparse24_mask(it["w"]), 0)  # 2:4-pruned in place (+0.0 for the dropped elements)
            it["v24"] = torch.empty(N, N // 2, dtype=torch.bfloat16, device=dev)

        def c24(i):
            it = items[i % NB]
            lib.ct_sparse24_compress(it["w"].data_ptr(), BF16, N, N, it["v24"].data_ptr(), it["bm2"].data_ptr(), stream)

        def d24(i):
            it = items[i % NB]
            lib.ct_bitmask_decompress(it["v24"].data_ptr(), it["v24"].numel(), it["bm2"].data_ptr(), None, N // 2, BF16, N, N, it["out"].data_ptr(), stream)

        for i in range(NB):
            c24(i)
        alg24 = 2 * N * N + N * N + N * N // 8
        us_c24, us_d24 = time_kernel(c24, 24), time_kernel(d24, 24, offset=NB // 2)
        it = items[0]
        rv, rb = O.sparse24_bitmask_compress(items[0]["w"][:256].cpu())
        ok24 = (torch.equal(it["out"].view(torch.int16), it["w"].view(torch.int16)) and torch.equal(items[0]["v24"][:256].cpu().view(torch.int16), rv.view(torch.int16))
                and torch.equal(items[0]["bm2"][:256].cpu(), rb))
        s24 = {"s24_alg_bytes": alg24, "s24_compress_us": round(us_c24, 2), "s24_compress_frac_hbm": round(alg24 / us_c24 / 1e3 / HBM_PEAK_GBPS, 4),
               "s24_decompress_us": round(us_d24, 2), "s24_decompress_frac_hbm": round(alg24 / us_d24 / 1e3 / HBM_PEAK_GBPS, 4), "s24_bit_exact": bool(ok24),
               "s24_workload": f"sparse-24-bitmask compress / decompress, {N}x{N} bf16 pruned 2:4, C ABI, {NB} rotating sets; 256 rows against the CPU oracle"}
    except Exception as e:
        s24 = {"s24_error": repr(e)}
    # float32 payloads (older sparse checkpoints keep fp32 weights): the resident kernel moves them as pairs of halves
    f32 = {}
    try:
        del items
        torch.cuda.empty_cache()
        F32, NF = _lib.F32, 4  # 4 x 268 MB of reads
        sets32 = []
        for _ in range(NF):
            w = torch.randn(N, N, dtype=torch.float32, device=dev, generator=g)
            w = w.masked_fill(torch.rand(N, N, device=dev, generator=g) < 0.5, 0)
            sets32.append(w)
        # every rotating set has its own compressed image, so that the decompress launches read HBM-cold values and masks too
        v32 = [torch.empty(N * N, dtype=torch.float32, device=dev) for _ in range(NF)]
        bm32 = [torch.empty(N, N // 8, dtype=torch.uint8, device=dev) for _ in range(NF)]
        ro32 = [torch.empty(N, dtype=torch.int64, device=dev) for _ in range(NF)]
        wk32 = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=dev)
        o32 = [torch.empty(N, N, dtype=torch.float32, device=dev) for _ in range(2)]

        def c32(i):
            k = i % NF
            lib.ct_bitmask_compress(sets32[k].data_ptr(), F32, N, N, v32[k].data_ptr(), v32[k].numel(), bm32[k].data_ptr(), ro32[k].data_ptr(), wk32[-1:].data_ptr(),
                                    wk32.data_ptr(), ws_bytes, stream)

        us_c32 = time_kernel(c32, 12)
        nnz32s = []
        for k in range(NF):
            c32(k)
            torch.cuda.synchronize()
            nnz32s.append(int(wk32[-1].item()))
        nnz32 = nnz32s[0]
        w0 = sets32[0]
        m0 = w0 != 0
        cnt0 = m0.sum(-1)
        ok32 = (nnz32 == int(cnt0.sum().item()) and torch.equal(v32[0][:nnz32], w0[m0]) and torch.equal(ro32[0], torch.cumsum(cnt0, 0) - cnt0)
                and torch.equal(bm32[0], (m0.view(N, N // 8, 8).to(torch.int32) * (1 << torch.arange(8, device=dev, dtype=torch.int32))).sum(-1).to(torch.uint8)))

        def d32(i):
            k = i % NF
            lib.ct_bitmask_decompress(v32[k].data_ptr(), nnz32s[k], bm32[k].data_ptr(), ro32[k].data_ptr(), -1, F32, N, N, o32[i % 2].data_ptr(), stream)

        us_d32 = time_kernel(d32, 12)
        d32(0)
        torch.cuda.synchronize()
        ok32 = ok32 and torch.equal(o32[0], w0)
        alg32 = 4 * N * N + 4 * nnz32 + N * N // 8 + 8 * N
        f32 = {"f32_alg_bytes": alg32, "f32_compress_us": round(us_c32, 2), "f32_compress_frac_hbm": round(alg32 / us_c32 / 1e3 / HBM_PEAK_GBPS, 4),
               "f32_decompress_us": round(us_d32, 2), "f32_decompress_frac_hbm": round(alg32 / us_d32 / 1e3 / HBM_PEAK_GBPS, 4), "f32_bit_exact": bool(ok32),
               "f32_workload": f"sparse-bitmask 50 % unstructured {N}x{N} float32, C ABI, {NF} rotating sets (dense and compressed images); outputs against eager torch ops on the device"}
        del sets32, v32, o32
    except Exception as e:
        f32 = {"f32_error": repr(e)}
    # 8-bit payloads (FP8 / int8 weights, gathered as bytes): round 6 put them on the resident kernel's row form
    i8 = {}
    try:
        I8, NI = _lib.I8, 8  # 8 x 67 MB of reads
        sets8 = []
        for _ in range(NI):
            w = torch.randint(-127, 128, (N, N), device=dev, generator=g, dtype=torch.int16).to(torch.int8)
            sets8.append(w.masked_fill_(torch.rand(N, N, device=dev, generator=g) < 0.5, 0))
        v8 = [torch.empty(N * N, dtype=torch.int8, device=dev) for _ in range(NI)]  # one compressed image per rotating set: decompress reads cold too
        bm8 = [torch.empty(N, N // 8, dtype=torch.uint8, device=dev) for _ in range(NI)]
        ro8 = [torch.empty(N, dtype=torch.int64, device=dev) for _ in range(NI)]
        wk8 = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=dev)
        o8 = [torch.empty(N, N, dtype=torch.int8, device=dev) for _ in range(2)]

        def c8(i):
            k = i % NI
            lib.ct_bitmask_compress(sets8[k].data_ptr(), I8, N, N, v8[k].data_ptr(), v8[k].numel(), bm8[k].data_ptr(), ro8[k].data_ptr(), wk8[-1:].data_ptr(), wk8.data_ptr(),
                                    ws_bytes, stream)

        us_c8 = time_kernel(c8, 24)
        nnz8s = []
        for k in range(NI):
            c8(k)
            torch.cuda.synchronize()
            nnz8s.append(int(wk8[-1].item()))
        nnz8 = nnz8s[0]
        w0 = sets8[0]
        m0 = w0 != 0
        cnt0 = m0.sum(-1)
        ok8 = (nnz8 == int(cnt0.sum().item()) and torch.equal(v8[0][:nnz8], w0[m0]) and torch.equal(ro8[0], torch.cumsum(cnt0, 0) - cnt0)
               and torch.equal(bm8[0], (m0.view(N, N // 8, 8).to(torch.int32) * (1 << torch.arange(8, device=dev, dtype=torch.int32))).sum(-1).to(torch.uint8)))

        def d8(i):
            k = i % NI
            lib.ct_bitmask_decompress(v8[k].data_ptr(), nnz8s[k], bm8[k].data_ptr(), ro8[k].data_ptr(), -1, I8, N, N, o8[i % 2].data_ptr(), stream)

        us_d8 = time_kernel(d8, 24)
        d8(0)
        torch.cuda.synchronize()
        ok8 = ok8 and torch.equal(o8[0], w0)
        # the 2:4 codec on the same bytes (sparse-24-bitmask of FP8 / int8 weights)
        for k in range(NI):
            sets8[k].masked_fill_(~codec.sparse24_mask(sets8[k]), 0)
        v24 = [torch.empty(N, N // 2, dtype=torch.int8, device=dev) for _ in range(NI)]

        def c248(i):
            k = i % NI
            lib.ct_sparse24_compress(sets8[k].data_ptr(), I8, N, N, v24[k].data_ptr(), bm8[k].data_ptr(), stream)

        def d248(i):
            k = i % NI
            lib.ct_bitmask_decompress(v24[k].data_ptr(), v24[k].numel(), bm8[k].data_ptr(), None, N // 2, I8, N, N, o8[i % 2].data_ptr(), stream)

        us_c248 = time_kernel(c248, 24)
        us_d248 = time_kernel(d248, 24)
        d248(0)
        torch.cuda.synchronize()
        ok248 = torch.equal(o8[0], sets8[0])
        alg248 = N * N + N * N // 2 + N * N // 8
        i8_24 = {"i8_s24_alg_bytes": alg248, "i8_s24_compress_us": round(us_c248, 2), "i8_s24_compress_frac_hbm": round(alg248 / us_c248 / 1e3 / HBM_PEAK_GBPS, 4),
                 "i8_s24_decompress_us": round(us_d248, 2), "i8_s24_decompress_frac_hbm": round(alg248 / us_d248 / 1e3 / HBM_PEAK_GBPS, 4), "i8_s24_round_trip": bool(ok248)}
        alg8 = N * N + nnz8 + N * N // 8 + 8 * N
        i8 = {"i8_alg_bytes": alg8, "i8_compress_us": round(us_c8, 2), "i8_compress_frac_hbm": round(alg8 / us_c8 / 1e3 / HBM_PEAK_GBPS, 4),
              "i8_decompress_us": round(us_d8, 2), "i8_decompress_frac_hbm": round(alg8 / us_d8 / 1e3 / HBM_PEAK_GBPS, 4), "i8_bit_exact": bool(ok8),
              "i8_workload": f"sparse-bitmask 50 % unstructured {N}x{N} int8 (FP8 weights ride the same bytes), C ABI, {NI} rotating sets (dense and compressed images); "
                             "outputs against eager torch ops on the device", **i8_24}
        del sets8, v8, o8, v24
    except Exception as e:
        i8 = {"i8_error": repr(e)}
    return {
        **s24, **f32, **i8, **api,
        "workload": f"sparse-bitmask 50% unstructured {N}x{N} bf16 (nnz={nnz})",
        "alg_bytes": alg,
        "decompress_us": round(us_d, 2), "decompress_GBps": round(alg / us_d / 1e3, 1), "decompress_frac_hbm": round(alg / us_d / 1e3 / HBM_PEAK_GBPS, 4),
        "compress_us": round(us_c1, 2), "compress_GBps": round(alg / us_c1 / 1e3, 1), "compress_frac_hbm": round(alg / us_c1 / 1e3 / HBM_PEAK_GBPS, 4),
        "compress_kernel": "flat16_resident_kernel (x read once, one launch, no scan kernel, no host round trip)",
        "compress_two_pass_us": round(us_c, 2),
        "round_trip_bit_exact": bool(ok and ok1),
    }


def int8_leg(dev):
    """BASELINE config 1 on the GPU: int8 per-tensor symmetric quantize / dequantize of 4096x4096 bf16
    (IntQuantizationCompressor's two kernels) through the C ABI; 50.3 MB algorithmic per direction."""
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    n, BF16, I8 = 4096, _lib.BF16, _lib.I8
    g = torch.Generator(device=dev).manual_seed(11)
    items = []
    for _ in range(24):  # 24 x 33.5 MB of weights: HBM-cold
        w = torch.randn(n, n, dtype=torch.bfloat16, device=dev, generator=g)
        scale = (w.abs().max().float() / 127.0).to(torch.bfloat16).reshape(1)
        items.append(dict(w=w, scale=scale, q=torch.empty(n, n, dtype=torch.int8, device=dev), out=torch.empty_like(w)))

    def quant(i):
        it = items[i % len(items)]
        lib.ct_quantize(it["w"].data_ptr(), BF16, it["scale"].data_ptr(), BF16, None, -1, n, n, n, n, 1, None, 8, BF16, it["q"].data_ptr(), I8, stream)

    def dequant(i):
        it = items[i % len(items)]
        lib.ct_dequantize(it["q"].data_ptr(), I8, it["scale"].data_ptr(), BF16, None, -1, n, n, n, n, 1, None, it["out"].data_ptr(), BF16, stream)

    for i in range(len(items)):
        quant(i)
    alg = 3 * n * n
    us_q, us_d = time_kernel(quant, 48), time_kernel(dequant, 48, offset=12)
    it = items[0]
    ok = torch.equal(it["out"].float(), (it["q"].float() * it["scale"].float()).to(torch.bfloat16).float())
    return {"workload": "int8 per-tensor symmetric quantize / dequantize, 4096x4096 bf16 (IntQuantizationCompressor kernels)",
            "alg_bytes_per_direction": alg,
            "quantize_us": round(us_q, 2), "quantize_frac_hbm": round(alg / us_q / 1e3 / HBM_PEAK_GBPS, 4),
            "dequantize_us": round(us_d, 2), "dequantize_frac_hbm": round(alg / us_d / 1e3 / HBM_PEAK_GBPS, 4),
            "dequantize_matches_torch": bool(ok)}


def quantize_leg(dev):
    """SURVEY 8(a) R5 / R6 / R7 as kernels: quantize -> int8 codes, dequantize, fake_quantize (int8 channel-wise, symmetric and with
    zero points) at 8192x8192 through the C ABI, bf16 and fp32 weights, HBM-cold rotation; the results of one set are compared with
    the oracle on a 256-row slice."""
    from compressed_tensors_amd import _lib

    O = _oracle()
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    n = N
    out = {"workload": f"int8 channel-wise quantize / dequantize / fake_quantize kernels, {n}x{n}, through the C ABI"}
    g = torch.Generator(device=dev).manual_seed(17)
    for dt in (torch.bfloat16, torch.float32):
        D = _lib.DT[dt]
        es = torch.empty(0, dtype=dt).element_size()
        nsets = 6 if es == 2 else 4
        ws = [torch.randn(n, n, dtype=torch.float32, device=dev, generator=g).to(dt) for _ in range(nsets)]
        sc = (ws[0].float().abs().amax(dim=1, keepdim=True) / 127.0).to(dt).contiguous()
        zp = torch.randint(-3, 4, (n, 1), dtype=torch.int8, device=dev, generator=g)
        nq = 8  # 8 x 67 MB of codes: the dequantize's reads cannot be served by the 256 MiB Infinity Cache
        qs = [torch.empty(n, n, dtype=torch.int8, device=dev) for _ in range(nq)]
        outs = [torch.empty(n, n, dtype=dt, device=dev) for _ in range(2)]
        for name, z in (("symmetric", None), ("asymmetric", zp)):
            zptr, zdt = (None, -1) if z is None else (z.data_ptr(), _lib.I8)

            def fq(i):
                _lib.check(lib.ct_quantize(ws[i % nsets].data_ptr(), D, sc.data_ptr(), D, zptr, zdt, n, n, 1, n, 1, None, 8, D, qs[i % nq].data_ptr(), _lib.I8, stream))

            def fd(i):
                _lib.check(lib.ct_dequantize(qs[i % nq].data_ptr(), _lib.I8, sc.data_ptr(), D, zptr, zdt, n, n, 1, n, 1, None, outs[i % 2].data_ptr(), D, stream))

            def ff(i):
                _lib.check(lib.ct_fake_quantize(ws[i % nsets].data_ptr(), D, sc.data_ptr(), D, zptr, zdt, n, n, 1, n, 1, None, 8, D, outs[i % 2].data_ptr(), D, stream))

            for i in range(nq):
                fq(i)
            us_q, us_d, us_f = time_kernel(fq, 24), time_kernel(fd, 24), time_kernel(ff, 24)
            # oracle gate on a slice of set 0
            rows = slice(0, 256)
            zc = torch.zeros(256, 1, dtype=torch.int8) if z is None else z[rows].cpu()
            kw = dict(num_bits=8, strategy="channel", group_size=None)
            fq(0); ff(0)
            torch.cuda.synchronize()
            q_ref = O.quantize(ws[0][rows].cpu(), sc[rows].cpu(), zc, dtype=torch.int8, **kw)
            ok = torch.equal(qs[0][rows].cpu(), q_ref)
            f_ref = O.fake_quantize(ws[0][rows].cpu(), sc[rows].cpu(), zc, **kw)
            ok = ok and torch.equal(outs[0][rows].cpu().view(torch.int16 if es == 2 else torch.int32), f_ref.view(torch.int16 if es == 2 else torch.int32))
            fd(0)
            torch.cuda.synchronize()
            d_ref = O.dequantize(q_ref, sc[rows].cpu(), zc, strategy="channel")
            ok = ok and torch.equal(outs[0][rows].cpu().view(torch.int16 if es == 2 else torch.int32), d_ref.view(torch.int16 if es == 2 else torch.int32))
            qd, fqb = n * n * (es + 1), n * n * 2 * es
            out[f"{str(dt).split('.')[-1]}_{name}"] = {
                "quantize_us": round(us_q, 2), "quantize_frac_hbm": round(qd / us_q / 1e3 / HBM_PEAK_GBPS, 4),
                "dequantize_us": round(us_d, 2), "dequantize_frac_hbm": round(qd / us_d / 1e3 / HBM_PEAK_GBPS, 4),
                "fake_quantize_us": round(us_f, 2), "fake_quantize_frac_hbm": round(fqb / us_f / 1e3 / HBM_PEAK_GBPS, 4),
                "alg_bytes_quantize_or_dequantize": qd, "alg_bytes_fake_quantize": fqb, "bit_exact_vs_oracle_256_rows": bool(ok)}
        del ws, qs, outs
        torch.cuda.empty_cache()
    return out


def marlin24_leg(dev):
    """BASELINE config 4: 2:4 semi-structured + int4 group-128 in the Marlin-24 layout, 8192x8192 bf16,
    through the Marlin24Compressor plug-in class (quantize -> 2:4 compress + metadata -> tile-permuted
    int4 packing -> scale permutation: four kernels plus the host glue)."""
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import codec

    args = cta.QuantizationArgs(num_bits=4, group_size=GROUP, symmetric=True, strategy="group")
    scheme = cta.QuantizationScheme(targets=["Linear"], weights=args)
    g = torch.Generator(device=dev).manual_seed(13)
    sds = []
    for _ in range(6):  # 6 x 134 MB of weights: HBM-cold
        w = torch.randn(N, N, dtype=torch.bfloat16, device=dev, generator=g)
        w = w * codec.sparse24_mask(w).to(w.dtype)
        scale, zp = codec.minmax_qparams(w, num_bits=BITS, group_size=GROUP, symmetric=True)
        sds.append({"weight": w, "weight_scale": scale, "weight_zero_point": zp})
    out = cta.Marlin24Compressor.compress(sds[0], scheme)
    torch.cuda.synchronize()
    # gate: all three outputs of the full 8192 x 8192 tensor against the CPU oracle (about 2 s of host time)
    O = _oracle()
    ref = O.marlin24_compress(sds[0]["weight"].cpu(), sds[0]["weight_scale"].cpu(), sds[0]["weight_zero_point"].cpu(),
                              num_bits=BITS, strategy="group", group_size=GROUP)
    exact = all(out[k].shape == ref[k].shape and torch.equal(out[k].cpu().contiguous().view(torch.int16 if out[k].dtype == torch.float16 else out[k].dtype),
                                                             ref[k].contiguous().view(torch.int16 if ref[k].dtype == torch.float16 else ref[k].dtype))
                for k in ("weight_packed", "scale_packed", "meta"))
    M = cta.Marlin24Compressor
    with M.deferred_structure_check():  # the batch form ModelCompressor uses: the 2:4 violation flags are read once (per 1024 calls / at the exit)
        us = time_kernel(lambda i: M.compress(sds[i % len(sds)], scheme), 18)
        # what the host spends issuing one call (no wait on the device): the API figure above is this if it exceeds the kernel
        host_us = []
        for _ in range(BLOCKS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(18):
                M.compress(sds[i % len(sds)], scheme)
            host_us.append((time.perf_counter() - t0) / 18 * 1e6)
        torch.cuda.synchronize()
    # upstream's semantics — the DEFAULT of the class: the ValueError is raised by the call itself, i.e. the host waits for the launch
    # (a spin on the stream; the verdict is a pinned mailbox word).  Wall time per call: the host is part of this path.
    us_strict, strict_min, strict_max = time_calls(lambda i: M.compress(sds[i % len(sds)], scheme))
    # the kernels alone, through the C ABI
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    bufs = (torch.empty_like(out["weight_packed"]), torch.empty(N, N // 16, dtype=torch.int16, device=dev), torch.empty_like(out["scale_packed"]))

    def kern(i):
        sd = sds[i % len(sds)]
        lib.ct_marlin24_compress_w4_full(sd["weight"].data_ptr(), _lib.BF16, sd["weight_scale"].data_ptr(), _lib.BF16, sd["weight_zero_point"].data_ptr(), _lib.I8,
                                         N, N, GROUP, 1, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), flag.data_ptr(), 0, stream)

    us_k = time_kernel(kern, 24)
    exact = exact and torch.equal(bufs[0], M.compress(sds[23 % len(sds)], scheme)["weight_packed"]) and int(flag.item()) == 0
    alg = 2 * N * N + 2 * N * (N // GROUP) + N * N // 4 + N * N // 8 + 2 * N * (N // GROUP)
    return {"workload": f"marlin-24 compress (2:4 + int4 g128), {N}x{N} bf16, plug-in class API",
            "alg_bytes": alg,
            # the class as a caller gets it by default: Marlin24Compressor.compress raises the 2:4 ValueError itself
            "compress_us_default": round(us_strict, 1), "compress_us_default_min_max": [round(strict_min, 1), round(strict_max, 1)],
            "compress_default_frac_hbm": round(alg / us_strict / 1e3 / HBM_PEAK_GBPS, 4),
            # inside `with Marlin24Compressor.deferred_structure_check()` (what compress_modules / ModelCompressor use for a batch)
            "compress_us_deferred_check": round(us, 1), "compress_deferred_check_frac_hbm": round(alg / us / 1e3 / HBM_PEAK_GBPS, 4),
            "compress_us": round(us_strict, 1), "compress_GBps": round(alg / us_strict / 1e3, 1),
            "compress_frac_hbm": round(alg / us_strict / 1e3 / HBM_PEAK_GBPS, 4),
            "compress_us_structure_check_per_call": round(us_strict, 1), "host_issue_us_per_call": round(median(host_us), 1),
            "kernels_us": round(us_k, 2), "kernels_frac_hbm": round(alg / us_k / 1e3 / HBM_PEAK_GBPS, 4),
            "kernels": "marlin24_fused_w4_lean_kernel + marlin24_pack_scales_kernel (ct_marlin24_compress_w4_full)",
            "bit_exact_vs_oracle": bool(exact),
            "outputs": {k: list(v.shape) for k, v in out.items() if hasattr(v, "shape")}}


def qparams_leg(dev):
    """SURVEY 8f N1, the step before compress: min-max observer + calculate_qparams (group 128, symmetric)
    over 8192x8192 bf16 — one streaming read of the weight (134.2 MB) + 1.6 MB of scales / zero points"""
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = [torch.randn(N, N, dtype=torch.bfloat16, device=dev) for _ in range(8)]
    sc = torch.empty(N, N // GROUP, dtype=torch.bfloat16, device=dev)
    zp = torch.empty(N, N // GROUP, dtype=torch.int8, device=dev)
    us = time_kernel(lambda i: lib.ct_minmax_qparams(ws[i % 8].data_ptr(), _lib.BF16, N, N, GROUP, BITS, 1, sc.data_ptr(), zp.data_ptr(), stream), 48)
    alg = 2 * N * N + 3 * N * (N // GROUP)
    # the same observer fused with the W4 compress (ct_rtn_quant_pack_w4): the weight is read once
    packed = [torch.empty(N, N // 8, dtype=torch.int32, device=dev) for _ in range(8)]
    us_f = time_kernel(lambda i: lib.ct_rtn_quant_pack_w4(ws[i % 8].data_ptr(), _lib.BF16, N, N, GROUP, 1, packed[i % 8].data_ptr(), sc.data_ptr(), zp.data_ptr(),
                                                           stream), 48)
    alg_f = alg + N * N // 2
    return {"workload": f"min-max observer + calculate_qparams, int4 g128 symmetric, {N}x{N} bf16", "alg_bytes": alg,
            "us": round(us, 2), "GBps": round(alg / us / 1e3, 1), "frac_hbm": round(alg / us / 1e3 / HBM_PEAK_GBPS, 4),
            "fused_with_compress": {"entry": "ct_rtn_quant_pack_w4 (observer + quantize + pack in one pass)", "alg_bytes": alg_f, "us": round(us_f, 2),
                                    "GBps": round(alg_f / us_f / 1e3, 1), "frac_hbm": round(alg_f / us_f / 1e3 / HBM_PEAK_GBPS, 4)}}


def pack_unpack_leg(dev):
    """R1 / R2 unfused: pack_to_int32 / unpack_from_int32 (4 bits) on 8192x8192 int8 codes through the C ABI:
    N^2 + N^2 / 2 bytes per direction"""
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    K = 16  # the smallest stream (the packed words, 33.5 MB each) must exceed 2 x the 256 MiB Infinity Cache: HBM-cold
    g = torch.Generator(device=dev).manual_seed(19)
    q = [torch.randint(-8, 8, (N, N), dtype=torch.int8, device=dev, generator=g) for _ in range(K)]
    pk = [torch.empty(N, N // 8, dtype=torch.int32, device=dev) for _ in range(K)]
    back = [torch.empty(N, N, dtype=torch.int8, device=dev) for _ in range(K)]
    pack = lambda i: lib.ct_pack_int32(q[i % K].data_ptr(), N, N, BITS, pk[i % K].data_ptr(), N // 8, stream)
    unpack = lambda i: lib.ct_unpack_int32(pk[i % K].data_ptr(), N, N // 8, N // 8, N, BITS, back[i % K].data_ptr(), stream)
    for i in range(K):
        pack(i)
    alg = N * N + N * N // 2
    us_p, us_u = time_kernel(pack, 36), time_kernel(unpack, 36, offset=3)
    ok = all(torch.equal(a, b) for a, b in zip(q, back))
    return {"workload": f"pack_to_int32 / unpack_from_int32, int4, {N}x{N} int8 codes", "alg_bytes_per_direction": alg,
            "pack_us": round(us_p, 2), "pack_frac_hbm": round(alg / us_p / 1e3 / HBM_PEAK_GBPS, 4),
            "unpack_us": round(us_u, 2), "unpack_frac_hbm": round(alg / us_u / 1e3 / HBM_PEAK_GBPS, 4), "round_trip_bit_exact": bool(ok)}


def float_formats_leg(dev):
    """the float formats at 8192x8192 bf16 through the C ABI, HBM-cold rotation.
    float-quantized (float8_e4m3fn, channel scales): 2 + 1 B/element; nvfp4 (group 16, float32 scales in, fp8 scales
    stored): 2 + 0.5 + 4/16 resp. 1/16; mxfp4 (group 32, bf16 scales in, E8M0 stored): 2 + 0.5 + 2/32 resp. 1/32."""
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    BF16, F32, F8 = _lib.BF16, _lib.F32, _lib.F8
    nsets = 12  # 12 x 134 MB of weights per format: HBM-cold
    g = torch.Generator(device=dev).manual_seed(17)
    ws = [torch.randn(N, N, dtype=torch.bfloat16, device=dev, generator=g) for _ in range(nsets)]
    out = {}

    def rate(alg, us):
        return {"us": round(us, 2), "GBps": round(alg / us / 1e3, 1), "frac_hbm": round(alg / us / 1e3 / HBM_PEAK_GBPS, 4)}

    # float8_e4m3fn, per-channel
    sc = [(w.abs().amax(dim=1, keepdim=True).float() / 448.0).to(torch.bfloat16) for w in ws]
    q8 = [torch.empty(N, N, dtype=torch.uint8, device=dev) for _ in range(nsets)]
    back = torch.empty(N, N, dtype=torch.bfloat16, device=dev)
    fq = lambda i: lib.ct_quantize_fp8(ws[i % nsets].data_ptr(), BF16, sc[i % nsets].data_ptr(), BF16, None, -1, N, N, 1, N, 1, None, BF16,
                                       q8[i % nsets].data_ptr(), F8, stream)
    fd = lambda i: lib.ct_dequantize(q8[i % nsets].data_ptr(), F8, sc[i % nsets].data_ptr(), BF16, None, -1, N, N, 1, N, 1, None, back.data_ptr(), BF16, stream)
    for i in range(nsets):
        fq(i)
    alg = 3 * N * N + 2 * N
    out["float8_channel"] = {"alg_bytes_per_direction": alg, "quantize": rate(alg, time_kernel(fq, 36)), "dequantize": rate(alg, time_kernel(fd, 36, offset=6))}
    rc = lambda i: lib.ct_rtn_quant_channel8(ws[i % nsets].data_ptr(), BF16, N, N, 1, 1, q8[i % nsets].data_ptr(), sc[i % nsets].data_ptr(), None, stream)
    out["float8_channel"]["rtn_one_pass"] = rate(alg, time_kernel(rc, 36))  # observer + scale + quantize in one pass over the weight
    # float8_e4m3fn, block 128 x 128 (the FP8-block checkpoints' strategy, forward.py:198-216): scale[r // 128][c // 128]
    B = 128
    sb = [(w.view(N // B, B, N // B, B).abs().amax(dim=(1, 3)).float() / 448.0).to(torch.bfloat16).contiguous() for w in ws]
    bq = lambda i: lib.ct_quantize_fp8(ws[i % nsets].data_ptr(), BF16, sb[i % nsets].data_ptr(), BF16, None, -1, N, N, B, B, N // B, None, BF16,
                                       q8[i % nsets].data_ptr(), F8, stream)
    bd = lambda i: lib.ct_dequantize(q8[i % nsets].data_ptr(), F8, sb[i % nsets].data_ptr(), BF16, None, -1, N, N, B, B, N // B, None, back.data_ptr(), BF16, stream)
    for i in range(nsets):
        bq(i)
    alg_b = 3 * N * N + 2 * (N // B) * (N // B)
    out["float8_block128"] = {"alg_bytes_per_direction": alg_b, "quantize": rate(alg_b, time_kernel(bq, 36)), "dequantize": rate(alg_b, time_kernel(bd, 36, offset=6))}
    del q8, sb
    # FP4
    p4 = [torch.empty(N, N // 2, dtype=torch.uint8, device=dev) for _ in range(nsets)]
    for name, group, sdt, sbytes_in in (("nvfp4", 16, torch.float32, 4), ("mxfp4", 32, torch.bfloat16, 2)):
        if name == "nvfp4":
            gs = torch.tensor([448.0 * 6.0 / 6.0], dtype=torch.float32, device=dev)
            ss = [(w.view(N, N // group, group).abs().amax(-1).float() * gs / 6.0).to(torch.float8_e4m3fn).float().clamp_(min=2.0 ** -9) for w in ws]
            stored = [s.to(torch.float8_e4m3fn).view(torch.uint8) for s in ss]
            gptr, kind = gs.data_ptr(), 1
        else:
            ss = [torch.exp2(torch.floor(torch.log2(w.view(N, N // group, group).abs().amax(-1).float().clamp_(min=1e-6))) - 2).to(torch.bfloat16) for w in ws]
            stored = [(127 + torch.floor(torch.log2(s.float()))).to(torch.uint8) for s in ss]
            gptr, kind = None, 2
        code = _lib.DT[sdt]
        cq = lambda i: lib.ct_fp4_quant_pack(ws[i % nsets].data_ptr(), BF16, ss[i % nsets].data_ptr(), code, gptr, N, N, group, p4[i % nsets].data_ptr(), stream)
        cd = lambda i: lib.ct_fp4_unpack_dequant(p4[i % nsets].data_ptr(), N, N, stored[i % nsets].data_ptr(), kind, -1, gptr, group, back.data_ptr(), BF16, stream)
        for i in range(nsets):
            cq(i)
        alg_c = int(N * N * (2.5 + sbytes_in / group))
        alg_d = int(N * N * (2.5 + 1.0 / group))
        out[name] = {"alg_bytes_compress": alg_c, "alg_bytes_decompress": alg_d, "compress": rate(alg_c, time_kernel(cq, 36)),
                     "decompress": rate(alg_d, time_kernel(cd, 36, offset=6))}
        del ss, stored
    # observer + E8M0 scale + quantize + pack in one pass (ct_rtn_mxfp4_quant_pack)
    codes = torch.empty(N, N // 32, dtype=torch.uint8, device=dev)
    rq = lambda i: lib.ct_rtn_mxfp4_quant_pack(ws[i % nsets].data_ptr(), BF16, N, N, p4[i % nsets].data_ptr(), codes.data_ptr(), None, stream)
    alg_r = int(N * N * (2.5 + 1.0 / 32))
    out["mxfp4_rtn_one_pass"] = dict(alg_bytes=alg_r, **rate(alg_r, time_kernel(rq, 36)))
    gs1 = torch.tensor([448.0], dtype=torch.float32, device=dev)
    s8 = torch.empty(N, N // 16, dtype=torch.uint8, device=dev)
    nq = lambda i: lib.ct_rtn_nvfp4_quant_pack(ws[i % nsets].data_ptr(), BF16, N, N, gs1.data_ptr(), p4[i % nsets].data_ptr(), s8.data_ptr(), None, stream)
    alg_n = int(N * N * (2.5 + 1.0 / 16))
    out["nvfp4_rtn_one_pass_given_global_scale"] = dict(alg_bytes=alg_n, **rate(alg_n, time_kernel(nq, 36)))
    out["workload"] = f"float-quantized (float8_e4m3fn, channel), nvfp4- and mxfp4-pack-quantized weight paths, {N}x{N} bf16, C ABI"
    return out


def roofline_rows(result):
    """one {kernel, config, alg_bytes, us, GBps, frac} row per extra leg, appended to roofline.kernels (the driver keeps `roofline` whole)"""
    rows = []

    def row(kernel, config, alg, us, **kw):
        if us:
            rows.append(dict(kernel=kernel, config=config, alg_bytes=int(alg), us=round(us, 2), GBps=round(alg / us / 1e3, 1), frac=round(alg / us / 1e3 / HBM_PEAK_GBPS, 4), **kw))

    def leg(key):
        v = result.get(key)
        return v if isinstance(v, dict) and "error" not in v else None

    b = leg("bitmask")
    if b:
        row("bitmask_decompress16_kernel", "sparse-bitmask 50 % 8192x8192 bf16 (config 3), decompress", b["alg_bytes"], b["decompress_us"], bit_exact=b["round_trip_bit_exact"])
        row("flat16_resident_kernel", "sparse-bitmask 50 % 8192x8192 bf16 (config 3), compress", b["alg_bytes"], b["compress_us"], bit_exact=b["round_trip_bit_exact"])
        if "api_compress_us" in b:
            row("BitmaskTensor.from_dense", "config 3 through the plug-in class, wall time per call (allocations + host wait for nnz); EXACT-size values (default)",
                b["alg_bytes"], b["api_compress_us"], bit_exact=b["api_bit_exact"], values_storage_bytes=b.get("api_compress_values_storage_bytes"))
            if "api_compress_view_us" in b:
                row("BitmaskTensor.from_dense(exact=False)", "config 3 through the plug-in class; values are a VIEW of a dense-sized buffer (no copy, pins numel x 2 bytes)",
                    b["alg_bytes"], b["api_compress_view_us"], bit_exact=b["api_bit_exact"], values_storage_bytes=b.get("api_compress_view_values_storage_bytes"))
            row("BitmaskTensor.decompress", "config 3 through the plug-in class, wall time per call", b["alg_bytes"], b["api_decompress_us"], bit_exact=b["api_bit_exact"])
        if "s24_compress_us" in b:
            row("sparse24_pair_kernel", "sparse-24-bitmask 8192x8192 bf16, compress", b["s24_alg_bytes"], b["s24_compress_us"], bit_exact=b["s24_bit_exact"])
            row("bitmask_decompress16_kernel<2:4 rows>", "sparse-24-bitmask 8192x8192 bf16, decompress", b["s24_alg_bytes"], b["s24_decompress_us"], bit_exact=b["s24_bit_exact"])
        if "f32_compress_us" in b:
            row("flat16_resident_kernel<float32 as pairs of halves>", "sparse-bitmask 50 % 8192x8192 float32, compress", b["f32_alg_bytes"], b["f32_compress_us"], bit_exact=b["f32_bit_exact"])
            row("bitmask_decompress16_kernel<float32 as pairs of halves>", "sparse-bitmask 50 % 8192x8192 float32, decompress", b["f32_alg_bytes"], b["f32_decompress_us"], bit_exact=b["f32_bit_exact"])
        if "i8_compress_us" in b:
            row("flat16_resident_kernel<8-bit payloads, row form>", "sparse-bitmask 50 % 8192x8192 int8 / fp8 bytes, compress", b["i8_alg_bytes"], b["i8_compress_us"], bit_exact=b["i8_bit_exact"])
            row("bitmask_decompress8_kernel<8-bit payloads>", "sparse-bitmask 50 % 8192x8192 int8 / fp8 bytes, decompress", b["i8_alg_bytes"], b["i8_decompress_us"], bit_exact=b["i8_bit_exact"])
    k4 = leg("kernels_4096")
    if k4:
        pb = k4.get("pair_batch") or {}
        pc = dict(pair_us=pb["compress_us"], pair_frac=pb["compress_frac_hbm"]) if pb else {}
        pd = dict(pair_us=pb["decompress_us"], pair_frac=pb["decompress_frac_hbm"]) if pb else {}
        row("w4_quant_pack_lean_kernel<bf16>", "W4A16 g128 4096x4096 bf16, compress", k4["alg_bytes_per_direction"], k4["compress_us"], **pc)
        row("w4_unpack_dequant_kernel<bf16>", "W4A16 g128 4096x4096 bf16, decompress", k4["alg_bytes_per_direction"], k4["decompress_us"], **pd)
    ko = leg("kernels_other") or {}
    for key in ("fp16_8192", "bf16_8192_asymmetric", "bf16_8192_actorder", "bf16_4096x28672_actorder"):
        v = ko.get(key)
        if isinstance(v, dict):
            shape = "4096x28672" if "28672" in key else "8192x8192"
            row("w4 compress", f"W4A16 g128 {shape} {key}", v["alg_bytes_per_direction"], v["compress_us"])
            row("w4 decompress", f"W4A16 g128 {shape} {key}", v["alg_bytes_per_direction"], v["decompress_us"])
    ow = leg("other_widths") or {}
    for b_ in (3, 2, 6):
        v = ow.get(f"w{b_}")
        if isinstance(v, dict):
            row(f"wb_quant_pack_lean_kernel<bf16, {b_}>", f"W{b_}A16 g128 8192x8192 bf16, compress", v["alg_bytes_per_direction"], v["compress_us"], bit_exact=v["bit_exact_vs_oracle_slice"])
            row(f"wb_unpack_dequant_kernel<bf16, {b_}>", f"W{b_}A16 g128 8192x8192 bf16, decompress", v["alg_bytes_per_direction"], v["decompress_us"], bit_exact=v["bit_exact_vs_oracle_slice"])
    i8 = leg("int8_per_tensor")
    if i8:
        row("q8_quant_kernel", "int8 per-tensor 4096x4096 bf16 (config 1), quantize", i8["alg_bytes_per_direction"], i8["quantize_us"])
        row("q8_dequant_kernel", "int8 per-tensor 4096x4096 bf16 (config 1), dequantize", i8["alg_bytes_per_direction"], i8["dequantize_us"])
    m = leg("marlin24")
    if m:
        row("marlin24_fused_w4_lean_kernel", "marlin-24 2:4 + int4 g128 8192x8192 bf16 (config 4), kernel", m["alg_bytes"], m["kernels_us"], bit_exact=m["bit_exact_vs_oracle"])
        row("Marlin24Compressor.compress (default: the call raises the 2:4 ValueError)", "config 4 through the plug-in class, wall time per call",
            m["alg_bytes"], m["compress_us_default"], bit_exact=m["bit_exact_vs_oracle"], deferred_check_us=m["compress_us_deferred_check"])
        row("Marlin24Compressor.compress (deferred_structure_check)", "config 4 through the plug-in class inside the batch context", m["alg_bytes"],
            m["compress_us_deferred_check"], bit_exact=m["bit_exact_vs_oracle"])
    t = leg("tinyllama_checkpoint")
    if t:
        row("w4_*_batch_kernel x 2", "TinyLlama-1.1B-shaped W4A16 checkpoint (config 5), C ABI", t["alg_bytes_all_ranks"], t["ms_whole_checkpoint"] * 1e3)
        a = t.get("api") or {}
        if a.get("ms_both"):
            row("ModelCompressor.compress_model + decompress_model", "config 5 through the drop-in API (154-module tree), wall time", t["alg_bytes_all_ranks"], a["ms_both"] * 1e3,
                api_over_kernels=a["api_over_kernels"])
        aa = a.get("asymmetric") or {}
        if aa.get("ms_both"):
            row("ModelCompressor.compress_model + decompress_model (asymmetric scheme)", "config 5 with int8 zero points stored packed, drop-in API, wall time",
                t["alg_bytes_all_ranks"], aa["ms_both"] * 1e3, api_over_kernels=aa["api_over_kernels"])
    l8 = leg("llama8b_checkpoint")
    if l8:
        row("w4_*_batch_kernel x 2 (8B)", "Llama-3-8B-shaped W4A16 checkpoint (224 modules, 13.96 GB bf16), C ABI", l8["alg_bytes"], l8["ms_kernels_only"] * 1e3)
        row("ModelCompressor.compress_model + decompress_model (8B)", "the same checkpoint through the drop-in API (224-module tree), wall time", l8["alg_bytes"],
            l8["ms_model_compressor"] * 1e3, api_over_kernels=l8["api_over_kernels"], bit_exact=l8["round_trip_equals_fake_quantize"])
    q = leg("minmax_qparams")
    if q:
        row("qparams_absmax_kernel", "min-max observer int4 g128 8192x8192 bf16", q["alg_bytes"], q["us"])
        row("rtn_w4_kernel", "observer + quantize + pack in one pass", q["fused_with_compress"]["alg_bytes"], q["fused_with_compress"]["us"])
    pu = leg("pack_unpack")
    if pu:
        row("pack_flat4_kernel", "pack_to_int32 b=4 8192x8192 int8", pu["alg_bytes_per_direction"], pu["pack_us"])
        row("unpack_flat4_kernel", "unpack_from_int32 b=4 8192x8192", pu["alg_bytes_per_direction"], pu["unpack_us"])
    return rows


LINE_CAP = 6000  # characters: the driver's record keeps the last 8081 of stdout, and the final line must sit inside that whole
DETAILS_FILE = "bench_details.json"

# short names for the rows roofline_rows() builds (kernel text, config text): the final line carries at most 18 of them
_HEADLINE_ROWS = (
    ("bitmask_decompress16_kernel", "(config 3), decompress", "cfg3 sparse-bitmask 50% 8192^2 bf16, decompress"),
    ("flat16_resident_kernel", "(config 3), compress", "cfg3 sparse-bitmask 50% 8192^2 bf16, compress"),
    ("BitmaskTensor.from_dense", "EXACT", "cfg3 via the plug-in class, exact-size values (default), wall/call"),
    ("BitmaskTensor.from_dense(exact=False)", "", "cfg3 via the plug-in class, values = view of a dense-sized buffer, wall/call"),
    ("marlin24_fused_w4_lean_kernel", "", "cfg4 marlin-24 2:4+int4 g128 8192^2 bf16, kernel"),
    ("Marlin24Compressor.compress (default", "", "cfg4 via the plug-in class (call raises the 2:4 ValueError), wall/call"),
    ("w4_*_batch_kernel x 2", "", "cfg5 TinyLlama-1.1B-shaped W4A16 checkpoint, C ABI"),
    ("ModelCompressor.compress_model + decompress_model", "drop-in API (154-module tree)", "cfg5 via ModelCompressor (154 modules), wall"),
    ("ModelCompressor.compress_model + decompress_model (asymmetric", "", "cfg5 asymmetric (packed zero points) via ModelCompressor, wall"),
    ("ModelCompressor.compress_model + decompress_model (8B)", "", "Llama-3-8B-shaped W4A16 checkpoint (224 modules, 14 GB) via ModelCompressor, wall"),
    ("w4_quant_pack_lean_kernel<bf16>", "4096x4096 bf16, compress", "W4A16 g128 4096^2 bf16, compress"),
    ("w4_unpack_dequant_kernel<bf16>", "4096x4096 bf16, decompress", "W4A16 g128 4096^2 bf16, decompress"),
    ("wb_quant_pack_lean_kernel<bf16, 3>", "", "W3A16 g128 8192^2 bf16, compress"),
    ("wb_unpack_dequant_kernel<bf16, 3>", "", "W3A16 g128 8192^2 bf16, decompress"),
    ("q8_quant_kernel", "", "cfg1 int8 per-tensor 4096^2 bf16, quantize"),
    ("q8_dequant_kernel", "", "cfg1 int8 per-tensor 4096^2 bf16, dequantize"),
)


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def headline_line(result, cap=LINE_CAP):
    """The ONE line the driver parses: the contract keys, `config`, `roofline` (with <= 17 kernel rows) and `cpu_baseline`, serialised
    in at most `cap` characters.  Everything else bench.py measures (per-dtype quantize legs, float formats, W8A8, thread sweeps, the
    restatement / port baselines, per-leg detail) stays in the full result, which main() writes to bench_details.json and to stderr.
    A plain run's result (no `roofline`; no details file) gives the contract keys and `config` alone.
    tests/test_bench_line.py feeds recorded results through this function and holds it to the cap and to the key list."""
    line = _pick(result, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype", "data"))
    line["vs_baseline"] = result.get("vs_baseline")
    line["config"] = _pick(result.get("config", {}), ("workload", "alg_bytes_per_step_per_gpu", "buffers", "boundary", "streams", "parallelism",
                                                       "value_one_stream", "ranks_seen", "per_rank_GBps"))
    if "roofline" not in result:
        return json.dumps(line, separators=(",", ":"))
    r = result["roofline"]
    roof = _pick(r, ("bound", "kernel", "achieved", "peak", "unit", "frac"))
    roof["traffic"] = r.get("traffic")
    roof.update(_pick(r, ("alg_bytes_per_launch", "traffic_source")))
    roof["step"] = _pick(r.get("step", {}), ("value_two_streams", "value_one_stream", "frac_two_streams", "frac_one_stream", "ms_per_step_blocks",
                                             "ms_per_step_without_device_warmup"))
    rows_in = r.get("kernels", [])
    rows = [_pick(x, ("kernel", "config", "alg_bytes", "us", "min_us", "GBps", "frac", "valu_busy_frac")) for x in rows_in[:2]]  # the headline kernels
    for x in rows:  # (say in the row itself that this one figure is not measured in the run)
        if "valu_busy_frac" in x:
            x["valu_busy_src"] = "committed SQ counter pass, not live"
    line["value_note"] = "value: the step's two launches on two HIP streams; value_one_stream is the figure comparable with roofline.frac"
    for kernel, cfg_part, short in _HEADLINE_ROWS:
        hit = [x for x in rows_in[2:] if x.get("kernel", "").startswith(kernel) and cfg_part in x.get("config", "")]
        if kernel.endswith("decompress_model"):  # the symmetric row: its name is a prefix of the asymmetric one's
            hit = [x for x in hit if "asymmetric" not in x["kernel"]]
        if hit:
            row = _pick(hit[0], ("alg_bytes", "us", "GBps", "frac", "bit_exact", "api_over_kernels", "deferred_check_us", "pair_us", "pair_frac", "values_storage_bytes"))
            rows.append({"kernel": kernel.split(" (")[0], "config": short, **row})
    roof["kernels"] = rows
    line["roofline"] = roof
    c = result.get("cpu_baseline")
    if isinstance(c, dict):
        cb = _pick(c, ("value", "unit", "cores", "host_cores", "kind"))
        cb["impl"] = "reference PackedQuantizationCompressor.compress/.decompress (pack_quantized/base.py:62-163), CPU tensors, staged by oracle/stage_ref.py" \
            if c.get("kind") == "reference" else str(c.get("impl", ""))[:160]
        cb["sample"] = str(c.get("sample", ""))[:170]
        cb.update(_pick(c, ("compress_s", "decompress_s", "gpu_bit_exact_vs_oracle")))
        cb["median_s"] = {k: v for k, v in (c.get("median_s") or {}).items() if k.startswith("reference_")}
        line["cpu_baseline"] = cb
    line.update(_pick(result, ("host_path", "parity_gate", "oracle_slice_check")))
    t = result.get("tinyllama_checkpoint")
    if isinstance(t, dict) and result.get("n_gpus", 1) > 1:  # N > 1: the sharded legs in brief (at N = 1 they are rows above)
        line["tinyllama_checkpoint"] = _pick(t, ("modules_this_rank", "modules_per_rank", "every_module_on_exactly_one_rank", "alg_bytes_all_ranks", "ms_whole_checkpoint",
                                                 "GBps", "frac_of_hbm_peak_per_gpu", "rotating_copies", "round_trip_equals_fake_quantize", "error"))
    rs = result.get("row_sharded")
    if isinstance(rs, dict):
        line["row_sharded"] = {**_pick(rs, ("ranks", "rows_this_rank", "error")),
                               **{k: _pick(v, ("us_per_tensor", "GBps_all_ranks", "frac_of_hbm_peak_per_gpu", "us_per_tensor_hip_graph", "sets", "shard_equals_slice_of_single_rank_result"))
                                  for k, v in rs.items() if isinstance(v, dict)}}
    w4k = result.get("w4a16_4096")
    if isinstance(w4k, dict):
        line["w4a16_4096"] = _pick(w4k, ("us_per_step", "GBps_all_ranks", "frac_of_hbm_peak_per_gpu", "us_per_step_hip_graph", "frac_of_hbm_peak_per_gpu_hip_graph", "ranks",
                                         "round_trip_equals_fake_quantize", "error"))
    line["details"] = DETAILS_FILE
    text = json.dumps(line, separators=(",", ":"))
    while len(text) > cap and len(roof["kernels"]) > 2:  # never expected (the test holds recorded results to the cap): shed rows, not the contract
        roof["kernels"].pop()
        text = json.dumps(line, separators=(",", ":"))
    if len(text) > cap:
        raise RuntimeError(f"bench.py's final line is {len(text)} characters (cap {cap})")
    return text


TINYLLAMA_LAYER = (("q_proj", 2048, 2048), ("k_proj", 256, 2048), ("v_proj", 256, 2048), ("o_proj", 2048, 2048),
                   ("gate_proj", 5632, 2048), ("up_proj", 5632, 2048), ("down_proj", 2048, 5632))


def tinyllama_leg(dev, rank, world, barrier, allreduce_max, allreduce_sum_vec=None):
    """BASELINE config 5: every Linear of a TinyLlama-1.1B-shaped checkpoint (22 layers x 7 = 154
    modules, 968,884,224 weights, synthetic) W4A16 g128 compressed then decompressed; the modules are
    split over the ranks with the reference's LPT rule (distributed/assign.py:33-42) and no rank ever
    exchanges data.  Timed region: this rank's launches through the C ABI, max over ranks."""
    from compressed_tensors_amd import _lib, codec
    from compressed_tensors_amd.distributed.shard import shard_items

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    BF16 = _lib.BF16
    mods = [(f"model.layers.{l}.{name}", r, c) for l in range(22) for (name, r, c) in TINYLLAMA_LAYER]
    mine = shard_items(mods, weight_fn=lambda m: m[1] * m[2] * 2, rank=rank, world_size=world)
    g = torch.Generator(device=dev).manual_seed(100 + rank)
    cargs, dargs, keep = [], [], []
    my_bytes = 0
    for _, r, c in mine:
        w = torch.randn(r, c, dtype=torch.bfloat16, device=dev, generator=g)
        scale, zp = codec.minmax_qparams(w, num_bits=BITS, group_size=GROUP, symmetric=True)
        packed = torch.empty(r, c // 8, dtype=torch.int32, device=dev)
        out = torch.empty_like(w)
        keep.append((w, scale, zp, packed, out))
        cargs.append((w.data_ptr(), BF16, scale.data_ptr(), BF16, zp.data_ptr(), _lib.I8, r, c, 1, GROUP, c // GROUP, None, BITS, BF16, packed.data_ptr(), stream))
        dargs.append((packed.data_ptr(), r, c // 8, c, BITS, scale.data_ptr(), BF16, None, -1, 1, GROUP, c // GROUP, None, out.data_ptr(), BF16, stream))
        my_bytes += 2 * (2 * r * c + 2 * r * (c // GROUP) + r * c // 2)

    def per_module():
        for a in cargs:
            lib.ct_quant_pack(*a)
        for a in dargs:
            lib.ct_unpack_dequant(*a)

    # the product path (ModelCompressor -> PackedQuantizationCompressor.compress_modules): ONE launch per
    # direction over the shard's module table
    cb = codec.W4Batch([(w, s, z, p, w.shape[0], w.shape[1], GROUP) for (w, s, z, p, o) in keep], "compress", torch.bfloat16)
    db = codec.W4Batch([(p, s, None, o, w.shape[0], w.shape[1], GROUP) for (w, s, z, p, o) in keep], "decompress", torch.bfloat16)

    def batched():
        cb.launch(stream)
        db.launch(stream)

    def timed(fn, passes=1):
        fn()
        best = None
        for _ in range(5):
            barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(passes):
                fn()
            torch.cuda.synchronize()
            dt = allreduce_max(time.perf_counter() - t0) / passes
            best = dt if best is None else min(best, dt)
        return best

    t_loop = timed(per_module)
    for (w, s, z, p, o) in keep:
        p.zero_(); o.zero_()
    best = timed(batched)
    # Round 6 (N > 1): a rank's share of the checkpoint shrinks with the world size (75 MB of distinct bytes per pass at 8 ranks) — one
    # pass is then ~0.1 ms between two barriers and a repeat would be served by the 256 MiB Infinity Cache.  The figure REPORTED at
    # N > 1 therefore comes from `world` copies of the rank's shard (different weights, their own tables) processed back to back per timed
    # block: >= 600 MB of distinct bytes per rotation at any world size (HBM-cold), `world` passes per barrier pair.
    rot = None
    if world > 1:
        copies = []
        for _ in range(world):
            kc = []
            for _, r, c in mine:
                w = torch.randn(r, c, dtype=torch.bfloat16, device=dev, generator=g)
                sc_, zp_ = codec.minmax_qparams(w, num_bits=BITS, group_size=GROUP, symmetric=True)
                kc.append((w, sc_, zp_, torch.empty(r, c // 8, dtype=torch.int32, device=dev), torch.empty_like(w)))
            copies.append((kc, codec.W4Batch([(w, s, z, p, w.shape[0], w.shape[1], GROUP) for (w, s, z, p, o) in kc], "compress", torch.bfloat16),
                           codec.W4Batch([(p, s, None, o, w.shape[0], w.shape[1], GROUP) for (w, s, z, p, o) in kc], "decompress", torch.bfloat16)))
        turn = [0]

        def rotating():
            _, c_, d_ = copies[turn[0] % world]
            turn[0] += 1
            c_.launch(stream)
            d_.launch(stream)

        for _ in range(world):
            rotating()
        rot = timed(rotating, passes=world)
        kc0 = copies[0][0]
        rot_ok = all(torch.equal(kc[0][4], codec.fake_quantize_tensor(kc[0][0], kc[0][1], kc[0][2], num_bits=BITS, strategy="group", group_size=GROUP)) for kc, _, _ in copies)
        del copies, kc0
        torch.cuda.empty_cache()
    # the same checkpoint with an ASYMMETRIC scheme (W4A16_ASYM: int8 zero points, stored packed along rows): one launch per
    # direction instead of two per module
    asym = []
    for (w, _, _, p, o) in keep:
        sa, za = codec.minmax_qparams(w, num_bits=BITS, group_size=GROUP, symmetric=False)
        asym.append((sa, za, torch.empty((-(-w.shape[0] * 4 // 32), za.shape[1]), dtype=torch.int32, device=dev), torch.empty_like(za)))
    # round 6: ONE launch per direction — the compress launch's tail workgroups write the stored (packed) zero points, the decompress launch reads
    # them in that form and writes the unpacked int8 back (ct_w4_item.zp_packed); rounds 2-5 ran ct_zp4_pack_dim0_batch twice beside them
    cba = codec.W4Batch([(w, sa, za, p, w.shape[0], w.shape[1], GROUP, zp_) for (w, _, _, p, _), (sa, za, zp_, _) in zip(keep, asym)], "compress", torch.bfloat16)
    dba = codec.W4Batch([(p, sa, zu, o, w.shape[0], w.shape[1], GROUP, zp_) for (w, _, _, p, o), (sa, _, zp_, zu) in zip(keep, asym)], "decompress", torch.bfloat16)

    def batched_asym():
        cba.launch(stream)
        dba.launch(stream)

    t_asym = timed(batched_asym)
    wa0, (sa0, za0, _, zu0) = keep[0][0], asym[0]
    asym_ok = bool(torch.equal(zu0, za0) and torch.equal(asym[0][2], codec.pack_to_int32(za0, BITS, packed_dim=0))
                   and torch.equal(keep[0][4], codec.fake_quantize_tensor(wa0, sa0, za0, num_bits=BITS, strategy="group", group_size=GROUP)))
    batched()  # leave the symmetric results in the buffers for the check below
    total_bytes = sum(2 * (2 * r * c + 2 * r * (c // GROUP) + r * c // 2) for _, r, c in mods)
    w0, s0, z0, p0, o0 = keep[0]
    fq = codec.fake_quantize_tensor(w0, s0, z0, num_bits=BITS, strategy="group", group_size=GROUP)
    api = {}
    if world == 1:  # the drop-in API on the same checkpoint (VERDICT r03 missing #3): a module TREE through ModelCompressor
        try:
            api = tinyllama_api_leg(dev, mine, keep, best, fq)
        except Exception as e:
            api = {"error": repr(e)}
        try:  # the same tree with the asymmetric scheme: its zero points ride a second table per direction (the C++ host loop takes these too)
            fqa = codec.fake_quantize_tensor(wa0, sa0, za0, num_bits=BITS, strategy="group", group_size=GROUP)
            a2 = tinyllama_api_leg(dev, mine, [(w, sa, za, None, None) for (w, _, _, _, _), (sa, za, _, _) in zip(keep, asym)], t_asym, fqa, symmetric=False)
            api["asymmetric"] = {k: a2[k] for k in ("ms_both", "ms_both_min_max", "ms_host_until_compress_model_returns", "ms_host_until_decompress_model_returns",
                                                    "ms_kernels_only", "api_over_kernels", "round_trip_equals_fake_quantize")}
        except Exception as e:
            api["asymmetric"] = {"error": repr(e)}
    # which rank took which module: every one of the 154 exactly once (summed over the ranks as they actually ran, not recomputed)
    cover = {}
    if allreduce_sum_vec is not None:
        index = {m[0]: i for i, m in enumerate(mods)}
        marks = [0.0] * len(mods)
        for m in mine:
            marks[index[m[0]]] += 1.0
        counts = [0.0] * world
        counts[rank] = float(len(mine))
        total_marks, per_rank = allreduce_sum_vec(marks), allreduce_sum_vec(counts)
        cover = {"modules_per_rank": [int(v) for v in per_rank], "every_module_on_exactly_one_rank": bool(all(v == 1.0 for v in total_marks))}
    single_pass = best
    if rot is not None:
        best = rot
        cover.update({"ms_whole_checkpoint_single_pass": round(single_pass * 1e3, 4), "rotating_copies": world,
                      "cache": f"HBM-cold: {world} copies of the rank's shard per timed block (>= 600 MB of distinct bytes per rotation)",
                      "rotating_round_trip_equals_fake_quantize": bool(rot_ok)})
    return {"api": api, "workload": "TinyLlama-1.1B-shaped checkpoint (154 Linear modules, 1.94 GB bf16), W4A16 g128 compress + decompress, "
                        f"LPT module shards over {world} rank(s), no collectives",
            "modules_this_rank": len(mine), "alg_bytes_all_ranks": total_bytes, "rank0_share_of_bytes": round(my_bytes / total_bytes, 4), **cover,
            "launches": "one ct_quant_pack_batch + one ct_unpack_dequant_batch per rank",
            "ms_whole_checkpoint": round(best * 1e3, 4), "GBps": round(total_bytes / best / 1e9, 1),
            "ms_whole_checkpoint_one_launch_per_module": round(t_loop * 1e3, 4),
            "ms_whole_checkpoint_asymmetric": round(t_asym * 1e3, 4), "asymmetric_round_trip_equals_fake_quantize": asym_ok,
            "frac_of_hbm_peak_per_gpu": round(total_bytes / best / 1e9 / world / HBM_PEAK_GBPS, 4),
            "round_trip_equals_fake_quantize": bool(torch.equal(o0, fq))}


def tinyllama_module_tree(mine, keep, scheme):
    """a TinyLlama-shaped nn.Module tree (model.layers[L].{q,k,v,o,gate,up,down}_proj: 154 Linear modules) over the tensors of the
    C-ABI leg, with the scheme attached the way upstream's apply_quantization_config does it: ONE scheme object per config group
    (quantization/lifecycle/apply.py:156-165) and weight_scale / weight_zero_point as non-trainable parameters"""
    root = torch.nn.Module()
    root.layers = torch.nn.ModuleList()
    root.first_linear = []  # (a plain list: not a child module) the Linear built over keep[0], for the round-trip check
    blocks = {}
    for (name, r, c), (w, s_, z, _, _) in zip(mine, keep):
        parts = name.split(".")
        layer, proj = int(parts[2]), parts[3]
        blk = blocks.get(layer)
        if blk is None:
            blk = blocks[layer] = torch.nn.Module()
            root.layers.append(blk)
        lin = torch.nn.Linear(c, r, bias=False, device="meta")
        lin.weight = torch.nn.Parameter(w, requires_grad=False)
        lin.weight_scale = torch.nn.Parameter(s_, requires_grad=False)
        lin.weight_zero_point = torch.nn.Parameter(z, requires_grad=False)
        lin.quantization_scheme = scheme
        setattr(blk, proj, lin)
        if not root.first_linear:
            root.first_linear.append(lin)
    return root


def tinyllama_api_leg(dev, mine, keep, kernels_s, fq0, symmetric=True):
    """ModelCompressor().compress_model(model) + .decompress_model(model) on the 154-module tree: WALL time, weights resident in HBM,
    median of 7 cycles after 2 warm-up cycles (reference model_compressors/model_compressor.py:138-207, utils/module.py:33-65).
    Everything the drop-in does is inside the timed region: the module walk, the format resolution, the table build and its upload,
    the output allocations, the two launches and the per-module parameter replacement."""
    import compressed_tensors_amd as cta

    args = cta.QuantizationArgs(num_bits=BITS, group_size=GROUP, symmetric=symmetric, strategy="group")
    scheme = cta.QuantizationScheme(targets=["Linear"], weights=args)
    model = tinyllama_module_tree(mine, keep, scheme)
    mc = cta.ModelCompressor()

    def cycle():
        mc.compress_model(model)
        mc.decompress_model(model)

    cycle()
    first_lin = model.first_linear[0]
    ok = bool(torch.equal(first_lin.weight.data, fq0))  # the module over keep[0] (the shard list is in LPT order): round trip == fake_quantize
    cycle()
    both, comp, dec, host_c, host_d = [], [], [], [], []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cycle()
        torch.cuda.synchronize()
        both.append(time.perf_counter() - t0)
    for _ in range(7):  # each direction on its own (a synchronisation in between), and the host's share of it (time until the call returns)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mc.compress_model(model)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        mc.decompress_model(model)
        t3 = time.perf_counter()
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        comp.append(t2 - t0); host_c.append(t1 - t0); dec.append(t4 - t2); host_d.append(t3 - t2)
    n = len(keep)
    out = {"entry": "compressed_tensors_amd.ModelCompressor().compress_model(model) + .decompress_model(model), 154-module TinyLlama-shaped nn.Module tree",
           "modules": n, "ms_both": round(median(both) * 1e3, 4), "ms_both_min_max": [round(min(both) * 1e3, 4), round(max(both) * 1e3, 4)],
           "ms_compress_model": round(median(comp) * 1e3, 4), "ms_decompress_model": round(median(dec) * 1e3, 4),
           "ms_host_until_compress_model_returns": round(median(host_c) * 1e3, 4), "ms_host_until_decompress_model_returns": round(median(host_d) * 1e3, 4),
           "host_us_per_module_compress": round(median(host_c) / n * 1e6, 2), "host_us_per_module_decompress": round(median(host_d) / n * 1e6, 2),
           "ms_kernels_only": round(kernels_s * 1e3, 4), "api_over_kernels": round(median(both) / kernels_s, 3),
           "round_trip_equals_fake_quantize": ok, "timing": "wall clock, synchronize on both sides, median of 7 cycles after 2 warm-up cycles"}
    return out


LLAMA8B_LAYER = (("q_proj", 4096, 4096), ("k_proj", 1024, 4096), ("v_proj", 1024, 4096), ("o_proj", 4096, 4096),
                 ("gate_proj", 14336, 4096), ("up_proj", 14336, 4096), ("down_proj", 4096, 14336))


def llama8b_api_leg(dev):
    """What the plug-in API costs at a real checkpoint's scale: a Llama-3-8B-shaped tree (32 layers x 7 = 224 Linear modules, 6.98 G weights,
    13.96 GB bf16, synthetic), W4A16 g128, `ModelCompressor().compress_model(model)` + `.decompress_model(model)` — wall clock, median of 5
    cycles after 2 warm-up cycles — against the same two table launches through the C ABI into preallocated buffers.  The working set (14 GB in,
    3.5 GB packed, 14 GB out) is 60 x the Infinity Cache: HBM-cold without rotation.  TinyLlama's 154 modules are 1-23 MB each, so the ~3.5 us the
    host spends per module and direction shows (1.25-1.6 x the kernels); here a module is 8-117 MB."""
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import codec

    stream = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(808)
    mine, keep, alg = [], [], 0
    for layer in range(32):
        for (proj, r, c) in LLAMA8B_LAYER:
            w = torch.randn(r, c, dtype=torch.bfloat16, device=dev, generator=g)
            scale, zp = codec.minmax_qparams(w, num_bits=BITS, group_size=GROUP, symmetric=True)
            mine.append((f"model.layers.{layer}.{proj}", r, c))
            keep.append((w, scale, zp, torch.empty(r, c // 8, dtype=torch.int32, device=dev), torch.empty(r, c, dtype=torch.bfloat16, device=dev)))
            alg += 2 * (2 * r * c + 2 * r * (c // GROUP) + r * c // 2)
    cb = codec.W4Batch([(w, s_, z, p, w.shape[0], w.shape[1], GROUP) for (w, s_, z, p, o) in keep], "compress", torch.bfloat16)
    db = codec.W4Batch([(p, s_, None, o, w.shape[0], w.shape[1], GROUP) for (w, s_, z, p, o) in keep], "decompress", torch.bfloat16)

    def kernels():
        cb.launch(stream)
        db.launch(stream)

    kernels()
    torch.cuda.synchronize()
    w0, s0, z0, _, o0 = keep[0]
    fq0 = codec.fake_quantize_tensor(w0, s0, z0, num_bits=BITS, strategy="group", group_size=GROUP)
    ok_k = bool(torch.equal(o0, fq0))
    ks = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kernels()
        torch.cuda.synchronize()
        ks.append(time.perf_counter() - t0)
    kernels_s = median(ks)
    del cb, db
    keep = [(w, s_, z, None, None) for (w, s_, z, p, o) in keep]  # the class allocates its own outputs
    torch.cuda.empty_cache()
    args = cta.QuantizationArgs(num_bits=BITS, group_size=GROUP, symmetric=True, strategy="group")
    scheme = cta.QuantizationScheme(targets=["Linear"], weights=args)
    model = tinyllama_module_tree(mine, keep, scheme)
    mc = cta.ModelCompressor()

    def cycle():
        mc.compress_model(model)
        mc.decompress_model(model)

    cycle()
    ok = bool(torch.equal(model.first_linear[0].weight.data, fq0))
    cycle()
    both, host = [], []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cycle()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        both.append(time.perf_counter() - t0)
        host.append(t1 - t0)
    return {"workload": "Llama-3-8B-shaped checkpoint (224 Linear modules, 6.98 G weights, 13.96 GB bf16, synthetic), W4A16 g128 symmetric, compress + decompress",
            "alg_bytes": alg, "modules": len(mine),
            "ms_kernels_only": round(kernels_s * 1e3, 3), "kernels_frac_hbm": round(alg / kernels_s / 1e9 / HBM_PEAK_GBPS, 4),
            "ms_model_compressor": round(median(both) * 1e3, 3), "ms_model_compressor_min_max": [round(min(both) * 1e3, 3), round(max(both) * 1e3, 3)],
            "model_compressor_frac_hbm": round(alg / median(both) / 1e9 / HBM_PEAK_GBPS, 4), "api_over_kernels": round(median(both) / kernels_s, 3),
            "ms_host_until_both_calls_return": round(median(host) * 1e3, 3),
            "round_trip_equals_fake_quantize": ok and ok_k,
            "timing": "wall clock, synchronize on both sides, median of 5 cycles after 2 warm-up cycles; HBM-cold by size (31.5 GB working set)"}


def fp4_api_leg(dev):
    """The float-4 formats through the plug-in API at a real checkpoint's module sizes (round 6): 16 layers of a Llama-3-8B-shaped tree (112 Linear modules,
    3.49 G weights, 6.98 GB bf16, synthetic), NVFP4 (groups of 16, float8 scales under a global scale) and MXFP4 (groups of 32, E8M0 scales),
    `ModelCompressor().compress_model(model)` + `.decompress_model(model)` — wall clock, median of 5 cycles after 2 warm-up cycles, HBM-cold by size —
    beside the same modules' launches through the C ABI into preallocated outputs (`ct_fp4_quant_pack_stored` + `ct_fp4_unpack_dequant_scale`, ONE PER MODULE
    and direction — the class path itself goes through the C++ host loop and the FP4 table launches, `ct_fp4_quant_pack_batch` / `ct_fp4_unpack_dequant_batch`,
    and so ends up below the per-module launches' time).  alg bytes per element and direction: 2 + 0.5 + the stored scale (1/16 resp. 1/32 B)
    + the float scale read (4/16 resp. 2/32 B) resp. the bfloat16 scale written (2/16, 2/32 B)."""
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import _lib, codec

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    F8 = torch.float8_e4m3fn
    out = {"workload": "16 layers of a Llama-3-8B-shaped tree (112 Linear modules, 3.49 G weights, 6.98 GB bf16, synthetic), NVFP4 / MXFP4, compress + decompress",
           "timing": "wall clock, synchronize on both sides, median of 5 cycles after 2 warm-up cycles"}
    for fmt, group, sdt_store in (("nvfp4", 16, F8), ("mxfp4", 32, torch.uint8)):
        g = torch.Generator(device=dev).manual_seed(909)
        if fmt == "nvfp4":
            args = cta.QuantizationArgs(num_bits=4, type="float", strategy="tensor_group", symmetric=True, group_size=16, scale_dtype=F8)
        else:
            args = cta.QuantizationArgs(num_bits=4, type="float", strategy="group", symmetric=True, group_size=32, scale_dtype=torch.uint8)
        scheme = cta.QuantizationScheme(targets=["Linear"], weights=args)
        scheme.format = fmt + "-pack-quantized"
        root = torch.nn.Module()
        root.layers = torch.nn.ModuleList()
        keep, alg, first = [], 0, None
        for layer in range(16):
            blk = torch.nn.Module()
            root.layers.append(blk)
            for (proj, r, c) in LLAMA8B_LAYER:
                w = torch.randn(r, c, dtype=torch.bfloat16, device=dev, generator=g)
                gs = codec.generate_gparam(w) if fmt == "nvfp4" else None
                sc = codec.minmax_qparams_float(w, kind=fmt, group_size=group, global_scale=gs)
                lin = torch.nn.Linear(c, r, bias=False, device="meta")
                lin.weight = torch.nn.Parameter(w, requires_grad=False)
                lin.weight_scale = torch.nn.Parameter(sc, requires_grad=False)
                if gs is not None:
                    lin.weight_global_scale = torch.nn.Parameter(gs, requires_grad=False)
                lin.quantization_scheme = scheme
                setattr(blk, proj, lin)
                first = first or lin
                keep.append((w, sc, gs, torch.empty(r, c // 2, dtype=torch.uint8, device=dev), torch.empty(r, c // group, dtype=sdt_store, device=dev),
                             torch.empty(r, c, dtype=torch.bfloat16, device=dev), torch.empty(r, c // group, dtype=torch.bfloat16, device=dev)))
                ng = r * c // group
                alg += 2 * (2 * r * c + r * c // 2 + ng) + ng * sc.element_size() + 2 * ng
        lut = codec._mx_code_table(torch.bfloat16, dev) if fmt == "mxfp4" else None
        BF16 = _lib.BF16
        ca = [(w.data_ptr(), BF16, sc.data_ptr(), _lib.DT[sc.dtype], None if gs is None else gs.data_ptr(), w.shape[0], w.shape[1], group, pk.data_ptr(), st.data_ptr(),
               None if lut is None else lut.data_ptr(), stream) for (w, sc, gs, pk, st, o, so) in keep]
        da = [(pk.data_ptr(), w.shape[0], w.shape[1], st.data_ptr(), 1 if fmt == "nvfp4" else 2, -1, None if gs is None else gs.data_ptr(), group, o.data_ptr(), BF16, so.data_ptr(), stream)
              for (w, sc, gs, pk, st, o, so) in keep]

        def kernels():
            for x in ca:
                _lib.check(lib.ct_fp4_quant_pack_stored(*x))
            for x in da:
                _lib.check(lib.ct_fp4_unpack_dequant_scale(*x))

        kernels()
        torch.cuda.synchronize()
        ks = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kernels()
            torch.cuda.synchronize()
            ks.append(time.perf_counter() - t0)
        kernels_s = median(ks)
        want_w, want_s = keep[0][5].clone(), keep[0][6].clone()
        keep = None
        ca = da = None
        torch.cuda.empty_cache()
        mc = cta.ModelCompressor()

        def cycle():
            mc.compress_model(root)
            mc.decompress_model(root)

        cycle()
        ok = bool(torch.equal(first.weight.data, want_w)) and bool(torch.equal(first.weight_scale.data, want_s))
        cycle()
        both, host = [], []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cycle()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            both.append(time.perf_counter() - t0)
            host.append(t1 - t0)
        out[fmt] = {"alg_bytes": alg, "modules": 112, "ms_launches_only": round(kernels_s * 1e3, 3), "launches_frac_hbm": round(alg / kernels_s / 1e9 / HBM_PEAK_GBPS, 4),
                    "ms_model_compressor": round(median(both) * 1e3, 3), "model_compressor_frac_hbm": round(alg / median(both) / 1e9 / HBM_PEAK_GBPS, 4),
                    "api_over_launches": round(median(both) / kernels_s, 3), "us_host_per_module_and_direction": round(median(host) * 1e6 / 224, 2),
                    "class_result_equals_c_abi_result": ok}
        del root, first
        torch.cuda.empty_cache()
    return out


def formats_api_leg(dev):
    """The other formats' module loops through the plug-in API (round 6, third session): 8 layers of a Llama-3-8B-shaped tree (56 Linear modules, 1.74 G weights,
    synthetic) per format — pack-quantized with 8 bits (the W8A16 preset), float8 channel-wise, float8 in blocks of 128 x 128, MXFP8, pack-quantized with 3 bits,
    activation-ordered W4 — `ModelCompressor().compress_model(model)` + `.decompress_model(model)`, wall clock, median of 5 cycles after 2 warm-up cycles, HBM-cold by
    size.  alg bytes per element and direction: the 16-bit weight + the stored codes (+ the stored scales where they are a thirty-second of the weight or more)."""
    import compressed_tensors_amd as cta
    from compressed_tensors_amd import codec

    F8 = torch.float8_e4m3fn
    QA, QS = cta.QuantizationArgs, cta.QuantizationScheme
    fmts = {
        "w8a16_pack_quantized": (QA(num_bits=8, symmetric=True, strategy="channel"), None, 3.0),
        "fp8_channel": (QA(num_bits=8, type="float", strategy="channel", symmetric=True), None, 3.0),
        "fp8_block128": (QA(num_bits=8, type="float", strategy="block", block_structure=[128, 128], symmetric=True), None, 3.0),
        "mxfp8": (QA(num_bits=8, type="float", strategy="group", symmetric=True, group_size=32, scale_dtype=torch.uint8), "mxfp8-quantized", 3.0 + 3.0 / 32),
        "w3_pack_quantized": (QA(num_bits=3, group_size=128, symmetric=True, strategy="group"), None, 2.0 + 3.0 / 8),
        "w4_activation_ordered": (QA(num_bits=4, group_size=128, symmetric=True, strategy="group", actorder="group"), None, 2.5),
    }
    out = {"workload": "8 layers of a Llama-3-8B-shaped tree (56 Linear modules, 1.74 G weights, synthetic) per format, ModelCompressor.compress_model + decompress_model",
           "timing": "wall clock, synchronize on both sides, median of 5 cycles after 2 warm-up cycles"}
    for name, (args, fmt, bytes_per_el) in fmts.items():
        g = torch.Generator(device=dev).manual_seed(77)
        scheme = QS(targets=["Linear"], weights=args)
        if fmt:
            scheme.format = fmt
        root = torch.nn.Module()
        root.layers = torch.nn.ModuleList()
        alg = 0
        for layer in range(8):
            blk = torch.nn.Module()
            root.layers.append(blk)
            for (proj, r, c) in LLAMA8B_LAYER:
                w = torch.randn(r, c, dtype=torch.bfloat16, device=dev, generator=g)
                lin = torch.nn.Linear(c, r, bias=False, device="meta")
                lin.weight = torch.nn.Parameter(w, requires_grad=False)
                z = None
                if name == "fp8_channel":
                    sc = codec.minmax_qparams_float(w, kind="fp8")
                elif name == "fp8_block128":
                    sc = (w.float().reshape(r // 128, 128, c // 128, 128).abs().amax(dim=(1, 3)) / 448.0).to(torch.bfloat16)
                elif name == "mxfp8":
                    sc = torch.exp2(torch.floor(torch.log2(w.float().reshape(r, -1, 32).abs().amax(-1).clamp(min=1e-4))) - 8).to(torch.bfloat16)
                else:
                    sc, z = codec.minmax_qparams(w, num_bits=int(args.num_bits), group_size=getattr(args, "group_size", None), symmetric=True)
                lin.weight_scale = torch.nn.Parameter(sc, requires_grad=False)
                if z is not None:
                    lin.weight_zero_point = torch.nn.Parameter(z, requires_grad=False)
                if name == "w4_activation_ordered":
                    lin.weight_g_idx = torch.nn.Parameter((torch.randperm(c, device=dev, generator=g) // 128).to(torch.int32), requires_grad=False)
                lin.quantization_scheme = scheme
                setattr(blk, proj, lin)
                alg += 2 * int(bytes_per_el * r * c)
        mc = cta.ModelCompressor()

        def cycle():
            mc.compress_model(root)
            mc.decompress_model(root)

        # the tree's first module against the per-module class call on a copy of it (names, order, bytes), in both directions
        import copy

        from compressed_tensors_amd.compressors.base import compress_module, decompress_module
        first = root.layers[0].q_proj
        twin = copy.deepcopy(first)
        twin.quantization_scheme = scheme

        def same_entries(a, b):
            if list(a._parameters) != list(b._parameters):
                return False
            for k, t in a._parameters.items():
                u = b._parameters[k]
                if (t is None) != (u is None) or (t is not None and (t.dtype != u.dtype or t.shape != u.shape or not torch.equal(t.data.view(torch.uint8).cpu(), u.data.view(torch.uint8).cpu()))):
                    return False
            return True

        mc.compress_model(root)
        compress_module(twin)
        same = same_entries(first, twin)
        mc.decompress_model(root)
        decompress_module(twin)
        same = same and same_entries(first, twin)
        del twin
        cycle()
        both, host = [], []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cycle()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            both.append(time.perf_counter() - t0)
            host.append(t1 - t0)
        out[name] = {"alg_bytes": alg, "modules": 56, "ms_model_compressor": round(median(both) * 1e3, 3), "frac_hbm": round(alg / median(both) / 1e9 / HBM_PEAK_GBPS, 4),
                     "us_host_per_module_and_direction": round(median(host) * 1e6 / 112, 2), "first_module_equals_per_module_class_call": bool(same)}
        del root, first
        torch.cuda.empty_cache()
    return out


def sparse_checkpoint_leg(dev):
    """A TinyLlama-1.1B-shaped checkpoint (154 tensors, 1.94 GB bf16), 50 % unstructured sparsity, through the sparse-bitmask codec's class API
    (VERDICT r05 next #6): `BitmaskTensor.from_dense_many` (one host wait per window of tensors) against `from_dense` tensor by tensor and
    against the summed kernels (the same 154 `ct_bitmask_compress` launches through the C ABI into preallocated worst-case buffers, no host
    wait, no copy).  Wall clock, synchronise on both sides, best of 5 passes."""
    from compressed_tensors_amd import _lib, codec
    from compressed_tensors_amd.compressors.sparse.sparse_bitmask import BitmaskTensor

    lib = _lib.load()
    BF16 = _lib.BF16
    stream = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(77)
    ws = []
    for _ in range(22):
        for (_, r, c) in TINYLLAMA_LAYER:
            w = torch.randn(r, c, dtype=torch.float32, device=dev, generator=g).to(torch.bfloat16)
            ws.append(w.masked_fill_(torch.rand(r, c, device=dev, generator=g) < 0.5, 0))
    bufs = {}
    args = []
    total = torch.empty(1, dtype=torch.int64, device=dev)
    for w in ws:
        r, c = w.shape
        if (r, c) not in bufs:
            wsb = int(lib.ct_bitmask_compress_workspace_bytes(r, c))
            bufs[(r, c)] = (torch.empty(r * c, dtype=torch.bfloat16, device=dev), torch.empty(r, c // 8, dtype=torch.uint8, device=dev), torch.empty(r, dtype=torch.int64, device=dev),
                            torch.empty(wsb // 8 + 1, dtype=torch.int64, device=dev), wsb)
        v, bm, ro, wk, wsb = bufs[(r, c)]
        args.append((w.data_ptr(), BF16, r, c, v.data_ptr(), r * c, bm.data_ptr(), ro.data_ptr(), total.data_ptr(), wk.data_ptr(), wsb, stream))

    def kernels():
        for a in args:
            rc = lib.ct_bitmask_compress(*a)
            if rc:
                _lib.check(rc)

    keep = {}

    def timed(fn, n=5):
        fn()
        best = None
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best

    t_k = timed(kernels)
    # the same 154 tensors as ONE table launch (ct_bitmask_compress_batch; what from_dense_many issues per window), outputs preallocated, no host wait
    import ctypes

    items = (_lib.BitmaskItem * len(ws))()
    bouts = []
    btot = torch.empty(len(ws), dtype=torch.int64, device=dev)
    for i, w in enumerate(ws):
        r, c = w.shape
        bo = (torch.empty(r * c, dtype=torch.bfloat16, device=dev), torch.empty(r, c // 8, dtype=torch.uint8, device=dev), torch.empty(r, dtype=torch.int64, device=dev))
        bouts.append(bo)
        it = items[i]
        it.x, it.values, it.bitmask, it.row_offsets, it.total = w.data_ptr(), bo[0].data_ptr(), bo[1].data_ptr(), bo[2].data_ptr(), btot[i:].data_ptr()
        it.rows, it.cols, it.values_capacity, it.dt = r, c, r * c, BF16
    wsb = ctypes.c_int64()
    blocks = int(lib.ct_bitmask_batch_plan(ctypes.cast(items, ctypes.c_void_p), len(ws), ctypes.byref(wsb)))
    if blocks < 0:
        raise RuntimeError(_lib.last_error())
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(dev)
    bws = torch.empty(wsb.value // 8 + 1, dtype=torch.int64, device=dev)

    def batch_kernel():
        rc = lib.ct_bitmask_compress_batch(table.data_ptr(), len(ws), blocks, 2, bws.data_ptr(), wsb.value, stream)
        if rc:
            _lib.check(rc)

    t_b = timed(batch_kernel)
    t_many = timed(lambda: keep.__setitem__("m", BitmaskTensor.from_dense_many(ws)))
    t_many_view = timed(lambda: keep.__setitem__("v", BitmaskTensor.from_dense_many(ws, exact=False)))
    t_loop = timed(lambda: keep.__setitem__("l", [BitmaskTensor.from_dense(w) for w in ws]), n=3)
    many, loop = keep["m"], keep["l"]
    ok = all(torch.equal(a.compressed.view(torch.int16), b.compressed.view(torch.int16)) and torch.equal(a.bitmask, b.bitmask) and torch.equal(a.row_offsets, b.row_offsets)
             for a, b in zip(many, loop)) and torch.equal(many[5].decompress().view(torch.int16), ws[5].view(torch.int16))
    ok = ok and all(int(btot[i]) == loop[i].compressed.numel() and torch.equal(bouts[i][0][: int(btot[i])].view(torch.int16), loop[i].compressed.view(torch.int16))
                    and torch.equal(bouts[i][1], loop[i].bitmask) and torch.equal(bouts[i][2], loop[i].row_offsets) for i in range(0, len(ws), 7))
    # the way back: loading the checkpoint.  154 single launches (C ABI, preallocated outputs) / one table launch / the class-level list call / tensor by tensor
    dd = [torch.empty_like(w) for w in ws]
    dargs = [(b.compressed.data_ptr(), b.compressed.numel(), b.bitmask.data_ptr(), b.row_offsets.data_ptr(), -1, BF16, w.shape[0], w.shape[1], o.data_ptr(), stream)
             for b, w, o in zip(loop, ws, dd)]

    def dkernels():
        for a in dargs:
            rc = lib.ct_bitmask_decompress(*a)
            if rc:
                _lib.check(rc)

    t_dk = timed(dkernels)
    dtab = (_lib.BitmaskDItem * len(ws))()
    for i, (b, w, o) in enumerate(zip(loop, ws, dd)):
        dtab[i].values, dtab[i].bitmask, dtab[i].row_offsets, dtab[i].out = b.compressed.data_ptr(), b.bitmask.data_ptr(), b.row_offsets.data_ptr(), o.data_ptr()
        dtab[i].rows, dtab[i].cols, dtab[i].values_len, dtab[i].dt = w.shape[0], w.shape[1], b.compressed.numel(), BF16
    dblocks = int(lib.ct_bitmask_decompress_batch_plan(ctypes.cast(dtab, ctypes.c_void_p), len(ws)))
    if dblocks < 0:
        raise RuntimeError(_lib.last_error())
    dtable = torch.frombuffer(bytearray(bytes(dtab)), dtype=torch.uint8).to(dev)

    def dbatch():
        rc = lib.ct_bitmask_decompress_batch(dtable.data_ptr(), len(ws), dblocks, 2, stream)
        if rc:
            _lib.check(rc)

    for o in dd:
        o.zero_()
    t_db = timed(dbatch)
    ok = ok and all(torch.equal(o.view(torch.int16), w.view(torch.int16)) for o, w in zip(dd[::7], ws[::7]))
    ditems = [(b.compressed, b.bitmask, w.shape, b.row_offsets) for b, w in zip(loop, ws)]
    t_dmany = timed(lambda: keep.__setitem__("d", codec.bitmask_decompress_many(ditems)))
    ok = ok and all(torch.equal(o.view(torch.int16), w.view(torch.int16)) for o, w in zip(keep["d"][::5], ws[::5]))
    t_dloop = timed(lambda: keep.__setitem__("d", [b.decompress() for b in loop]), n=3)
    nnz = sum(int(b.compressed.numel()) for b in many)
    numel = sum(w.numel() for w in ws)
    alg = 2 * numel + 2 * nnz + numel // 8 + 8 * sum(w.shape[0] for w in ws)
    stored = sum(b.compressed.untyped_storage().nbytes() for b in many)
    keep.clear()
    return {"workload": "TinyLlama-1.1B-shaped checkpoint (154 tensors, 1.94 GB bf16), 50 % unstructured sparsity, sparse-bitmask compress",
            "alg_bytes": alg, "ms_kernels_only": round(t_k * 1e3, 4), "kernels_frac_hbm": round(alg / t_k / 1e9 / HBM_PEAK_GBPS, 4),
            "ms_one_table_launch": round(t_b * 1e3, 4), "one_table_launch_frac_hbm": round(alg / t_b / 1e9 / HBM_PEAK_GBPS, 4),
            "ms_from_dense_many": round(t_many * 1e3, 4), "many_over_kernels": round(t_many / t_k, 3), "many_over_one_table_launch": round(t_many / t_b, 3),
            "ms_from_dense_many_view": round(t_many_view * 1e3, 4), "many_view_over_kernels": round(t_many_view / t_k, 3),
            "ms_from_dense_one_by_one": round(t_loop * 1e3, 4), "one_by_one_over_kernels": round(t_loop / t_k, 3),
            "decompress_ms_kernels_only": round(t_dk * 1e3, 4), "decompress_ms_one_table_launch": round(t_db * 1e3, 4),
            "decompress_one_table_launch_frac_hbm": round(alg / t_db / 1e9 / HBM_PEAK_GBPS, 4),
            "decompress_ms_many": round(t_dmany * 1e3, 4), "decompress_ms_one_by_one": round(t_dloop * 1e3, 4), "decompress_many_over_kernels": round(t_dmany / t_dk, 3),
            "values_storage_bytes": stored, "nnz_bytes": 2 * nnz,
            "note": "exact mode (default) adds one device copy of the kept values per tensor (2 x nnz x 2 bytes of traffic that `kernels only` does not have); "
                    "the view mode skips it and pins a dense-sized buffer per tensor",
            "many_equals_one_by_one": bool(ok)}


def tinyllama_w8_leg(dev):
    """the same TinyLlama-1.1B-shaped checkpoint as W8A8 (int8 weights, channel-wise scales — IntQuantizationCompressor — and
    float8_e4m3fn — FloatQuantizationCompressor): ONE ct_q8_quant_batch + ONE ct_q8_dequant_batch launch for all 154 modules
    against one launch per module; 3 B per element and direction"""
    from compressed_tensors_amd import _lib, codec

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    BF16 = _lib.BF16
    mods = [(r, c) for _ in range(22) for (_, r, c) in TINYLLAMA_LAYER]
    g = torch.Generator(device=dev).manual_seed(77)
    keep = []
    for r, c in mods:
        w = torch.randn(r, c, dtype=torch.bfloat16, device=dev, generator=g)
        scale, zp = codec.minmax_qparams(w, num_bits=8, group_size=None, symmetric=True)
        keep.append((w, scale, zp, torch.empty(r, c, dtype=torch.int8, device=dev), torch.empty_like(w)))
    total = sum(2 * (3 * r * c + 2 * r) for r, c in mods)
    out = {"workload": "TinyLlama-1.1B-shaped checkpoint (154 Linear modules), W8A8 channel-wise quantize + dequantize, one launch per direction",
           "alg_bytes": total}

    def timed(fn):
        fn()
        best = None
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best

    for kind, qdt, code in (("int8", torch.int8, _lib.I8), ("fp8", torch.float8_e4m3fn, _lib.F8)):
        qs = [q.view(qdt) for (_, _, _, q, _) in keep]
        zps = [None if kind == "fp8" else z for (_, _, z, _, _) in keep]
        cb = codec.W4Batch([(w, s, z, q, w.shape[0], w.shape[1], w.shape[1]) for (w, s, _, _, _), q, z in zip(keep, qs, zps)], "compress", torch.bfloat16,
                           kind=kind, bits=8)
        db = codec.W4Batch([(q, s, z, o, w.shape[0], w.shape[1], w.shape[1]) for (w, s, _, _, o), q, z in zip(keep, qs, zps)], "decompress", torch.bfloat16,
                           kind=kind)

        def batched():
            cb.launch(stream)
            db.launch(stream)

        def per_module():
            for (w, s, _, _, o), q, z in zip(keep, qs, zps):
                r, c = w.shape
                zp_, zdt = (None, -1) if z is None else (z.data_ptr(), _lib.I8)
                if kind == "fp8":
                    lib.ct_quantize_fp8(w.data_ptr(), BF16, s.data_ptr(), BF16, zp_, zdt, r, c, 1, c, 1, None, BF16, q.data_ptr(), code, stream)
                else:
                    lib.ct_quantize(w.data_ptr(), BF16, s.data_ptr(), BF16, zp_, zdt, r, c, 1, c, 1, None, 8, BF16, q.data_ptr(), code, stream)
                lib.ct_dequantize(q.data_ptr(), code, s.data_ptr(), BF16, zp_, zdt, r, c, 1, c, 1, None, o.data_ptr(), BF16, stream)

        t_loop = timed(per_module)
        ref = [(q.clone(), o.clone()) for (_, _, _, _, o), q in zip(keep[:3], qs)]
        for (_, _, _, q, o) in keep:
            q.zero_(); o.zero_()
        t_b = timed(batched)
        same = all(torch.equal(q.view(torch.uint8), rq.view(torch.uint8)) and torch.equal(o.view(torch.int16), ro.view(torch.int16))
                   for (_, _, _, _, o), q, (rq, ro) in zip(keep[:3], qs, ref))
        out[kind] = {"ms_whole_checkpoint": round(t_b * 1e3, 4), "GBps": round(total / t_b / 1e9, 1), "frac_of_hbm_peak": round(total / t_b / 1e9 / HBM_PEAK_GBPS, 4),
                     "ms_one_launch_per_module": round(t_loop * 1e3, 4), "batch_equals_per_module": bool(same)}
    return out


IC_BYTES = 256 * 2 ** 20  # the Infinity Cache (memory-side, shared by the eight XCDs)


def rows_of_set(dev, set_index, a, b, n=N, dtype=torch.bfloat16, sparsity=None):
    """rows [a, b) of synthetic tensor number `set_index`, generated 64 rows at a time from a (set, row block) seed: every rank — and a
    single rank making the whole tensor — gets the same rows without anyone materialising more than its own shard"""
    assert a % 64 == 0 and (b % 64 == 0 or b == n)
    out = torch.empty(b - a, n, dtype=dtype, device=dev)
    g = torch.Generator(device=dev)
    for r in range(a, b, 64):
        g.manual_seed(4242 + set_index * 100003 + r // 64)
        hi = min(r + 64, b)
        blk = torch.randn(hi - r, n, dtype=torch.float32, device=dev, generator=g)
        if sparsity is not None:
            blk = blk.masked_fill(torch.rand(hi - r, n, device=dev, generator=g) < sparsity, 0)
        out[r - a:hi - a] = blk.to(dtype)
    return out


def timed_blocks(step, iters, barrier, allreduce_max):
    """the protocol of the headline loop for a sharded leg: KERNEL_WARM_MS of the same launches, then BLOCKS blocks of `iters` steps, each
    bracketed by barrier + synchronize on both sides, wall clock, MAX over the ranks; returns the per-block seconds per step"""
    device_warmup([step], KERNEL_WARM_MS)
    per = []
    for _ in range(BLOCKS):
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(iters):
            step(i)
        torch.cuda.synchronize()
        barrier()
        per.append(allreduce_max(time.perf_counter() - t0) / iters)
    return per


def graph_blocks(launch_step, iters, dev, barrier, allreduce_max):
    """the same `iters` steps captured ONCE into a HIP graph (torch.cuda.CUDAGraph over the C-ABI launches: they allocate nothing and never
    synchronise, so they are capturable) and replayed per timed block — what a C host with a launch-bound inner loop would do; BLOCKS replays between
    barriers, max over ranks.  `launch_step(i, stream)` issues step i on the raw stream it is given.  Returns per-block seconds per step."""
    from compressed_tensors_amd import _lib

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for i in range(4):
            launch_step(i, _lib.stream_on(dev, side.cuda_stream))
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = _lib.stream_on(dev, torch.cuda.current_stream(dev).cuda_stream)
        for i in range(iters):
            launch_step(i, st)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    per = []
    for _ in range(BLOCKS):
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        graph.replay()
        torch.cuda.synchronize()
        barrier()
        per.append(allreduce_max(time.perf_counter() - t0) / iters)
    return per


def row_shard_leg(dev, rank, world, barrier, allreduce_max, allreduce_min, iters=MIN_LAUNCHES_PER_BLOCK):
    """SURVEY 8e for the single-tensor configs: ONE 8192x8192 tensor split by row blocks (`shard_rows`, multiples of 64
    rows) over the ranks — strong scaling, no data-path collective.  Config 2 (W4A16 compress + decompress of the rank's
    rows) and config 3 (sparse-bitmask compress + decompress; the shard's row_offsets are local, the global ones are
    local + the number of non-zeros in the earlier shards).

    Round 6 (VERDICT r05 missing #1): on the protocol of the rest of this file — prebuilt C-ABI launches (no allocation, no Python codec
    call in the timed loop), a fixed-duration device warm-up, BLOCKS blocks of >= MIN_LAUNCHES_PER_BLOCK steps, and enough rotating
    tensors that THIS RANK's smallest read stream is >= 2x the 256 MiB Infinity Cache at the actual world size (16 x world tensors for
    config 2: the rank's packed words; 8 x world for config 3: values + bitmask >= 2.3x) — the memory per rank stays ~4.8 GiB at any
    world size, and every row is HBM-cold.  Every rank also computes tensor 0 whole, by itself, and checks that what its launches wrote
    for its shard is exactly the corresponding slice of that single-rank result."""
    from compressed_tensors_amd import _lib, codec
    from compressed_tensors_amd.distributed.shard import shard_rows

    lib = _lib.load()
    BF16 = _lib.BF16
    stream = torch.cuda.current_stream(dev).cuda_stream
    a, b = shard_rows(N, rank=rank, world_size=world, multiple=64)
    rows = b - a
    kw = dict(num_bits=BITS, strategy="group", group_size=GROUP)
    out = {"rows_this_rank": [a, b], "ranks": world, "launches_per_block": iters, "blocks": BLOCKS}

    # ---- config 2: the rank's packed words are the smallest read stream
    packed_bytes = max(rows, 1) * N // 2
    nsets = max(4, -(-2 * IC_BYTES // packed_bytes))
    sets = []
    for j in range(nsets):
        w = rows_of_set(dev, j, a, b)
        sc, zp = codec.minmax_qparams(w, num_bits=BITS, group_size=GROUP, symmetric=True)
        sets.append((w, sc, zp, torch.empty(rows, N // 8, dtype=torch.int32, device=dev), torch.empty(rows, N, dtype=torch.bfloat16, device=dev)))
    ca = [(w.data_ptr(), BF16, sc.data_ptr(), BF16, zp.data_ptr(), _lib.I8, rows, N, 1, GROUP, N // GROUP, None, BITS, BF16, pk.data_ptr(), stream)
          for (w, sc, zp, pk, o) in sets]
    da = [(pk.data_ptr(), rows, N // 8, N, BITS, sc.data_ptr(), BF16, None, -1, 1, GROUP, N // GROUP, None, o.data_ptr(), BF16, stream)
          for (w, sc, zp, pk, o) in sets]

    def step2(i):
        rc = lib.ct_quant_pack(*ca[i % nsets]) or lib.ct_unpack_dequant(*da[(i + nsets // 2) % nsets])
        if rc:
            _lib.check(rc)

    for i in range(nsets):  # every packed buffer populated, every output written once
        step2(i)
    per2 = timed_blocks(step2, iters, barrier, allreduce_max)

    def step2_on(i, st):  # the same two launches on a given stream (for the graph capture)
        rc = lib.ct_quant_pack(*ca[i % nsets][:-1], st) or lib.ct_unpack_dequant(*da[(i + nsets // 2) % nsets][:-1], st)
        if rc:
            _lib.check(rc)

    try:
        per2g = graph_blocks(step2_on, iters, dev, barrier, allreduce_max)
    except Exception as e:  # a graph capture must never take the leg down
        per2g = None
        out["hip_graph_error"] = repr(e)
    # the single-rank result of tensor 0 (the plug-in's tensor-level calls on the WHOLE tensor) against what this rank's launches wrote
    w_full = rows_of_set(dev, 0, 0, N)
    s_full, z_full = codec.minmax_qparams(w_full, num_bits=BITS, group_size=GROUP, symmetric=True)
    p_full = codec.quantize_and_pack(w_full, s_full, z_full, **kw)
    d_full = codec.unpack_and_dequantize(p_full, (N, N), s_full, None, **kw)
    ok = (torch.equal(sets[0][0], w_full[a:b]) and torch.equal(sets[0][3], p_full[a:b]) and torch.equal(sets[0][4].view(torch.int16), d_full[a:b].view(torch.int16)))
    del w_full, s_full, z_full, p_full, d_full
    t2 = median(per2)
    alg2 = 2 * alg_bytes_one_direction()
    out["w4a16"] = {"us_per_tensor": round(t2 * 1e6, 2), "GBps_all_ranks": round(alg2 / t2 / 1e9, 1),
                    "frac_of_hbm_peak_per_gpu": round(alg2 / t2 / 1e9 / world / HBM_PEAK_GBPS, 4),
                    "us_per_tensor_blocks": [round(x * 1e6, 2) for x in per2], "sets": nsets,
                    "us_per_tensor_hip_graph": None if per2g is None else round(median(per2g) * 1e6, 2),  # the same steps replayed from ONE captured HIP graph
                    "GBps_all_ranks_hip_graph": None if per2g is None else round(alg2 / median(per2g) / 1e9, 1),
                    "cache": f"HBM-cold: {nsets} rotating tensors, this rank's packed words {nsets * packed_bytes / 2 ** 20:.0f} MiB >= 2 x 256 MiB",
                    "shard_equals_slice_of_single_rank_result": bool(allreduce_min(1.0 if ok else 0.0) == 1.0)}
    del sets, ca, da
    torch.cuda.empty_cache()

    # ---- config 3
    nb = 8 * world  # reads of the decompress direction: (67 + 8) MB x 8 per WHOLE tensor = 2.3x the Infinity Cache per rank at any world size
    ws_bytes = int(lib.ct_bitmask_compress_workspace_bytes(rows, N))
    items = []
    for j in range(nb):
        x = rows_of_set(dev, 1000 + j, a, b, sparsity=0.5)
        v, bm, ro = codec.bitmask_compress(x)
        items.append(dict(x=x, v=v.clone(), bm=bm, ro=ro, out=torch.empty_like(x), v2=torch.empty(rows * N, dtype=torch.bfloat16, device=dev), bm2=torch.empty_like(bm),
                          ro2=torch.empty_like(ro), ws=torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=dev)))
    cargs = [(it["x"].data_ptr(), BF16, rows, N, it["v2"].data_ptr(), it["v2"].numel(), it["bm2"].data_ptr(), it["ro2"].data_ptr(), it["ws"][-1:].data_ptr(),
              it["ws"].data_ptr(), ws_bytes, stream) for it in items]
    dargs = [(it["v"].data_ptr(), it["v"].numel(), it["bm"].data_ptr(), it["ro"].data_ptr(), -1, BF16, rows, N, it["out"].data_ptr(), stream) for it in items]

    def step3(i):
        rc = lib.ct_bitmask_compress(*cargs[i % nb]) or lib.ct_bitmask_decompress(*dargs[(i + nb // 2) % nb])
        if rc:
            _lib.check(rc)

    for i in range(nb):
        step3(i)
    per3 = timed_blocks(step3, iters, barrier, allreduce_max)
    x_full = rows_of_set(dev, 1000, 0, N, sparsity=0.5)
    v_full, bm_full, ro_full = codec.bitmask_compress(x_full)
    nnz = v_full.numel()
    base = int(ro_full[a].item()) if a < N else nnz
    stop = int(ro_full[b].item()) if b < N else nnz
    it0 = items[0]
    n0 = int(it0["ws"][-1].item())
    ok3 = (n0 == stop - base and torch.equal(it0["v2"][:n0].view(torch.int16), v_full[base:stop].view(torch.int16)) and torch.equal(it0["bm2"], bm_full[a:b])
           and torch.equal(it0["ro2"] + base, ro_full[a:b]) and torch.equal(it0["out"].view(torch.int16), x_full[a:b].view(torch.int16)))
    del x_full, v_full, bm_full
    t3 = median(per3)
    alg3 = 2 * (2 * N * N + 2 * nnz + N * N // 8 + 8 * N)
    out["sparse_bitmask"] = {"us_per_tensor": round(t3 * 1e6, 2), "GBps_all_ranks": round(alg3 / t3 / 1e9, 1),
                             "frac_of_hbm_peak_per_gpu": round(alg3 / t3 / 1e9 / world / HBM_PEAK_GBPS, 4),
                             "us_per_tensor_blocks": [round(x * 1e6, 2) for x in per3], "sets": nb,
                             "cache": f"HBM-cold: {nb} rotating tensors, this rank's values + bitmask {nb * (2 * nnz + N * N // 8) / world / 2 ** 20:.0f} MiB >= 2 x 256 MiB",
                             "row_offsets": "local per shard; global = local + nnz of the earlier shards",
                             "shard_equals_slice_of_single_rank_result": bool(allreduce_min(1.0 if ok3 else 0.0) == 1.0)}
    out["workload"] = (f"ONE {N}x{N} bf16 tensor split by row blocks over {world} rank(s) (strong scaling, no collectives), through the C ABI "
                       f"(prebuilt launches on one stream; ct_quant_pack + ct_unpack_dequant, ct_bitmask_compress + ct_bitmask_decompress), "
                       f"{BLOCKS} blocks of {iters} steps, median block, max over ranks")
    return out


def w4_weak_leg(dev, n, rank, world, barrier, allreduce_max, steps=MIN_LAUNCHES_PER_BLOCK):
    """north_star's second size at EVERY world size (VERDICT r05 missing #2): one `n` x `n` bf16 weight shard per rank (weak scaling, no
    collective), W4A16 g128 compress + decompress through the C ABI on one stream, HBM-cold (packed words of the rotating sets >= 2x the
    Infinity Cache per rank), BLOCKS blocks of `steps` steps between barriers, max over ranks; round trip of one set == fake_quantize."""
    from compressed_tensors_amd import _lib, codec

    lib = _lib.load()
    BF16 = _lib.BF16
    stream = torch.cuda.current_stream(dev).cuda_stream
    nsets = max(4, -(-2 * IC_BYTES // (n * n // 2)))
    g = torch.Generator(device=dev).manual_seed(77 + rank)
    sets = []
    for _ in range(nsets):
        w = torch.randn(n, n, dtype=torch.float32, device=dev, generator=g).to(torch.bfloat16)
        sc, zp = codec.minmax_qparams(w, num_bits=BITS, group_size=GROUP, symmetric=True)
        sets.append((w, sc, zp, torch.empty(n, n // 8, dtype=torch.int32, device=dev), torch.empty(n, n, dtype=torch.bfloat16, device=dev)))
    ca = [(w.data_ptr(), BF16, sc.data_ptr(), BF16, zp.data_ptr(), _lib.I8, n, n, 1, GROUP, n // GROUP, None, BITS, BF16, pk.data_ptr(), stream) for (w, sc, zp, pk, o) in sets]
    da = [(pk.data_ptr(), n, n // 8, n, BITS, sc.data_ptr(), BF16, None, -1, 1, GROUP, n // GROUP, None, o.data_ptr(), BF16, stream) for (w, sc, zp, pk, o) in sets]

    def step(i):
        rc = lib.ct_quant_pack(*ca[i % nsets]) or lib.ct_unpack_dequant(*da[(i + nsets // 2) % nsets])
        if rc:
            _lib.check(rc)

    for i in range(nsets):
        step(i)
    per = timed_blocks(step, steps, barrier, allreduce_max)

    def step_on(i, st):
        rc = lib.ct_quant_pack(*ca[i % nsets][:-1], st) or lib.ct_unpack_dequant(*da[(i + nsets // 2) % nsets][:-1], st)
        if rc:
            _lib.check(rc)

    try:
        perg = graph_blocks(step_on, steps, dev, barrier, allreduce_max)
    except Exception:
        perg = None
    w, sc, zp, pk, o = sets[0]
    ok = torch.equal(o, codec.fake_quantize_tensor(w, sc, zp, num_bits=BITS, strategy="group", group_size=GROUP))
    t = median(per)
    alg = 2 * alg_bytes_one_direction(n)
    return {"workload": f"W4A16 g128 compress+decompress, one {n}x{n} bf16 weight shard per rank, C ABI, one stream, HBM-cold ({nsets} rotating sets)",
            "alg_bytes_per_step_per_gpu": alg, "us_per_step": round(t * 1e6, 2), "us_per_step_blocks": [round(x * 1e6, 2) for x in per],
            "GBps_all_ranks": round(world * alg / t / 1e9, 1), "frac_of_hbm_peak_per_gpu": round(alg / t / 1e9 / HBM_PEAK_GBPS, 4),
            "us_per_step_hip_graph": None if perg is None else round(median(perg) * 1e6, 2),  # the same steps replayed from ONE captured HIP graph
            "frac_of_hbm_peak_per_gpu_hip_graph": None if perg is None else round(alg / median(perg) / 1e9 / HBM_PEAK_GBPS, 4),
            "ranks": world, "round_trip_equals_fake_quantize": bool(ok)}


def self_launch(n: int) -> int:
    """re-exec this command under torch.distributed.run: one process per GPU, rendezvous on 127.0.0.1 and a free port"""
    import socket
    import subprocess

    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__), *sys.argv[1:]]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # the host driver only supports dmabuf IPC (RCCL / cross-process device memory)
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(cmd, env=env)


DUMP_ROWS = 512  # rows of the 8192-row outputs written by --dump-outputs: 4 MiB of packed words (float64) + 16 MiB of weight (float32)


def dump_outputs(path, sets, last, dev, suffix=""):
    """--dump-outputs: what timed step `last` computed, as a caller of the C ABI would receive it — the int32 words its compress wrote
    (`compress_weight_packed`, as float64: exact) and the bf16 weight its decompress wrote (`decompress_weight`, as float32: exact) —
    on DUMP_ROWS rows drawn with a fixed seed (`sample_rows`, the same every run)."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(0))[:DUMP_ROWS].sort().values
    idx = rows.to(dev)
    arrays = {"compress_weight_packed": sets[last % NSETS]["packed"].index_select(0, idx).double(),
              "decompress_weight": sets[(last + NSETS // 2) % NSETS]["out"].index_select(0, idx).float(),
              "sample_rows": rows.double()}
    for name, t in arrays.items():
        np.save(os.path.join(path, f"{name}{suffix}.npy"), t.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline (other configurations, sizes and formats, per-kernel "
                         "roofline, multi-rank legs, CPU baseline, oracle check) and write the full result to " + DETAILS_FILE)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the extra legs and the cache-warm kernel timings")
    ap.add_argument("--one-stream", action="store_true", help="issue the step's two launches on one HIP stream")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed to DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--shard", choices=("tensors", "rows"), default="tensors",
                    help="tensors (default): one 8192^2 weight shard per rank, weak scaling.  rows: with --full, additionally force the row-block "
                         "leg (ONE tensor split by rows over the ranks, strong scaling) — under --full it always runs when N > 1")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1
    if a.gpus != world and distributed:
        raise SystemExit(f"--gpus {a.gpus} does not match WORLD_SIZE {world}")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (the command the driver would have used) and hand
        # its exit code back; rank 0 of that run prints the one JSON line on the stdout this process shares with it
        raise SystemExit(self_launch(a.gpus))

    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    # CT_BENCH_SHARE_GPU=1 (test knob): every rank uses cuda:0 and the timing collectives go over gloo, so
    # that the N > 1 code path can be exercised on a one-GPU box
    share_gpu = os.environ.get("CT_BENCH_SHARE_GPU") == "1"
    if share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    red_dev = torch.device("cpu") if share_gpu else dev
    if distributed:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share_gpu:
            dist.init_process_group(backend="gloo", init_method="env://")
        else:
            dist.init_process_group(backend="nccl", init_method="env://", device_id=dev)

    import __graft_entry__ as ge

    if distributed:  # one rank (re)builds if the in-tree library is stale, the others wait: no concurrent writers
        if rank == 0:
            ge.build_hip()
        dist.barrier()
    ge.build_hip()  # no-op when the in-tree library is current
    sets = make_sets(dev, rank)
    stream = torch.cuda.current_stream(dev).cuda_stream
    compress, decompress = make_launchers(sets, stream)
    # the step's two operations are independent (different tensors): the timed loop issues the compress
    # on one HIP stream and the decompress on another, so the ramp / tail of one launch overlaps the
    # other; --one-stream keeps both on a single stream.  (The decompress reads a
    # packed buffer whose last rewrite, with identical bytes, was issued 8 steps earlier on the other stream.)
    s_c, s_d = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    compress2, decompress2 = make_launchers(sets, s_c.cuda_stream, s_d.cuda_stream)

    def barrier():
        if distributed:
            dist.barrier()

    def timed_steps(c, d, cold_probe=None):
        """ONE timed region of EXACTLY --steps steps, bracketed by barrier + synchronize on both sides and max-reduced over the
        ranks; returns its wall time.  Before it: every packed buffer is populated, a fixed-duration warm-up of the same launches
        (WARM_MS, independent of --warmup), then the --warmup untimed steps."""
        for i in range(NSETS):  # populate every packed buffer once
            c(i)
        torch.cuda.synchronize()

        def block():
            barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                c(i)
                d(i + NSETS // 2)  # a packed buffer written 8 steps (1.3 GB of traffic) ago: evicted from the Infinity Cache
            torch.cuda.synchronize()
            local = time.perf_counter() - t0  # this rank's own work, before it waits for the others
            barrier()
            el = time.perf_counter() - t0
            if distributed:
                t = torch.tensor([el], dtype=torch.float64, device=red_dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)  # timing only; the data path has no collective
                el = float(t.item())
            local_times.append(local)
            return el

        if cold_probe is not None:  # what round 2's protocol measured: --warmup steps only, on a device that has done nothing yet
            for i in range(a.warmup):
                c(i)
                d(i + NSETS // 2)
            cold_probe.append(block())
        device_warmup([c, lambda i: d(i + NSETS // 2)], WARM_MS)
        for i in range(a.warmup):
            c(i)
            d(i + NSETS // 2)
        return block()

    cold = []
    local_times = []
    if a.full:  # the one-stream region (value_one_stream, and the same region without the device warm-up) goes first
        elapsed_one = timed_steps(compress, decompress, cold_probe=cold)
        elapsed = elapsed_one if a.one_stream else timed_steps(compress2, decompress2)
    else:
        elapsed = timed_steps(compress, decompress) if a.one_stream else timed_steps(compress2, decompress2)
    if a.dump_outputs:  # before anything else writes the buffers of the last timed step
        dump_outputs(a.dump_outputs, sets, a.steps - 1, dev, f"_rank{rank}" if distributed else "")
    # what every rank did on its own (its timed region of the reported configuration), gathered for the line: a rank that lags shows
    step_bytes = 2 * alg_bytes_one_direction()
    mine = step_bytes * a.steps / local_times[-1] / 1e9
    ranks_seen, per_rank = 1, [round(mine, 1)]
    if distributed:
        ranks_seen = dist.get_world_size()
        t = torch.zeros(ranks_seen, dtype=torch.float64, device=red_dev)
        t[rank] = mine
        dist.all_reduce(t, op=dist.ReduceOp.SUM)  # reporting only
        per_rank = [round(float(v), 1) for v in t.tolist()]
    value = world * step_bytes * a.steps / elapsed / 1e9

    result = None
    if rank == 0:
        result = {
            "metric": "GB/s pack+unpack (int4 g128, bitmask) vs HBM peak; bit-exact round-trip",
            "value": round(value, 1),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(elapsed / a.steps * 1e3, 5),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic",
            "config": {
                "workload": f"W4A16 pack-quantized (int4, group_size=128, symmetric) compress+decompress, {N}x{N} bf16 per GPU",
                "alg_bytes_per_step_per_gpu": step_bytes,
                "buffers": f"{NSETS} rotating sets (HBM-cold)",
                "boundary": "C ABI (ct_quant_pack + ct_unpack_dequant), inputs resident in HBM",
                "streams": 1 if a.one_stream else 2,
                "parallelism": f"{world} independent weight shards, no collectives",
                "ranks_seen": ranks_seen,
                "per_rank_GBps": per_rank,
            },
            "frac_of_hbm_peak": round(value / world / HBM_PEAK_GBPS, 4),
        }
    if not a.full:  # a plain run ends with its headline
        if distributed:
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print(headline_line(result), flush=True)
        return

    if rank == 0:
        one = alg_bytes_one_direction()
        sp_c, sp_d = {}, {}
        us_c = time_kernel(compress, 60, spread=sp_c)
        us_d = time_kernel(decompress, 60, offset=NSETS // 2, spread=sp_d)
        # the same launches on ONE buffer set: its 168 MB stay in the 256 MiB Infinity Cache (reported, never `value`)
        # (not under --no-extra: the rocprof headline pass runs with it, so that its per-kernel average is over HBM-cold launches only)
        warm_c = None if a.no_extra else time_kernel(lambda i: compress(0), 60)
        warm_d = None if a.no_extra else time_kernel(lambda i: decompress(0), 60)
        kernels = {
            "w4_quant_pack_lean_kernel<bf16>": {"avg_us": round(us_c, 2), "GBps": round(one / us_c / 1e3, 1), "frac": round(one / us_c / 1e3 / HBM_PEAK_GBPS, 4),
                                                "avg_us_cache_warm": warm_c and round(warm_c, 2), **sp_c},
            "w4_unpack_dequant_kernel<bf16>": {"avg_us": round(us_d, 2), "GBps": round(one / us_d / 1e3, 1), "frac": round(one / us_d / 1e3 / HBM_PEAK_GBPS, 4),
                                               "avg_us_cache_warm": warm_d and round(warm_d, 2), **sp_d},
        }
        # VALU utilisation next to the GB/s (a VALU-bound result must not be misread as a memory problem): from the committed
        # SQ counter pass of the same two kernels (tools/profile_round.sh headline_sq), not measured live
        for kname, busy in valu_busy_from_profile().items():
            if kname in kernels:
                kernels[kname].update(busy)
        dom = max(kernels, key=lambda k: kernels[k]["avg_us"])
        traffic, traffic_src = committed_traffic(dom)
        result["config"]["value_one_stream"] = round(world * step_bytes * a.steps / elapsed_one / 1e9, 1)
        result.update({
            "value_one_stream": round(world * step_bytes * a.steps / elapsed_one / 1e9, 1),
            "roofline": {
                "bound": "hbm",
                "kernel": dom,
                "achieved": kernels[dom]["GBps"],
                "peak": HBM_PEAK_GBPS,
                "unit": "GB/s",
                "frac": kernels[dom]["frac"],
                "traffic": traffic,
                "alg_bytes_per_launch": one,
                "traffic_source": traffic_src,
                # everything below is measured live in this run; it sits INSIDE `roofline` so that it survives the driver's parse
                "step": {"value_two_streams": round(world * step_bytes * a.steps / elapsed / 1e9, 1),
                         "value_one_stream": round(world * step_bytes * a.steps / elapsed_one / 1e9, 1),
                         "frac_two_streams": round(value / world / HBM_PEAK_GBPS, 4),
                         "frac_one_stream": round(step_bytes * a.steps / elapsed_one / 1e9 / HBM_PEAK_GBPS, 4),
                         "protocol": f"{WARM_MS:.0f} ms device warm-up of the same launches, then --warmup steps, then ONE timed region of --steps steps "
                                     "(barrier + synchronize on both sides, wall clock, max over ranks); region / --steps is ms_per_step",
                         "ms_per_step_without_device_warmup": round(cold[0] / a.steps * 1e3, 5) if cold else None},
                "kernels": [dict(kernel=k, config=f"W4A16 g128 {N}x{N} bf16", alg_bytes=one, us=v["avg_us"], min_us=v.get("min_us"), max_us=v.get("max_us"),
                                 GBps=v["GBps"], frac=v["frac"], valu_busy_frac=v.get("valu_busy_frac")) for k, v in kernels.items()],
            },
            "kernels": kernels,
            "parity_gate": parity_gate(sets),
        })
        if world == 1 and not a.no_extra:
            del sets
            torch.cuda.empty_cache()
            for key, leg in (("kernels_other", w4_variants_leg), ("other_widths", other_widths_leg), ("bitmask", bitmask_leg), ("int8_per_tensor", int8_leg), ("quantize_dequantize_fake_quantize", quantize_leg), ("marlin24", marlin24_leg), ("minmax_qparams", qparams_leg),
                             ("float_formats", float_formats_leg), ("pack_unpack", pack_unpack_leg), ("tinyllama_w8a8", tinyllama_w8_leg),
                             ("sparse_checkpoint", sparse_checkpoint_leg), ("llama8b_checkpoint", llama8b_api_leg), ("fp4_checkpoint_api", fp4_api_leg), ("formats_api", formats_api_leg)):
                try:
                    result[key] = leg(dev)
                except Exception as e:  # an extra leg must never take the headline line down
                    result[key] = {"error": repr(e)}
                torch.cuda.empty_cache()
            if isinstance(result.get("kernels_other"), dict) and "bf16_4096" in result["kernels_other"]:
                result["kernels_4096"] = result["kernels_other"]["bf16_4096"]  # north_star names both sizes
    if not a.no_extra:  # every rank takes part: the checkpoint is sharded over the ranks
        sets = None  # the headline's 4.8 GiB of rotating buffers are done with (the launchers keep only addresses, and are not called again)
        torch.cuda.empty_cache()

        def _allreduce(x, op):
            if not distributed:
                return x
            t = torch.tensor([x], dtype=torch.float64, device=red_dev)
            dist.all_reduce(t, op=op)  # timing / pass-fail flags only
            return float(t.item())

        def allreduce_max(x):
            return _allreduce(x, dist.ReduceOp.MAX) if distributed else x

        def allreduce_min(x):
            return _allreduce(x, dist.ReduceOp.MIN) if distributed else x

        def allreduce_sum_vec(xs):
            if not distributed:
                return list(xs)
            t = torch.tensor(list(xs), dtype=torch.float64, device=red_dev)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)  # bookkeeping only
            return [float(v) for v in t.tolist()]

        try:
            leg = tinyllama_leg(dev, rank, world, barrier, allreduce_max, allreduce_sum_vec)
        except Exception as e:
            leg = {"error": repr(e)}
        if rank == 0:
            result["tinyllama_checkpoint"] = leg
            if world == 1:
                result["roofline"]["kernels"] += roofline_rows(result)  # every extra leg's row, inside `roofline` so that the driver's parse keeps it
        if distributed or a.shard == "rows":
            torch.cuda.empty_cache()
            try:
                leg = row_shard_leg(dev, rank, world, barrier, allreduce_max, allreduce_min)
            except Exception as e:
                leg = {"error": repr(e)}
            if rank == 0:
                result["row_sharded"] = leg
        torch.cuda.empty_cache()
        try:  # north_star names 4096x4096 beside 8192x8192 "at 1/2/4/8 GPUs": the same step at the second size, at every world size
            leg = w4_weak_leg(dev, 4096, rank, world, barrier, allreduce_max)
        except Exception as e:
            leg = {"error": repr(e)}
        if rank == 0:
            result["w4a16_4096"] = leg
    if rank == 0:
        # LAST, after every GPU leg: the CPU baseline's imports dlopen libraries with TLS segments, after which glibc 2.35 keeps this thread on
        # the slow __tls_get_addr path (BZ 19924) — the host-bound figure of the run, ModelCompressor on the 154-module tree, measured
        # 1.16-1.68 ms behind it against 1.03-1.08 ms in front of it on the same lease (runs T-Y); the baseline does not care
        if world == 1 and not a.no_cpu_baseline:
            result["cpu_baseline"], result["cpu_baseline_port"] = cpu_baseline(dev)
        result["oracle_slice_check"] = oracle_slice_check(dev)  # never skipped: no configuration runs without the real checker
    if distributed:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        from compressed_tensors_amd import _lib as ctlib

        result["host_path"] = ctlib.host_path_kind()  # "native": the C++ host loop ran the class / model API rows; "python": it did not import
        full = json.dumps(result)
        here = os.path.dirname(os.path.abspath(__file__))
        for d in (here, os.path.join(here, "gpurun_out")):  # beside the script; and where gpurun merges files back from, when that exists
            if d == here or os.path.isdir(d):
                try:
                    with open(os.path.join(d, DETAILS_FILE), "w") as f:
                        f.write(full + "\n")
                except OSError:
                    pass
        print(full, file=sys.stderr, flush=True)
        sys.stdout.flush()
        print(headline_line(result), flush=True)  # LAST line of stdout, <= LINE_CAP characters


if __name__ == "__main__":
    main()
