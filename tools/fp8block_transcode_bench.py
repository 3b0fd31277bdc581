"""developer script: FP8 block-quantized weights to MXFP8 or NVFP4, the fused form against the composition it replaces, on the two whole tables of
tools/fp8block_bench.py: DeepSeek-V3.2-shaped layers (62 modules) and a Qwen3-4B-shaped model (252 modules); 128 x 128 blocks, float32 scales,
bfloat16 as the dense dtype.  The sibling of tools/fp8block_mxfp4_bench.py, whose protocol this is.

    python tools/fp8block_transcode_bench.py --target mxfp8|nvfp4 [--steps 10] [--warmup 2] [--run N] [--out FILE.jsonl]

mxfp8  fused: ct_fp8block_mxfp8_batch.  composition: ct_fp8block_dequant_batch into a dense buffer, ct_rtn_quant_group8_batch (kind MXFP8) over it.
nvfp4  fused: the fill of the amax keys, ct_fp8block_nvfp4_amax_batch, ct_fp8block_nvfp4_batch.  composition: ct_fp8block_dequant_batch, the fill of
       its keys, ct_rtn_nvfp4_amax_batch, ct_rtn_nvfp4_quant_pack_batch.  A sample is all of a form's launches, the fill included.

Per table, event times (profiler off) of the two forms ALTERNATED on the same buffers, launch by launch: medians, minima and maxima.  HBM-cold by
construction, as in the sibling.  Rates are over the algorithmic bytes of the fused form — mxfp8 1 + 1 + 1/32 per element, nvfp4 1 + (1 + 0.5 +
1/16), plus 4 per scale read — against the 8 TB/s HBM peak.  The outputs of the two forms are compared byte for byte first.
Prints one JSON line and, with --out, appends it to FILE.  `--run` tags the line: the dispatch rule reads two separate runs."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from fp8block_bench import BLOCK, HBM_PEAK, nblocks, shapes  # noqa: E402
from fp8block_mxfp4_bench import COLD_BYTES, _upload, alternated  # noqa: E402

# per element: (fused, composed) algorithmic bytes without the block scales
PER_ELEMENT = {"mxfp8": (1 + 1 + 1 / 32, (1 + 2) + (2 + 1 + 1 / 32)), "nvfp4": (1 + (1 + 0.5 + 1 / 16), (1 + 2) + 2 + (2 + 0.5 + 1 / 16))}


def algorithmic_bytes(shp, target, form):
    scale_reads = (2 if target == "nvfp4" and form == 0 else 1) * 4
    return sum(int(R * C * PER_ELEMENT[target][form]) + nblocks(R) * nblocks(C) * scale_reads for _, R, C in shp)


def forms_of(target, shp, dev):
    """(keep, fused(), composed(), outputs [(fused outputs, composed outputs)]) over device tensors of every module"""
    from compressed_tensors_amd import _lib, codec

    lib, s, n = _lib.load(), _lib.stream_on(dev), len(shp)
    gen = torch.Generator(device=dev).manual_seed(0)
    nv = target == "nvfp4"
    item_type = _lib.Fp8BlockNvItem if nv else _lib.Fp8BlockMxItem
    keys = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)] if nv else None
    keep, fused, deq, second, outs = [keys], [], [], [], []
    for i, (_, R, C) in enumerate(shp):
        w = torch.randint(0, 256, (R, C), generator=gen, dtype=torch.int32, device=dev).to(torch.uint8)
        sc = torch.rand(nblocks(R), nblocks(C), generator=gen, device=dev) * 1e-3 + 1e-5
        dense = torch.empty(R, C, dtype=torch.bfloat16, device=dev)
        if nv:
            o = [(torch.empty(R, C // 2, dtype=torch.uint8, device=dev), torch.empty(R, C // 16, dtype=torch.uint8, device=dev),
                  torch.empty(1, dtype=torch.float32, device=dev)) for _ in range(2)]
        else:
            o = [(torch.empty(R, C, dtype=torch.uint8, device=dev), torch.empty(R, C // 32, dtype=torch.uint8, device=dev)) for _ in range(2)]
        keep += [w, sc, dense]
        outs.append(o)
        for it in (item_type(), _lib.Fp8BlockItem()):
            it.w, it.scale = w.data_ptr(), sc.data_ptr()
            it.rows, it.cols, it.block_h, it.block_w = R, C, BLOCK, BLOCK
            it.scale_shape[0], it.scale_shape[1] = sc.shape
            it.sdt = _lib.F32
            (fused if isinstance(it, item_type) else deq).append(it)
        deq[-1].out = dense.data_ptr()
        row = _lib.W4Item()
        row.src, row.rows, row.cols, row.group = dense.data_ptr(), R, C, 16 if nv else 32
        row.dst, row.zp_packed = o[1][0].data_ptr(), o[1][1].data_ptr()
        if nv:
            fused[-1].packed, fused[-1].scale_f8, fused[-1].global_scale = (t.data_ptr() for t in o[0])
            fused[-1].key = keys[0].data_ptr() + 4 * i
            row.zp, row.scale = keys[1].data_ptr() + 4 * i, o[1][2].data_ptr()
        else:
            fused[-1].packed, fused[-1].e8m0 = o[0][0].data_ptr(), o[0][1].data_ptr()
        second.append(row)
    (ft, fb) = _upload(fused, item_type, lib.ct_fp8block_nvfp4_plan if nv else lib.ct_fp8block_mxfp8_plan, dev)
    (dt, db) = _upload(deq, _lib.Fp8BlockItem, lib.ct_fp8block_dequant_plan, dev)
    (st, sb) = _upload(second, _lib.W4Item, lib.ct_rtn_nvfp4_batch_plan if nv else lib.ct_rtn_group8_batch_plan, dev)
    lut = None if nv else codec._mx_code_table(torch.bfloat16, dev)
    keep += [ft, dt, st, lut]
    torch.cuda.synchronize(dev)
    bf = _lib.BF16

    if nv:
        def go_fused():
            keys[0].zero_()
            _lib.check(lib.ct_fp8block_nvfp4_amax_batch(ft.data_ptr(), n, fb, bf, s))
            _lib.check(lib.ct_fp8block_nvfp4_batch(ft.data_ptr(), n, fb, bf, s))

        def go_composed():
            _lib.check(lib.ct_fp8block_dequant_batch(dt.data_ptr(), n, db, bf, s))
            keys[1].zero_()
            _lib.check(lib.ct_rtn_nvfp4_amax_batch(st.data_ptr(), n, sb, bf, s))
            _lib.check(lib.ct_rtn_nvfp4_quant_pack_batch(st.data_ptr(), n, sb, bf, s))
    else:
        def go_fused():
            _lib.check(lib.ct_fp8block_mxfp8_batch(ft.data_ptr(), n, fb, bf, lut.data_ptr(), s))

        def go_composed():
            _lib.check(lib.ct_fp8block_dequant_batch(dt.data_ptr(), n, db, bf, s))
            _lib.check(lib.ct_rtn_quant_group8_batch(st.data_ptr(), n, sb, bf, codec._QP_MXFP8, 1, 0, lut.data_ptr(), s))
    return keep, go_fused, go_composed, outs


def launches(name, args):
    dev = torch.device("cuda:0")
    shp = shapes(name, args)
    codes = sum(R * C for _, R, C in shp)
    if codes < COLD_BYTES:
        raise SystemExit(f"{name}: {codes} bytes of codes are less than twice the Infinity Cache; the launches would not be HBM-cold")
    keep, fused, composed, outs = forms_of(args.target, shp, dev)
    fused()
    composed()
    torch.cuda.synchronize(dev)
    for i, (a, b) in enumerate(outs):  # faster and different is not faster
        if not all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b)):
            raise SystemExit(f"{name}: module {i} of the fused form differs from the composition")
    ts = alternated({"fused": fused, "composed": composed}, args.steps, args.warmup, dev)
    del keep, outs
    torch.cuda.empty_cache()
    f, c = ts["fused"], ts["composed"]
    nbytes = algorithmic_bytes(shp, args.target, 0)
    med = f[len(f) // 2]
    return {"modules": len(shp), "elements": codes, "fused_algorithmic_bytes": nbytes, "composed_algorithmic_bytes": algorithmic_bytes(shp, args.target, 1),
            "samples": len(f), "fused_s_median": med, "fused_s_min": f[0], "fused_s_max": f[-1],
            "composed_s_median": c[len(c) // 2], "composed_s_min": c[0], "composed_s_max": c[-1],
            "fused_TB_per_s": nbytes / med / 1e12, "fused_share_of_hbm_peak": nbytes / med / HBM_PEAK,
            "composed_over_fused_medians": c[len(c) // 2] / med, "fused_median_below_composed_min": med < c[0]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--target", choices=("mxfp8", "nvfp4"), required=True)
    p.add_argument("--layers", type=int, default=2, help="DeepSeek-shaped layers")
    p.add_argument("--experts", type=int, default=8, help="routed experts per DeepSeek-shaped layer")
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--run", type=int, default=1, help="tag of this run in its JSON line")
    p.add_argument("--out", default=None, help="a .jsonl file the line is appended to")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fp8block_transcode_bench needs an MI355X: nothing here is measured on a CPU")
    res = {"bench": f"fp8block_{args.target}", "run": args.run, "steps": args.steps, "warmup": args.warmup}
    for name in ("deepseek", "qwen3_4b"):
        res[name] = launches(name, args)
    res["fused_median_below_composed_min_on_both_tables"] = all(res[t]["fused_median_below_composed_min"] for t in ("deepseek", "qwen3_4b"))
    line = json.dumps(res)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
