"""The characterisation sweep of the seventeen `ct_*_plan` entries (tools/record_plan_tables.py records it into tests/plan_tables.json,
tests/test_plan_tables.py replays it).  The planners are host functions that look at pointers and never follow them, so every address here is
made up.  A case is plain data: the entry, its extra arguments, the table's input fields, and how it is called (n, NULL table)."""
import ctypes

F32, F16, BF16, I8, I64 = 0, 1, 2, 3, 7  # enum ct_dtype
SENTINEL = -7  # derived fields hold this before the call: a field the planner leaves alone shows as -7 (0xfffffff9 in g_magic / gen)

# struct name in _lib, the derived fields that are recorded; the rest of a struct's fields are inputs
STRUCTS = {
    "W4Item": ("first_block", "units", "upg_shift", "upg", "main_blocks", "g_magic", "g_shift"),
    # `gen` is a process-wide counter; `tpw` / `nwg` depend on the device's CU count: both left out of the record
    "BitmaskItem": ("is_float", "first_block", "units", "upr", "slots_offset", "mask_dwords"),
    "BitmaskDItem": ("single", "first_block"),
    "CopyItem": ("first_block",),
    "AwqItem": ("wide", "first_block", "weight_blocks", "zp_blocks"),
    "Fp8BlockItem": ("fast", "scale_stride", "units_per_row", "first_block"),
}
UNRECORDED = {"BitmaskItem": ("nwg", "tpw", "gen")}


def addr(i, k, off=0):
    """a 16-byte aligned made-up address of buffer k of item i, plus `off` bytes"""
    return 0x100000 * (i + 1) + 0x1000 * k + off


def w4(rows=8, cols=512, group=128, **kw):
    d = dict(src=("a", 0, 0), scale=("a", 1, 0), zp=("a", 2, 0), dst=("a", 3, 0), rows=rows, cols=cols, group=group, zp_packed=0)
    d.update(kw)
    return d


def blk(bh, bw):
    return -((bh << 24) | bw)


def off(k, o):
    return ("a", k, o)


def _sweep(entry, struct, args, good, refusals, cross, bad_args=()):
    """the cases the issue lists for one entry and one set of extra arguments"""
    tag = entry + ("" if not args else "[" + ",".join(map(str, args)) + "]")
    out = [dict(id=f"{tag}/admitted", entry=entry, struct=struct, args=list(args), items=good),
           dict(id=f"{tag}/n0", entry=entry, struct=struct, args=list(args), items=good, n=0),
           dict(id=f"{tag}/null0", entry=entry, struct=struct, args=list(args), items=None, n=0),
           dict(id=f"{tag}/null1", entry=entry, struct=struct, args=list(args), items=None, n=1),
           dict(id=f"{tag}/nneg", entry=entry, struct=struct, args=list(args), items=good, n=-1),
           dict(id=f"{tag}/cross", entry=entry, struct=struct, args=list(args), items=cross)]
    for label, item in refusals:  # the offending item is never first
        out.append(dict(id=f"{tag}/refuse:{label}", entry=entry, struct=struct, args=list(args), items=[good[0], item]))
    for a in bad_args:
        out.append(dict(id=f"{tag}/badarg:{a}", entry=entry, struct=struct, args=list(a), items=good))
    return out


def _ptr_refusals(make, null=(), mis=()):
    """one refusal per NULL pointer and per misalignment: (field, buffer index) resp. (field, buffer index, byte offset)"""
    return [(f"{f}=NULL", make(**{f: 0})) for f in null] + [(f"{f}+{o}", make(**{f: off(k, o)})) for f, k, o in mis]


BIG = (1 << 24, 1 << 20, 128)  # 2^41 units: past 2^31 workgroups for every ct_w4_item planner that counts units


def cases():
    c = []
    # ---- ct_w4_batch_plan
    for d in (0, 1):
        zpk = off(4, 0)
        good = [w4(5, 256, 32), w4(8, 512, 128), w4(3, 2048, 0), w4(16, 64, 64), w4(8, 512, 128, zp_packed=zpk)]
        if d == 1:
            good.append(w4(64, 1024, 128, zp_packed=zpk, zp=0))
        ref = [("rows=0", w4(rows=0)), ("cols=0", w4(cols=0)), ("cols%32", w4(cols=48, group=0)), ("g%32", w4(cols=96, group=48)), ("cols%g", w4(cols=512, group=96)),
               ("groups>2^31", w4(1, 1 << 37, 32))]
        ref += _ptr_refusals(w4, null=("src", "scale", "dst"), mis=(("src", 0, 8), ("dst", 3, 8)))
        if d == 0:
            ref.append(("zp_packed without zp", w4(zp=0, zp_packed=zpk)))
        else:
            ref += [("zpk:g!=128", w4(8, 512, 64, zp_packed=zpk)), ("zpk:cols%512", w4(8, 256, 128, zp_packed=zpk)), ("zpk:units>=2^31", w4(1 << 22, 1 << 12, 128, zp_packed=zpk)),
                    ("zpk:zp_packed+8", w4(zp_packed=off(4, 8))), ("zpk:scale+4", w4(scale=off(1, 4), zp_packed=zpk))]
        c += _sweep("ct_w4_batch_plan", "W4Item", (d,), good, ref, [w4(), w4(*BIG)], bad_args=[(2,), (-1,)] if d == 0 else ())
    # ---- ct_rtn_w4_batch_plan / ct_rtn_wb_batch_plan: the same item rule, dst 16- resp. 4-byte aligned
    rtn_ref = [("rows=0", w4(rows=0)), ("cols=0", w4(cols=0)), ("g%32", w4(cols=48, group=0)), ("g>2048", w4(cols=4096, group=0)), ("g!=32*2^k", w4(cols=192, group=96)),
               ("cols%g", w4(cols=160, group=64)), ("zp_packed", w4(zp_packed=off(4, 0)))] + _ptr_refusals(w4, null=("src", "dst", "scale"), mis=(("src", 0, 8),))
    rtn_good = [w4(5, 256, 32), w4(8, 512, 128), w4(3, 2048, 0), w4(16, 64, 64), w4(7, 1024, 2048)]
    c += _sweep("ct_rtn_w4_batch_plan", "W4Item", (), rtn_good, rtn_ref + [("dst+8", w4(dst=off(3, 8)))], [w4(), w4(*BIG)])
    for bits in (3, 6):
        c += _sweep("ct_rtn_wb_batch_plan", "W4Item", (bits,), rtn_good + [w4(dst=off(3, 4))], (rtn_ref if bits == 3 else []) + [("dst+2", w4(dst=off(3, 2)))], [w4(), w4(*BIG)],
                    bad_args=[(4,), (8,), (9,), (0,)] if bits == 3 else ())
    c.append(dict(id="ct_rtn_wb_batch_plan[4]/null1", entry="ct_rtn_wb_batch_plan", struct="W4Item", args=[4], items=None, n=1))  # the width is looked at first
    # ---- ct_q8_batch_plan: group / channel / whole-tensor items and block items
    for d in (0, 1):
        good = [w4(4, 256, 64), w4(8, 512, blk(4, 128)), w4(3, 2048, 0), w4(2, 64, 1 << 20), w4(128, 256, blk(128, 128))]
        ref = [("rows=0", w4(rows=0)), ("cols%16", w4(cols=24, group=0)), ("g%16", w4(cols=48, group=24)), ("cols%g", w4(cols=64, group=48)), ("group too large", w4(2, 1 << 35, 0)),
               ("blk:rows=0", w4(0, 512, blk(4, 128))), ("blk:bh=0", w4(8, 512, blk(0, 128))), ("blk:bw<16", w4(8, 512, blk(4, 8))), ("blk:bh!=2^k", w4(8, 512, blk(3, 128))),
               ("blk:bw!=2^k", w4(8, 192, blk(4, 48))), ("blk:cols%bw", w4(8, 192, blk(4, 128))), ("blk:numel>=2^34", w4(1 << 20, 1 << 14, blk(4, 128)))]
        ref += _ptr_refusals(w4, null=("src", "scale", "dst"), mis=(("src", 0, 8), ("dst", 3, 8)))
        ref += [("blk:" + label, it) for label, it in _ptr_refusals(lambda **kw: w4(8, 512, blk(4, 128), **kw), null=("src", "scale", "dst"), mis=(("src", 0, 8), ("dst", 3, 8)))]
        # the refusals do not look at the direction: swept once
        c += _sweep("ct_q8_batch_plan", "W4Item", (d,), good, ref if d == 0 else ref[:1], [w4(), w4(*BIG), w4(*BIG)], bad_args=[(2,)] if d == 0 else ())
    # ---- the one-pass 8-bit planners
    ch = lambda rows=4, cols=4096, **kw: w4(rows, cols, 0, **kw)  # noqa: E731
    c += _sweep("ct_rtn_channel8_batch_plan", "W4Item", (), [ch(4, 256), ch(4, 4096, zp=0), ch(4, 32768, zp=0), ch(9, 8192), ch(5, 2048, zp=0)],
                [("rows=0", ch(rows=0)), ("cols%8", ch(cols=12)), ("cols>65536", ch(cols=65544)), ("2^31 workgroups", ch(1 << 31, 4096, zp=0))] +
                _ptr_refusals(ch, null=("src", "dst", "scale"), mis=(("src", 0, 8), ("dst", 3, 8))), [ch(1 << 30, 4096, zp=0)] * 2)
    b8 = lambda rows=256, cols=512, b=(128, 128), **kw: w4(rows, cols, blk(*b), **kw)  # noqa: E731
    c += _sweep("ct_rtn_block8_batch_plan", "W4Item", (), [b8(), b8(100, 384, (64, 128)), b8(8, 64, (1, 16), zp=0), b8(300, 1024, (128, 128), dst=0), b8(7, 160, (4, 32))],
                [("group>=0", w4(256, 512, 128)), ("rows=0", b8(rows=0)), ("bh!=2^k", b8(b=(3, 128))), ("bw!=2^k", b8(cols=192, b=(4, 48))), ("bw<16", b8(b=(4, 8))),
                 ("bh*bw>16384", b8(b=(256, 128))), ("cols%bw", b8(cols=192)), ("2^31 blocks", b8(1 << 24, 1 << 20, (1, 16)))] +
                _ptr_refusals(b8, null=("src", "scale"), mis=(("src", 0, 8), ("dst", 3, 8))), [b8(1 << 20, 1 << 17, (1, 128))] * 2)
    g8 = lambda rows=8, cols=512, g=128, **kw: w4(rows, cols, g, **kw)  # noqa: E731
    c += _sweep("ct_rtn_group8_batch_plan", "W4Item", (), [g8(5, 256, 32), g8(), g8(3, 2048, 1024), g8(16, 64, 64, scale=0, zp_packed=off(4, 0)), g8(1, 32, 32, zp=0)],
                [("rows=0", g8(rows=0)), ("g<32", g8(g=16)), ("g%32", g8(cols=96, g=48)), ("g!=32*2^k", g8(cols=192, g=96)), ("g>1024", g8(cols=4096, g=2048)), ("cols%g", g8(cols=160, g=64)),
                 ("no scale output", g8(scale=0))] + _ptr_refusals(g8, null=("src", "dst"), mis=(("src", 0, 8), ("dst", 3, 8), ("scale", 1, 1))), [g8(), g8(*BIG)])
    # ---- the FP4 family
    nv = lambda rows=8, cols=512, **kw: w4(rows, cols, 16, **dict(dict(zp_packed=off(4, 0)), **kw))  # noqa: E731
    mx = lambda rows=8, cols=512, **kw: w4(rows, cols, 32, **dict(dict(zp_packed=off(4, 0), zp=0), **kw))  # noqa: E731
    for d in (0, 1):
        ref = [("rows=0", nv(rows=0)), ("cols=0", mx(cols=0)), ("group", w4(8, 512, 64, zp_packed=off(4, 0))), ("cols%g", mx(cols=48)), ("numel%32", nv(1, 16)),
               ("g16 without zp", nv(zp=0)), ("g32 with zp", mx(zp=off(2, 0)))] + _ptr_refusals(nv, null=("src", "scale", "dst", "zp_packed"), mis=(("dst", 3, 8), ("zp_packed", 4, 1)))
        ref += _ptr_refusals(mx, mis=(("src", 0, 8), ("scale", 1, 4)) if d == 0 else (("src", 0, 2),))
        c += _sweep("ct_fp4_batch_plan", "W4Item", (d,), [nv(), mx(5, 64), nv(3, 2048), mx(16, 96)] + ([mx(src=off(0, 4))] if d else []), ref, [nv(), nv(1 << 24, 1 << 20)],
                    bad_args=[(2,)] if d == 0 else ())
    ms = lambda rows=4096, **kw: w4(rows, 0, 0, **kw)  # noqa: E731
    c += _sweep("ct_mx_scale_batch_plan", "W4Item", (), [ms(), ms(1), ms(2049, src=off(0, 2)), ms(8, dst=off(3, 6))],
                [("rows=0", ms(0))] + _ptr_refusals(ms, null=("src", "dst"), mis=(("src", 0, 1), ("dst", 3, 1))), [ms(), ms(1 << 42)])
    c += _sweep("ct_rtn_mxfp4_batch_plan", "W4Item", (), [mx(), mx(5, 64), mx(3, 2048, scale=0), mx(16, 96, scale=off(1, 2))],
                [("rows=0", mx(rows=0)), ("cols=0", mx(cols=0)), ("group!=32", nv(zp=0)), ("cols%32", mx(cols=48))] +
                _ptr_refusals(mx, null=("src", "dst", "zp_packed"), mis=(("src", 0, 8), ("dst", 3, 8), ("scale", 1, 1))), [mx(), mx(1 << 24, 1 << 20)])
    c += _sweep("ct_rtn_nvfp4_batch_plan", "W4Item", (), [nv(), nv(5, 64), nv(3, 2048, zp=off(2, 4)), nv(16, 96, scale=off(1, 12))],
                [("rows=0", nv(rows=0)), ("cols=0", nv(cols=0)), ("group!=16", mx(zp=off(2, 0))), ("cols%32", nv(cols=48))] +
                _ptr_refusals(nv, null=("src", "dst", "zp_packed", "zp", "scale"), mis=(("src", 0, 8), ("dst", 3, 8), ("zp_packed", 4, 1), ("zp", 2, 2), ("scale", 1, 2))),
                [nv(), nv(1 << 24, 1 << 20)])
    zq = lambda rows=40, cols=64, **kw: w4(rows, cols, 0, **kw)  # noqa: E731
    c += _sweep("ct_zp4_batch_plan", "W4Item", (), [zq(), zq(1, 1), zq(33, 257), zq(64, 4, src=off(0, 1))],
                [("rows=0", zq(rows=0)), ("cols=0", zq(cols=0))] + _ptr_refusals(zq, null=("src", "dst")), [zq(), zq(1 << 24, 1 << 20)])
    # ---- the sparse tables
    bm = lambda rows=16, cols=256, dt=BF16, **kw: dict(dict(x=off(0, 0), values=off(1, 0), bitmask=off(2, 0), row_offsets=off(3, 0), total=off(4, 0), rows=rows, cols=cols,  # noqa: E731
                                                            values_capacity=rows * cols, dt=dt), **kw)
    wsb = ("workspace_bytes",)
    bm_ref = [("element size", bm(dt=I64)), ("mixed element sizes", bm(dt=F32)), ("rows=0", bm(rows=0)), ("cols%8", bm(cols=12)), ("values_capacity<0", bm(values_capacity=-1)),
              ("more than 1 GiB", bm(1 << 17, 8192))]
    bm_ref += _ptr_refusals(bm, null=("x", "values", "bitmask", "row_offsets", "total"), mis=(("x", 0, 8), ("values", 1, 8), ("total", 4, 4)))
    c += _sweep("ct_bitmask_batch_plan", "BitmaskItem", wsb, [bm(), bm(3, 8, F16), bm(64, 1024, bitmask=off(2, 2)), bm(5, 40, values_capacity=7)], bm_ref,
                [dict(bm(1 << 16, 8192), repeat=(1 << 18))], bad_args=[("null_workspace_bytes",)])
    for label, items in (("[i8]/admitted", [bm(16, 256, I8), bm(3, 16, I8), bm(7, 48, I8)]), ("[i8]/refuse:cols%16", [bm(16, 256, I8), bm(16, 24, I8)]),
                         ("[f32]/admitted", [bm(16, 256, F32), bm(3, 8, F32), bm(9, 40, F32)])):
        c.append(dict(id="ct_bitmask_batch_plan" + label, entry="ct_bitmask_batch_plan", struct="BitmaskItem", args=list(wsb), items=items))
    bd = lambda rows=16, cols=256, dt=BF16, **kw: dict(dict(values=off(0, 0), bitmask=off(1, 0), row_offsets=off(2, 0), out=off(3, 0), rows=rows, cols=cols, values_len=rows * cols // 2,  # noqa: E731
                                                            dt=dt), **kw)
    c += _sweep("ct_bitmask_decompress_batch_plan", "BitmaskDItem", (), [bd(), bd(4, 16384), bd(3, 8192), bd(5, 32, values=0, values_len=0), bd(2, 24576, bitmask=off(1, 4))],
                [("element size", bd(dt=I8)), ("mixed element sizes", bd(dt=F32)), ("rows=0", bd(rows=0)), ("cols%32", bd(cols=48)), ("values_len<0", bd(values_len=-1)),
                 ("values NULL with a length", bd(values=0))] + _ptr_refusals(bd, null=("bitmask", "row_offsets", "out"), mis=(("values", 0, 8), ("out", 3, 8), ("bitmask", 1, 2))),
                [bd(), bd(1 << 24, 1 << 20)])
    c.append(dict(id="ct_bitmask_decompress_batch_plan[f32]/admitted", entry="ct_bitmask_decompress_batch_plan", struct="BitmaskDItem", args=[],
                  items=[bd(16, 256, F32), bd(3, 4096, F32), bd(2, 16, F32), bd(5, 8192, F32)]))
    cp = lambda nbytes=100000, **kw: dict(dict(src=off(0, 0), dst=off(1, 0), bytes=nbytes), **kw)  # noqa: E731
    c += _sweep("ct_copy_batch_plan", "CopyItem", (), [cp(), cp(0, src=0, dst=0), cp(16384), cp(16385, src=off(0, 3)), cp(1)],
                [("bytes<0", cp(-1)), ("src=NULL", cp(src=0)), ("dst=NULL", cp(dst=0))], [cp(), cp(1 << 45)])
    # ---- the two converters' tables (their own cap, checked item by item)
    def aw(K=512, N=256, G=4, **kw):
        d = dict(qweight=off(0, 0), qzeros=off(1, 0), scales=off(2, 0), weight_packed=off(3, 0), zp_packed=off(4, 0), scale_t=off(5, 0), K=K, N=N, G=G, scale_shape=[G, N],
                 zp_shape=[G, N // 8], scale_dt=F16)
        d.update(kw)
        return d
    c += _sweep("ct_awq_repack_plan", "AwqItem", (), [aw(), aw(100, 24, 1, scale_dt=BF16), aw(qzeros=0, zp_packed=0, zp_shape=[0, 0]), aw(64, 64, 2, qweight=off(0, 4)), aw(300, 40, 3, weight_packed=off(3, 8))],
                [("qzeros without zp_packed", aw(zp_packed=0)), ("K=0", aw(K=0)), ("N>=2^31", aw(N=1 << 31)), ("N%8", aw(N=12)), ("scale dtype", aw(scale_dt=F32)),
                 ("scale shape", aw(scale_shape=[256, 4])), ("zp shape", aw(zp_shape=[4, 256]))] + _ptr_refusals(aw, null=("qweight", "scales", "weight_packed", "scale_t")),
                [aw(), aw(1 << 20, 1 << 20, 8), aw()])
    def fb(rows=256, cols=512, bh=128, bw=128, **kw):
        d = dict(w=off(0, 0), scale=off(1, 0), out=off(2, 0), rows=rows, cols=cols, block_h=bh, block_w=bw, scale_shape=[-(-rows // max(bh, 1)), -(-cols // max(bw, 1))], sdt=F32)
        d.update(kw)
        return d
    c += _sweep("ct_fp8block_dequant_plan", "Fp8BlockItem", (), [fb(), fb(100, 72, 64, 40, sdt=BF16), fb(scale_shape=[1, 4]), fb(scale_shape=[2, 1], sdt=F16), fb(33, 48, 16, 16, w=off(0, 4))],
                [("rows=0", fb(rows=0)), ("cols>=2^31", fb(cols=1 << 31)), ("block_h=0", fb(bh=0)), ("scale dtype", fb(sdt=I8)), ("scale shape", fb(scale_shape=[3, 4]))] +
                _ptr_refusals(fb, null=("w", "scale", "out")), [fb(), fb(1 << 20, 1 << 20), fb()])
    ids = [x["id"] for x in c]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    return c


def _value(v, i):
    return addr(i, v[1], v[2]) if isinstance(v, tuple) or (isinstance(v, list) and v and v[0] == "a") else v


def run_case(lib, _lib, case):
    """call the entry on the case's table; returns {"ret", "error", "items": [[derived fields of item 0], ...]} (plain JSON values)"""
    cls = getattr(_lib, case["struct"])
    derived = STRUCTS[case["struct"]]
    types = dict(cls._fields_)
    spec = case["items"]
    tab = None
    if spec is not None:
        rows = []
        for i, item in enumerate(spec):
            it = cls()
            for f in derived + UNRECORDED.get(case["struct"], ()):
                setattr(it, f, types[f](SENTINEL, SENTINEL) if hasattr(types[f], "_length_") else SENTINEL)
            for f, v in item.items():
                if f == "repeat":
                    continue
                v = _value(v, i)
                setattr(it, f, (types[f])(*v) if isinstance(v, list) else v)
            rows.append(bytes(it) * int(item.get("repeat", 1)))
        raw = b"".join(rows)
        tab = (cls * (len(raw) // ctypes.sizeof(cls))).from_buffer_copy(raw)
    n = case.get("n", 0 if tab is None else len(tab))
    args, ws = [], None
    for a in case["args"]:
        if a == "workspace_bytes":
            ws = ctypes.c_int64(SENTINEL)
            args.append(ctypes.addressof(ws))
        elif a == "null_workspace_bytes":
            args.append(None)
        else:
            args.append(a)
    ret = int(getattr(lib, case["entry"])(ctypes.cast(tab, ctypes.c_void_p) if tab is not None else None, n, *args))
    out = {"error": _lib.last_error() if ret < 0 else None}
    # ct_bitmask_batch_plan's count follows the device's CU count through tpw / nwg: only its sign is a function of the input
    out["ret"] = (min(ret, 0) if case["entry"] == "ct_bitmask_batch_plan" else ret)
    if ws is not None:
        out["workspace_bytes"] = ws.value
    shown = [] if tab is None else list(tab[:8]) + (list(tab[-2:]) if len(tab) > 10 else list(tab[8:]))  # a repeated item: both ends of the table
    out["items"] = [[list(getattr(it, f)) if hasattr(types[f], "_length_") else int(getattr(it, f)) for f in derived] for it in shown]
    return out
