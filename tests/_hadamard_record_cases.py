"""The characterisation sweeps of the rotation family (tools/record_hadamard.py records them, tests/test_hadamard_refusals.py and
tests/test_hadamard_plans.py replay them).

refusal_cases(): bad arguments for the six `ct_hadamard*` row / column entries and ct_hadamard_k_workspace_bytes.  The entries look at pointers
and never follow them before a launch, and every case here is refused before the first launch, so every address is made up.  The admitted side of a
size cap cannot be recorded as such (it would launch): it is paired with a misaligned tensor, whose refusal comes later and so shows that the cap
let the size through.

plan_cases(): arguments for plan_hadamard, plan_hadamard_k and plan_hadamard_perm (shapes and dtypes alone, no tensor)."""
F32, F16, BF16, I8 = 0, 1, 2, 3  # enum ct_dtype
X, OUT, WS, HK, SG, GI, GO = (0x100000 * i for i in range(1, 8))  # 16-byte aligned made-up addresses

# argument order of include/ct_hip.h without the trailing stream, and an admitted call of each entry
ENTRIES = {
    "ct_hadamard_rows": (("x", "out", "dt", "numel", "n", "acc64"), dict(x=X, out=OUT, dt=BF16, numel=4096, n=64, acc64=0)),
    "ct_hadamard_cols": (("x", "out", "ws", "dt", "rows", "cols", "n", "acc64"), dict(x=X, out=OUT, ws=WS, dt=BF16, rows=128, cols=32, n=64, acc64=0)),
    "ct_hadamard_k_rows": (("x", "out", "dt", "numel", "n", "k", "had_k", "signs", "transposed", "acc64", "ws"),
                           dict(x=X, out=OUT, dt=BF16, numel=4096, n=64, k=1, had_k=0, signs=SG, transposed=0, acc64=0, ws=0)),
    "ct_hadamard_k_cols": (("x", "out", "dt", "rows", "cols", "n", "k", "had_k", "signs", "transposed", "acc64", "ws"),
                           dict(x=X, out=OUT, dt=BF16, rows=128, cols=32, n=64, k=1, had_k=0, signs=SG, transposed=0, acc64=0, ws=WS)),
    "ct_hadamard_perm_rows": (("x", "out", "dt", "numel", "n", "acc64", "gin", "gout", "signs", "transposed"),
                              dict(x=X, out=OUT, dt=BF16, numel=4096, n=64, acc64=0, gin=GI, gout=GO, signs=0, transposed=0)),
    "ct_hadamard_perm_cols": (("x", "out", "ws", "dt", "rows", "cols", "n", "acc64", "gin", "gout", "signs", "transposed"),
                              dict(x=X, out=OUT, ws=WS, dt=BF16, rows=128, cols=32, n=64, acc64=0, gin=GI, gout=GO, signs=0, transposed=0)),
}
WORKSPACE_ARGS = ("dt", "numel", "n", "k", "acc64", "cols_form")


def _size(n):
    """an element count / row count that n divides"""
    return dict(size=4 * n)


def _common(cap32, cap64):
    """(label, overrides) for the checks every entry has; `size` stands for numel (row entries) or rows (column entries)"""
    mis = dict(x=X + 8)
    c = [("dt=I8", dict(dt=I8)), ("dt=-1", dict(dt=-1)), ("dt=9", dict(dt=9)),
         ("n=0", dict(n=0)), ("n=3", dict(n=3, size=12)), ("n=12", dict(n=12, size=48)), ("n=-8", dict(n=-8)),
         ("size%n", dict(size=100)), ("size<0", dict(size=-64)),
         ("acc64=2", dict(acc64=2)), ("acc64=-1", dict(acc64=-1)),
         ("n>cap32", dict(n=2 * cap32, **_size(2 * cap32))), ("n>cap64", dict(n=2 * cap64, acc64=1, **_size(2 * cap64))),
         ("n=cap32,x+8", dict(n=cap32, **_size(cap32), **mis)), ("n=cap64,x+8", dict(n=cap64, acc64=1, **_size(cap64), **mis)),
         ("x+8", mis), ("x+2", dict(x=X + 2)), ("out+8", dict(out=OUT + 8)), ("x+8,out+8", dict(x=X + 8, out=OUT + 8)),
         # two at once: the first in the entry's order answers
         ("dt=I8,n=3", dict(dt=I8, n=3)), ("n=3,size%n", dict(n=3, size=100)), ("size%n,acc64=2", dict(size=100, acc64=2)),
         ("acc64=2,n>cap32", dict(acc64=2, n=2 * cap32, **_size(2 * cap32))), ("n>cap32,x+8", dict(n=2 * cap32, **_size(2 * cap32), **mis)),
         ("dt=I8,x+8", dict(dt=I8, **mis)), ("n=0,acc64=2", dict(n=0, acc64=2))]
    return c


_K = [("transposed=2", dict(transposed=2)), ("transposed=-1", dict(transposed=-1)),
      ("k=3,had_k=NULL", dict(n=12, k=3, size=48)), ("k=1,had_k", dict(had_k=HK)),
      ("n%k", dict(n=64, k=3, had_k=HK)), ("n/k!=2^m", dict(n=36, k=3, had_k=HK, size=72)), ("k=0", dict(k=0)), ("k=-1", dict(k=-1)),
      ("k=257", dict(n=257 * 8, k=257, had_k=HK, **_size(257 * 8))), ("k=256,x+8", dict(n=2048, k=256, had_k=HK, **_size(2048), x=X + 8)),
      ("k=3,n>32768", dict(n=3 * 16384, k=3, had_k=HK, **_size(3 * 16384))),
      ("k=3,run=8192", dict(n=3 * 8192, k=3, had_k=HK, **_size(3 * 8192))), ("k=3,run=4096,x+8", dict(n=3 * 4096, k=3, had_k=HK, **_size(3 * 4096), x=X + 8)),
      ("k=3,f32,run=8192", dict(dt=F32, n=3 * 8192, k=3, had_k=HK, **_size(3 * 8192))), ("k=3,acc64,run=8192", dict(acc64=1, n=3 * 8192, k=3, had_k=HK, **_size(3 * 8192))),
      ("k=3,mfma,run=128,x+8", dict(n=384, k=3, had_k=HK, **_size(384), x=X + 8)),
      ("signs+4", dict(signs=SG + 4)), ("signs+1", dict(signs=SG + 1)), ("signs=NULL,x+8", dict(signs=0, x=X + 8)),
      ("acc64=2,transposed=2", dict(acc64=2, transposed=2)), ("transposed=2,k=1,had_k", dict(transposed=2, had_k=HK)),
      ("k=1,had_k,n>cap", dict(had_k=HK, n=32768, **_size(32768))), ("k=257,n>32768", dict(n=257 * 256, k=257, had_k=HK, **_size(257 * 256))),
      ("n>32768,run", dict(n=3 * 16384, k=3, had_k=HK, dt=F32, **_size(3 * 16384))), ("run,x+8", dict(n=3 * 8192, k=3, had_k=HK, **_size(3 * 8192), x=X + 8)),
      ("x+8,signs+4", dict(x=X + 8, signs=SG + 4)), ("n=12,k=1", dict(n=12, k=1, size=48))]

_P = [("transposed=2", dict(transposed=2)), ("gin=NULL", dict(gin=0)), ("gout=NULL", dict(gout=0)), ("gin+8", dict(gin=GI + 8)), ("gout+8", dict(gout=GO + 8)),
      ("gin+2", dict(gin=GI + 2)), ("signs+4", dict(signs=SG + 4)), ("signs,x+8", dict(signs=SG, x=X + 8)),
      ("acc64=2,transposed=2", dict(acc64=2, transposed=2)), ("transposed=2,gin=NULL", dict(transposed=2, gin=0)),
      ("gin=NULL,n>cap", dict(gin=0, n=32768, **_size(32768))), ("x+8,gin+8", dict(x=X + 8, gin=GI + 8)), ("gout+8,signs+4", dict(gout=GO + 8, signs=SG + 4))]

_COLS = [("rows<0", dict(rows=-64)), ("cols<0", dict(cols=-1)), ("ws=NULL", dict(ws=0)), ("ws+8", dict(ws=WS + 8)),
         ("2^31 tiles", dict(rows=1 << 22, cols=1 << 21)),
         ("rows<0,dt=I8", dict(rows=-64, dt=I8)), ("cols<0,n=3", dict(cols=-1, n=3)), ("dt=I8,ws=NULL", dict(dt=I8, ws=0)), ("x+8,ws=NULL", dict(x=X + 8, ws=0)),
         ("ws=NULL,2^31 tiles", dict(ws=0, rows=1 << 22, cols=1 << 21)), ("ws=NULL,cols=0", dict(ws=0, cols=0)), ("ws+8,rows=0", dict(ws=WS + 8, rows=0))]

# refused inside the row dispatch, after the checks and before the launch
_ROWS = {
    "ct_hadamard_rows": [("2^31 workgroups", dict(n=8, numel=1 << 43)), ("2^31 workgroups,acc64", dict(n=512, numel=1 << 43, acc64=1))],
    "ct_hadamard_k_rows": [("2^31 workgroups", dict(n=8, numel=1 << 43)), ("signs=NULL,2^31 workgroups", dict(n=8, numel=1 << 43, signs=0)),
                           ("valu,ws=NULL", dict(dt=F32, n=12, k=3, had_k=HK, numel=48)), ("valu,ws+8", dict(dt=F32, n=12, k=3, had_k=HK, numel=48, ws=WS + 8)),
                           ("valu,acc64,ws=NULL", dict(acc64=1, n=96, k=3, had_k=HK, numel=96)), ("valu,run=4,ws=NULL", dict(n=12, k=3, had_k=HK, numel=48)),
                           ("valu,2^31 workgroups", dict(dt=F32, n=12, k=3, had_k=HK, numel=12 << 40, ws=WS))],
    "ct_hadamard_perm_rows": [("2^31 workgroups", dict(n=8, numel=1 << 43)), ("2^31 workgroups,signs", dict(n=256, numel=1 << 43, signs=SG, transposed=1))],
}


def refusal_cases():
    out = []
    for entry, (order, good) in ENTRIES.items():
        perm, k, cols = "perm" in entry, "_k_" in entry, entry.endswith("cols")
        sweep = _common(16384, 8192 if perm else 16384) + (_K if k else []) + (_P if perm else []) + (_COLS if cols else []) + _ROWS.get(entry, [])
        for label, over in sweep:
            args = dict(good)
            for key, v in over.items():
                args["rows" if cols and key == "size" else "numel" if key == "size" else key] = v
            out.append(dict(id=f"{entry}/{label}", entry=entry, args=[args[a] for a in order]))
    ws = dict(dt=BF16, numel=4096, n=64, k=1, acc64=0, cols_form=0)
    for label, over in [("butterfly", {}), ("butterfly,cols", dict(cols_form=1)), ("butterfly,cols,odd", dict(numel=36, n=4, cols_form=1)), ("f32,cols,odd", dict(dt=F32, numel=3, n=1, cols_form=2)),
                        ("mfma", dict(n=96, k=3, numel=960)), ("mfma,cols", dict(n=96, k=3, numel=960, cols_form=1)), ("valu:f32", dict(dt=F32, n=12, k=3, numel=1200)),
                        ("valu:acc64", dict(n=96, k=3, numel=960, acc64=1)), ("valu:run<8,cols", dict(n=12, k=3, numel=36, cols_form=1)), ("valu:run>128", dict(n=768, k=3, numel=768)),
                        ("valu:lds", dict(n=241 * 128, k=241, numel=241 * 128)), ("mfma:lds", dict(n=240 * 128, k=240, numel=240 * 128)), ("valu:n>32768", dict(n=3 * 16384, k=3, numel=3 * 16384)),
                        ("numel=0", dict(numel=0)), ("numel%n", dict(numel=100)), ("acc64=2,valu", dict(dt=F32, n=12, k=3, numel=12, acc64=2)),
                        ("dt=I8", dict(dt=I8)), ("dt=-1", dict(dt=-1)), ("numel<0", dict(numel=-1)), ("n=0", dict(n=0)), ("k=0", dict(k=0)), ("n%k", dict(n=64, k=3)), ("k=-1", dict(k=-1)),
                        ("dt=I8,n=0", dict(dt=I8, n=0))]:
        out.append(dict(id=f"ct_hadamard_k_workspace_bytes/{label}", entry="ct_hadamard_k_workspace_bytes", args=[dict(ws, **over)[a] for a in WORKSPACE_ARGS]))
    return out


def run_refusal(lib, case):
    """{ret, error}: the entry's return value and ct_last_error's text (None for the workspace query, which sets none)"""
    fn = getattr(lib, case["entry"])
    if case["entry"] == "ct_hadamard_k_workspace_bytes":
        return dict(ret=int(fn(*case["args"])), error=None)
    ret = int(fn(*case["args"], None))
    msg = lib.ct_last_error()
    return dict(ret=ret, error=msg.decode("utf-8", "replace") if msg else None)


# ---- the Python plans ------------------------------------------------------------------------------------------------------------------
DTYPES = ("bfloat16", "float16", "float32", "int32")
PRECISIONS = ("float32", "float64", "bfloat16", "float16")


def _shapes(n):
    return [(), (n,), (n, 1), (3, n), (n, 3), (2, n, 3), (2, 3, 2 * n)]


def _plan(fn, shape, dtype="bfloat16", size=64, dim=-1, precision="float32", **kw):
    d = dict(fn=fn, shape=list(shape), dtype=dtype, size=size, dim=dim, precision=precision, kw=kw)
    d["id"] = fn + ":" + ",".join(str(v) for v in (tuple(shape), dtype, size, dim, precision)) + "".join(f",{a}={v}" for a, v in sorted(kw.items()))
    return d


def plan_cases():
    """plan_hadamard and plan_hadamard_k at k = 3 take the whole sweep; the other k and plan_hadamard_perm, which adds the form to the base plan it calls,
    take every shape at four dims, the sizes around their own caps and every `form`"""
    c = []
    sizes = {1: [0, -4, 1, 2, 12, 96, 512, 1024, 4096, 8192, 16384, 32768, 65536],
             # around the caps of the mix: k, n, the run of the vector form, the staged row of the matrix-core form
             3: [0, 1, 2, 12, 96, 3 * 128, 3 * 256, 3 * 4096, 3 * 8192, 3 * 16384],
             12: [0, 1, 2, 12, 96, 12 * 4, 12 * 8, 12 * 2048, 12 * 4096],
             240: [240 * 128], 241: [241 * 128], 256: [256 * 8, 256 * 256], 257: [257 * 8], 0: [64], -1: [64]}
    for fn, ks in (("plan_hadamard", (1,)), ("plan_hadamard_k", tuple(sizes)), ("plan_hadamard_perm", (1, 3)), ("plan_hadamard_perm:random", (1,))):
        name, random = fn.split(":")[0], fn.endswith("random")
        extra = dict(random=True) if random else {}
        for k in ks:
            kk = {} if name == "plan_hadamard" else dict(k=k)
            full = (name, k) in (("plan_hadamard", 1), ("plan_hadamard_k", 3))
            perm = name == "plan_hadamard_perm"
            n = 64 if k == 1 else 96 if k in (3, 12) else None
            if not perm or (k == 1 and not random):  # sizes x accumulators
                for size in sizes[k]:
                    for precision in PRECISIONS[:2]:
                        c.append(_plan(name, (3, 2 * size if size > 0 else 8), "bfloat16", size, -1, precision, **kk, **extra))
            if n is None:
                continue
            for shape in _shapes(n):  # shapes x dims
                for dim in range(-4, 4) if full else (-1, 0, 1, 3):
                    c.append(_plan(name, shape, "bfloat16", n, dim, **kk, **extra))
            for kw in (dict(device_type="cpu"), dict(contiguous=False), dict(device_type="cpu", contiguous=False), dict(device_type="meta")):
                c.append(_plan(name, (3, n), "bfloat16", n, -1, **kw, **kk, **extra))
            if full or (perm and k == 1 and not random):
                for dtype in DTYPES:  # dtypes x precisions, row and column form (the workspace of the column form)
                    for precision in PRECISIONS:
                        for shape, dim in (((3, n), -1), ((n, 3), 0)) if precision in PRECISIONS[:2] and dtype != "int32" else (((3, n), -1),):
                            c.append(_plan(name, shape, dtype, n, dim, precision, **kk, **extra))
                # two conditions at once: the first in the planner's order answers
                big = 65536 if k == 1 else k * 16384
                for shape, dtype, size, dim, precision, kw in [
                        ((3, n), "bfloat16", 0, 5, "float32", {}), ((), "bfloat16", 7 * k, 0, "float32", {}), ((), "bfloat16", n, 0, "float32", {}), ((3, n), "bfloat16", n, 2, "bfloat16", {}),
                        ((3, n + 1), "bfloat16", n, 5, "float32", {}), ((3, n + 1), "bfloat16", n, -1, "bfloat16", {}), ((3, n), "int32", n, -1, "float16", {}),
                        ((3, n), "int32", n, -1, "int32", {}), ((3, n), "int32", n, -1, "float32", dict(device_type="cpu")), ((3, n), "bfloat16", n, -1, "float32", dict(device_type="cpu", contiguous=False)),
                        ((3, big), "bfloat16", big, -1, "float32", dict(contiguous=False)), ((2, big, 3), "bfloat16", big, 1, "float32", {}), ((2, n, 3), "bfloat16", n, 1, "float64", dict(contiguous=False)),
                        ((2, n, 3), "int32", n, 1, "float32", {}), ((0, n), "bfloat16", n, -1, "float32", {}), ((n, 0), "bfloat16", n, 0, "float32", {}), ((0,), "bfloat16", n, 0, "float32", {}),
                        ((2, 0, 3), "bfloat16", n, 1, "float32", {}), ((3, 1), "bfloat16", 1, 0, "float32", {}), ((2, 3, 4), "bfloat16", 1, 1, "float32", {})]:
                    c.append(_plan(name, shape, dtype, size, dim, precision, **kw, **kk, **extra))
            if perm:
                fsizes = [n] + ([512, 1024, 8192, 16384, 32768] if k == 1 and not random else [16384] if k == 1 else [k * 4096])
                for form in (None, "fused", "composed", "x"):
                    for size in fsizes:
                        for precision in PRECISIONS[:2]:
                            for shape, dim in (((3, size), -1), ((size, 3), 0), ((2, size, 3), 1)) if size == n else (((3, size), -1),):
                                c.append(_plan(name, shape, "bfloat16", size, dim, precision, form=form, **kk, **extra))
                    c.append(_plan(name, (3, n), "int32", n, -1, form=form, **kk, **extra))
                    c.append(_plan(name, (3, n), "bfloat16", 0, -1, form=form, **kk, **extra))
                    c.append(_plan(name, (3, n), "bfloat16", n, -1, "float16", form=form, **kk, **extra))
    return list({x["id"]: x for x in c}.values())  # the sweeps overlap: a case is kept once


def _enc(v):
    """a plan as JSON: a named tuple becomes [type name, fields...]"""
    if isinstance(v, tuple) and hasattr(v, "_fields"):
        return [type(v).__name__] + [_enc(x) for x in v]
    if isinstance(v, (tuple, list)):
        return [_enc(x) for x in v]
    return v


def run_plan(codec, case):
    """{"plan": ...} (a permuted plan with what launches() counts) or {"raises": [type, message]}"""
    import torch

    fn = getattr(codec, case["fn"])
    try:
        plan = fn(tuple(case["shape"]), getattr(torch, case["dtype"]), case["size"], dim=case["dim"], precision=getattr(torch, case["precision"]), **case["kw"])
    except Exception as e:  # noqa: BLE001  (the record holds whatever the planner raises)
        return dict(raises=[type(e).__name__, str(e)])
    out = dict(plan=_enc(plan))
    if hasattr(plan, "launches"):
        out["launches"] = plan.launches()
    return out
