"""The sweep behind tests/hostpath_plans.json: the twelve module-loop entries and the five finish functions of csrc/host/ct_hostpath.cpp called DIRECTLY
(not through the compressors) on small CPU trees, and everything they hand back written down with pointers replaced by symbols.  Shared by
tools/record_hostpath_plans.py (writes the record) and tests/test_hostpath_plans.py (replays it).  CPU only: `set_allow_cpu(True)`.

Per call the record holds the batch keys in returned order, `n` and the second table's `n`, every row of both tables (all words of struct ct_w4_item; a pointer
word reads `m<i>.<entry>` when it is the data pointer of an entry module i held before the call, else `new<k>=<where it ended up after the finish>` with
`temp` for an allocation no module holds afterwards), the indices of `rest`, every job tuple element by kind, and after the finish every module's entries
(names, order, kinds, trainability, shapes, dtypes: `_state`) and status.  A module a loop hands back stays as it is for the case's next call.  The two
`wb_*` loops build no table: their record holds the launches the stand-ins bound through `bind_pack` saw (none on CPU tensors, where the loops skip the
call), `rest`, the entries that are still the tensors they were, and the modules' entries."""
import ctypes
import re

import torch

SHAPES = [(64, 256), (32, 512), (96, 128), (20, 256)]  # (20 rows: the packed zero points round up; 256 and 128 columns: no multiple of 512)
POINTER_WORDS = (0, 1, 2, 3, 10)  # src, scale, zp, dst, zp_packed of struct ct_w4_item (include/ct_hip.h)
HALF_AT = (1, 3)  # the modules of every tree that are float16 (the others bfloat16): more than one batch key per call

_W4 = dict(num_bits=4, type="int", strategy="group", group_size=128, symmetric=True)
_FP8 = dict(num_bits=8, type="float", strategy="channel", symmetric=True)
_NV = dict(num_bits=4, type="float", strategy="tensor_group", symmetric=True, group_size=16, scale_dtype="float8_e4m3fn")
_MX4 = dict(num_bits=4, type="float", strategy="group", symmetric=True, group_size=32, scale_dtype="uint8")
_MX8 = dict(num_bits=8, type="float", strategy="group", symmetric=True, group_size=32, scale_dtype="uint8")
_I8 = dict(num_bits=8, type="int", strategy="channel", symmetric=True)


def _case(cid, family, weights, scale, zp, **kw):
    return dict(id=cid, family=family, weights=weights, scale=scale, zp=zp, **kw)


def cases():
    out = []
    for v in ("plain", "trainable_scale", "buffer_zp", "odd_class", "g_idx"):
        out.append(_case("w4/" + v, "w4", _W4, "g128", "int8", flags={} if v == "plain" else {v: True}))
    out.append(_case("w4/asymmetric", "w4", dict(_W4, symmetric=False), "g128", "int8", rounds=2))
    static_in = dict(num_bits=8, type="float", strategy="tensor", symmetric=True)
    out += [
        _case("q8/fp8", "q8", _FP8, "channel", None),
        _case("q8/fp8_zero_point", "q8", _FP8, "channel", "float8_e4m3fn", rounds=2),
        _case("q8/fp8_static_input", "q8", _FP8, "channel", "float8_e4m3fn", input=static_in),
        _case("q8/int8_channel", "q8", _I8, "channel", "int8"),
        _case("q8/int8_asymmetric_group", "q8", dict(_I8, strategy="group", group_size=128, symmetric=False), "g128", "int8"),
        _case("q8/int8_tensor", "q8", dict(_I8, strategy="tensor"), "tensor", "int8"),
        _case("q8/int6", "q8", dict(_I8, num_bits=6), "channel", "int8"),
        _case("q8/block", "q8", dict(_FP8, strategy="block", block_structure=[16, 128]), "block", "float8_e4m3fn"),
        _case("q8/float32", "q8", _FP8, "channel", "float8_e4m3fn", other_dtype="float32"),
        _case("mx8/mxfp8", "mx8", _MX8, "g32", "float8_e4m3fn", rounds=2),
        _case("w8/channel", "w8", _I8, "channel", "int8", rounds=2),
        _case("w8/group", "w8", dict(_I8, strategy="group", group_size=128), "g128", "int8"),
        _case("w8/odd_cols", "w8", _I8, "channel", "int8", shapes=SHAPES[:3] + [(20, 264)]),
        _case("w8/activations", "w8", _I8, "channel", "int8", input=dict(num_bits=8, type="int", strategy="tensor", symmetric=True, dynamic=True)),
        _case("fp4/nvfp4/plain", "fp4", _NV, "g16", None, rounds=2),
        _case("fp4/nvfp4/f32_scale", "fp4", _NV, "g16", None, scale_dtype="float32"),
        _case("fp4/nvfp4/odd_global_scale", "fp4", _NV, "g16", None, odd_global_scale=True),
        _case("fp4/nvfp4/other_scale_dtype", "fp4", dict(_NV, scale_dtype="uint8"), "g16", None),
        _case("fp4/mxfp4/plain", "fp4", _MX4, "g32", None),
        _case("fp4/mxfp4/other_scale_dtype", "fp4", dict(_MX4, scale_dtype="float8_e4m3fn"), "g32", None),
    ]
    wb = dict(num_bits=3, type="int", strategy="group", group_size=128, symmetric=True)
    out += [
        _case("wb/w3_group", "wb", wb, "g128", "int8"),
        _case("wb/w6_channel", "wb", dict(wb, num_bits=6, strategy="channel", group_size=None), "channel", "int8"),
        _case("wb/w2_asymmetric", "wb", dict(wb, num_bits=2, symmetric=False), "g128", "int8"),
        _case("wb/w4_g_idx", "wb", _W4, "g128", "int8", flags={"g_idx": True}),
    ]
    return out


def _args(cta, spec):
    spec = dict(spec)
    if "scale_dtype" in spec:
        spec["scale_dtype"] = getattr(torch, spec["scale_dtype"])
    return cta.QuantizationArgs(**{k: v for k, v in spec.items() if v is not None})


def _put(m, name, tensor):
    """replace (or add as a parameter) entry `name`, keeping its place, its kind (parameter / buffer) and its trainability"""
    if name in m._buffers:
        m._buffers[name] = tensor
        return
    old = m._parameters.get(name)
    m._parameters[name] = torch.nn.Parameter(tensor, requires_grad=bool(old is not None and old.requires_grad and tensor.is_floating_point()))


def _take(m, name):
    m._parameters.pop(name, None)
    m._buffers.pop(name, None)


def _scale_shape(kind, r, c):
    return {"g128": (r, c // 128), "channel": (r, 1), "tensor": (1,), "block": (r // 16, c // 128), "g16": (r, c // 16), "g32": (r, c // 32)}[kind]


def build(cta, case):
    """the case's tree through test_host_logic._tree, then the entries the case's format has; returns (root, its quantized Linear modules, scheme)"""
    from test_host_logic import _tree

    ia = _args(cta, case["input"]) if case.get("input") else None
    scheme = cta.QuantizationScheme(targets=["Linear"], weights=_args(cta, case["weights"]), input_activations=ia)
    root = _tree(cta, scheme, [tuple(s) for s in case.get("shapes", SHAPES)], **case.get("flags", {}))
    mods = [m for m in root.modules() if isinstance(m, torch.nn.Linear)]
    for k, m in enumerate(mods):
        r, c = m.weight.shape
        wdt = getattr(torch, case.get("other_dtype", "float16")) if k in HALF_AT else torch.bfloat16
        shape = _scale_shape(case["scale"], r, c)
        _put(m, "weight", torch.zeros(r, c, dtype=wdt))
        _put(m, "weight_scale", torch.ones(shape, dtype=getattr(torch, case["scale_dtype"]) if case.get("scale_dtype") else wdt))
        if case["zp"] is None:
            _take(m, "weight_zero_point")
        else:
            _put(m, "weight_zero_point", torch.zeros(shape, dtype=getattr(torch, case["zp"])))
        if case["family"] == "fp4" and case["weights"]["group_size"] == 16:
            _put(m, "weight_global_scale", torch.ones(1, dtype=torch.float64 if case.get("odd_global_scale") and k == 0 else torch.float32))
        if ia is not None and not case["input"].get("dynamic"):
            _put(m, "input_scale", torch.ones(1, dtype=wdt))
            _put(m, "input_zero_point", torch.zeros(1, dtype=torch.float8_e4m3fn))
    return root, mods, scheme


def _plans(hp, case, scheme):
    """{direction: (plan(modules) -> (batches, rest), finish(jobs, status))} of a table family, with `infos` as the compressors pass them: a callable per scheme"""
    from compressed_tensors_amd.compressors.base import zp_drop_mask
    from compressed_tensors_amd.compressors.naive_quantized import base as nq
    from compressed_tensors_amd.compressors.pack_quantized import base as pq

    fam = case["family"]
    if fam == "w4":
        return {"compress": (lambda ms: hp.w4_plan_compress(ms, pq._compress_info), hp.w4_finish_compress),
                "decompress": (lambda ms: hp.w4_plan_decompress(ms, pq._decompress_info), hp.w4_finish_decompress)}
    if fam == "w8":
        return {"compress": (lambda ms: hp.w8_plan_compress(ms, pq._w8_info), hp.w4_finish_compress),
                "decompress": (lambda ms: hp.w8_plan_decompress(ms, pq._w8_info), hp.w4_finish_decompress)}
    if fam == "q8":
        return {"compress": (lambda ms: hp.q8_plan_compress(ms, nq._q8_compress_info), hp.q8_finish),
                "decompress": (lambda ms: hp.q8_plan_decompress(ms, nq._q8_decompress_info), hp.q8_finish)}
    info = lambda s: 1 | (zp_drop_mask(s) << 1)
    if fam == "mx8":
        return {"compress": (lambda ms: hp.mx8_plan_compress(ms, info), hp.mx8_finish), "decompress": (hp.mx8_plan_decompress, hp.mx8_finish)}
    group = int(case["weights"]["group_size"])
    want = torch.float8_e4m3fn if group == 16 else torch.uint8
    fp4_info = lambda s: info(s) if (getattr(s.weights, "scale_dtype", None) or want) is want else 0  # as compressors/fp4/base.py
    return {"compress": (lambda ms: hp.fp4_plan_compress(ms, fp4_info, group), lambda jobs, st: hp.fp4_finish(jobs, st, True)),
            "decompress": (lambda ms: hp.fp4_plan_decompress(ms, group), lambda jobs, st: hp.fp4_finish(jobs, st, False))}


def _entries(mods):
    """{data pointer: "m<i>.<entry>"} of every tensor the modules hold"""
    held = {}
    for i, m in enumerate(mods):
        for name, t in list(m._parameters.items()) + list(m._buffers.items()):
            if t is not None:
                held.setdefault(t.data_ptr(), f"m{i}.{name}")
    return held


class _Symbols:
    def __init__(self, mods):
        self.before, self.new = _entries(mods), {}

    def of(self, ptr):
        if ptr == 0:
            return 0
        return self.before.get(ptr) or self.new.setdefault(ptr, f"new{len(self.new)}")

    def resolve(self, mods, record):
        """`new<k>` -> `new<k>=<the entry that holds it now, or temp>` throughout `record`"""
        after = _entries(mods)
        final = {sym: f"{sym}={after.get(ptr, 'temp')}" for ptr, sym in self.new.items()}

        def walk(x):
            if isinstance(x, list):
                return [walk(y) for y in x]
            if isinstance(x, dict):
                return {k: walk(y) for k, y in x.items()}
            return re.sub(r"\bnew\d+\b", lambda m: final.get(m.group(), m.group()), x) if isinstance(x, str) else x

        return walk(record)


_SHORT = {"torch.bfloat16": "bf16", "torch.float16": "f16", "torch.float32": "f32", "torch.float8_e4m3fn": "f8", "torch.int8": "i8", "torch.int32": "i32",
          "torch.int64": "i64", "torch.uint8": "u8"}


def _state(m):
    """`status | name:P[shape]dtype ...` in dictionary order — P a Parameter, P* a trainable one, B a buffer, `name:-` a None entry"""
    from test_host_logic import _module_state_no_ptr

    params, buffers = _module_state_no_ptr(m)
    one = lambda k, v, kind: f"{k}:-" if v is None else f"{k}:{kind}{list(v[-2] if kind != 'B' else v[-1])}{_SHORT.get(str(v[-1]), '') if kind != 'B' else ''}".replace(" ", "")
    status = None if not hasattr(m, "quantization_status") else str(getattr(m.quantization_status, "value", m.quantization_status))
    return " ".join([f"{status} |"] + [one(k, v, "P" if v is None or v[0] == "Parameter" and not v[1] else "P*" if v[0] == "Parameter" else v[0]) for k, v in params]
                    + [one(k, v, "B") for k, v in buffers])


def pack(results):
    """{case id: calls} as the record file holds it: the modules' states, which repeat from call to call, once in a table and by index in the calls"""
    table = []
    for calls in results.values():
        for c in calls:
            c["modules"] = [table.index(s) if s in table else (table.append(s) or len(table) - 1) for s in c["modules"]]
    return {"states": table, "cases": results}


def unpack(doc):
    return {k: [dict(c, modules=[doc["states"][i] for i in c["modules"]]) for c in calls] for k, calls in doc["cases"].items()}


def _job(job, mods, syms):
    out = []
    for x in job:
        if isinstance(x, torch.nn.Module):
            out.append(f"module:m{[id(m) for m in mods].index(id(x))}")
        elif isinstance(x, torch.Tensor):
            out.append(("param:" if isinstance(x, torch.nn.Parameter) else "tensor:") + str(syms.of(x.data_ptr())))
        else:
            out.append("none" if x is None else f"{type(x).__name__}:{x}")
    return " ".join(out)


def _table(words, n, syms):
    width = words.numel() // n if n else 0
    rows = words.reshape(n, width).tolist() if n else []
    return [" ".join(str(syms.of(w) if k in POINTER_WORDS else w) for k, w in enumerate(r)) for r in rows]


def _status(direction):
    from compressed_tensors_amd.quantization.quant_args import QuantizationStatus

    return QuantizationStatus.COMPRESSED if direction == "compress" else QuantizationStatus.DECOMPRESSED


def _run_tables(hp, case, mods, scheme, keep):
    calls = []
    plans = _plans(hp, case, scheme)
    for rnd in range(case.get("rounds", 1)):
        for direction in ("compress", "decompress"):
            plan, finish = plans[direction]
            keep += [t for m in mods for t in list(m._parameters.values()) + list(m._buffers.values())]  # no address of an old entry is handed out again
            syms = _Symbols(mods)
            batches, rest = plan(list(mods))
            rec = {"call": f"{direction}{rnd}", "keys": [list(k) for k in batches], "batches": [], "rest": [[id(m) for m in mods].index(id(m)) for m in rest]}
            for words, n, jobs, aux_words, aux_n in batches.values():
                keep += [words, aux_words, jobs]
                rec["batches"].append({"n": n, "aux_n": aux_n, "rows": _table(words, n, syms), "aux_rows": _table(aux_words, aux_n, syms),
                                       "jobs": [_job(j, mods, syms) for j in jobs]})
            for _, _, jobs, _, _ in batches.values():
                finish(jobs, _status(direction))
            rec = syms.resolve(mods, rec)
            rec["modules"] = [_state(m) for m in mods]
            calls.append(rec)
    return calls


V, L, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
_PACK_TYPES = (ctypes.CFUNCTYPE(I, V, I, V, I, V, I, L, L, L, L, L, V, I, I, V, V), ctypes.CFUNCTYPE(I, V, L, L, L, I, V, I, V, I, L, L, L, V, V, I, V),
               ctypes.CFUNCTYPE(I, V, L, L, V, V, V), ctypes.CFUNCTYPE(I, V, L, L, I, V, V), ctypes.CFUNCTYPE(I, V, L, L, L, I, V, V))
_PACK_NAMES = ("ct_quant_pack", "ct_unpack_dequant", "ct_gidx_col_group", "ct_pack_int32_dim0", "ct_unpack_int32_dim0")


def _run_wb(hp, case, mods, scheme, keep):
    """the two loops that launch per module by address: recording stand-ins behind bind_pack (tests/test_host_logic.py binds its ABI stand-ins the same way)"""
    from compressed_tensors_amd.compressors.pack_quantized import base as pq

    calls, seen = [], []
    syms = None

    def stand_in(name):
        def call(*a):
            seen.append(" ".join([name] + [str(syms.of(x) if isinstance(x, int) and x > (1 << 20) else x) for x in a]))
            return 0
        return call

    cbs = [t(stand_in(n)) for t, n in zip(_PACK_TYPES, _PACK_NAMES)]
    keep += cbs
    hp.bind_pack(*[ctypes.cast(cb, ctypes.c_void_p).value for cb in cbs])
    for rnd in range(case.get("rounds", 1)):
        for direction in ("compress", "decompress"):
            keep += [t for m in mods for t in list(m._parameters.values()) + list(m._buffers.values())]
            syms = _Symbols(mods)
            del seen[:]
            fn = hp.wb_compress_modules if direction == "compress" else hp.wb_decompress_modules
            rest = fn(list(mods), pq._wb_info, 0, 0x5000, _status(direction))
            after = _entries(mods)
            rec = {"call": f"{direction}{rnd}", "launches": list(seen), "rest": [[id(m) for m in mods].index(id(m)) for m in rest],
                   "kept": sorted(name for ptr, name in after.items() if ptr in syms.before)}  # the entries that are the tensors they were (not re-made)
            rec = syms.resolve(mods, rec)
            rec["modules"] = [_state(m) for m in mods]
            calls.append(rec)
    return calls


def run_case(cta, hp, case):
    """everything the record holds of one case; leaves `hp` as it found it apart from bind_pack (see `restore`)"""
    root, mods, scheme = build(cta, case)
    assert [id(m) for m in hp.quantized_modules(root)] == [id(m) for m in mods]
    keep = []
    hp.set_allow_cpu(True)
    try:
        return (_run_wb if case["family"] == "wb" else _run_tables)(hp, case, mods, scheme, keep)
    finally:
        hp.set_allow_cpu(False)


def restore():
    """the extension's launches bound to the library again (after the `wb` cases' stand-ins)"""
    from compressed_tensors_amd import _lib

    _lib._HOSTPATH.clear()
    return _lib.hostpath()
