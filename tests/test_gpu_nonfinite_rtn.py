"""NaN and +-inf weights through every one-pass round-to-nearest kernel and its table form (ct_rtn_quant_pack_w4 / _wb, ct_rtn_quant_channel8,
ct_rtn_quant_block8, ct_rtn_quant_group8, ct_rtn_mxfp4_quant_pack, ct_rtn_nvfp4_quant_pack, ct_generate_gparam, every *_batch) over the case matrix
of tests/_nonfinite_rtn_cases.py: against the reference's recorded results (tests/golden/nonfinite_rtn.safetensors, outside the manifest's listed MX
groups), the pinned oracle (everywhere) and the composition kernels the one pass replaces; the groups that hold no plant against a second run with
the plants replaced by 0.25; the tables against the single launches; compress_rtn against compress.  Everything is compared under
`_nonfinite_rtn_cases.comparable` — raw bits with every NaN rewritten to one NaN, the sign bit of an FP4 nibble whose quotient is NaN cleared —
without a tolerance.
Every test here needs an MI355X:  python -m pytest tests -m gpu"""
import pytest
import torch

import _nonfinite_rtn_cases as C
import oracle as O

pytestmark = pytest.mark.gpu

BF16, F16, F32, F8 = C.BF16, C.F16, C.F32, C.F8
CASES = dict(C.case_list())
KEYS = list(CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cta():
    import compressed_tensors_amd as m
    from compressed_tensors_amd import _lib

    _lib.load()  # fail loudly if the HIP extension is missing
    return m


@pytest.fixture(scope="module")
def fixture():
    return C.load_fixture()


@pytest.fixture(scope="module")
def ref():
    """key -> (weight, {kind: the oracle composition's outputs}, {kind: the FP4 sign mask or None}), computed once and never written to"""
    out = {}
    for key, r in CASES.items():
        x = C.weight(r)
        out[key] = (x, {kind: C.oracle_outputs(O, x, r, kind) for kind in C.kinds_of(r)},
                    {kind: C.fp4_sign_mask(O, x, r, kind) if r["family"] == "fp4" else None for kind in C.kinds_of(r)})
    return out


def mismatches(got, want, kind, mask=None, names=None):
    """the names on which two sets of outputs differ under `comparable`: dtype, shape or compared bits"""
    names = list(names or got)
    a, b = C.comparable({n: got[n] for n in names}, kind, mask), C.comparable({n: want[n] for n in names}, kind, mask)
    return [(n, int((a[n] != b[n]).sum()) if a[n].shape == b[n].shape else (tuple(a[n].shape), tuple(b[n].shape))) for n in names
            if got[n].dtype != want[n].dtype or a[n].shape != b[n].shape or not torch.equal(a[n], b[n])]


# ---- the entries and the compositions they replace, under the fixture's names ----------------------------------------------------------------
def args8(kind):
    a = C.KINDS8["fp8" if kind == "mxfp8" else kind]
    return a["type"], a["symmetric"]


def one_pass(cta, w, r, kind, **kw):
    """{name: output} of the one-pass entry of this case's family; kw: words=True (group8), codes=False (block8), global_scale (NVFP4)"""
    codec, family = cta.codec, r["family"]
    if family == "pack":
        bits, symmetric = C.pack_kind(kind)
        return dict(zip(("packed", "scale", "zero_point"), codec.rtn_quantize_and_pack(w, group_size=r["group"], symmetric=symmetric, num_bits=bits)))
    if family == "channel8":
        qtype, symmetric = args8(kind)
        q, scale, zp = codec.rtn_quantize_channel8(w, qtype=qtype, symmetric=symmetric)
        return dict(q=q, scale=scale) if kind == "fp8" else dict(q=q, scale=scale, zero_point=zp)
    if family == "block8":
        qtype, symmetric = args8(kind)
        q, scale, zp = codec.rtn_quantize_block8(w, block_structure=r["block"], qtype=qtype, symmetric=symmetric, **kw)
        return dict(scale=scale, zero_point=zp) if q is None else dict(q=q, scale=scale, zero_point=zp)
    if family == "group8":
        qtype, symmetric = args8(kind)
        got = codec.rtn_quantize_group8(w, group_size=r["group"], qtype=qtype, symmetric=symmetric, mx=(kind == "mxfp8"), **kw)
        out = {"packed" if kw.get("words") else "q": got[0], "scale": got[1]}
        if qtype == "int":
            out["zero_point"] = got[2]
        if kind == "mxfp8":
            out["e8m0"] = got[3]
        return out
    if kind == "mxfp4":
        return dict(zip(("packed", "e8m0", "scale"), codec.rtn_mxfp4_quantize_and_pack(w, return_scale=True)))
    gs = kw.get("global_scale", None if r["global_scale"] is None else torch.tensor([r["global_scale"]], dtype=F32, device=w.device))
    return dict(zip(("packed", "scale_f8", "global_scale", "scale"), codec.rtn_nvfp4_quantize_and_pack(w, gs, return_scale=True)))


def composition(cta, w, r, kind):
    """the existing kernels the one pass replaces: the min-max observer (generate_gparam in front for NVFP4), then the quantize / pack kernel
    (and compress_mx_scale for the MX kinds)"""
    from compressed_tensors_amd.quantization.utils import _block_rows

    codec, family, group = cta.codec, r["family"], r.get("group")
    if family == "pack":
        bits, symmetric = C.pack_kind(kind)
        scale, zp = codec.minmax_qparams(w, num_bits=bits, group_size=group, symmetric=symmetric)
        packed = codec.quantize_and_pack(w, scale, zp, num_bits=bits, strategy="group" if group else "channel", group_size=group)
        return dict(packed=packed, scale=scale, zero_point=zp)
    if family == "fp4":
        if kind == "mxfp4":
            scale = codec.minmax_qparams_float(w, kind="mxfp4", group_size=32)
            return dict(packed=codec.fp4_quantize_and_pack(w, scale, None, group_size=32), e8m0=codec.compress_mx_scale(scale), scale=scale)
        gs = codec.generate_gparam(w) if r["global_scale"] is None else torch.tensor([r["global_scale"]], dtype=F32, device=w.device)
        scale = codec.minmax_qparams_float(w, kind="nvfp4", group_size=16, global_scale=gs)
        return dict(packed=codec.fp4_quantize_and_pack(w, scale, gs, group_size=16), scale_f8=scale.to(F8), global_scale=gs, scale=scale)
    qtype, symmetric = args8(kind)
    if family == "block8":
        rows, grid = _block_rows(w, r["block"])
        strategy = dict(strategy="block", block_structure=list(r["block"]))
    else:
        rows, grid = w, None
        strategy = dict(strategy="group", group_size=group) if family == "group8" else dict(strategy="channel")
    if qtype == "float":
        scale = codec.minmax_qparams_float(rows, kind=kind, group_size=group if family == "group8" else None)
        zp = torch.zeros(scale.shape, dtype=F8, device=w.device)
    else:
        scale, zp = codec.minmax_qparams(rows, num_bits=8, group_size=group if family == "group8" else None, symmetric=symmetric)
    if grid is not None:
        scale, zp = scale.reshape(grid), zp.reshape(grid)
    q = codec.quantize_tensor(w, scale, zp, num_bits=8, dtype=F8 if qtype == "float" else torch.int8, qtype=qtype, **strategy)
    out = dict(q=q, scale=scale)
    if qtype == "int" or family == "block8":
        out["zero_point"] = zp
    if kind == "mxfp8":
        out["e8m0"] = codec.compress_mx_scale(scale)
    if family == "group8" and qtype == "int":
        out["packed"] = codec.quantize_and_pack(w, scale, zp, num_bits=8, strategy="group", group_size=group)
    return out


# ---- single entries ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_one_pass_equals_fixture_oracle_and_composition(cta, dev, ref, fixture, key):
    """every kind of the case: the one-pass entry == what the reference recorded (outside the listed MX groups), == the oracle (everywhere), == the
    composition kernels; group8's word form and block8's observer form (codes=False) too"""
    r = CASES[key]
    x, want, masks = ref[key]
    w = x.to(dev)
    failed = []
    for kind in C.kinds_of(r):
        runs = [("entry", one_pass(cta, w, r, kind))]
        if r["family"] == "group8" and kind.startswith("int8"):
            runs.append(("words", one_pass(cta, w, r, kind, words=True)))
        if r["family"] == "block8":
            runs.append(("observer", one_pass(cta, w, r, kind, codes=False)))
        two = composition(cta, w, r, kind)
        for form, got in runs:
            assert set(got) <= set(want[kind]), (key, kind, form)
            bad = C.fixture_mismatches(fixture, key, kind, {n: t.cpu() for n, t in got.items()}, masks[kind])
            failed += [(kind, form, "fixture", bad)] if bad else []
            for other, what in ((want[kind], "oracle"), (two, "composition")):
                bad = mismatches(got, other, kind, masks[kind])
                failed += [(kind, form, what, bad)] if bad else []
    assert not failed, (key, failed)


def unplanted(r, kind, name, t):
    """bool, the shape of output `name`: the entries that belong to no planted group, row or block"""
    rows, cols = r["shape"]
    m = C.planted_mask(r)
    if name in ("scale", "zero_point", "e8m0", "scale_f8"):
        return ~C.planted_regions(r, kind).reshape(t.shape)
    if name == "packed" and r["family"] == "pack":  # 32 elements are `bits` words
        return ~m.reshape(rows, cols // 32, 32).any(-1).repeat_interleave(C.pack_kind(kind)[0], dim=1)
    per = cols // t.shape[1]  # q: 1; the FP4 bytes: 2; group8's words: 4
    return ~m.reshape(rows, t.shape[1], per).any(-1)


@pytest.mark.parametrize("key", [k for k in KEYS if CASES[k]["plants"]])
def test_groups_without_a_plant_are_those_of_the_weight_without_plants(cta, dev, ref, key):
    """isolation, asserted directly: every group, row or block that holds no plant has the scale, zero point and codes of the same weight with its
    plants replaced by 0.25 — a second run of the same entry (NVFP4: under the first run's global scale, which the plant decides)"""
    r = CASES[key]
    x, _, masks = ref[key]
    w, flat = x.to(dev), C.plant(C.make_weight(r), r, value=0.25).to(dev)
    failed = []
    for kind in C.kinds_of(r):
        got = one_pass(cta, w, r, kind)
        kw = dict(global_scale=got["global_scale"]) if kind == "nvfp4" else {}
        clean = one_pass(cta, flat, r, kind, **kw)
        a, b = C.comparable(got, kind, masks[kind]), C.comparable(clean, kind, masks[kind])
        for name in got:
            if name == "global_scale":
                continue
            keep = unplanted(r, kind, name, a[name])
            assert keep.shape == a[name].shape and bool(keep.any()), (key, kind, name)
            if not torch.equal(a[name][keep], b[name][keep]):
                failed.append((kind, name, int((a[name][keep] != b[name][keep]).sum())))
            if name == "scale":  # and the clean run is finite everywhere: the plants were the only non-finite values
                assert bool(torch.isfinite(clean[name].float()).all()), (key, kind)
    assert not failed, (key, failed)


# ---- tables ------------------------------------------------------------------------------------------------------------------------------
def counted(cta, monkeypatch, fn):
    """fn() with the ct_rtn_* calls recorded as (name, n items)"""
    calls, real = [], cta.codec.call
    monkeypatch.setattr(cta.codec, "call", lambda name, *args: calls.append((name, args[1])) or real(name, *args))
    out = fn()
    monkeypatch.setattr(cta.codec, "call", real)
    return out, [c for c in calls if c[0].startswith("ct_rtn")]


def check_table(cta, dev, ref, keys, kind, got, names, **kw):
    """every item of a table == its single launch and the oracle"""
    failed = []
    for key, item in zip(keys, got):
        x, want, masks = ref[key]
        mine = dict(zip(names, item))
        mine = {n: t for n, t in mine.items() if t is not None and n in want[kind]}
        single = one_pass(cta, x.to(dev), CASES[key], kind, **kw)
        for other, what in ((single, "single"), (want[kind], "oracle")):
            bad = mismatches(mine, other, kind, masks[kind])
            failed += [(key, kind, what, bad)] if bad else []
    assert not failed, failed


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_pack_tables_over_all_cases_equal_the_single_launches(cta, dev, ref, dtype, monkeypatch):
    keys = [k for k in KEYS if CASES[k]["family"] == "pack" and CASES[k]["dtype"] == dtype]
    xs, groups = [ref[k][0].to(dev) for k in keys], [CASES[k]["group"] for k in keys]
    assert len(keys) == 5
    for kind in C.PACK_KINDS:
        bits, symmetric = C.pack_kind(kind)
        got, calls = counted(cta, monkeypatch, lambda: cta.codec.rtn_quantize_and_pack_many(xs, group_size=groups, symmetric=symmetric, num_bits=bits))
        assert calls == [("ct_rtn_quant_pack_w4_batch" if bits == 4 else "ct_rtn_quant_pack_wb_batch", len(keys))], (kind, calls)
        check_table(cta, dev, ref, keys, kind, got, ("packed", "scale", "zero_point"))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_channel8_tables_over_all_cases_equal_the_single_launches(cta, dev, ref, dtype, monkeypatch):
    keys = [k for k in KEYS if CASES[k]["family"] == "channel8" and CASES[k]["dtype"] == dtype]
    xs = [ref[k][0].to(dev) for k in keys]
    assert len(keys) == 8
    for kind in C.KINDS8:
        qtype, symmetric = args8(kind)
        got, calls = counted(cta, monkeypatch, lambda: cta.codec.rtn_quantize_channel8_many(xs, qtype=qtype, symmetric=symmetric))
        assert calls == [("ct_rtn_quant_channel8_batch", len(keys))], (kind, calls)
        check_table(cta, dev, ref, keys, kind, got, ("q", "scale", "zero_point"))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_block8_tables_over_all_cases_equal_the_single_launches(cta, dev, ref, dtype, monkeypatch):
    """(a block table serves one block structure: one table per structure over all of its cases)"""
    for block, n in (([128, 128], 5), ([4, 16], 3), ([16, 1024], 10)):
        keys = [k for k in KEYS if CASES[k]["family"] == "block8" and CASES[k]["dtype"] == dtype and CASES[k]["block"] == block]
        xs = [ref[k][0].to(dev) for k in keys]
        assert len(keys) == n
        for kind in C.KINDS8:
            qtype, symmetric = args8(kind)
            got, calls = counted(cta, monkeypatch, lambda: cta.codec.rtn_quantize_block8_many(xs, block_structure=block, qtype=qtype, symmetric=symmetric))
            assert calls == [("ct_rtn_quant_block8_batch", len(keys))], (kind, calls)
            check_table(cta, dev, ref, keys, kind, got, ("q", "scale", "zero_point"))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_group8_tables_over_all_cases_equal_the_single_launches(cta, dev, ref, dtype, monkeypatch):
    for kind, words in [(k, False) for k in ("mxfp8", *C.KINDS8)] + [("int8", True), ("int8_zp", True)]:
        keys = [k for k in KEYS if CASES[k]["family"] == "group8" and CASES[k]["dtype"] == dtype and kind in C.kinds_of(CASES[k])]
        xs, groups = [ref[k][0].to(dev) for k in keys], [CASES[k]["group"] for k in keys]
        assert len(keys) == (1 if kind == "mxfp8" else 3)
        qtype, symmetric = args8(kind)
        got, calls = counted(cta, monkeypatch, lambda: cta.codec.rtn_quantize_group8_many(xs, group_size=groups, qtype=qtype, symmetric=symmetric,
                                                                                          mx=(kind == "mxfp8"), words=words))
        assert calls == [("ct_rtn_quant_group8_batch", len(keys))], (kind, words, calls)
        check_table(cta, dev, ref, keys, kind, got, ("packed" if words else "q", "scale", "zero_point", "e8m0"), **(dict(words=True) if words else {}))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fp4_tables_over_all_cases_equal_the_single_launches(cta, dev, ref, fixture, dtype, monkeypatch):
    """MXFP4: one launch.  NVFP4: one fold and one quantize launch over the planted weight, the clean one and the two whose only plant is their last
    element; the table's global scales are the reference's — 1 for a NaN item, 0 for a +inf item (448 * 6 / inf is finite: nan_to_num leaves it),
    the clean item's own value — and each owns its storage"""
    keys = [k for k in KEYS if CASES[k]["family"] == "fp4" and CASES[k]["dtype"] == dtype and "mxfp4" in C.kinds_of(CASES[k])]
    assert len(keys) == 2
    got, calls = counted(cta, monkeypatch, lambda: cta.codec.rtn_mxfp4_quantize_and_pack_many([ref[k][0].to(dev) for k in keys]))
    assert calls == [("ct_rtn_mxfp4_quant_pack_batch", len(keys))], calls
    check_table(cta, dev, ref, keys, "mxfp4", got, ("packed", "e8m0"))
    keys = [k for k in KEYS if CASES[k]["family"] == "fp4" and CASES[k]["dtype"] == dtype and CASES[k]["global_scale"] is None]
    assert [k.split(".")[1] for k in keys] == ["g32", "clean", "last_nan", "last_inf"]
    got, calls = counted(cta, monkeypatch, lambda: cta.codec.rtn_nvfp4_quantize_and_pack_many([ref[k][0].to(dev) for k in keys]))
    assert calls == [("ct_rtn_nvfp4_amax_batch", len(keys)), ("ct_rtn_nvfp4_quant_pack_batch", len(keys))], calls
    check_table(cta, dev, ref, keys, "nvfp4", got, ("packed", "scale_f8", "global_scale"))
    scales = [t[2] for t in got]
    recorded = [float(fixture[0][f"{k}.nvfp4.global_scale"]) for k in keys]
    assert [float(s) for s in scales] == recorded and recorded[0] == recorded[2] == 1.0 and recorded[3] == 0.0 and 1.0 < recorded[1] < float("inf")
    assert all(s.dtype == F32 and s.shape == (1,) and s.untyped_storage().nbytes() == 4 and s.storage_offset() == 0 for s in scales)
    assert len({s.untyped_storage().data_ptr() for s in scales}) == len(scales)


# ---- one level up ------------------------------------------------------------------------------------------------------------------------
def same_dicts(one, two, mask=None, ordered=True):
    """entries, order, dtypes, shapes and compared bits.  `ordered=False` where compress_rtn's one-pass branch is known to return compress's entries
    in another order on finite data too (W4, the wave / row forms of channel8, block8, NVFP4: their own tests compare sorted names)"""
    if (list(one) != list(two)) if ordered else (sorted(one) != sorted(two)):
        return False
    for k in one:
        a, b = C.canonical(one[k].cpu()), C.canonical(two[k].cpu())
        if mask is not None and k == "weight_packed":
            a, b = a & ~mask, b & ~mask
        if one[k].dtype != two[k].dtype or a.shape != b.shape or not torch.equal(a, b):
            return False
    return True


def force_gates(monkeypatch):
    """every measured-dispatch gate of compress_rtn on: the one-pass branch itself is under test"""
    from compressed_tensors_amd.compressors.naive_quantized import base as naive
    from compressed_tensors_amd.compressors.pack_quantized import base as pack

    for mod, name in ((pack, "RTN_PACKW_MEASURED_FASTER"), (naive, "RTN_GROUP8_MEASURED_FASTER"), (naive, "RTN_CHANNEL8_LONG_MEASURED_FASTER")):
        monkeypatch.setattr(mod, name, dict.fromkeys(getattr(mod, name), True))


def rtn_calls(cta, monkeypatch, fn):
    calls, real = [], cta.codec.call
    monkeypatch.setattr(cta.codec, "call", lambda name, *a: calls.append(name) or real(name, *a))
    out = fn()
    monkeypatch.setattr(cta.codec, "call", real)
    return out, calls


@pytest.mark.parametrize("kind", ["w3", "w3a", "w4", "w4a", "w6a"])
def test_pack_compress_rtn_one_pass_equals_the_composition(cta, dev, ref, fixture, kind, monkeypatch):
    key = "pack.b.bf16"
    x, want, _ = ref[key]
    w, (bits, symmetric) = x.to(dev), C.pack_kind(kind)
    packer = cta.BaseCompressor.get_value_from_registry("pack-quantized")
    scheme = cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(num_bits=bits, symmetric=symmetric, strategy="group", group_size=128))
    scale, zp = cta.codec.minmax_qparams(w, num_bits=bits, group_size=128, symmetric=symmetric)
    two = packer.compress({"weight": w, "weight_scale": scale, "weight_zero_point": zp}, scheme)
    force_gates(monkeypatch)
    one, calls = rtn_calls(cta, monkeypatch, lambda: packer.compress_rtn(w, scheme))
    assert calls[0] == ("ct_rtn_quant_pack_w4" if bits == 4 else "ct_rtn_quant_pack_wb") and "ct_minmax_qparams" not in calls, calls
    assert sorted(one) == sorted(["weight_scale"] + ([] if symmetric else ["weight_zero_point"]) + ["weight_packed", "weight_shape"])
    assert same_dicts(one, two, ordered=bits != 4), (list(one), list(two))
    got = dict(packed=one["weight_packed"], scale=one["weight_scale"])
    if not symmetric:
        got["zp_packed"] = one["weight_zero_point"]
    assert not mismatches(got, want[kind], kind) and C.fixture_mismatches(fixture, key, kind, {n: t.cpu() for n, t in got.items()}) == []


@pytest.mark.parametrize("key,kind", [("channel8.wave.bf16", k) for k in C.KINDS8] + [("channel8.long1.bf16", k) for k in C.KINDS8]
                         + [("block8.b128x128.v0.bf16", k) for k in C.KINDS8] + [("group8.g32.bf16", k) for k in ("mxfp8", *C.KINDS8)])
def test_eight_bit_compress_rtn_one_pass_equals_the_composition(cta, dev, ref, fixture, key, kind, monkeypatch):
    """float- / int- / mxfp8-quantized compress_rtn on a planted case == compress fed with the observer's qparams: entries, order, dtypes, bits"""
    from compressed_tensors_amd.quantization.utils import calculate_qparams_from_weight

    r = CASES[key]
    x, want, _ = ref[key]
    w = x.to(dev)
    a = dict(num_bits=8, type="float", symmetric=True, scale_dtype=torch.uint8, zp_dtype=torch.uint8) if kind == "mxfp8" else C.KINDS8[kind]
    strategy = {"channel8": dict(strategy="channel"), "block8": dict(strategy="block", block_structure=r.get("block")),
                "group8": dict(strategy="group", group_size=r.get("group"))}[r["family"]]
    act = cta.QuantizationArgs(num_bits=8, type=a["type"], strategy="token", symmetric=True, dynamic=True)
    scheme = cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(**strategy, **a), input_activations=act)
    comp = cta.BaseCompressor.get_value_from_registry({"mxfp8": "mxfp8-quantized", "fp8": "float-quantized"}.get(kind, "int-quantized"))
    scale, zp = calculate_qparams_from_weight(w, scheme.weights)
    two = comp.compress({"weight": w, "weight_scale": scale, "weight_zero_point": zp}, scheme)
    force_gates(monkeypatch)
    one, calls = rtn_calls(cta, monkeypatch, lambda: comp.compress_rtn(w, scheme))
    assert calls == [{"channel8": "ct_rtn_quant_channel8", "block8": "ct_rtn_quant_block8", "group8": "ct_rtn_quant_group8"}[r["family"]]], calls
    assert same_dicts(one, two, ordered=r["family"] == "group8" or r["form"].startswith("long")), (list(one), list(two))
    got = {"q": one["weight"], "e8m0" if kind == "mxfp8" else "scale": one["weight_scale"]}
    if kind == "int8_zp":
        got["zero_point"] = one["weight_zero_point"]
    assert not mismatches(got, want[kind], kind) and C.fixture_mismatches(fixture, key, kind, {n: t.cpu() for n, t in got.items()}) == []


def test_fp4_compress_rtn_one_pass_equals_the_composition(cta, dev, ref, fixture):
    key = "fp4.g32.bf16"
    x, want, masks = ref[key]
    w = x.to(dev)
    mx = cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(num_bits=4, type="float", strategy="group", symmetric=True, group_size=32,
                                                                                   scale_dtype=torch.uint8))
    one = cta.MXFP4PackedCompressor.compress_rtn(w, mx)
    two = cta.MXFP4PackedCompressor.compress({"weight": w, "weight_scale": cta.codec.minmax_qparams_float(w, kind="mxfp4", group_size=32)}, mx)
    assert same_dicts(one, two, masks["mxfp4"]), (list(one), list(two))
    got = dict(packed=one["weight_packed"], e8m0=one["weight_scale"])
    assert not mismatches(got, want["mxfp4"], "mxfp4", masks["mxfp4"])
    assert C.fixture_mismatches(fixture, key, "mxfp4", {n: t.cpu() for n, t in got.items()}, masks["mxfp4"]) == []
    nv = cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(num_bits=4, type="float", strategy="tensor_group", symmetric=True,
                                                                                   group_size=16, scale_dtype=F8))
    one = cta.NVFP4PackedCompressor.compress_rtn(w, nv)
    gs = cta.codec.generate_gparam(w)
    scale = cta.codec.minmax_qparams_float(w, kind="nvfp4", group_size=16, global_scale=gs)
    two = cta.NVFP4PackedCompressor.compress({"weight": w, "weight_scale": scale, "weight_global_scale": gs}, nv)
    assert same_dicts(one, two, masks["nvfp4"], ordered=False), (list(one), list(two))
    got = dict(packed=one["weight_packed"], scale_f8=one["weight_scale"], global_scale=one["weight_global_scale"])
    assert not mismatches(got, want["nvfp4"], "nvfp4", masks["nvfp4"])
    assert C.fixture_mismatches(fixture, key, "nvfp4", {n: t.cpu() for n, t in got.items()}, masks["nvfp4"]) == []
