"""The one-pass round-to-nearest compress of the widths next to 4 and 8 (ct_rtn_quant_pack_wb and its table form: pack-quantized W2 / W3 / W5 / W6 /
W7 from a dense model) and what stands on it — codec.rtn_quantize_and_pack(num_bits=...), its list form, compress_rtn and the window hook of
PackedQuantizationCompressor, PackQuantizedQuantizer — against the reference's recorded results (tests/golden/packw_rtn.safetensors), the pinned
oracle's composition (tests/_packw_rtn_cases.oracle_outputs) and the composition kernels the one pass replaces (minmax_qparams +
quantize_and_pack).  Everything is compared on raw bits, without a tolerance.
Every test here needs an MI355X:  python -m pytest tests -m gpu"""
import copy
import json
import os

import pytest
import torch

import _packw_rtn_cases as C
import oracle as O

pytestmark = pytest.mark.gpu

BF16, F16, F32 = C.BF16, C.F16, C.F32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packw_rtn.safetensors")
CASES = dict(C.case_list())
FAST_KEYS = [k for k, r in CASES.items() if r["fast"]]
FALLBACK_KEYS = [k for k, r in CASES.items() if not r["fast"]]
SCHEMES = [(b, s) for b in C.BITS for s in (True, False)]
bits_of = C.bits_of


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
def golden():
    from safetensors.torch import load_file

    return load_file(GOLDEN)


@pytest.fixture(scope="module")
def ref(golden):
    """key -> (weight, {(bits, symmetric): the oracle composition's outputs}), computed once and never written to; the weight is the fixture's input"""
    out = {}
    for key, r in CASES.items():
        x = golden[f"{key}.x"]
        assert torch.equal(bits_of(x), bits_of(C.make_weight(r))), key
        out[key] = (x, {(b, s): C.oracle_outputs(O, x, r["group"], b, s) for b in r["bits"] for s in (True, False)})
    return out


def same(a, b):
    """equal shapes, dtypes and raw bits"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits_of(a.cpu().contiguous()), bits_of(b.cpu().contiguous()))


def check(got, want, names, what):
    for name in names:
        a, b = got[name], want[name]
        assert same(a, b), (*what, name, int((bits_of(a.cpu().contiguous()).reshape(-1) != bits_of(b.cpu().contiguous()).reshape(-1)).sum())
                            if a.shape == b.shape and a.dtype == b.dtype else (a.shape, b.shape, a.dtype, b.dtype))


def scheme_of(cta, bits, symmetric, group):
    args = (cta.QuantizationArgs(num_bits=bits, symmetric=symmetric, strategy="group", group_size=group) if group
            else cta.QuantizationArgs(num_bits=bits, symmetric=symmetric, strategy="channel"))
    return cta.QuantizationScheme(targets=["Linear"], weights=args)


def packer(cta):
    return cta.BaseCompressor.get_value_from_registry("pack-quantized")


def composition(cta, w, group, b, s):
    """the existing kernels the one pass replaces: the observer, then the compress"""
    scale, zp = cta.codec.minmax_qparams(w, num_bits=b, group_size=group, symmetric=s)
    packed = cta.codec.quantize_and_pack(w, scale, zp, num_bits=b, strategy="group" if group else "channel", group_size=group)
    return dict(packed=packed, scale=scale, zero_point=zp)


def force_gates(monkeypatch, value: bool):
    from compressed_tensors_amd.compressors.pack_quantized import base

    monkeypatch.setattr(base, "RTN_PACKW_MEASURED_FASTER", dict.fromkeys(base.RTN_PACKW_MEASURED_FASTER, value))
    monkeypatch.setattr(base, "RTN_PACKW_TABLE_MEASURED_FASTER", dict.fromkeys(base.RTN_PACKW_TABLE_MEASURED_FASTER, value))


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", FAST_KEYS)
def test_one_pass_equals_fixture_oracle_and_composition(cta, dev, ref, golden, key):
    """ct_rtn_quant_pack_wb == group min / max + calculate_qparams + quantize + pack_to_int32: 0 ulp against the reference's recorded results, the
    oracle and the kernels it replaces, for every width and both symmetries"""
    r = CASES[key]
    x, want = ref[key]
    w = x.to(dev)
    for b in r["bits"]:
        for s in (True, False):
            packed, scale, zp = cta.codec.rtn_quantize_and_pack(w, group_size=r["group"], symmetric=s, num_bits=b)
            got = dict(packed=packed, scale=scale, zero_point=zp)
            assert packed.dtype == torch.int32 and tuple(packed.shape) == (x.shape[0], x.shape[1] * b // 32) and scale.dtype == x.dtype and zp.dtype == torch.int8
            fixture = {n: golden[f"{key}.{C.tag(b, s)}.{n}"] for n in got}
            for other, what in ((fixture, "fixture"), (want[(b, s)], "oracle"), (composition(cta, w, r["group"], b, s), "composition")):
                check(got, other, list(got), (key, b, s, what))


def test_the_default_width_is_still_four_bits(cta, dev, ref):
    x = ref["4x512.g64.bf16"][0].to(dev)
    four = cta.codec.rtn_quantize_and_pack(x, group_size=64)
    assert all(same(a, b) for a, b in zip(four, cta.codec.rtn_quantize_and_pack(x, group_size=64, num_bits=4)))
    two = composition(cta, x, 64, 4, True)
    assert same(four[0], two["packed"]) and same(four[1], two["scale"]) and same(four[2], two["zero_point"])


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,s", SCHEMES)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_one_table_over_all_cases_equals_the_single_launches(cta, dev, ref, dtype, b, s, monkeypatch):
    """rtn_quantize_and_pack_many: ONE launch over every fast case of a (dtype, width, symmetry), whatever its group == the single launches; a table of
    one; an empty list; items the plan refuses take the single path with identical results"""
    codec = cta.codec
    keys = [k for k in FAST_KEYS if CASES[k]["dtype"] == dtype and b in CASES[k]["bits"]]
    xs, groups = [ref[k][0].to(dev) for k in keys], [CASES[k]["group"] for k in keys]
    calls, real = [], codec.call
    monkeypatch.setattr(codec, "call", lambda name, *args: calls.append((name, args[1])) or real(name, *args))
    got = codec.rtn_quantize_and_pack_many(xs, group_size=groups, symmetric=s, num_bits=b)
    assert [c for c in calls if c[0].startswith("ct_rtn")] == [("ct_rtn_quant_pack_wb_batch", len(keys))], calls
    del calls[:]
    one = codec.rtn_quantize_and_pack_many(xs[:1], group_size=groups[:1], symmetric=s, num_bits=b)
    assert [c for c in calls if c[0].startswith("ct_rtn")] == [("ct_rtn_quant_pack_wb_batch", 1)], calls
    monkeypatch.setattr(codec, "call", real)
    singles = [codec.rtn_quantize_and_pack(x, group_size=g, symmetric=s, num_bits=b) for x, g in zip(xs, groups)]
    for k, g, single in zip(keys, got, singles):
        assert len(g) == 3 and all(same(u, v) for u, v in zip(single, g)), (k, b, s)
        check(dict(zip(("packed", "scale", "zero_point"), g)), ref[k][1][(b, s)], ("packed", "scale", "zero_point"), (k, b, s, "oracle"))
    assert all(same(u, v) for u, v in zip(one[0], singles[0]))
    assert codec.rtn_quantize_and_pack_many([], symmetric=s, num_bits=b) == []
    assert codec.launch_rtn_wb_words([], 0, BF16, dev, b, s) is None  # an empty table: nothing is touched
    # what the plan refuses — float32, a group of 48, a view one element into its storage — between two items it takes
    f32 = ref["4x64.g32.f32"][0].to(dev)
    g48 = ref[f"2x96.g48.{dtype}"][0].to(dev)
    store = torch.zeros(xs[0].numel() + 1, dtype=xs[0].dtype, device=dev)
    view = store[1:].view(xs[0].shape)
    view.copy_(xs[0])
    assert view.data_ptr() % 16 and view.is_contiguous()
    mixed, mixed_groups = [xs[0], f32, g48, view, xs[1]], [groups[0], 32, 48, groups[0], groups[1]]
    monkeypatch.setattr(codec, "call", lambda name, *args: calls.append((name, args[1])) or real(name, *args))
    del calls[:]
    got = codec.rtn_quantize_and_pack_many(mixed, group_size=mixed_groups, symmetric=s, num_bits=b)
    monkeypatch.setattr(codec, "call", real)
    rtn = [c[0] for c in calls if c[0].startswith("ct_rtn")]
    assert rtn.count("ct_rtn_quant_pack_wb_batch") == 1 and rtn.count("ct_rtn_quant_pack_wb") == 1 and ("ct_rtn_quant_pack_wb_batch", 2) in calls, calls
    for i, j in ((0, 0), (3, 0), (4, 1)):
        assert all(same(u, v) for u, v in zip(got[i], singles[j])), (i, b, s)
    for i, key in ((1, "4x64.g32.f32"), (2, f"2x96.g48.{dtype}")):
        check(dict(zip(("packed", "scale", "zero_point"), got[i])), ref[key][1][(b, s)], ("packed", "scale", "zero_point"), (key, b, s, "refused"))


# ---- compress_rtn ----------------------------------------------------------------------------------------------------------------------
def _composed(cta, w, scheme):
    wa = scheme.weights
    scale, zp = cta.codec.minmax_qparams(w, num_bits=int(wa.num_bits), group_size=wa.group_size if wa.group_size else None, symmetric=bool(wa.symmetric))
    return packer(cta).compress({"weight": w, "weight_scale": scale, "weight_zero_point": zp}, scheme)


def _same_dicts(one, two):
    return list(one) == list(two) and all(same(one[k], two[k]) for k in one)


@pytest.mark.parametrize("key", FAST_KEYS + FALLBACK_KEYS)
def test_compress_rtn_equals_the_composition_with_the_gate_on_and_off(cta, dev, ref, golden, key, monkeypatch):
    """compress_rtn on every fast case (one pass where the gate holds) and on what the plan refuses (float32, group 48, the first group above the plan's
    maximum, a row that is no whole pack groups: always the composition) == cls.compress of the composition's qparams: entries, order, dtypes, shapes,
    bits — and the reference's recorded words, scales and stored zero points"""
    r = CASES[key]
    x, want = ref[key]
    w = x.to(dev)
    codec = cta.codec
    assert bool(codec.rtn_w4_group(x.shape, r["group"])) == (r["fast"] or x.dtype == F32)
    for b in r["bits"]:
        for s in (True, False):
            scheme = scheme_of(cta, b, s, r["group"])
            two = _composed(cta, w, scheme)
            assert list(two) == ["weight_scale"] + ([] if s else ["weight_zero_point"]) + ["weight_packed", "weight_shape"]
            for gate in (True, False):
                force_gates(monkeypatch, gate)
                calls, real = [], codec.call
                monkeypatch.setattr(codec, "call", lambda name, *a: calls.append(name) or real(name, *a))
                one = packer(cta).compress_rtn(w, scheme)
                monkeypatch.setattr(codec, "call", real)
                if gate and r["fast"]:
                    assert calls == ["ct_rtn_quant_pack_wb"] + ([] if s else ["ct_pack_int32_dim0"]), (key, b, s, calls)
                else:
                    assert not any(c.startswith("ct_rtn") for c in calls) and calls[0] == "ct_minmax_qparams", (key, b, s, gate, calls)
                assert _same_dicts(one, two), (key, b, s, gate, list(one), list(two))
            fixture = {n: golden[f"{key}.{C.tag(b, s)}.{n}"] for n in want[(b, s)]}
            for other in (fixture, want[(b, s)]):
                assert same(one["weight_packed"], other["packed"]) and same(one["weight_scale"], other["scale"]), (key, b, s)
                assert s or same(one["weight_zero_point"], other["zp_packed"]), (key, b, s)
            assert one["weight_shape"].dtype == torch.int64 and one["weight_shape"].tolist() == list(x.shape)
    if not r["fast"]:
        with pytest.raises(NotImplementedError):  # the codec entry refuses by name: there is no fallback below compress_rtn
            codec.rtn_quantize_and_pack(w, group_size=r["group"], num_bits=3)


# ---- the window hook -------------------------------------------------------------------------------------------------------------------
def _tree(cta, dev, n=34):
    """34 Linear(128, 128): more than one window of 32; W3 symmetric, W3 asymmetric, W6 and W4 in turn, every weight its own integer formula"""
    kinds = [(3, True), (3, False), (6, True), (4, True)]
    schemes = {k: scheme_of(cta, k[0], k[1], 128 if k[0] != 6 else 64) for k in kinds}
    layers, recipes = [], []
    for i in range(n):
        k = kinds[i % 4]
        r = dict(shape=[128, 128], group=128 if k[0] != 6 else 64, dtype="bf16", special=None, salt=i % 7 + 1 + i)
        m = torch.nn.Linear(128, 128, bias=(i == 1)).to(dev).to(BF16)
        m.weight.data.copy_(C.make_weight(r))
        m.quantization_scheme = schemes[k]
        layers.append(m)
        recipes.append((k, r))
    return torch.nn.Sequential(*layers), recipes


def _entries(m):
    return [(n, t.dtype, tuple(t.shape), bits_of(t.data.cpu())) for n, t in (*m._parameters.items(), *m._buffers.items()) if t is not None]


def test_the_window_hook_leaves_what_compress_rtn_module_leaves(cta, dev, monkeypatch):
    """with the table gate forced on, the modules of the new widths leave in one table launch per window and (width, symmetry); every module ends in
    exactly the state `compress_rtn_module` leaves it in (gate off: the composition), and decompress_model returns the oracle's fake-quantized weights"""
    codec = cta.codec
    hook, recipes = _tree(cta, dev)
    each = copy.deepcopy(hook)
    force_gates(monkeypatch, False)
    for m in each:
        packer(cta).compress_rtn_module(m)
    force_gates(monkeypatch, True)
    calls, real = [], codec.call
    monkeypatch.setattr(codec, "call", lambda name, *a: calls.append((name, a[1])) or real(name, *a))
    cta.ModelCompressor().compress_model_rtn(hook)
    monkeypatch.setattr(codec, "call", real)
    rtn = [c for c in calls if c[0].startswith("ct_rtn") or c[0] == "ct_minmax_qparams"]
    # window one: modules 0..31 = 8 of each kind; window two: modules 32, 33 = one W3 symmetric, one W3 asymmetric
    assert sorted(rtn) == sorted([("ct_rtn_quant_pack_wb_batch", 8)] * 3 + [("ct_rtn_quant_pack_w4_batch", 8)] + [("ct_rtn_quant_pack_wb_batch", 1)] * 2), rtn
    for i, (m, e) in enumerate(zip(hook, each)):
        a, b = _entries(m), _entries(e)
        assert [x[:3] for x in a] == [x[:3] for x in b] and all(torch.equal(x[3], y[3]) for x, y in zip(a, b)), (i, [x[:3] for x in a], [x[:3] for x in b])
        assert str(getattr(m.quantization_status, "value", m.quantization_status)) == "compressed"
    cta.ModelCompressor().decompress_model(hook)
    for i, (m, ((b, s), r)) in enumerate(zip(hook, recipes)):
        x = C.make_weight(r)
        scale, zp = O.calculate_qparams_minmax(x, num_bits=b, group_size=r["group"], symmetric=s)
        fq = O.fake_quantize(x, scale, zp, num_bits=b, strategy="group", group_size=r["group"])
        assert m.weight.dtype == BF16 and torch.equal(m.weight.data.cpu(), fq), (i, b, s)  # value equality: fake_quantize may carry -0.0


# ---- the converter --------------------------------------------------------------------------------------------------------------------
SHARD_KEYS = {"model.layers.0.self_attn.q_proj": "4x512.g64.bf16", "model.layers.0.mlp.up_proj": "3x256.gch.bf16",
              "model.layers.0.mlp.down_proj": "2x256.g128.f16.maxima"}
CONVERSIONS = [(3, True), (4, False)]


def _tensors():
    """four modules — two bf16 and one fp16 targeted, the ignored lm_head — and what stands around them"""
    t = {"model.embed_tokens.weight": torch.ones((32, 96), dtype=BF16)}
    for m, key in SHARD_KEYS.items():
        t[f"{m}.weight"] = C.make_weight(CASES[key])
    t["model.layers.0.input_layernorm.weight"] = torch.ones(96, dtype=BF16)
    t["model.norm.weight"] = torch.full((96,), 0.5, dtype=BF16)
    t["lm_head.weight"] = C.make_weight(CASES["1x32.g32.bf16"])
    return t


@pytest.mark.parametrize("b,s", CONVERSIONS)
def test_quantizer_process_equals_compress_rtn_per_module(cta, dev, b, s):
    from compressed_tensors_amd.entrypoints.convert import PackQuantizedQuantizer

    tensors = _tensors()
    conv = PackQuantizedQuantizer(b, 128, s, device=dev)
    conv.validate({k: None for k in tensors})
    out = conv.process(dict(tensors))
    want = []
    for name in tensors:
        if name.endswith(".weight") and name[:-7] in SHARD_KEYS:
            want += [name + "_packed", name + "_scale"] + ([] if s else [name + "_zero_point"]) + [name + "_shape"]
        else:
            want.append(name)
    assert list(out) == want and not out.ready and not out.keep  # the input's order, a module's entries where its weight was; settled
    scheme = scheme_of(cta, b, s, 128)
    for m in SHARD_KEYS:
        one = packer(cta).compress_rtn(tensors[f"{m}.weight"].to(dev), scheme)
        assert sorted(k for k in out if k.startswith(m + ".")) == sorted(f"{m}.{k}" for k in one)
        for k, t in one.items():
            assert not out[f"{m}.{k}"].is_cuda and same(out[f"{m}.{k}"], t), (m, k)
    for name, t in tensors.items():
        if not (name.endswith(".weight") and name[:-7] in SHARD_KEYS):
            assert out[name] is t, name  # the same object
    conv.stream_results = True
    streamed = conv.process(dict(tensors))
    assert streamed.ready
    streamed.wait()
    assert all(same(streamed[n], out[n]) for n in out)
    ragged = dict(tensors)
    ragged["model.layers.0.mlp.gate_proj.weight"] = torch.ones((2, 40), dtype=BF16)
    with pytest.raises(ValueError):
        conv.process(ragged)


def test_quantizer_sends_what_the_plan_refuses_through_compress_rtn(cta, dev, golden):
    """a group of 48 is no table item: the module goes through `compress_rtn` and still carries the reference's recorded bits"""
    from compressed_tensors_amd.entrypoints.convert import PackQuantizedQuantizer

    key = "2x96.g48.bf16"
    tensors = {"model.layers.0.self_attn.q_proj.weight": golden[f"{key}.x"], "model.norm.weight": torch.ones(96, dtype=BF16)}
    for b, s in ((3, True), (6, False)):
        out = PackQuantizedQuantizer(b, 48, s, device=dev).process(dict(tensors))
        m, tag = "model.layers.0.self_attn.q_proj", C.tag(b, s)
        assert same(out[f"{m}.weight_packed"], golden[f"{key}.{tag}.packed"]) and same(out[f"{m}.weight_scale"], golden[f"{key}.{tag}.scale"])
        assert s or same(out[f"{m}.weight_zero_point"], golden[f"{key}.{tag}.zp_packed"])
        assert out[f"{m}.weight_shape"].tolist() == [2, 96]


@pytest.mark.parametrize("b,s", CONVERSIONS)
def test_convert_checkpoint_then_dequantize_gives_the_oracles_weights(cta, dev, tmp_path, b, s):
    from safetensors.torch import load_file, save_file

    from compressed_tensors_amd.entrypoints.convert import CompressedTensorsDequantizer, PackQuantizedQuantizer, convert_checkpoint

    tensors = _tensors()
    src, mid, dst = (tmp_path / n for n in ("dense", "packed", "back"))
    src.mkdir()
    s1, s2 = "model-00001-of-00002.safetensors", "model-00002-of-00002.safetensors"
    shards = {s1: {}, s2: {}}
    for k, v in tensors.items():
        shards[s2 if ("down_proj" in k or k.startswith("lm_head")) else s1][k] = v
    wm = {}
    for fn, t in shards.items():
        save_file(t, str(src / fn))
        wm.update({k: fn for k in t})
    (src / "model.safetensors.index.json").write_text(json.dumps({"metadata": {"total_size": 0}, "weight_map": wm}))
    (src / "config.json").write_text(json.dumps({"model_type": "llama", "torch_dtype": "bfloat16"}))
    convert_checkpoint(str(src), str(mid), PackQuantizedQuantizer(b, 128, s, targets=["re:.*proj$"], device=dev), max_workers=1)
    cfg = json.loads((mid / "config.json").read_text())["quantization_config"]
    assert cfg["quant_method"] == "compressed-tensors" and cfg["format"] == "pack-quantized" and cfg["ignore"] == ["lm_head", "re:.*embed_tokens$"]
    group = cfg["config_groups"]["config_group_0"]
    assert group["targets"] == ["re:.*proj$"] and (group["weights"]["num_bits"], group["weights"]["symmetric"], group["weights"]["group_size"]) == (b, s, 128)
    stored = {}
    for fn in shards:
        stored.update(load_file(str(mid / fn)))
    scheme = scheme_of(cta, b, s, 128)
    for m in SHARD_KEYS:
        assert f"{m}.weight" not in stored
        for k, t in packer(cta).compress_rtn(tensors[f"{m}.weight"].to(dev), scheme).items():
            assert same(stored[f"{m}.{k}"], t), (m, k)
    assert same(stored["lm_head.weight"], tensors["lm_head.weight"])
    convert_checkpoint(str(mid), str(dst), CompressedTensorsDequantizer(str(mid), dtype=BF16, device=dev), max_workers=1)
    back = {}
    for fn in shards:
        back.update(load_file(str(dst / fn)))
    for m in SHARD_KEYS:
        x = tensors[f"{m}.weight"]
        scale, zp = O.calculate_qparams_minmax(x, num_bits=b, group_size=128, symmetric=s)
        fq = O.fake_quantize(x, scale, zp, num_bits=b, strategy="group", group_size=128).to(BF16)
        assert back[f"{m}.weight"].dtype == BF16 and torch.equal(back[f"{m}.weight"], fq), m  # value equality: fake_quantize may carry -0.0
    assert set(back) == set(tensors) and same(back["model.norm.weight"], tensors["model.norm.weight"])
