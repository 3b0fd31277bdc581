"""Group-wise 8-bit round-to-nearest in one pass (ct_rtn_quant_group8 and its table form) and what stands on it — compress_rtn of the group
schemes, MXFP8's compress_rtn and window hook, pack-quantized's 8-bit words, MXFP8Quantizer — against the reference's recorded results
(tests/golden/group8_rtn.safetensors), the pinned oracle's composition (tests/_group8_rtn_cases.oracle_outputs) and the composition kernels the
one pass replaces (the observer, quantize / quantize_and_pack, compress_mx_scale).  Everything is compared on raw bits, without a tolerance.
Every test here needs an MI355X:  python -m pytest tests -m gpu"""
import json
import os

import pytest
import torch

import _group8_rtn_cases as C
import oracle as O

pytestmark = pytest.mark.gpu

BF16, F16, F32, F8 = C.BF16, C.F16, C.F32, C.F8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "group8_rtn.safetensors")
CASES = dict(C.case_list())
FAST_KEYS = [k for k, r in CASES.items() if r["fast"]]
FALLBACK_KEYS = [k for k, r in CASES.items() if not r["fast"]]
KINDS = list(C.KINDS)
bits = C.bits


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
    """key -> (weight, {kind: the oracle composition's outputs}), computed once and never written to; the weight is the fixture's input"""
    out = {}
    for key, r in CASES.items():
        x = golden[f"{key}.x"]
        assert torch.equal(bits(x), bits(C.make_weight(r))), key
        out[key] = (x, {kind: C.oracle_outputs(O, x, r["group"], kind) for kind in C.kinds_of(r)})
    return out


def same(a, b):
    """equal shapes and raw bits (the fixture keeps float8 tensors as bytes)"""
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and torch.equal(bits(a.cpu().contiguous()), bits(b.cpu().contiguous()))


def weights_args(cta, kind, group):
    return cta.QuantizationArgs(strategy="group", group_size=group, **C.KINDS[kind])


def scheme_of(cta, kind, group, weights_only=False):
    act = None if weights_only else cta.QuantizationArgs(num_bits=8, type=C.KINDS[kind]["type"], strategy="token", symmetric=True, dynamic=True)
    return cta.QuantizationScheme(targets=["Linear"], weights=weights_args(cta, kind, group), input_activations=act)


def compressor_of(cta, kind):
    return cta.BaseCompressor.get_value_from_registry({"mxfp8": "mxfp8-quantized", "fp8": "float-quantized"}.get(kind, "int-quantized"))


def one_pass(cta, w, group, kind, words=False):
    """the new entry's outputs under the fixture's names"""
    a = C.KINDS[kind]
    got = cta.codec.rtn_quantize_group8(w, group_size=group, qtype=a["type"], symmetric=a["symmetric"], mx=(kind == "mxfp8"), words=words)
    out = {"packed" if words else "q": got[0], "scale": got[1]}
    if a["type"] == "int":
        out["zero_point"] = got[2]
    else:
        assert got[2] is None
    if kind == "mxfp8":
        out["e8m0"] = got[3]
    return out


def composition(cta, w, group, kind):
    """the existing kernels the one pass replaces: observer, quantize (and the 8-bit words), compress_mx_scale"""
    codec = cta.codec
    if kind in ("fp8", "mxfp8"):
        scale = codec.minmax_qparams_float(w, kind=kind, group_size=group)
        zp = torch.zeros(scale.shape, dtype=F8, device=w.device)
        out = dict(scale=scale, q=codec.quantize_tensor(w, scale, zp, num_bits=8, strategy="group", group_size=group, dtype=F8, qtype="float"))
        if kind == "mxfp8":
            out["e8m0"] = codec.compress_mx_scale(scale)
        return out
    scale, zp = codec.minmax_qparams(w, num_bits=8, group_size=group, symmetric=C.KINDS[kind]["symmetric"])
    return dict(scale=scale, zero_point=zp, q=codec.quantize_tensor(w, scale, zp, num_bits=8, strategy="group", group_size=group, dtype=torch.int8),
                packed=codec.quantize_and_pack(w, scale, zp, num_bits=8, strategy="group", group_size=group))


def check(got, want, names, what):
    for name in names:
        a, b = got[name], want[name]
        assert same(a, b), (*what, name, int((bits(a.cpu().contiguous()).reshape(-1) != bits(b.cpu().contiguous()).reshape(-1)).sum()) if a.shape == b.shape else (a.shape, b.shape))


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", FAST_KEYS)
def test_one_pass_equals_fixture_oracle_and_composition(cta, dev, ref, golden, key, kind):
    """ct_rtn_quant_group8 == group min / max + calculate_qparams + quantize (+ compress_mx_scale; + the 8-bit words): 0 ulp against the reference's
    recorded results, the oracle and the kernels it replaces"""
    r = CASES[key]
    if kind not in C.kinds_of(r):
        with pytest.raises(NotImplementedError):  # MXFP8 groups hold 32 elements
            one_pass(cta, ref[key][0].to(dev), r["group"], kind)
        return
    x, want = ref[key]
    w = x.to(dev)
    got = one_pass(cta, w, r["group"], kind)
    assert got["q"].dtype == (torch.int8 if kind.startswith("int8") else F8) and got["scale"].dtype == x.dtype
    names = [n for n in want[kind] if n != "packed"]
    fixture = {n: golden[f"{key}.{kind}.{n}"] for n in want[kind]}
    two = composition(cta, w, r["group"], kind)
    for other, what in ((fixture, "fixture"), (want[kind], "oracle"), (two, "composition")):
        check(got, other, names, (key, kind, what))
    if kind.startswith("int8"):
        packed = one_pass(cta, w, r["group"], kind, words=True)
        assert packed["packed"].dtype == torch.int32
        for other, what in ((fixture, "fixture"), (want[kind], "oracle"), (two, "composition")):
            check(packed, other, ["packed", "scale", "zero_point"], (key, kind, "words", what))
    if kind == "mxfp8":
        assert got["e8m0"].dtype == torch.uint8


def test_extreme_rows_give_the_references_finite_codes(cta, dev, golden):
    """rows of +- the largest finite value: the MXFP8 scale of a bf16 row is inf, every code is zero and the exponent byte is the reference's"""
    key = "3x128.g32.bf16.extremes"
    q, scale, _, code = cta.codec.rtn_quantize_group8(golden[f"{key}.x"].to(dev), group_size=32, qtype="float", mx=True)
    assert bool(torch.isinf(scale[0].float()).all()) and int(bits(q.cpu())[0].count_nonzero()) == 0
    assert torch.equal(code.cpu(), golden[f"{key}.mxfp8.e8m0"])
    assert bool(torch.isfinite(q.cpu().view(F8).float()).all())


@pytest.mark.parametrize("kind,words", [(k, False) for k in KINDS] + [("int8", True), ("int8_zp", True)])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_one_table_over_all_cases_equals_the_single_launches(cta, dev, ref, kind, dtype, words, monkeypatch):
    """rtn_quantize_group8_many: ONE launch over every fast case of a dtype, whatever its group == the single launches; an empty list and an empty table"""
    a = C.KINDS[kind]
    kw = dict(qtype=a["type"], symmetric=a["symmetric"], mx=(kind == "mxfp8"), words=words)
    keys = [k for k in FAST_KEYS if CASES[k]["dtype"] == dtype and kind in C.kinds_of(CASES[k])]
    xs, groups = [ref[k][0].to(dev) for k in keys], [CASES[k]["group"] for k in keys]
    calls, real = [], cta.codec.call
    monkeypatch.setattr(cta.codec, "call", lambda name, *args: calls.append((name, args[1])) or real(name, *args))
    got = cta.codec.rtn_quantize_group8_many(xs, group_size=groups, **kw)
    monkeypatch.undo()
    assert [c for c in calls if c[0].startswith("ct_rtn")] == [("ct_rtn_quant_group8_batch", len(keys))], calls
    for k, x, group, g in zip(keys, xs, groups, got):
        single = cta.codec.rtn_quantize_group8(x, group_size=group, **kw)
        assert len(g) == len(single) and all((s is None and t is None) or same(s, t) for s, t in zip(single, g)), (k, kind)
    assert cta.codec.rtn_quantize_group8_many([], group_size=32, **kw) == []
    assert cta.codec.launch_rtn_group8_words([], 0, BF16, dev, 4) is None  # an empty table: nothing is touched


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _composed(cta, comp, w, scheme):
    from compressed_tensors_amd.quantization.utils import calculate_qparams_from_weight

    scale, zp = calculate_qparams_from_weight(w, scheme.weights)
    return comp.compress({"weight": w, "weight_scale": scale, "weight_zero_point": zp}, scheme)


def _same_dicts(one, two):
    return list(one) == list(two) and all(one[k].dtype == two[k].dtype and same(one[k], two[k]) for k in one)


@pytest.mark.parametrize("key,kind", [(key, kind) for key in FALLBACK_KEYS for kind in C.kinds_of(CASES[key])])
def test_compress_rtn_of_what_the_plan_refuses_is_the_composition(cta, dev, ref, golden, key, kind):
    """float32, group 48 and the first group above the plan's maximum: the codec refuses by name, compress_rtn composes — the reference's bits"""
    from compressed_tensors_amd.quantization.utils import group_one_pass

    r = CASES[key]
    x, want = ref[key]
    w = x.to(dev)
    assert not cta.codec.rtn_group8_group(x.shape, r["group"]) or x.dtype == F32
    with pytest.raises(NotImplementedError):
        one_pass(cta, w, r["group"], kind)
    scheme = scheme_of(cta, kind, r["group"])
    assert group_one_pass(w, scheme.weights) == ""
    got = compressor_of(cta, kind).compress_rtn(w, scheme)
    assert _same_dicts(got, _composed(cta, compressor_of(cta, kind), w, scheme))
    assert same(got["weight"], golden[f"{key}.{kind}.q"]) and same(got["weight"], want[kind]["q"]), (key, kind)
    assert same(got["weight_scale"], golden[f"{key}.{kind}.e8m0" if kind == "mxfp8" else f"{key}.{kind}.scale"]), (key, kind)
    if kind == "int8_zp":
        assert same(got["weight_zero_point"], golden[f"{key}.{kind}.zero_point"])


@pytest.mark.parametrize("kind", KINDS)
def test_a_misaligned_view_and_ragged_columns(cta, dev, ref, kind):
    """a view one element into its storage takes the composition with the same bits; cols % g != 0 raises the reference's ValueError"""
    from compressed_tensors_amd.quantization.utils import group_one_pass

    group = 32 if kind == "mxfp8" else 128
    key = C.key_of((3, 3 * group), group, "bf16", "planted")
    x, want = ref[key]
    store = torch.zeros(x.numel() + 1, dtype=x.dtype, device=dev)
    view = store[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 and view.is_contiguous()
    scheme = scheme_of(cta, kind, group)
    comp = compressor_of(cta, kind)
    assert group_one_pass(view, scheme.weights) == "" and group_one_pass(x.to(dev), scheme.weights) != ""
    got = comp.compress_rtn(view, scheme)
    assert _same_dicts(got, _composed(cta, comp, view, scheme)) and same(got["weight"], want[kind]["q"])
    direct = one_pass(cta, view, group, kind)  # the codec itself realigns
    assert same(direct["q"], want[kind]["q"]) and same(direct["scale"], want[kind]["scale"])
    ragged = x[:, :-8].contiguous().to(dev)
    with pytest.raises(ValueError):
        one_pass(cta, ragged, group, kind)
    with pytest.raises(ValueError):
        comp.compress_rtn(ragged, scheme)


# ---- compress_rtn ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_compress_rtn_one_pass_equals_the_composition(cta, dev, ref, kind, dtype, monkeypatch):
    """every one-pass branch of compress_rtn (forced on, whatever the measured dispatch says) returns the composition's state dict: entries, order,
    dtypes, shapes, bits — naive / int / float-quantized and mxfp8-quantized, and pack-quantized's 8-bit words (group, and a channel as one group)"""
    from compressed_tensors_amd.compressors.naive_quantized import base as naive

    group = 32 if kind == "mxfp8" else 128
    key = C.key_of((3, 3 * group), group, dtype, "planted")
    x, want = ref[key]
    w = x.to(dev)
    comp, scheme = compressor_of(cta, kind), scheme_of(cta, kind, group)
    two = _composed(cta, comp, w, scheme)
    calls, real = [], cta.codec.call
    monkeypatch.setattr(naive, "RTN_GROUP8_MEASURED_FASTER", dict.fromkeys(naive.RTN_GROUP8_MEASURED_FASTER, True))
    monkeypatch.setattr(cta.codec, "call", lambda name, *a: calls.append(name) or real(name, *a))
    one = comp.compress_rtn(w, scheme)
    assert calls == ["ct_rtn_quant_group8"], calls
    assert _same_dicts(one, two), (list(one), list(two))
    assert same(one["weight"], want[kind]["q"])
    if kind.startswith("int8"):
        packer = cta.BaseCompressor.get_value_from_registry("pack-quantized")
        wide = ref[C.key_of((4, 512), 256, dtype)][0].to(dev)  # a row of 512 as one group
        for w, args in ((w, weights_args(cta, kind, group)), (wide, cta.QuantizationArgs(strategy="channel", **C.KINDS[kind]))):
            sch = cta.QuantizationScheme(targets=["Linear"], weights=args)
            del calls[:]
            one = packer.compress_rtn(w, sch)
            assert calls[0] == "ct_rtn_quant_group8" and "ct_minmax_qparams" not in calls, calls
            monkeypatch.setattr(naive, "RTN_GROUP8_MEASURED_FASTER", dict.fromkeys(naive.RTN_GROUP8_MEASURED_FASTER, False))
            two = packer.compress_rtn(w, sch)
            monkeypatch.setattr(naive, "RTN_GROUP8_MEASURED_FASTER", dict.fromkeys(naive.RTN_GROUP8_MEASURED_FASTER, True))
            assert _same_dicts(one, two), (list(one), list(two))
        assert same(packer.compress_rtn(x.to(dev), cta.QuantizationScheme(targets=["Linear"], weights=weights_args(cta, kind, group)))["weight_packed"], want[kind]["packed"])


# ---- modules --------------------------------------------------------------------------------------------------------------------------
TREE_KEYS = ("3x96.g32.bf16.planted", "1x8224.g32.bf16", "4x64.g32.f32")


def _tree(cta, dev):
    """three MXFP8 Linears: the planted groups and the partial last workgroup, both one pass, and a float32 weight, which the plan refuses; one bias"""
    scheme = scheme_of(cta, "mxfp8", 32)
    scheme.format = "mxfp8-quantized"
    layers = []
    for k, key in enumerate(TREE_KEYS):
        x = C.make_weight(CASES[key])
        m = torch.nn.Linear(x.shape[1], x.shape[0], bias=(k == 1)).to(dev).to(x.dtype)
        m.weight.data.copy_(x)
        if m.bias is not None:
            m.bias.data.copy_(torch.arange(x.shape[0]) % 7 - 3)
        m.quantization_scheme = scheme
        layers.append(m)
    return torch.nn.Sequential(*layers)


def _entries(m):
    return [(n, t.dtype, tuple(t.shape), bits(t.data.cpu())) for n, t in (*m._parameters.items(), *m._buffers.items()) if t is not None]


def test_three_ways_through_a_tree_give_identical_modules(cta, dev, ref, golden, monkeypatch):
    """compress_model_rtn per module (batched=False), the MXFP8 window hook and compress_rtn per module leave identical modules — entry names, order,
    dtypes, bits — with the one pass on and off; decompress_model then gives the composition's weights"""
    from compressed_tensors_amd.compressors.mxfp8.base import MXFP8QuantizationCompressor as MX
    from compressed_tensors_amd.compressors.naive_quantized import base as naive

    for name in ("float-quantized", "int-quantized", "naive-quantized"):
        assert not hasattr(cta.BaseCompressor.get_value_from_registry(name), "compress_rtn_modules")
    assert "compress_rtn_modules" in vars(MX) and "RTN_TABLE_MEASURED_FASTER" in vars(MX)
    composed = _tree(cta, dev)
    monkeypatch.setattr(naive, "RTN_GROUP8_MEASURED_FASTER", dict.fromkeys(naive.RTN_GROUP8_MEASURED_FASTER, False))
    cta.ModelCompressor().compress_model_rtn(composed, batched=False)
    monkeypatch.setattr(naive, "RTN_GROUP8_MEASURED_FASTER", dict.fromkeys(naive.RTN_GROUP8_MEASURED_FASTER, True))
    loop, hook, each = _tree(cta, dev), _tree(cta, dev), _tree(cta, dev)
    bias = loop[1].bias.data.clone()
    cta.ModelCompressor().compress_model_rtn(loop, batched=False)
    calls, real = [], cta.codec.call
    monkeypatch.setattr(cta.codec, "call", lambda name, *a: calls.append((name, a[1])) or real(name, *a))
    MX.compress_rtn_modules(list(hook))
    assert [c for c in calls if c[0].startswith("ct_rtn")] == [("ct_rtn_quant_group8_batch", 2)]  # one table of the two weights the plan takes
    monkeypatch.setattr(cta.codec, "call", real)
    for m in each:
        MX.compress_rtn_module(m)
    for k, key in enumerate(TREE_KEYS):
        a = _entries(composed[k])
        for other in (loop, hook, each):
            b = _entries(other[k])
            assert [e[:3] for e in a] == [e[:3] for e in b] and all(torch.equal(x[3], y[3]) for x, y in zip(a, b)), (key, [e[:3] for e in a], [e[:3] for e in b])
            assert str(getattr(other[k].quantization_status, "value", other[k].quantization_status)) == "compressed"
        assert sorted(e[0] for e in a) == sorted(["weight", "weight_scale"] + (["bias"] if k == 1 else []))
        assert same(loop[k].weight.data, golden[f"{key}.mxfp8.q"]) and same(loop[k].weight_scale.data, golden[f"{key}.mxfp8.e8m0"]), key
    assert torch.equal(loop[1].bias.data, bias)
    cta.ModelCompressor().decompress_model(loop)
    cta.ModelCompressor().decompress_model(composed)
    for k, key in enumerate(TREE_KEYS):
        assert loop[k].weight.dtype == composed[k].weight.dtype and same(loop[k].weight.data, composed[k].weight.data), key
        q, code = ref[key][1]["mxfp8"]["q"], ref[key][1]["mxfp8"]["e8m0"]
        dq = O.dequantize(q, O.e8m0_decode(code), None, strategy="group", group_size=32)
        assert same(loop[k].weight.data, dq.to(loop[k].weight.dtype)), key


# ---- the converter --------------------------------------------------------------------------------------------------------------------
def _shard(bias: bool):
    """a dense shard: two targeted weights (bf16 and fp16: a table each), with `bias` a bias (CompressedTensorsDequantizer's validate takes none beside
    a compressed module), two norms, the ignored embedding and lm_head"""
    keys = {"model.layers.0.self_attn.q_proj": "3x96.g32.bf16.planted", "model.layers.0.mlp.down_proj": "2x256.g32.f16.maxima"}
    t = {"model.embed_tokens.weight": torch.ones((32, 96), dtype=BF16)}
    for m, key in keys.items():
        t[f"{m}.weight"] = C.make_weight(CASES[key])
    if bias:
        t["model.layers.0.self_attn.q_proj.bias"] = torch.arange(3, dtype=torch.float32).to(BF16)
    t["model.layers.0.input_layernorm.weight"] = torch.ones(96, dtype=BF16)
    t["model.norm.weight"] = torch.full((96,), 0.5, dtype=BF16)
    t["lm_head.weight"] = C.make_weight(CASES["1x32.g32.bf16"])
    return t, keys


def test_quantizer_process_on_a_two_module_shard(cta, dev, golden):
    from compressed_tensors_amd.entrypoints.convert import MXFP8Quantizer

    tensors, keys = _shard(bias=True)
    conv = MXFP8Quantizer(device=dev)
    conv.validate({k: None for k in tensors})
    out = conv.process(dict(tensors))
    want = []
    for name in tensors:
        want.append(name)
        if name.endswith(".weight") and name[:-7] in keys:
            want.append(name + "_scale")
    assert list(out) == want and not out.ready and not out.keep  # the input's order, the scale behind its weight; settled
    for m, key in keys.items():
        q, code = out[f"{m}.weight"], out[f"{m}.weight_scale"]
        assert not q.is_cuda and q.dtype == F8 and code.dtype == torch.uint8
        assert same(q, golden[f"{key}.mxfp8.q"]) and same(code, golden[f"{key}.mxfp8.e8m0"]), m
    for name, t in tensors.items():
        if not (name.endswith(".weight") and name[:-7] in keys):
            assert out[name] is t, name  # the same object
    conv.stream_results = True
    streamed = conv.process(dict(tensors))
    assert streamed.ready
    streamed.wait()
    assert all(same(streamed[n], out[n]) for n in out)
    ragged = dict(tensors)
    ragged["model.layers.0.mlp.up_proj.weight"] = torch.ones((2, 40), dtype=BF16)
    with pytest.raises(ValueError):
        conv.process(ragged)


def test_convert_checkpoint_then_dequantize_gives_the_oracles_weights(cta, dev, ref, golden, tmp_path):
    from safetensors.torch import load_file, save_file

    from compressed_tensors_amd.entrypoints.convert import CompressedTensorsDequantizer, MXFP8Quantizer, convert_checkpoint

    tensors, keys = _shard(bias=False)
    src, mid, dst = (tmp_path / n for n in ("dense", "mxfp8", "back"))
    src.mkdir()
    save_file(tensors, str(src / "model.safetensors"))
    (src / "config.json").write_text(json.dumps({"model_type": "llama", "torch_dtype": "bfloat16"}))
    convert_checkpoint(str(src), str(mid), MXFP8Quantizer(targets=["re:.*proj$"], device=dev), max_workers=1)
    cfg = json.loads((mid / "config.json").read_text())["quantization_config"]
    assert cfg["quant_method"] == "compressed-tensors" and cfg["format"] == "mxfp8-quantized" and cfg["ignore"] == ["lm_head", "re:.*embed_tokens$"]
    assert cfg["config_groups"]["config_group_0"]["targets"] == ["re:.*proj$"]
    stored = load_file(str(mid / "model.safetensors"))
    for m, key in keys.items():
        assert same(stored[f"{m}.weight"], golden[f"{key}.mxfp8.q"]) and same(stored[f"{m}.weight_scale"], golden[f"{key}.mxfp8.e8m0"]), m
    assert same(stored["lm_head.weight"], tensors["lm_head.weight"])
    convert_checkpoint(str(mid), str(dst), CompressedTensorsDequantizer(str(mid), dtype=BF16, device=dev), max_workers=1)
    back = load_file(str(dst / "model.safetensors"))
    for m, key in keys.items():
        o = ref[key][1]["mxfp8"]
        dq = O.dequantize(o["q"], O.e8m0_decode(o["e8m0"]), None, strategy="group", group_size=32).to(BF16)
        assert same(back[f"{m}.weight"], dq), m
    assert set(back) == set(tensors) and same(back["model.norm.weight"], tensors["model.norm.weight"])
