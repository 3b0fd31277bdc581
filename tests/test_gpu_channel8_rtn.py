"""Channel-wise 8-bit round-to-nearest in one pass (ct_rtn_quant_channel8 with its long-row form, and its table form) and what stands on it —
compress_rtn of the channel schemes, the window driver, FP8DynamicQuantizer / W8A8Quantizer — against the reference's recorded results
(tests/golden/channel8_rtn.safetensors), the pinned oracle's composition (tests/_channel8_rtn_cases.oracle_outputs) and the composition kernels the
one pass replaces (the observer, quantize).  Everything is compared on raw bits, without a tolerance.
Every test here needs an MI355X:  python -m pytest tests -m gpu"""
import json
import os

import pytest
import torch

import _channel8_rtn_cases as C
import oracle as O

pytestmark = pytest.mark.gpu

BF16, F16, F32, F8 = C.BF16, C.F16, C.F32, C.F8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "channel8_rtn.safetensors")
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
    """key -> (weight, {kind: the oracle composition's outputs}), computed once and never written to; the weight is the fixture's input where the
    fixture stores it"""
    out = {}
    for key, r in CASES.items():
        x = C.make_weight(r)
        if C.x_stored(r):
            assert torch.equal(bits(x), bits(golden[f"{key}.x"])), key
        out[key] = (x, {kind: C.oracle_outputs(O, x, kind) for kind in KINDS})
    return out


def same(a, b):
    """equal shapes and raw bits (the fixture keeps float8 tensors as bytes)"""
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and torch.equal(bits(a.cpu().contiguous()), bits(b.cpu().contiguous()))


def scheme_of(cta, kind, weights_only=False):
    act = None if weights_only else cta.QuantizationArgs(num_bits=8, type=C.KINDS[kind]["type"], strategy="token", symmetric=True, dynamic=True)
    return cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(strategy="channel", **C.KINDS[kind]), input_activations=act)


def compressor_of(cta, kind):
    return cta.BaseCompressor.get_value_from_registry("float-quantized" if kind == "fp8" else "int-quantized")


def named(kind, got):
    """a (codes, scale, zero_point) triple under the fixture's names"""
    out = {"q": got[0], "scale": got[1]}
    if kind != "fp8":
        out["zero_point"] = got[2]
    return out


def one_pass(cta, w, kind):
    a = C.KINDS[kind]
    return named(kind, cta.codec.rtn_quantize_channel8(w, qtype=a["type"], symmetric=a["symmetric"]))


def composition(cta, w, kind):
    """the existing kernels the one pass replaces: the observer, then quantize"""
    codec = cta.codec
    if kind == "fp8":
        scale = codec.minmax_qparams_float(w, kind="fp8")
        zp = torch.zeros(scale.shape, dtype=F8, device=w.device)
        return dict(scale=scale, q=codec.quantize_tensor(w, scale, zp, num_bits=8, strategy="channel", dtype=F8, qtype="float"))
    scale, zp = codec.minmax_qparams(w, num_bits=8, symmetric=C.KINDS[kind]["symmetric"])
    return dict(scale=scale, zero_point=zp, q=codec.quantize_tensor(w, scale, zp, num_bits=8, strategy="channel", dtype=torch.int8))


def check(got, want, what):
    for name in want:
        a, b = got[name], want[name]
        assert same(a, b), (*what, name, int((bits(a.cpu().contiguous()).reshape(-1) != bits(b.cpu().contiguous()).reshape(-1)).sum()) if a.shape == b.shape else (a.shape, b.shape))


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", FAST_KEYS)
def test_one_pass_equals_fixture_oracle_and_composition(cta, dev, ref, golden, key, kind):
    """ct_rtn_quant_channel8 == per-row min / max + calculate_qparams + quantize in every form — a wave per row, a workgroup per row, the long
    form: 0 ulp against the reference's recorded results (where the fixture stores the case), the oracle and the kernels it replaces"""
    r = CASES[key]
    x, want = ref[key]
    w = x.to(dev)
    assert cta.codec.rtn_channel8_form(x.shape, C.KINDS[kind]["symmetric"]) in ("wave", "row", "long")
    got = one_pass(cta, w, kind)
    assert got["q"].dtype == (F8 if kind == "fp8" else torch.int8) and got["scale"].dtype == x.dtype and got["scale"].shape == (x.shape[0], 1)
    others = [(want[kind], "oracle"), (composition(cta, w, kind), "composition")]
    if r["stored"]:
        others.insert(0, ({n: golden[f"{key}.{kind}.{n}"] for n in want[kind]}, "fixture"))
    for other, what in others:
        check(got, other, (key, kind, what))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_one_table_over_all_cases_equals_the_single_launches(cta, dev, ref, kind, dtype, monkeypatch):
    """rtn_quantize_channel8_many: ONE launch over every fast case of a dtype, whatever its form == the single launches; an empty list and an
    empty table"""
    a = C.KINDS[kind]
    kw = dict(qtype=a["type"], symmetric=a["symmetric"])
    keys = [k for k in FAST_KEYS if CASES[k]["dtype"] == dtype]
    assert {cta.codec.rtn_channel8_form(CASES[k]["shape"], a["symmetric"]) for k in keys} == {"wave", "row", "long"}
    xs = [ref[k][0].to(dev) for k in keys]
    calls, real = [], cta.codec.call
    monkeypatch.setattr(cta.codec, "call", lambda name, *args: calls.append((name, args[1])) or real(name, *args))
    got = cta.codec.rtn_quantize_channel8_many(xs, **kw)
    monkeypatch.undo()
    assert [c for c in calls if c[0].startswith("ct_rtn")] == [("ct_rtn_quant_channel8_batch", len(keys))], calls
    for k, x, g in zip(keys, xs, got):
        single = cta.codec.rtn_quantize_channel8(x, **kw)
        assert len(g) == len(single) == 3 and all(s.dtype == t.dtype and same(s, t) for s, t in zip(single, g)), (k, kind)
        check(named(kind, g), ref[k][1][kind], (k, kind, "oracle"))
    assert cta.codec.rtn_quantize_channel8_many([], **kw) == []
    assert cta.codec.launch_rtn_channel8_words([], 0, BF16, dev, a["type"] == "float", a["symmetric"]) is None  # an empty table: nothing is touched


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _composed(cta, comp, w, scheme):
    from compressed_tensors_amd.quantization.utils import calculate_qparams_from_weight

    scale, zp = calculate_qparams_from_weight(w, scheme.weights)
    return comp.compress({"weight": w, "weight_scale": scale, "weight_zero_point": zp}, scheme)


def _same_dicts(one, two):
    return list(one) == list(two) and all(one[k].dtype == two[k].dtype and same(one[k], two[k]) for k in one)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", FALLBACK_KEYS)
def test_what_the_plan_refuses_takes_the_composition(cta, dev, ref, golden, key, kind, monkeypatch):
    """float32, cols % 8 != 0 and one unit above the maximum: the codec refuses by name; the list form and compress_rtn compose — the oracle's bits"""
    r = CASES[key]
    x, want = ref[key]
    w = x.to(dev)
    a = C.KINDS[kind]
    assert cta.codec.rtn_channel8_form(x.shape, a["symmetric"]) == "" or x.dtype == F32
    with pytest.raises(NotImplementedError, match="65536"):
        one_pass(cta, w, kind)
    short = ref[C.key_of((2, 2056), "bf16")][0].to(dev)
    calls, real = [], cta.codec.call
    monkeypatch.setattr(cta.codec, "call", lambda name, *args: calls.append((name, args[1])) or real(name, *args))
    many = cta.codec.rtn_quantize_channel8_many([w, short, w], qtype=a["type"], symmetric=a["symmetric"])
    monkeypatch.undo()
    assert [c for c in calls if c[0].startswith("ct_rtn")] == [("ct_rtn_quant_channel8_batch", 1)], calls  # the one tensor the plan takes
    two = composition(cta, w, kind)
    for g in (many[0], many[2]):
        check(named(kind, g), two, (key, kind, "composition"))
        check(named(kind, g), want[kind], (key, kind, "oracle"))
    check(named(kind, many[1]), ref[C.key_of((2, 2056), "bf16")][1][kind], (key, kind, "the tensor between"))
    comp, scheme = compressor_of(cta, kind), scheme_of(cta, kind)
    got = comp.compress_rtn(w, scheme)
    assert _same_dicts(got, _composed(cta, comp, w, scheme))
    assert same(got["weight"], want[kind]["q"]) and same(got["weight_scale"], want[kind]["scale"]), (key, kind)
    if r["stored"]:
        assert same(got["weight"], golden[f"{key}.{kind}.q"]) and same(got["weight_scale"], golden[f"{key}.{kind}.scale"]), (key, kind)
    if kind == "int8_zp":
        assert same(got["weight_zero_point"], want[kind]["zero_point"])


# ---- compress_rtn ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", [True, False])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_compress_rtn_of_a_long_row_equals_the_composition(cta, dev, ref, kind, dtype, gate, monkeypatch):
    """float-quantized and int-quantized on a down_proj-length row: with the long form's dispatch on, ONE ct_rtn_quant_channel8 launch; off, the
    composition; either way the composition's state dict — entries, order, dtypes, shapes, bits"""
    from compressed_tensors_amd.compressors.naive_quantized import base as naive

    key = C.key_of((1, 29568), dtype)
    x, want = ref[key]
    w = x.to(dev)
    comp, scheme = compressor_of(cta, kind), scheme_of(cta, kind)
    two = _composed(cta, comp, w, scheme)
    calls, real = [], cta.codec.call
    monkeypatch.setattr(naive, "RTN_CHANNEL8_LONG_MEASURED_FASTER", dict.fromkeys(naive.RTN_CHANNEL8_LONG_MEASURED_FASTER, gate))
    monkeypatch.setattr(cta.codec, "call", lambda name, *a: calls.append(name) or real(name, *a))
    one = comp.compress_rtn(w, scheme)
    monkeypatch.undo()
    assert (calls == ["ct_rtn_quant_channel8"]) if gate else (calls and "ct_rtn_quant_channel8" not in calls), calls
    assert _same_dicts(one, two), (list(one), list(two))
    assert list(one) == ["weight_scale"] + (["weight_zero_point"] if kind == "int8_zp" else []) + ["weight"]  # `compress` re-adds the weight last
    assert same(one["weight"], want[kind]["q"]) and same(one["weight_scale"], want[kind]["scale"])


# ---- modules --------------------------------------------------------------------------------------------------------------------------
# (rows whose asymmetric scale overflows — +- the largest finite value — stay with the kernel tests: their fake_quantize is NaN, which int8 codes do not carry)
TREE_KEYS = ("2x2048.bf16", "1x16392.bf16", "4x64.f32")


def _tree(cta, dev, kind):
    """three Linears: a short row (the wave form), a long row, and a float32 weight, which the plan refuses; one bias"""
    scheme = scheme_of(cta, kind)
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


@pytest.mark.parametrize("kind", KINDS)
def test_three_ways_through_a_tree_give_identical_modules(cta, dev, ref, kind, monkeypatch):
    """rtn_channel8_windows (one table of the two weights the plan takes), compress_rtn_module per module and compress_model_rtn(batched=False) leave
    identical modules — entry names, order, dtypes, bits; decompress_model then gives the oracle's fake_quantize"""
    from compressed_tensors_amd.compressors.naive_quantized.base import rtn_channel8_windows

    cls = compressor_of(cta, kind)
    assert not hasattr(cls, "compress_rtn_modules")
    windows, each, loop = _tree(cta, dev, kind), _tree(cta, dev, kind), _tree(cta, dev, kind)
    calls, real = [], cta.codec.call
    monkeypatch.setattr(cta.codec, "call", lambda name, *a: calls.append((name, a[1])) or real(name, *a))
    rtn_channel8_windows(cls, list(windows))
    monkeypatch.undo()
    assert [c for c in calls if c[0].startswith("ct_rtn")] == [("ct_rtn_quant_channel8_batch", 2)], calls
    for m in each:
        cls.compress_rtn_module(m)
    cta.ModelCompressor().compress_model_rtn(loop, batched=False)
    names = ["weight", "weight_scale"] + (["weight_zero_point"] if kind == "int8_zp" else [])
    for k, key in enumerate(TREE_KEYS):
        a = _entries(windows[k])
        for other in (each, loop):
            b = _entries(other[k])
            assert [e[:3] for e in a] == [e[:3] for e in b] and all(torch.equal(x[3], y[3]) for x, y in zip(a, b)), (key, [e[:3] for e in a], [e[:3] for e in b])
            assert str(getattr(other[k].quantization_status, "value", other[k].quantization_status)) == "compressed"
        assert str(getattr(windows[k].quantization_status, "value", windows[k].quantization_status)) == "compressed"
        assert sorted(e[0] for e in a) == sorted(names + (["bias"] if k == 1 else []))
        o = ref[key][1][kind]
        assert same(windows[k].weight.data, o["q"]) and same(windows[k].weight_scale.data, o["scale"]), key
    cta.ModelCompressor().decompress_model(windows)
    a = C.KINDS[kind]
    for k, key in enumerate(TREE_KEYS):
        x, o = ref[key][0], ref[key][1][kind]
        zp = o.get("zero_point", torch.zeros(o["scale"].shape, dtype=F8))
        fq = O.fake_quantize(x, o["scale"], zp, num_bits=8, strategy="channel", qtype=a["type"])
        assert windows[k].weight.dtype == fq.dtype and torch.equal(windows[k].weight.data.cpu(), fq), key  # values: fake_quantize may carry -0.0
        assert same(windows[k].weight.data, O.dequantize(o["q"], o["scale"], o.get("zero_point"), strategy="channel")), key


# ---- the converters -------------------------------------------------------------------------------------------------------------------
SHARD_KEYS = {"model.layers.0.self_attn.q_proj": "5x512.bf16", "model.layers.0.mlp.down_proj": "1x16392.f16"}


def _shard(bias: bool):
    """a dense shard: two targeted weights (bf16, and fp16 with a long row: a table each), with `bias` a bias (CompressedTensorsDequantizer's
    validate takes none beside a compressed module), two 1-D norms, the ignored embedding and lm_head"""
    t = {"model.embed_tokens.weight": torch.ones((32, 512), dtype=BF16)}
    for m, key in SHARD_KEYS.items():
        t[f"{m}.weight"] = C.make_weight(CASES[key])
    if bias:
        t["model.layers.0.self_attn.q_proj.bias"] = torch.arange(5, dtype=torch.float32).to(BF16)
    t["model.layers.0.input_layernorm.weight"] = torch.ones(512, dtype=BF16)
    t["model.norm.weight"] = torch.full((512,), 0.5, dtype=BF16)
    t["lm_head.weight"] = C.make_weight(CASES["1x8.bf16"])
    return t


def _converter(name):
    from compressed_tensors_amd.entrypoints import convert

    return getattr(convert, name)


@pytest.mark.parametrize("name,kind", [("FP8DynamicQuantizer", "fp8"), ("W8A8Quantizer", "int8")])
def test_quantizer_process_on_a_two_module_shard(cta, dev, ref, golden, name, kind, monkeypatch):
    tensors = _shard(bias=True)
    conv = _converter(name)(device=dev)
    conv.validate({k: None for k in tensors})
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    launches, real = [], lib.ct_rtn_quant_channel8_batch
    monkeypatch.setattr(lib, "ct_rtn_quant_channel8_batch", lambda table, n, *a: launches.append(n) or real(table, n, *a))
    out = conv.process(dict(tensors))
    monkeypatch.undo()
    assert launches == [1, 1], launches  # one table per dtype
    want = []
    for key in tensors:
        want.append(key)
        if key.endswith(".weight") and key[:-7] in SHARD_KEYS:
            want.append(key + "_scale")
    assert list(out) == want and not out.ready and not out.keep  # the input's order, the scale behind its weight, no zero point; settled
    comp, scheme = compressor_of(cta, kind), scheme_of(cta, kind)
    for m, key in SHARD_KEYS.items():
        q, scale = out[f"{m}.weight"], out[f"{m}.weight_scale"]
        x = tensors[f"{m}.weight"]
        assert not q.is_cuda and q.dtype == (F8 if kind == "fp8" else torch.int8) and scale.dtype == x.dtype and scale.shape == (x.shape[0], 1)
        rtn = comp.compress_rtn(x.to(dev), scheme)
        assert sorted(rtn) == ["weight", "weight_scale"] and same(q, rtn["weight"]) and same(scale, rtn["weight_scale"]), m
        assert same(q, golden[f"{key}.{kind}.q"]) and same(scale, golden[f"{key}.{kind}.scale"]), m
    for key, t in tensors.items():
        if not (key.endswith(".weight") and key[:-7] in SHARD_KEYS):
            assert out[key] is t, key  # the same object: the ignored lm_head, the embedding, the 1-D norms, the bias
    conv.stream_results = True
    streamed = conv.process(dict(tensors))
    assert streamed.ready
    streamed.wait()
    assert all(same(streamed[n], out[n]) for n in out)


@pytest.mark.parametrize("name,kind,fmt", [("FP8DynamicQuantizer", "fp8", "float-quantized"), ("W8A8Quantizer", "int8", "int-quantized")])
def test_convert_checkpoint_then_dequantize_gives_the_oracles_weights(cta, dev, ref, golden, tmp_path, name, kind, fmt):
    from safetensors.torch import load_file, save_file

    from compressed_tensors_amd.entrypoints.convert import CompressedTensorsDequantizer, convert_checkpoint

    tensors = _shard(bias=False)
    tensors["model.layers.0.mlp.down_proj.weight"] = C.make_weight(CASES["1x16392.bf16"])  # one dense dtype: the checkpoint's
    keys = dict(SHARD_KEYS, **{"model.layers.0.mlp.down_proj": "1x16392.bf16"})
    src, mid, dst = (tmp_path / n for n in ("dense", "q8", "back"))
    src.mkdir()
    save_file(tensors, str(src / "model.safetensors"))
    (src / "config.json").write_text(json.dumps({"model_type": "llama", "torch_dtype": "bfloat16"}))
    convert_checkpoint(str(src), str(mid), _converter(name)(targets=["re:.*proj$"], device=dev), max_workers=1)
    cfg = json.loads((mid / "config.json").read_text())["quantization_config"]
    assert cfg["quant_method"] == "compressed-tensors" and cfg["format"] == fmt and cfg["ignore"] == ["lm_head", "re:.*embed_tokens$"]
    assert cfg["quantization_status"] == "compressed"
    group = cfg["config_groups"]["config_group_0"]
    assert group["targets"] == ["re:.*proj$"] and group["format"] == fmt
    assert group["weights"]["strategy"] == "channel" and group["weights"]["type"] == C.KINDS[kind]["type"] and group["weights"]["num_bits"] == 8
    assert group["weights"]["symmetric"] is True and group["weights"]["dynamic"] is False
    assert group["input_activations"]["strategy"] == "token" and group["input_activations"]["dynamic"] is True
    stored = load_file(str(mid / "model.safetensors"))
    for m, key in keys.items():
        assert same(stored[f"{m}.weight"], golden[f"{key}.{kind}.q"]) and same(stored[f"{m}.weight_scale"], golden[f"{key}.{kind}.scale"]), m
        assert f"{m}.weight_zero_point" not in stored
    assert same(stored["lm_head.weight"], tensors["lm_head.weight"])
    convert_checkpoint(str(mid), str(dst), CompressedTensorsDequantizer(str(mid), dtype=BF16, device=dev), max_workers=1)
    back = load_file(str(dst / "model.safetensors"))
    a = C.KINDS[kind]
    for m, key in keys.items():
        x, o = ref[key][0], ref[key][1][kind]
        zp = o.get("zero_point", torch.zeros(o["scale"].shape, dtype=F8))
        fq = O.fake_quantize(x, o["scale"], zp, num_bits=8, strategy="channel", qtype=a["type"])
        assert back[f"{m}.weight"].dtype == BF16 and torch.equal(back[f"{m}.weight"], fq.to(BF16)), m  # values: fake_quantize may carry -0.0
        assert same(back[f"{m}.weight"], O.dequantize(o["q"], o["scale"], o.get("zero_point"), strategy="channel").to(BF16)), m
    assert set(back) == set(tensors) and same(back["model.norm.weight"], tensors["model.norm.weight"])
