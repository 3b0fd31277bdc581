"""Block-wise 8-bit round-to-nearest in one pass (ct_rtn_quant_block8 and its table form) and what stands on it — calculate_qparams_from_weight's
block branch, compress_rtn, compress_model_rtn on FP8_BLOCK modules, FP8BlockQuantizer — against the pinned oracle (the blocks as rows under its
channel-wise calculate_qparams, then its block quantize: tests/_block_rtn_cases.oracle_triple) and the reference's recorded results
(tests/golden/block_rtn.*).  Everything is compared on raw bits, without a tolerance.  Every test here needs an MI355X:  python -m pytest tests -m gpu"""
import json
import os

import pytest
import torch

import _block_rtn_cases as C
import oracle as O

pytestmark = pytest.mark.gpu

BF16, F16, F32, F8 = C.BF16, C.F16, C.F32, C.F8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
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
def ref():
    """key -> (weight, {kind: (scale, zero_point, q)}) of the oracle recipe, computed once and never written to"""
    out = {}
    for key, r in CASES.items():
        x = C.make_weight(r)
        out[key] = (x, {kind: C.oracle_triple(O, x, r["block"], kind) for kind in KINDS})
    return out


@pytest.fixture(scope="module")
def golden():
    from safetensors.torch import load_file

    return load_file(os.path.join(GOLDEN, "block_rtn.safetensors")), json.load(open(os.path.join(GOLDEN, "block_rtn_manifest.json")))["cases"]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def scheme_of(cta, kind, block):
    act = cta.QuantizationArgs(num_bits=8, type=C.KINDS[kind]["type"], strategy="group", group_size=128, symmetric=True, dynamic=True)
    return cta.QuantizationScheme(targets=["Linear"], weights=cta.QuantizationArgs(strategy="block", block_structure=list(block), **C.KINDS[kind]),
                                  input_activations=act)


def compressor_of(cta, kind):
    return cta.BaseCompressor.get_value_from_registry("float-quantized" if kind == "fp8" else "int-quantized")


def check_golden(golden, key, kind, scale, zp, q):
    """the reference's recorded results: sha256 of everything, and the tensors the fixture holds in full"""
    stored, manifest = golden
    for name, t in (("scale", scale), ("zero_point", zp), ("q", q)):
        m = manifest[key]["out"][f"{kind}.{name}"]
        assert (str(t.dtype).replace("torch.", ""), list(t.shape), C.sha(t.cpu())) == (m["dtype"], m["shape"], m["sha256"]), (key, kind, name)
        full = stored.get(f"{key}.{kind}.{name}")
        if full is not None:
            assert torch.equal(bits(full), bits(t.cpu())), (key, kind, name)


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", FAST_KEYS)
def test_one_pass_equals_oracle_and_golden(cta, dev, ref, golden, key, kind):
    """ct_rtn_quant_block8 == block min / max + calculate_qparams + quantize, and its observer form (no codes) gives the same qparams"""
    x, want = ref[key]
    block = CASES[key]["block"]
    a = C.KINDS[kind]
    q, scale, zp = cta.codec.rtn_quantize_block8(x.to(dev), block_structure=block, qtype=a["type"], symmetric=a["symmetric"])
    s_ref, z_ref, q_ref = want[kind]
    assert same(scale, s_ref), (key, kind, scale.cpu(), s_ref)
    assert same(zp, z_ref), (key, kind, zp.cpu(), z_ref)
    assert same(q, q_ref), (key, kind, int((bits(q.cpu()) != bits(q_ref)).sum()))
    check_golden(golden, key, kind, scale, zp, q)
    none, s_obs, z_obs = cta.codec.rtn_quantize_block8(x.to(dev), block_structure=block, qtype=a["type"], symmetric=a["symmetric"], codes=False)
    assert none is None and same(s_obs, scale) and same(z_obs, zp)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", FALLBACK_KEYS)
def test_compress_rtn_of_what_the_plan_refuses_equals_oracle_and_golden(cta, dev, ref, golden, key, kind):
    """ragged columns and float32 weights: compress_rtn composes the block observer with `compress` — the same bits"""
    x, want = ref[key]
    r = CASES[key]
    assert not cta.codec.rtn_block8_group(x.shape, r["block"]) or x.dtype == F32
    with pytest.raises(NotImplementedError):
        cta.codec.rtn_quantize_block8(x.to(dev), block_structure=r["block"], qtype=C.KINDS[kind]["type"], symmetric=C.KINDS[kind]["symmetric"])
    scheme = scheme_of(cta, kind, r["block"])
    got = compressor_of(cta, kind).compress_rtn(x.to(dev), scheme)
    s_ref, z_ref, q_ref = want[kind]
    assert set(got) == {"weight", "weight_scale"} | ({"weight_zero_point"} if kind == "int8_zp" else set())
    assert same(got["weight_scale"], s_ref) and same(got["weight"], q_ref), (key, kind)
    if kind == "int8_zp":
        assert same(got["weight_zero_point"], z_ref)
    check_golden(golden, key, kind, got["weight_scale"], got.get("weight_zero_point", z_ref), got["weight"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_table_of_all_fast_cases_equals_the_single_calls(cta, dev, ref, dtype, kind):
    """rtn_quantize_block8_many: ONE launch over every fast case of a block size (the 8-unit body serves blocks of 16 to 2048 units), plus a tensor
    the table refuses, equals the single calls"""
    a = C.KINDS[kind]
    for block in ([128, 128], [64, 64], [32, 128], [1, 128]):
        keys = [k for k in FAST_KEYS if CASES[k]["dtype"] == dtype and CASES[k]["block"] == block]
        xs = [ref[k][0].to(dev) for k in keys] + [torch.ones((block[0], block[1] + 8), dtype=C.DTYPES[dtype], device=dev)]
        calls, real = [], cta.codec.call
        try:
            cta.codec.call = lambda name, *args: calls.append(name) or real(name, *args)
            got = cta.codec.rtn_quantize_block8_many(xs[:-1], block_structure=block, qtype=a["type"], symmetric=a["symmetric"])
        finally:
            cta.codec.call = real
        assert calls == ["ct_rtn_quant_block8_batch"] and len(got) == len(keys)
        for k, t in zip(keys, got):
            for mine, want in zip(t, (ref[k][1][kind][2], ref[k][1][kind][0], ref[k][1][kind][1])):
                assert same(mine, want), (k, kind)
        with pytest.raises(NotImplementedError):  # the tensor no table takes goes to the single call, which names the reason
            cta.codec.rtn_quantize_block8_many(xs, block_structure=block, qtype=a["type"], symmetric=a["symmetric"])


@pytest.mark.parametrize("kind", KINDS)
def test_qparams_from_weight_plus_compress_equals_compress_rtn(cta, dev, ref, kind):
    """both paths of calculate_qparams_from_weight's block branch — the observer form of the kernel, and the blocks as rows under the channel-wise
    observer — return the oracle's bits, and `compress` on them is compress_rtn"""
    from compressed_tensors_amd.quantization.utils import _block_rows, block_one_pass, calculate_qparams_from_weight

    comp = compressor_of(cta, kind)
    for key in FAST_KEYS + FALLBACK_KEYS:
        x, want = ref[key]
        scheme = scheme_of(cta, kind, CASES[key]["block"])
        w = x.to(dev)
        assert block_one_pass(w, scheme.weights) == CASES[key]["fast"]
        scale, zp = calculate_qparams_from_weight(w, scheme.weights)
        assert same(scale, want[kind][0]) and same(zp, want[kind][1]), (key, kind)
        if CASES[key]["fast"]:  # the composition the fallback takes gives the kernel's bits on the weights the kernel takes, too
            rows, grid = _block_rows(w, CASES[key]["block"])
            s2 = (cta.codec.minmax_qparams_float(rows, kind="fp8") if kind == "fp8"
                  else cta.codec.minmax_qparams(rows, num_bits=8, symmetric=C.KINDS[kind]["symmetric"])[0]).reshape(grid)
            assert same(s2, scale), (key, kind)
        two = comp.compress({"weight": w, "weight_scale": scale, "weight_zero_point": zp}, scheme)
        one = comp.compress_rtn(w, scheme)
        assert set(one) == set(two) and all(same(one[k], two[k]) for k in one), (key, kind)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_a_planted_maximum_is_found_wherever_it_sits(cta, dev, dtype):
    """the block maximum at the block's first element, its last element, and in the last in-range row of a ragged block: one unit of one thread each"""
    base = (torch.arange(200 * 256, dtype=torch.float32).reshape(200, 256) % 13 - 6) / 64
    spots = [(0, 0), (127, 127), (127, 255), (0, 128), (128, 0), (199, 0), (199, 255), (199, 128)]  # the last three: row 71 of a block with 72 live rows
    for r, c in spots:
        x = base.clone()
        x[r, c] = -96.0
        x = x.to(dtype)
        q, scale, _ = cta.codec.rtn_quantize_block8(x.to(dev), block_structure=[128, 128])
        s_ref, _, q_ref = C.oracle_triple(O, x, [128, 128], "fp8")
        assert same(scale, s_ref) and same(q, q_ref), (r, c)
        assert float(scale[r // 128, c // 128]) == float(torch.tensor(96.0 / 448.0).to(dtype)) and int(bits(q.cpu())[r, c]) == 0xFE, (r, c)
        assert int((scale.cpu().float() > 0.1).sum()) == 1


# ---- modules --------------------------------------------------------------------------------------------------------------------------
TREE_KEYS = ("256x384.b128x128.bf16.planted", "128x128.b128x128.bf16", "256x256.b128x128.f32")


def _tree(cta, dev):
    """three FP8_BLOCK Linears of whole blocks (the strategy `decompress` infers from a scale's shape has no ragged blocks): 2 x 3 blocks with the
    planted ones and one block, both one pass, and a float32 weight, which the plan refuses (the composition); one bias"""
    scheme = scheme_of(cta, "fp8", [128, 128])
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


def test_compress_model_rtn_on_fp8_block_modules(cta, dev, ref, monkeypatch):
    """compress_model_rtn per module (batched=False), grouped (batched=True, the gate forced on) and the block-wise window driver leave identical
    modules — entry names, order, dtypes, bits —, the oracle's; decompress_model then gives the oracle's fake_quantize"""
    from compressed_tensors_amd.compressors.naive_quantized.base import FloatQuantizationCompressor, rtn_block8_windows

    loop, grouped, windows = _tree(cta, dev), _tree(cta, dev), _tree(cta, dev)
    bias = loop[1].bias.data.clone()
    cta.ModelCompressor().compress_model_rtn(loop, batched=False)
    monkeypatch.setattr(FloatQuantizationCompressor, "RTN_TABLE_MEASURED_FASTER", True)
    cta.ModelCompressor().compress_model_rtn(grouped, batched=True)
    monkeypatch.undo()
    calls, real = [], cta.codec.call
    monkeypatch.setattr(cta.codec, "call", lambda name, *a: calls.append((name, a[1])) or real(name, *a))
    for m in windows:
        m.quantization_scheme.format = "float-quantized"
    rtn_block8_windows(FloatQuantizationCompressor, list(windows))
    monkeypatch.undo()
    assert [c for c in calls if c[0].startswith("ct_rtn")] == [("ct_rtn_quant_block8_batch", 2)]  # one table of the two weights the plan takes
    keys = TREE_KEYS
    for k, key in enumerate(keys):
        s_ref, _, q_ref = ref[key][1]["fp8"]
        a = _entries(loop[k])
        for other in (grouped, windows):
            b = _entries(other[k])
            assert [e[:3] for e in a] == [e[:3] for e in b] and all(torch.equal(x[3], y[3]) for x, y in zip(a, b)), key
            assert str(getattr(other[k].quantization_status, "value", other[k].quantization_status)) == "compressed"
        names = [e[0] for e in a]
        assert sorted(names) == sorted(["weight", "weight_scale"] + (["bias"] if k == 1 else [])), names
        assert same(loop[k].weight.data, q_ref) and same(loop[k].weight_scale.data, s_ref), key
    assert torch.equal(loop[1].bias.data, bias)
    cta.ModelCompressor().decompress_model(loop)
    for k, key in enumerate(keys):
        x, want = ref[key]
        s_ref, z_ref, _ = want["fp8"]
        fq = O.fake_quantize(x, s_ref, z_ref, num_bits=8, strategy="block", block_structure=[128, 128], qtype="float")
        assert same(loop[k].weight.data, fq), key


# ---- the converter --------------------------------------------------------------------------------------------------------------------
def _shard(ragged: bool):
    """a dense shard: two targeted weights of whole blocks (bf16 and fp16: a table each) and, with `ragged`, one with ragged rows of blocks and one
    with ragged columns, which the plan refuses, and a bias; two norms, the ignored embedding and lm_head"""
    keys = {"model.layers.0.self_attn.q_proj": "256x384.b128x128.bf16.planted", "model.layers.0.mlp.down_proj": "128x128.b128x128.f16"}
    if ragged:
        keys.update({"model.layers.0.self_attn.k_proj": "200x256.b128x128.bf16", "model.layers.0.mlp.up_proj": "128x200.b128x128.f16"})
    t = {"model.embed_tokens.weight": torch.ones((32, 256), dtype=BF16)}
    for m, key in keys.items():
        t[f"{m}.weight"] = C.make_weight(CASES[key])
    if ragged:
        t["model.layers.0.self_attn.q_proj.bias"] = torch.arange(256, dtype=torch.float32).to(BF16)
    t["model.layers.0.input_layernorm.weight"] = torch.ones(256, dtype=BF16)
    t["model.norm.weight"] = torch.full((256,), 0.5, dtype=BF16)
    t["lm_head.weight"] = C.make_weight(CASES["128x128.b128x128.bf16"])
    return t, keys


def test_quantizer_process_on_a_small_shard(cta, dev, ref):
    from compressed_tensors_amd.entrypoints.convert import FP8BlockQuantizer

    tensors, keys = _shard(ragged=True)
    conv = FP8BlockQuantizer(device=dev)
    conv.validate({k: None for k in tensors})
    out = conv.process(dict(tensors))
    want = []
    for name in tensors:
        want.append(name)
        if name.endswith(".weight") and name[:-7] in keys:
            want.append(name + "_scale")
    assert list(out) == want and not out.ready and not out.keep  # the input's order, the scale behind its weight; settled
    for m, key in keys.items():
        s_ref, _, q_ref = ref[key][1]["fp8"]
        assert not out[f"{m}.weight"].is_cuda and same(out[f"{m}.weight"], q_ref) and same(out[f"{m}.weight_scale"], s_ref), m
    for name, t in tensors.items():
        if not (name.endswith(".weight") and name[:-7] in keys):
            assert out[name] is t, name  # the same object
    conv.stream_results = True
    streamed = conv.process(dict(tensors))
    assert streamed.ready
    streamed.wait()
    assert all(same(streamed[n], out[n]) for n in out)


def test_convert_checkpoint_then_dequantize_gives_the_oracles_weights(cta, dev, ref, tmp_path):
    from safetensors.torch import load_file, save_file

    from compressed_tensors_amd.entrypoints.convert import CompressedTensorsDequantizer, FP8BlockQuantizer, convert_checkpoint

    tensors, keys = _shard(ragged=False)
    src, mid, dst = (tmp_path / n for n in ("dense", "fp8block", "back"))
    src.mkdir()
    save_file(tensors, str(src / "model.safetensors"))
    (src / "config.json").write_text(json.dumps({"model_type": "llama", "torch_dtype": "bfloat16"}))
    convert_checkpoint(str(src), str(mid), FP8BlockQuantizer(targets=["re:.*proj$"], device=dev), max_workers=1)
    cfg = json.loads((mid / "config.json").read_text())["quantization_config"]
    assert cfg["quant_method"] == "compressed-tensors" and cfg["format"] == "float-quantized" and cfg["ignore"] == ["lm_head", "re:.*embed_tokens$"]
    assert cfg["config_groups"]["config_group_0"]["targets"] == ["re:.*proj$"]
    stored = load_file(str(mid / "model.safetensors"))
    for m, key in keys.items():
        s_ref, _, q_ref = ref[key][1]["fp8"]
        assert same(stored[f"{m}.weight"], q_ref) and same(stored[f"{m}.weight_scale"], s_ref), m
    assert same(stored["lm_head.weight"], tensors["lm_head.weight"])
    convert_checkpoint(str(mid), str(dst), CompressedTensorsDequantizer(str(mid), dtype=BF16, device=dev), max_workers=1)
    back = load_file(str(dst / "model.safetensors"))
    for m, key in keys.items():
        x, want = ref[key]
        s_ref, z_ref, q_ref = want["fp8"]
        dq = O.dequantize(q_ref, s_ref, None, strategy="block", block_structure=[128, 128]).to(BF16)
        assert same(back[f"{m}.weight"], dq), m
    assert set(back) == set(tensors) and same(back["model.norm.weight"], tensors["model.norm.weight"])
