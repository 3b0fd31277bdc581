"""`ct_nvfp4_mxfp4_batch`, `codec.nvfp4_to_mxfp4` and NVFP4ToMXFP4Converter on the GPU: every comparison is byte for byte, on `weight_packed` and
`weight_scale`, against tests/golden/nvfp4_mxfp4.json (the reference's NVFP4 decompress + MXFP4 compress on the CPU, tools/gen_golden_nvfp4_mxfp4.py),
between the fused launch and the composition, or against a property that needs no recorded bytes.  Shapes: tests/_nvfp4_mxfp4_cases.py."""
import json

import pytest
import torch

import _nvfp4_mxfp4_cases as C

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
TARGETS = ["re:.*proj$"]
OUT = ("weight_packed", "weight_scale")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _shard(modules):
    """{module: (packed, scale, global scale)} -> a compressed-tensors NVFP4 shard"""
    shard = {}
    for m, (p, s, g) in modules.items():
        shard[f"{m}.weight_packed"], shard[f"{m}.weight_scale"], shard[f"{m}.weight_global_scale"] = p, s, g
    return shard


def _convert(modules, dev, fused):
    from compressed_tensors_amd.entrypoints.convert import NVFP4ToMXFP4Converter

    out = NVFP4ToMXFP4Converter(targets=TARGETS, device=dev, fused=fused).process(_shard(modules))
    assert list(out) == [f"{m}.{p}" for m in modules for p in OUT] and not out.ready and not out.keep
    return {m: (out[f"{m}.weight_packed"], out[f"{m}.weight_scale"]) for m in modules}


def _count(monkeypatch, lib, symbols, launches):
    for symbol in symbols:
        real = getattr(lib, symbol)
        monkeypatch.setattr(lib, symbol, lambda *a, real=real, symbol=symbol: launches.append((symbol, a[1])) or real(*a))


FUSED, DECOMPRESS, COMPRESS = "ct_nvfp4_mxfp4_batch", "ct_fp4_unpack_dequant_batch", "ct_rtn_mxfp4_quant_pack_batch"


# ------------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("key", C.SHAPE_KEYS)
def test_shape_cases_match_the_golden(dev, key, fused):
    """one group, an item inside a wave, rows that end inside a workgroup, one lane short of a workgroup's 1024 groups, exactly that, one more"""
    (packed, e8m0), = _convert({"m.q_proj": C.inputs(key)}, dev, fused).values()
    assert packed.device.type == "cpu" and e8m0.device.type == "cpu"  # host tensors in, host tensors out
    C.assert_golden(key, packed, e8m0)


@pytest.mark.parametrize("fused", [True, False])
def test_the_kv_a_shape_matches_its_sha256(dev, fused):
    C.assert_golden("kv_a_576x7168", *_convert({"m.q_proj": C.inputs("kv_a_576x7168")}, dev, fused)["m.q_proj"])


def test_the_codec_entry_matches_the_golden_and_device_tensors_stay_on_the_device(dev):
    from compressed_tensors_amd import codec

    p, s, g = C.inputs("r200x320")
    packed, e8m0 = codec.nvfp4_to_mxfp4(p, s, g)
    assert packed.device.type == "cpu" and e8m0.device.type == "cpu"
    C.assert_golden("r200x320", packed, e8m0)
    packed, e8m0 = codec.nvfp4_to_mxfp4(p.to(dev), s.to(dev), g.to(dev))
    assert packed.device == dev and e8m0.device == dev
    C.assert_golden("r200x320", packed, e8m0)
    packed, e8m0 = codec.nvfp4_to_mxfp4(p.to(dev), s.to(dev), g)  # a host global scale beside device tensors is staged
    assert packed.device == dev
    C.assert_golden("r200x320", packed, e8m0)


# ------------------------------------------------------------------------------------------------------------------- the scale domain
def test_fused_equals_the_composition_over_the_whole_scale_domain(dev, monkeypatch):
    """every scale byte (both NaN bytes included) in either half of an MX group, under finite, tiny, huge, zero, negative and infinite global scales:
    one table of 20 modules per path, each module under its own global scale"""
    from compressed_tensors_amd import _lib

    modules = {f"{layout}.{name}.q_proj": C.sweep_inputs(layout, name) for layout in C.SWEEP_LAYOUTS for name in C.SWEEP_SCALES}
    assert len(modules) == 20 and {0x7F, 0xFF} <= set(modules["first.1.q_proj"][1].view(torch.uint8)[:, 0].tolist())
    launches = []
    _count(monkeypatch, _lib.load(), (FUSED, DECOMPRESS, COMPRESS), launches)
    fused = _convert(modules, dev, True)
    assert launches == [(FUSED, 20)]
    launches.clear()
    composed = _convert(modules, dev, False)
    assert launches == [(DECOMPRESS, 20), (COMPRESS, 20)]
    for m in modules:
        for name, a, b in zip(OUT, fused[m], composed[m]):
            bad = (a != b).nonzero()
            assert bad.numel() == 0, (m, name, f"{bad.shape[0]} bytes differ, first at {bad[0].tolist()}: fused {int(a[tuple(bad[0])]):#x}, composed {int(b[tuple(bad[0])]):#x}")
    # the sweep is no sweep of one answer: the outputs differ between global scales
    assert len({C.sha(fused[f"first.{name}.q_proj"][1]) for name in C.SWEEP_SCALES}) >= 6


@pytest.mark.parametrize("fused", [True, False])
def test_the_finite_part_of_the_scale_domain_matches_the_golden(dev, fused):
    keys = {f"{layout}.{name}.q_proj": C.sweep_key(layout, name) for layout in C.SWEEP_LAYOUTS for name in C.GOLDEN_SCALES}
    got = _convert({m: C.sweep_inputs(*m.split(".")[:2], finite=True) for m in keys}, dev, fused)
    for m, key in keys.items():
        C.assert_golden(key, *got[m])


# ------------------------------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("fused", [True, False])
def test_power_of_two_scales_give_the_nibbles_back(dev, fused):
    """every scale byte a power of two 2^k (both NVFP4 groups of an MX group the same one), the global scale 1.0 and a +-6 code in every MX group: the
    dense values are code * 2^k, the group's amax is 6 * 2^k = 1.5 * 2^(k + 2), whose MX scale is 2^k — so the nibbles come back and the exponent
    byte is 127 + k.  No recorded bytes: this pins the order of nibbles and groups.  (The code 8, -0.0, is kept out: its dense value -0.0 quantizes
    to +0.0, the code 0.)"""
    rows, cols = 36, 96
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    g = torch.arange(cols // 32, dtype=torch.int64)[None, :]
    k = (r + 7 * g) % 18 - 9  # 2^-9 .. 2^8: the three subnormal powers of two of float8_e4m3fn and every normal one
    assert sorted(set(k.flatten().tolist())) == list(range(-9, 9))
    byte = torch.where(k < -6, 1 << (k + 9).clamp(min=0), (k + 7).clamp(min=0) << 3).to(torch.uint8)
    assert torch.equal(byte.view(C.F8).float(), 2.0 ** k.float())
    scale = byte.repeat_interleave(2, dim=1).view(C.F8)
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    codes = ((r * 7919 + c * 104729 + 5) * 2654435761 >> 11) % 16
    codes = torch.where(codes == 8, 0, codes)
    six = (c % 32) == ((r * 5 + (c // 32) * 11) % 32)  # one element of every MX group, at a hashed place
    codes = torch.where(six, torch.where((r + c // 32) % 2 == 0, 7, 15), codes).to(torch.uint8)
    packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
    out_packed, e8m0 = _convert({"m.q_proj": (packed, scale, C.global_scale(1.0))}, dev, fused)["m.q_proj"]
    assert torch.equal(out_packed, packed)
    assert torch.equal(e8m0.to(torch.int64), 127 + k)


# ------------------------------------------------------------------------------------------------------------------- tables
def _mixed_modules():
    names = {"mixed.down_proj": "model.layers.2.mlp.down_proj", "mixed.q_proj": "model.layers.2.self_attn.q_proj", "mixed.o_proj": "model.layers.2.self_attn.o_proj",
             "mixed.k_proj": "model.layers.2.self_attn.k_proj", "mixed.v_proj": "model.layers.2.self_attn.v_proj"}
    assert list(names) == C.MIXED_KEYS
    return {m: C.inputs(key) for key, m in names.items()}, {m: key for key, m in names.items()}


def test_one_table_of_mixed_modules_takes_one_launch(dev, monkeypatch):
    from compressed_tensors_amd import _lib, codec

    modules, keys = _mixed_modules()
    assert len({float(g) for _, _, g in modules.values()}) == len(modules)  # a global scale per item
    launches = []
    _count(monkeypatch, _lib.load(), (FUSED, DECOMPRESS, COMPRESS), launches)
    got = _convert(modules, dev, True)
    assert launches == [(FUSED, 5)]
    monkeypatch.undo()
    for m, key in keys.items():
        C.assert_golden(key, *got[m])
        one = codec.nvfp4_to_mxfp4(*modules[m])
        assert torch.equal(one[0], got[m][0]) and torch.equal(one[1], got[m][1]), m


@pytest.mark.parametrize("fused", [True, False])
def test_both_paths_of_the_converter_match_the_golden_on_the_mixed_shard(dev, monkeypatch, fused):
    from compressed_tensors_amd import _lib
    from compressed_tensors_amd.entrypoints.convert import NVFP4ToMXFP4Converter

    modules, keys = _mixed_modules()
    shard = _shard(modules)
    shard["model.norm.weight"] = torch.ones(32, dtype=BF16)
    shard["model.layers.2.self_attn.q_proj.input_global_scale"] = torch.tensor([3.0])
    launches = []
    _count(monkeypatch, _lib.load(), (FUSED, DECOMPRESS, COMPRESS), launches)
    conv = NVFP4ToMXFP4Converter(targets=TARGETS, device=dev, fused=fused)
    out = conv.process(dict(shard))
    assert [s for s, _ in launches] == ([FUSED] if fused else [DECOMPRESS, COMPRESS])
    assert list(out) == [f"{m}.{p}" for m in modules for p in OUT] + ["model.norm.weight"] and not out.ready and not out.keep
    assert out["model.norm.weight"] is shard["model.norm.weight"]
    for m, key in keys.items():
        assert not out[f"{m}.weight_packed"].is_cuda
        C.assert_golden(key, out[f"{m}.weight_packed"], out[f"{m}.weight_scale"])
    conv.stream_results = True
    streamed = conv.process(dict(shard))
    assert streamed.ready
    streamed.wait()
    assert all(torch.equal(streamed[n], out[n]) for n in out)


def test_rows_the_plan_would_refuse_take_the_composition(dev, monkeypatch):
    from compressed_tensors_amd import _lib
    from compressed_tensors_amd.entrypoints.convert import NVFP4ToMXFP4Converter

    launches = []
    _count(monkeypatch, _lib.load(), (FUSED, DECOMPRESS, COMPRESS), launches)
    # a device-resident weight_packed that starts 8 bytes into its storage, beside a module the plan admits
    p, s, g = C.inputs("r200x320")
    store = torch.empty(p.numel() + 8, dtype=torch.uint8, device=dev)
    view = store[8:].view(p.shape)
    view.copy_(p.to(dev))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    modules = {"a.q_proj": (view, s.to(dev), g.to(dev)), "b.q_proj": C.inputs("r27x1216")}
    out = NVFP4ToMXFP4Converter(targets=TARGETS, device=dev, fused=True).process(_shard(modules))
    assert launches == [(FUSED, 1), (DECOMPRESS, 1), (COMPRESS, 1)]
    C.assert_golden("r200x320", out["a.q_proj.weight_packed"], out["a.q_proj.weight_scale"])
    C.assert_golden("r27x1216", out["b.q_proj.weight_packed"], out["b.q_proj.weight_scale"])
    # a global scale that is not float32: the composition reads it as the float32 of its value (2688 is exact in bfloat16)
    launches.clear()
    p, s, g = C.inputs("r1x32")
    assert float(g) == 2688.0
    out = NVFP4ToMXFP4Converter(targets=TARGETS, device=dev, fused=True).process(_shard({"a.q_proj": (p, s, g.to(BF16))}))
    assert FUSED not in [s for s, _ in launches] and launches[-1] == (COMPRESS, 1)
    C.assert_golden("r1x32", out["a.q_proj.weight_packed"], out["a.q_proj.weight_scale"])


# ------------------------------------------------------------------------------------------------------------------- checkpoints
S1, S2 = "model-00001-of-00002.safetensors", "model-00002-of-00002.safetensors"
EXTRA = {"lm_head.weight": torch.full((16, 64), 0.25, dtype=BF16), "model.norm.weight": torch.full((64,), 0.5, dtype=BF16),
         "model.embed_tokens.weight": torch.arange(16 * 64, dtype=torch.float32).reshape(16, 64).to(BF16)}


def _write_source(root, source):
    """a two-shard NVFP4 checkpoint of the mixed modules in `source`'s names; the global scale of the second module lives in the other shard"""
    from safetensors.torch import save_file

    from compressed_tensors_amd.entrypoints.convert import ModelOptNvfp4Converter

    modules, _ = _mixed_modules()
    mods = list(modules)
    files = {S1: {}, S2: {}}
    for i, (m, (p, s, g)) in enumerate(modules.items()):
        home, other = (S1, S2) if i < 2 else (S2, S1)
        if source == "modelopt":
            entries = {"weight": p, "weight_scale": s, "weight_scale_2": 1 / g, "input_scale": torch.tensor([0.5 + i])}
            far = "weight_scale_2"
        else:
            entries = {"weight_packed": p, "weight_scale": s, "weight_global_scale": g}
            if i % 2 == 1:
                entries["input_global_scale"] = torch.tensor([2.0 + i])
            far = "weight_global_scale"
        for name, t in entries.items():
            files[other if (i == 1 and name == far) else home][f"{m}.{name}"] = t
    files[S1].update({k: v for k, v in EXTRA.items() if k.startswith("model.")})
    files[S2].update({k: v for k, v in EXTRA.items() if k.startswith("lm_head")})
    root.mkdir()
    for fn, t in files.items():
        save_file(t, str(root / fn))
    weight_map = {k: fn for fn, t in files.items() for k in t}
    (root / "model.safetensors.index.json").write_text(json.dumps({"metadata": {"total_size": 0}, "weight_map": weight_map}))
    qcfg = ({"quant_method": "modelopt", "quant_algo": "NVFP4"} if source == "modelopt"
            else ModelOptNvfp4Converter(ignore=["lm_head"], targets=TARGETS).create_config().model_dump())
    (root / "config.json").write_text(json.dumps({"architectures": ["Toy"], "quantization_config": qcfg}))
    return mods, weight_map


def _load(root):
    from safetensors.torch import load_file

    got = {}
    for fn in (S1, S2):
        got.update(load_file(str(root / fn)))
    return got


@pytest.fixture(scope="module")
def composed_checkpoints(dev, tmp_path_factory):
    """per source: the MXFP4 tensors the long road writes — (ModelOptNvfp4Converter,) CompressedTensorsDequantizer, MXFP4Quantizer — computed once"""
    from compressed_tensors_amd.entrypoints.convert import CompressedTensorsDequantizer, ModelOptNvfp4Converter, MXFP4Quantizer, convert_checkpoint

    got = {}
    for source in ("compressed-tensors", "modelopt"):
        root = tmp_path_factory.mktemp(source.replace("-", "_"))
        _write_source(root / "src", source)
        nv = root / "src"
        if source == "modelopt":
            nv = root / "nvfp4"
            convert_checkpoint(str(root / "src"), str(nv), ModelOptNvfp4Converter(ignore=["lm_head"], targets=TARGETS), max_workers=1)
        convert_checkpoint(str(nv), str(root / "dense"), CompressedTensorsDequantizer(str(nv), dtype=BF16, device=dev), max_workers=1)
        convert_checkpoint(str(root / "dense"), str(root / "mxfp4"), MXFP4Quantizer(ignore=["lm_head"], targets=TARGETS, device=dev), max_workers=1)
        got[source] = _load(root / "mxfp4")
    return got


@pytest.mark.parametrize("activations", [False, True])
@pytest.mark.parametrize("source", ["compressed-tensors", "modelopt"])
def test_convert_checkpoint_on_two_shards(dev, tmp_path, composed_checkpoints, source, activations):
    from compressed_tensors_amd.compressors.fp4.base import MXFP4PackedCompressor
    from compressed_tensors_amd.entrypoints.convert import NVFP4ToMXFP4Converter, convert_checkpoint

    mods, weight_map = _write_source(tmp_path / "src", source)
    conv = NVFP4ToMXFP4Converter(ignore=["lm_head"], targets=TARGETS, activations=activations, source=source, device=dev, fused=True)
    convert_checkpoint(str(tmp_path / "src"), str(tmp_path / "mxfp4"), conv, max_workers=2)
    out = _load(tmp_path / "mxfp4")
    # every targeted module became its two entries; the global scales (and ModelOpt's names) are gone; everything else is there
    assert set(out) == {f"{m}.{p}" for m in mods for p in OUT} | set(EXTRA)
    assert not [k for k in out if k.endswith(("global_scale", "weight_scale_2", "input_scale"))]
    primary = "weight" if source == "modelopt" else "weight_packed"
    index = json.loads((tmp_path / "mxfp4" / "model.safetensors.index.json").read_text())
    assert set(index["weight_map"]) == set(out) and all(index["weight_map"][f"{m}.{p}"] == weight_map[f"{m}.{primary}"] for m in mods for p in OUT)
    assert index["metadata"]["total_size"] == sum(t.numel() * t.element_size() for t in out.values())
    for k, v in EXTRA.items():
        assert out[k].dtype == v.dtype and torch.equal(out[k].view(torch.int16), v.view(torch.int16)), k
    cfg = json.loads((tmp_path / "mxfp4" / "config.json").read_text())
    preset = C.load_fixture()["presets"]["MXFP4" if activations else "MXFP4A16"]
    group = cfg["quantization_config"]["config_groups"]["config_group_0"]
    written = {k: v for k, v in cfg["quantization_config"].items() if k != "version"}  # (the writer stamps the package's version beside the config)
    assert written == conv.create_config().model_dump() and cfg["architectures"] == ["Toy"]
    assert group["weights"] == preset["weights"] and group["input_activations"] == preset["input_activations"] and group["format"] == "mxfp4-pack-quantized"
    # the same bytes as the long road, and so the same bfloat16 weights through the project's MXFP4 decompress
    want = composed_checkpoints[source]
    assert set(want) == set(out)
    for m in mods:
        got_w, want_w = (MXFP4PackedCompressor.decompress({p: sd[f"{m}.{p}"].to(dev) for p in OUT}, None)["weight"] for sd in (out, want))
        assert got_w.dtype == BF16 and tuple(got_w.shape) == (out[f"{m}.weight_packed"].shape[0], 2 * out[f"{m}.weight_packed"].shape[1])
        assert torch.equal(got_w.view(torch.int16), want_w.view(torch.int16)), m
        for p in OUT:
            assert torch.equal(out[f"{m}.{p}"], want[f"{m}.{p}"]), (m, p)
    if source == "compressed-tensors":  # the same global scales as the golden's: its bytes too
        _, keys = _mixed_modules()
        for m in mods:
            C.assert_golden(keys[m], out[f"{m}.weight_packed"], out[f"{m}.weight_scale"])
