"""`ct_fp8block_mxfp8_batch`, `ct_fp8block_nvfp4_amax_batch` / `ct_fp8block_nvfp4_batch`, `codec.fp8block_to_mxfp8` / `fp8block_to_nvfp4` and the two
converters on the GPU.  Every comparison is of every byte, against tests/golden/fp8block_transcode.* (the reference's FP8BlockDequantizer + MXFP8 / NVFP4
compress on the CPU, tools/gen_golden_fp8block_transcode.py) or between the fused launch(es) and the composition; against the fixture the two NaN codes
of a float8 output count as one NaN (`C.canonical`), between the two GPU paths nothing is set aside.  Shapes:
tests/_fp8block_transcode_cases.py."""
import json

import pytest
import torch

import _fp8block_transcode_cases as C

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
TARGETS = ["re:.*proj(_with_mqa)?$"]
FUSED = {"mxfp8": ["ct_fp8block_mxfp8_batch"], "nvfp4": ["ct_fp8block_nvfp4_amax_batch", "ct_fp8block_nvfp4_batch"]}
COMPOSED = {"mxfp8": ["ct_fp8block_dequant_batch", "ct_rtn_quant_group8_batch"],
            "nvfp4": ["ct_fp8block_dequant_batch", "ct_rtn_nvfp4_amax_batch", "ct_rtn_nvfp4_quant_pack_batch"]}
PRESET = {("mxfp8", False): "MXFP8", ("mxfp8", True): "MXFP8", ("nvfp4", False): "NVFP4A16", ("nvfp4", True): "NVFP4"}
MIXED = {"mixed.down_proj": "model.layers.2.mlp.down_proj", "mixed.q_proj": "model.layers.2.self_attn.q_proj",
         "mixed.kv_b_proj": "model.layers.2.self_attn.kv_b_proj", "mixed.o_proj": "model.layers.2.self_attn.o_proj"}
BOTH = pytest.mark.parametrize("target", C.TARGETS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _cls(target):
    from compressed_tensors_amd.entrypoints import convert

    return {"mxfp8": convert.FP8BlockToMXFP8Converter, "nvfp4": convert.FP8BlockToNVFP4Converter}[target]


def _suffixes(target):
    return [suffix for _, suffix in C.OUTPUTS[target]]


def _entries(target, out, m):
    return [out[f"{m}.{suffix}"] for suffix in _suffixes(target)]


def _transcode(target, key, dtype):
    from compressed_tensors_amd import codec

    w, s = C.inputs(key)
    return getattr(codec, f"fp8block_to_{target}")(w, s, weight_block_size=tuple(C.CASES[key]["block"]), dtype=C.DTYPES[dtype])


def _single_cases():
    return [(t, k) for t in C.TARGETS for k in C.cases_of(t) if not k.startswith("mixed.") and k != "kv_a_576x7168"]


@pytest.mark.parametrize("dtype", C.DENSE_DTYPES)
@pytest.mark.parametrize("target, key", _single_cases())
def test_single_tensor_matches_the_golden(dev, target, key, dtype):
    """the shapes (an item inside a wave, ragged block rows and columns, the narrowest block widths, one group fewer / more than a workgroup's share,
    for NVFP4 an odd number of groups per row and per block), the scale dtypes and broadcasts, the block each plan refuses, and the all-codes sweeps
    (the sign of a zero product, NaN codes, inf scales); NVFP4's comparison includes the global scale"""
    got = _transcode(target, key, dtype)
    assert all(t.device.type == "cpu" for t in got)  # host tensors in, host tensors out
    C.assert_golden(target, key, dtype, got)


@BOTH
def test_device_tensors_stay_on_the_device(dev, target):
    from compressed_tensors_amd import codec

    w, s = C.inputs("r200x320")
    got = getattr(codec, f"fp8block_to_{target}")(w.to(dev), s.to(dev))
    assert all(t.device == dev for t in got)
    assert len({t.untyped_storage().data_ptr() for t in got}) == len(got)  # tensors of their own
    C.assert_golden(target, "r200x320", "bfloat16", got)


def _mixed_shard():
    shard = {}
    for key, m in MIXED.items():
        shard[f"{m}.weight"], shard[f"{m}.weight_scale_inv"] = C.inputs(key)
    return shard, {m: key for key, m in MIXED.items()}


def _count(monkeypatch, lib, symbols, log, run=True):
    for symbol in symbols:
        real = getattr(lib, symbol)
        monkeypatch.setattr(lib, symbol, lambda *a, real=real, symbol=symbol: log.append((symbol, a[1])) or (real(*a) if run else 0))


@pytest.mark.parametrize("dtype", C.DENSE_DTYPES)
@BOTH
def test_one_table_of_mixed_modules_takes_the_fused_launches_alone(dev, monkeypatch, target, dtype):
    from compressed_tensors_amd import _lib, codec

    shard, keys = _mixed_shard()
    assert len({shard[f"{m}.weight_scale_inv"].dtype for m in keys}) == 3  # a scale dtype per item
    lib = _lib.load()
    calls, others = [], []
    _count(monkeypatch, lib, FUSED[target], calls)
    _count(monkeypatch, lib, ["ct_fp8block_dequant_batch"], others, run=False)
    out = _cls(target)(targets=TARGETS, dtype=C.DTYPES[dtype], device=dev, fused=True).process(dict(shard))
    assert calls == [(symbol, 4) for symbol in FUSED[target]] and others == []  # one call each, of 4 items; no dequantize launch
    monkeypatch.undo()
    for m, key in keys.items():
        got = _entries(target, out, m)
        C.assert_golden(target, key, dtype, got)
        one = getattr(codec, f"fp8block_to_{target}")(shard[f"{m}.weight"], shard[f"{m}.weight_scale_inv"], dtype=C.DTYPES[dtype])
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(one, got)), m


@pytest.mark.parametrize("fused", [True, False])
@BOTH
def test_both_paths_of_the_converter_match_the_golden_on_the_mixed_shard(dev, monkeypatch, target, fused):
    from compressed_tensors_amd import _lib

    shard, keys = _mixed_shard()
    shard["model.norm.weight"] = torch.ones(32, dtype=BF16)
    lib = _lib.load()
    launches = []
    _count(monkeypatch, lib, sorted(set(FUSED[target] + COMPOSED[target])), launches)
    conv = _cls(target)(targets=TARGETS, device=dev, fused=fused)
    out = conv.process(dict(shard))
    assert [symbol for symbol, _ in launches] == (FUSED[target] if fused else COMPOSED[target])
    want = []
    for name in shard:
        m, _, p = name.rpartition(".")
        want += [f"{m}.{suffix}" for suffix in _suffixes(target)] if (m in keys and p == "weight") else [] if m in keys else [name]
    assert list(out) == want and not out.ready and not out.keep  # the entries where the weight was, in the target's order; settled
    assert out["model.norm.weight"] is shard["model.norm.weight"]
    for m, key in keys.items():
        assert not any(t.is_cuda for t in _entries(target, out, m))
        C.assert_golden(target, key, "bfloat16", _entries(target, out, m))
    conv.stream_results = True
    streamed = conv.process(dict(shard))
    assert streamed.ready
    streamed.wait()
    assert all(torch.equal(streamed[n].view(torch.uint8), out[n].view(torch.uint8)) for n in out)


@pytest.mark.parametrize("dtype", [BF16, F16])
@BOTH
def test_fused_equals_the_composition_on_random_data(dev, target, dtype):
    """every byte value, NaN codes included, under random positive scales: what holds the NaN and inf behaviour of the fused launches to the
    composition's"""
    gen = torch.Generator(device=dev).manual_seed(7)
    w = torch.randint(0, 256, (1024, 2048), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8).view(C.F8)
    s = torch.rand(8, 16, generator=gen, device=dev) * 0.02 + 1e-4
    shard = {"m.q_proj.weight": w, "m.q_proj.weight_scale_inv": s}
    got = [_cls(target)(targets=TARGETS, dtype=dtype, device=dev, fused=f).process(dict(shard)) for f in (True, False)]
    for suffix in _suffixes(target):
        a, b = got[0][f"m.q_proj.{suffix}"], got[1][f"m.q_proj.{suffix}"]
        assert a.shape[0] in (1, 1024) and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), suffix


@BOTH
def test_rows_the_plan_would_refuse_take_the_composition(dev, monkeypatch, target):
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    fused_rows = []
    _count(monkeypatch, lib, FUSED[target][-1:], fused_rows)
    # a block width that is no multiple of the group ((96, 80) for MXFP8; the NVFP4 plan admits that one and refuses (96, 40))
    key = C.REFUSED[target]
    w, s = C.inputs(key)
    out = _cls(target)(targets=TARGETS, weight_block_size=C.CASES[key]["block"], device=dev, fused=True).process({"m.o_proj.weight": w, "m.o_proj.weight_scale_inv": s})
    assert fused_rows == []
    C.assert_golden(target, key, "bfloat16", _entries(target, out, "m.o_proj"))
    # a device-resident weight that starts 8 bytes into its storage, beside one the plan admits
    w, s = C.inputs("r200x320")
    store = torch.empty(w.numel() + 8, dtype=torch.uint8, device=dev)
    view = store[8:].view(C.F8).view(w.shape)
    view.copy_(w.to(dev))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    w2, s2 = C.inputs("sq128")
    shard = {"a.q_proj.weight": view, "a.q_proj.weight_scale_inv": s.to(dev), "b.q_proj.weight": w2, "b.q_proj.weight_scale_inv": s2}
    out = _cls(target)(targets=TARGETS, device=dev, fused=True).process(shard)
    assert [n for _, n in fused_rows] == [1]
    C.assert_golden(target, "r200x320", "bfloat16", _entries(target, out, "a.q_proj"))
    C.assert_golden(target, "sq128", "bfloat16", _entries(target, out, "b.q_proj"))


@BOTH
def test_the_kv_a_shape_matches_its_sha256(dev, target):
    C.assert_golden(target, "kv_a_576x7168", "bfloat16", _transcode(target, "kv_a_576x7168", "bfloat16"))


def test_the_mxfp4_converter_keeps_its_golden_bytes_through_the_shared_body(dev, monkeypatch):
    from compressed_tensors_amd import _lib
    from compressed_tensors_amd.entrypoints.convert import FP8BlockToMXFP4Converter

    shard, keys = _mixed_shard()
    lib = _lib.load()
    launches = []
    _count(monkeypatch, lib, ["ct_fp8block_mxfp4_batch", "ct_fp8block_dequant_batch", "ct_rtn_mxfp4_quant_pack_batch"], launches)
    for fused, want in ((True, [("ct_fp8block_mxfp4_batch", 4)]), (False, [("ct_fp8block_dequant_batch", 4), ("ct_rtn_mxfp4_quant_pack_batch", 4)])):
        del launches[:]
        out = FP8BlockToMXFP4Converter(targets=TARGETS, device=dev, fused=fused).process(dict(shard))
        assert launches == want
        for m, key in keys.items():
            C.M.assert_golden(f"{key}.bfloat16", out[f"{m}.weight_packed"], out[f"{m}.weight_scale"])


# ------------------------------------------------------------------------------------------------------------------- checkpoints
def _oracle():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(C.GOLDEN)), "oracle"))
    import oracle as O

    return O


def _decompressed(target, entries):
    """the oracle's decompress of a module's entries, as bfloat16"""
    O = _oracle()
    if target == "mxfp8":
        q, e8m0 = entries
        return O.dequantize(q, O.e8m0_decode(e8m0), None, strategy="group", group_size=32).to(BF16)
    packed, scale, gs = entries
    return O.fp4_decompress({"weight_packed": packed, "weight_scale": scale, "weight_global_scale": gs}, fmt="nvfp4-pack-quantized")["weight"].to(BF16)


def _bits(t):
    """bfloat16 bits with every NaN as one NaN"""
    return torch.where(torch.isnan(t), torch.full_like(t.view(torch.int16), 0x7FC0), t.view(torch.int16))


@pytest.mark.parametrize("activations", [False, True])
@BOTH
def test_convert_checkpoint_on_two_shards_and_back(dev, tmp_path, target, activations):
    from safetensors.torch import load_file, save_file

    from compressed_tensors_amd.entrypoints.convert import CompressedTensorsDequantizer, convert_checkpoint

    shard, keys = _mixed_shard()
    mods = list(keys)
    extra = {"lm_head.weight": C.synth_codes(16, 256, 77), "lm_head.weight_scale_inv": C.synth_scales(1, 2, 77, torch.float32),
             "model.norm.weight": torch.full((256,), 0.5, dtype=BF16)}
    s1, s2 = "model-00001-of-00002.safetensors", "model-00002-of-00002.safetensors"
    files = {s1: {}, s2: {}}
    for name, t in shard.items():
        m, _, p = name.rpartition(".")
        home = s1 if mods.index(m) < 2 else s2
        files[s2 if (m == mods[1] and p == "weight_scale_inv") else home][name] = t  # the weight_scale_inv of the second module lives in the other shard
    files[s1]["model.norm.weight"] = extra["model.norm.weight"]
    files[s2].update({k: v for k, v in extra.items() if k.startswith("lm_head")})
    src, mid, dst = (tmp_path / n for n in ("fp8", target, "dense"))
    src.mkdir()
    for fn, t in files.items():
        save_file(t, str(src / fn))
    weight_map = {k: fn for fn, t in files.items() for k in t}
    (src / "model.safetensors.index.json").write_text(json.dumps({"metadata": {"total_size": 0}, "weight_map": weight_map}))
    qcfg = {"quant_method": "fp8", "fmt": "e4m3", "activation_scheme": "dynamic", "weight_block_size": [128, 128]}
    (src / "config.json").write_text(json.dumps({"architectures": ["Toy"], "quantization_config": qcfg}))

    conv = _cls(target)(ignore=["re:lm_head.*"], targets=TARGETS, activations=activations, device=dev, fused=True)
    convert_checkpoint(str(src), str(mid), conv, max_workers=2)
    out, home = {}, {}
    for fn in files:
        got = load_file(str(mid / fn))
        out.update(got)
        home.update(dict.fromkeys(got, fn))
    # every targeted weight became its entries in the shard of the weight, its weight_scale_inv is gone; the ignored module keeps its own
    want = {k for k in weight_map if k.rpartition(".")[0] not in mods} | {f"{m}.{suffix}" for m in mods for suffix in _suffixes(target)}
    assert set(out) == want
    for m in mods:
        assert {home[f"{m}.{suffix}"] for suffix in _suffixes(target)} == {weight_map[f"{m}.weight"]}, m
        C.assert_golden(target, keys[m], "bfloat16", _entries(target, out, m))
    for k, v in extra.items():
        assert torch.equal(out[k].view(torch.uint8), v.view(torch.uint8)), k
    cfg = json.loads((mid / "config.json").read_text())
    preset = C.load_fixture()[1]["presets"][PRESET[target, activations]]
    group = cfg["quantization_config"]["config_groups"]["config_group_0"]
    written = {k: v for k, v in cfg["quantization_config"].items() if k != "version"}  # (the writer stamps the package's version beside the config)
    assert written == conv.create_config().model_dump() and cfg["architectures"] == ["Toy"]
    assert group["weights"] == preset["weights"] and group["input_activations"] == preset["input_activations"] and group["format"] == conv.format

    # and back: CompressedTensorsDequantizer reads the result; its weights are the oracle's decompress of the golden bytes
    convert_checkpoint(str(mid), str(dst), CompressedTensorsDequantizer(str(mid), dtype=BF16, device=dev), max_workers=1)
    back = {}
    for fn in files:
        back.update(load_file(str(dst / fn)))
    for m in mods:
        want_w = _decompressed(target, _entries(target, out, m))  # (equal to the golden bytes: asserted above)
        assert back[f"{m}.weight"].dtype == BF16 and torch.equal(_bits(back[f"{m}.weight"]), _bits(want_w)), m
    assert set(back) == {k for k in weight_map if not k.endswith("_scale_inv") or k.startswith("lm_head")}
