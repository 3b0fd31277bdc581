"""`ct_fp8block_mxfp4_batch`, `codec.fp8block_to_mxfp4`, FP8BlockToMXFP4Converter and MXFP4Quantizer on the GPU: every comparison is byte for byte, on
`weight_packed` and `weight_scale`, against tests/golden/fp8block_mxfp4.* (the reference's FP8BlockDequantizer + MXFP4 compress on the CPU,
tools/gen_golden_fp8block_mxfp4.py) or between the fused launch and the composition.  Shapes: tests/_fp8block_mxfp4_cases.py."""
import json

import pytest
import torch

import _fp8block_mxfp4_cases as C

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
TARGETS = ["re:.*proj(_with_mqa)?$"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _transcode(key, dtype):
    from compressed_tensors_amd import codec

    w, s = C.inputs(key)
    return codec.fp8block_to_mxfp4(w, s, weight_block_size=tuple(C.CASES[key]["block"]), dtype=C.DTYPES[dtype])


SHAPE_KEYS = ["r1x32", "r3x32", "sq128", "r200x320", "r130x160_b128x64", "r96x96_b64x32", "sq256_b1x128", "r1x8192", "g511_r73x224", "g513_r27x608"]
SCALE_KEYS = ["r200x320_b64_bf16", "r200x320_b64_f16", "r200x320_b64_bcast11", "r200x320_b64_bcast_row", "r200x320_b64_bcast_col"]
SWEEP_KEYS = ["allcodes_b1x256", "allcodes_b1x32"]


@pytest.mark.parametrize("dtype", C.DENSE_DTYPES)
@pytest.mark.parametrize("key", SHAPE_KEYS + SCALE_KEYS + SWEEP_KEYS)
def test_single_tensor_matches_the_golden(dev, key, dtype):
    """the shapes (an item inside a wave, ragged block rows and columns, the narrowest block width, one group less / more than a workgroup's 512),
    the scale dtypes and broadcasts, and the all-codes sweep (the sign of a zero product, NaN codes, the inf scale's byte)"""
    packed, e8m0 = _transcode(key, dtype)
    assert packed.device.type == "cpu" and e8m0.device.type == "cpu"  # host tensors in, host tensors out
    C.assert_golden(f"{key}.{dtype}", packed, e8m0)


def test_device_tensors_stay_on_the_device(dev):
    from compressed_tensors_amd import codec

    w, s = C.inputs("r200x320")
    packed, e8m0 = codec.fp8block_to_mxfp4(w.to(dev), s.to(dev))
    assert packed.device == dev and e8m0.device == dev
    C.assert_golden("r200x320.bfloat16", packed, e8m0)


def _mixed_shard():
    names = {"mixed.down_proj": "model.layers.2.mlp.down_proj", "mixed.q_proj": "model.layers.2.self_attn.q_proj",
             "mixed.kv_b_proj": "model.layers.2.self_attn.kv_b_proj", "mixed.o_proj": "model.layers.2.self_attn.o_proj"}
    shard = {}
    for key, m in names.items():
        shard[f"{m}.weight"], shard[f"{m}.weight_scale_inv"] = C.inputs(key)
    return shard, {m: key for key, m in names.items()}


@pytest.mark.parametrize("dtype", C.DENSE_DTYPES)
def test_one_table_of_mixed_modules_takes_one_launch(dev, monkeypatch, dtype):
    from compressed_tensors_amd import _lib, codec
    from compressed_tensors_amd.entrypoints.convert import FP8BlockToMXFP4Converter

    shard, keys = _mixed_shard()
    assert len({shard[f"{m}.weight_scale_inv"].dtype for m in keys}) == 3  # a scale dtype per item
    lib = _lib.load()
    calls, others = [], []
    real = lib.ct_fp8block_mxfp4_batch
    monkeypatch.setattr(lib, "ct_fp8block_mxfp4_batch", lambda *a: calls.append(a[1]) or real(*a))
    monkeypatch.setattr(lib, "ct_fp8block_dequant_batch", lambda *a: others.append(a[1]) or 0)
    out = FP8BlockToMXFP4Converter(targets=TARGETS, dtype=C.DTYPES[dtype], device=dev, fused=True).process(dict(shard))
    assert calls == [4] and others == []
    monkeypatch.undo()
    for m, key in keys.items():
        C.assert_golden(f"{key}.{dtype}", out[f"{m}.weight_packed"], out[f"{m}.weight_scale"])
        one = codec.fp8block_to_mxfp4(shard[f"{m}.weight"], shard[f"{m}.weight_scale_inv"], dtype=C.DTYPES[dtype])
        assert torch.equal(one[0], out[f"{m}.weight_packed"]) and torch.equal(one[1], out[f"{m}.weight_scale"]), m


@pytest.mark.parametrize("fused", [True, False])
def test_both_paths_of_the_converter_match_the_golden_on_the_mixed_shard(dev, monkeypatch, fused):
    from compressed_tensors_amd import _lib
    from compressed_tensors_amd.entrypoints.convert import FP8BlockToMXFP4Converter

    shard, keys = _mixed_shard()
    shard["model.norm.weight"] = torch.ones(32, dtype=BF16)
    lib = _lib.load()
    launches = []
    for symbol in ("ct_fp8block_mxfp4_batch", "ct_fp8block_dequant_batch", "ct_rtn_mxfp4_quant_pack_batch"):
        real = getattr(lib, symbol)
        monkeypatch.setattr(lib, symbol, lambda *a, real=real, symbol=symbol: launches.append(symbol) or real(*a))
    conv = FP8BlockToMXFP4Converter(targets=TARGETS, device=dev, fused=fused)
    out = conv.process(dict(shard))
    assert launches == (["ct_fp8block_mxfp4_batch"] if fused else ["ct_fp8block_dequant_batch", "ct_rtn_mxfp4_quant_pack_batch"])
    want = []
    for name in shard:
        m, _, p = name.rpartition(".")
        want += [f"{m}.weight_packed", f"{m}.weight_scale"] if (m in keys and p == "weight") else [] if m in keys else [name]
    assert list(out) == want and not out.ready and not out.keep  # `weight_packed` where the weight was, `weight_scale` behind it; settled
    assert out["model.norm.weight"] is shard["model.norm.weight"]
    for m, key in keys.items():
        assert not out[f"{m}.weight_packed"].is_cuda
        C.assert_golden(f"{key}.bfloat16", out[f"{m}.weight_packed"], out[f"{m}.weight_scale"])
    conv.stream_results = True
    streamed = conv.process(dict(shard))
    assert streamed.ready
    streamed.wait()
    assert all(torch.equal(streamed[n], out[n]) for n in out)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_fused_equals_the_composition_on_random_data(dev, dtype):
    from compressed_tensors_amd.entrypoints.convert import FP8BlockToMXFP4Converter

    gen = torch.Generator(device=dev).manual_seed(7)
    w = torch.randint(0, 256, (1024, 2048), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8).view(C.F8)
    s = torch.rand(8, 16, generator=gen, device=dev) * 0.02 + 1e-4
    shard = {"m.q_proj.weight": w, "m.q_proj.weight_scale_inv": s}
    got = [FP8BlockToMXFP4Converter(targets=TARGETS, dtype=dtype, device=dev, fused=f).process(dict(shard)) for f in (True, False)]
    for name in ("m.q_proj.weight_packed", "m.q_proj.weight_scale"):
        assert got[0][name].shape[0] == 1024 and torch.equal(got[0][name], got[1][name]), name


def test_rows_the_plan_would_refuse_take_the_composition(dev, monkeypatch):
    from compressed_tensors_amd import _lib
    from compressed_tensors_amd.entrypoints.convert import FP8BlockToMXFP4Converter

    lib = _lib.load()
    fused_rows = []
    real = lib.ct_fp8block_mxfp4_batch
    monkeypatch.setattr(lib, "ct_fp8block_mxfp4_batch", lambda *a: fused_rows.append(a[1]) or real(*a))
    # a block width that is no multiple of 32
    w, s = C.inputs("refused_b96x80")
    out = FP8BlockToMXFP4Converter(targets=TARGETS, weight_block_size=(96, 80), device=dev, fused=True).process({"m.o_proj.weight": w, "m.o_proj.weight_scale_inv": s})
    assert fused_rows == []
    C.assert_golden("refused_b96x80.bfloat16", out["m.o_proj.weight_packed"], out["m.o_proj.weight_scale"])
    # a device-resident weight that starts 8 bytes into its storage, beside one the plan admits
    w, s = C.inputs("r200x320")
    store = torch.empty(w.numel() + 8, dtype=torch.uint8, device=dev)
    view = store[8:].view(C.F8).view(w.shape)
    view.copy_(w.to(dev))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    w2, s2 = C.inputs("sq128")
    shard = {"a.q_proj.weight": view, "a.q_proj.weight_scale_inv": s.to(dev), "b.q_proj.weight": w2, "b.q_proj.weight_scale_inv": s2}
    out = FP8BlockToMXFP4Converter(targets=TARGETS, device=dev, fused=True).process(shard)
    assert fused_rows == [1]
    C.assert_golden("r200x320.bfloat16", out["a.q_proj.weight_packed"], out["a.q_proj.weight_scale"])
    C.assert_golden("sq128.bfloat16", out["b.q_proj.weight_packed"], out["b.q_proj.weight_scale"])


def test_the_kv_a_shape_matches_its_sha256(dev):
    C.assert_golden("kv_a_576x7168.bfloat16", *_transcode("kv_a_576x7168", "bfloat16"))


# ------------------------------------------------------------------------------------------------------------------- checkpoints
def _oracle():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(C.GOLDEN)), "oracle"))
    import oracle as O

    return O


def _decompressed(packed, e8m0):
    return _oracle().fp4_decompress({"weight_packed": packed, "weight_scale": e8m0}, fmt="mxfp4-pack-quantized")["weight"]


@pytest.mark.parametrize("activations", [False, True])
def test_convert_checkpoint_on_two_shards_and_back(dev, tmp_path, activations):
    from safetensors.torch import load_file, safe_open, save_file

    from compressed_tensors_amd.entrypoints.convert import CompressedTensorsDequantizer, FP8BlockToMXFP4Converter, convert_checkpoint

    shard, keys = _mixed_shard()
    mods = list(keys)
    extra = {"lm_head.weight": C.synth_codes(16, 256, 77), "lm_head.weight_scale_inv": C.synth_scales(1, 2, 77, torch.float32),
             "model.norm.weight": torch.full((256,), 0.5, dtype=BF16), "model.embed_tokens.weight": C.synth_dense(16, 256, 5, BF16)}
    s1, s2 = "model-00001-of-00002.safetensors", "model-00002-of-00002.safetensors"
    files = {s1: {}, s2: {}}
    for name, t in shard.items():
        m, _, p = name.rpartition(".")
        home = s1 if mods.index(m) < 2 else s2
        # the weight_scale_inv of the second module lives in the other shard
        files[s2 if (m == mods[1] and p == "weight_scale_inv") else home][name] = t
    files[s1].update({k: v for k, v in extra.items() if k.startswith("model.")})
    files[s2].update({k: v for k, v in extra.items() if k.startswith("lm_head")})
    src, mid, dst = (tmp_path / n for n in ("fp8", "mxfp4", "dense"))
    src.mkdir()
    for fn, t in files.items():
        save_file(t, str(src / fn))
    weight_map = {k: fn for fn, t in files.items() for k in t}
    (src / "model.safetensors.index.json").write_text(json.dumps({"metadata": {"total_size": 0}, "weight_map": weight_map}))
    qcfg = {"quant_method": "fp8", "fmt": "e4m3", "activation_scheme": "dynamic", "weight_block_size": [128, 128]}
    (src / "config.json").write_text(json.dumps({"architectures": ["Toy"], "quantization_config": qcfg}))

    conv = FP8BlockToMXFP4Converter(ignore=["re:lm_head.*"], targets=TARGETS, activations=activations, device=dev, fused=True)
    convert_checkpoint(str(src), str(mid), conv, max_workers=2)
    out, order = {}, {}
    for fn in files:
        out.update(load_file(str(mid / fn)))
        with safe_open(str(mid / fn), "pt") as f:
            # the writer stores a shard's tensors by sorted name (safetensors_io.write_safetensors), so a file's own order says nothing about the
            # converter: the order `process` hands over is asserted in test_both_paths_of_the_converter_match_the_golden_on_the_mixed_shard; here
            # the file must hold its keys in that sorted order, `weight_packed` in front of `weight_scale` for every module
            assert list(f.keys()) == sorted(f.keys()), fn
            order[fn] = set(f.keys())
    # every targeted weight became its two entries in the shard of the weight, its weight_scale_inv is gone; the ignored module keeps its own
    want = {k for k in weight_map if not (k.endswith("_scale_inv") and k[: -len(".weight_scale_inv")] in mods) and k[: -len(".weight")] not in mods}
    want |= {f"{m}.{p}" for m in mods for p in ("weight_packed", "weight_scale")}
    assert set(out) == want
    for m in mods:
        assert {f"{m}.weight_packed", f"{m}.weight_scale"} <= order[weight_map[f"{m}.weight"]], m
        C.assert_golden(f"{keys[m]}.bfloat16", out[f"{m}.weight_packed"], out[f"{m}.weight_scale"])
    for k, v in extra.items():
        assert torch.equal(out[k].view(torch.uint8), v.view(torch.uint8)), k
    index = json.loads((mid / "model.safetensors.index.json").read_text())
    assert set(index["weight_map"]) == set(out) and all(index["weight_map"][k] == fn for fn in files for k in order[fn])
    assert index["metadata"]["total_size"] == sum(t.numel() * t.element_size() for t in out.values())
    cfg = json.loads((mid / "config.json").read_text())
    preset = C.load_fixture()[1]["presets"]["MXFP4" if activations else "MXFP4A16"]
    group = cfg["quantization_config"]["config_groups"]["config_group_0"]
    written = {k: v for k, v in cfg["quantization_config"].items() if k != "version"}  # (the writer stamps the package's version beside the config)
    assert written == conv.create_config().model_dump() and cfg["architectures"] == ["Toy"]
    assert group["weights"] == preset["weights"] and group["input_activations"] == preset["input_activations"] and group["format"] == "mxfp4-pack-quantized"

    # and back: CompressedTensorsDequantizer reads the result; its weights are the oracle's MXFP4 decompress of the golden bytes
    convert_checkpoint(str(mid), str(dst), CompressedTensorsDequantizer(str(mid), dtype=BF16, device=dev), max_workers=1)
    back = {}
    for fn in files:
        back.update(load_file(str(dst / fn)))
    for m in mods:
        want_w = _decompressed(out[f"{m}.weight_packed"], out[f"{m}.weight_scale"])  # (equal to the golden bytes: asserted above)
        assert back[f"{m}.weight"].dtype == BF16 and torch.equal(back[f"{m}.weight"].view(torch.int16), want_w.view(torch.int16)), m
    assert set(back) == {k for k in weight_map if not k.endswith("_scale_inv") or k.startswith("lm_head")}


@pytest.mark.parametrize("dtype", C.DENSE_DTYPES)
def test_mxfp4_quantizer_matches_the_reference_and_round_trips(dev, tmp_path, dtype):
    from safetensors.torch import load_file, save_file

    from compressed_tensors_amd.entrypoints.convert import CompressedTensorsDequantizer, MXFP4Quantizer, convert_checkpoint

    mods = {f"model.layers.0.mlp.{n}": n for n in C.QUANTIZER_SHAPES}
    tensors = {f"{m}.weight": C.dense_inputs(n, dtype) for m, n in mods.items()}
    tensors["model.norm.weight"] = torch.ones(32, dtype=C.DTYPES[dtype])
    tensors["lm_head.weight"] = C.dense_inputs("o_proj", dtype)
    conv = MXFP4Quantizer(targets=TARGETS, device=dev)
    conv.validate(dict.fromkeys(tensors))
    out = conv.process(dict(tensors))
    want = []
    for name in tensors:
        want += [name[:-7] + ".weight_packed", name[:-7] + ".weight_scale"] if name[:-7] in mods else [name]
    assert list(out) == want and out["lm_head.weight"] is tensors["lm_head.weight"]
    for m, n in mods.items():
        C.assert_golden(f"quantizer.{n}.{dtype}", out[f"{m}.weight_packed"], out[f"{m}.weight_scale"])
    with pytest.raises(ValueError, match="tensor column shape must be divisble by the given group_size 32 but got 300"):
        conv.process({"m.q_proj.weight": torch.zeros(8, 300, dtype=C.DTYPES[dtype])})

    src, mid, dst = (tmp_path / n for n in ("dense", "mxfp4", "back"))
    src.mkdir()
    save_file(tensors, str(src / "model.safetensors"))
    (src / "config.json").write_text(json.dumps({"model_type": "llama"}))
    convert_checkpoint(str(src), str(mid), conv, max_workers=1)
    stored = load_file(str(mid / "model.safetensors"))
    assert all(torch.equal(stored[k], out[k]) for k in out if k.endswith(("weight_packed", "weight_scale")))
    convert_checkpoint(str(mid), str(dst), CompressedTensorsDequantizer(str(mid), dtype=BF16, device=dev), max_workers=1)
    back = load_file(str(dst / "model.safetensors"))
    assert set(back) == set(tensors)
    for m in mods:
        want_w = _decompressed(out[f"{m}.weight_packed"], out[f"{m}.weight_scale"])
        assert torch.equal(back[f"{m}.weight"].view(torch.int16), want_w.view(torch.int16)), m
