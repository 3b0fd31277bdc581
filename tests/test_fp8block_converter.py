"""FP8BlockDequantizer (reference entrypoints/convert/converters/fp8block_dequantizer.py): FP8 block-quantized checkpoints to dense
weights through one `ct_fp8block_dequant_batch` launch per shard.  CPU tests: the converter's host logic, the C planner through
ctypes, and an eager restatement of the reference expression against the fixtures.  GPU tests: `process` against the reference's
outputs in tests/golden/fp8block.safetensors (tools/gen_golden_fp8block.py), one launch per shard, a DeepSeek-V3.2-layer-shaped
table against the restatement on the GPU and against the live reference, and convert_checkpoint end to end."""
import ctypes
import hashlib
import json
import os
import sys

import pytest
import torch
from safetensors.torch import load_file, save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from compressed_tensors_amd.entrypoints.convert import FP8BlockDequantizer, convert_checkpoint  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FP8 = torch.float8_e4m3fn


def _manifest():
    with open(os.path.join(GOLDEN, "fp8block_manifest.json")) as f:
        return json.load(f)


_BLOB = {}


def _case_tensors(name, side):
    if not _BLOB:
        _BLOB.update(load_file(os.path.join(GOLDEN, "fp8block.safetensors")))
    pre = f"{name}.{side}."
    return {k[len(pre):]: v for k, v in _BLOB.items() if k.startswith(pre)}


# the integer recipes of the large fixture cases (tools/gen_golden_fp8block.py)
def synth_codes(rows, cols, salt):
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    return ((r * 7919 + c * 104729 + salt * 13) * 2654435761 >> 13).remainder(256).to(torch.uint8).view(FP8)


def synth_scales(rows, cols, salt, dtype):
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    h = ((r * 31 + c * 17 + salt) * 2246822519 >> 7).remainder(1 << 23)
    e = (h >> 20).remainder(8) + 115
    bits = (e << 23) | (h & ((1 << 23) - 1))
    if dtype != F32:
        bits = bits & ~((1 << 13) - 1)
    return bits.to(torch.int32).view(F32).to(dtype)


def canonical_sha(t):
    t = t.cpu().clone()
    t[torch.isnan(t)] = float("nan")
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def case_inputs(case):
    """the input shard of a fixture case, in its original order: the stored tensors and the ones synthesised from their recipe"""
    t = dict(_case_tensors(case["name"], "in"))
    for m in case["synth"]:
        t[f"{m['name']}.weight"] = synth_codes(m["rows"], m["cols"], m["salt"])
        t[f"{m['name']}.weight_scale_inv"] = synth_scales(*m["scale_shape"], m["salt"], getattr(torch, m["scale_dtype"]))
    return {k: t[k] for k in case["in_order"]}


def assert_reference(case, name, got):
    """`got` against the reference's dequantized `name` of a fixture case: stored whole, or its canonical sha256 and NaN count"""
    rec = next((m for m in case["synth"] if f"{m['name']}.weight" == name), None)
    if rec is None:
        assert_same(got, _case_tensors(case["name"], "out")[name], (case["name"], name))
    else:
        assert got.dtype == getattr(torch, case["dtype"]) and tuple(got.shape) == (rec["rows"], rec["cols"]), (case["name"], name)
        assert canonical_sha(got) == rec["sha256"] and int(torch.isnan(got.float()).sum()) == rec["nan"], (case["name"], name)


def targeted(inp, name):
    return name.endswith(".weight") and f"{name}_scale_inv" in inp and not name.startswith("lm_head")


def restated(w, s, block, dtype):
    """the reference expression, eager torch, on the tensors' device: every element times the scale of its block (a 0-D / 1-D
    scale or a size-1 dimension broadcasts like torch), float32 arithmetic, one cast"""
    R, C = w.shape
    bh, bw = block
    s2 = s.reshape((1,) * (2 - s.dim()) + tuple(s.shape)).float().expand(-(-R // bh), -(-C // bw))
    full = s2.repeat_interleave(bh, 0)[:R].repeat_interleave(bw, 1)[:, :C]
    return (w.float() * full).to(dtype)


def assert_same(got, want, what):
    """bit-equal where the reference is a number, NaN where it is NaN (NaN payload and sign are not compared)"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    got, want = got.cpu(), want.cpu()
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), (what, int((gn != wn).sum()))
    iview = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}[got.dtype]
    g, w = got.masked_fill(gn, 0).view(iview), want.masked_fill(wn, 0).view(iview)
    bad = (g != w).nonzero()
    assert bad.numel() == 0, (what, bad[:4].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())


def _conv(case, **kw):
    return FP8BlockDequantizer(ignore=case["ignore"], targets=case["targets"], weight_block_size=tuple(case["block"]),
                               dtype=getattr(torch, case["dtype"]), **kw)


# ------------------------------------------------------------------------------------------------------------------- host logic
def test_constructor_defaults_and_errors():
    c = FP8BlockDequantizer()
    assert (c.ignore, c.targets, c.weight_block_size, c.dtype, c.device, c.param_names) == ((), (), (128, 128), BF16, None,
                                                                                             ["weight", "weight_scale_inv"])
    assert FP8BlockDequantizer(dtype=F32, device="cuda:1").device == torch.device("cuda", 1)
    assert FP8BlockDequantizer(weight_block_size=[96, 80]).weight_block_size == [96, 80]
    for dtype in (torch.float64, torch.int8, FP8):
        with pytest.raises(ValueError, match="dtype"):
            FP8BlockDequantizer(dtype=dtype)
    for block in ((128,), (0, 128), (128, -1), (128.0, 128), (True, 128), 128, (1, 2, 3), "ab"):
        with pytest.raises(ValueError, match="weight_block_size"):
            FP8BlockDequantizer(weight_block_size=block)
    with pytest.raises(TypeError):
        FP8BlockDequantizer((), (), (128, 128), BF16, "cuda:0")  # device is keyword-only


def test_dependencies():
    c = FP8BlockDequantizer(ignore=["re:.*mlp.gate$"], targets=["re:.*proj$", "re:.*mlp.gate$"])
    assert c.get_dependencies("model.layers.0.mlp.down_proj.weight") == {"model.layers.0.mlp.down_proj.weight_scale_inv"}
    assert c.get_dependencies("model.layers.0.mlp.down_proj.weight_scale_inv") == set()
    assert c.get_dependencies("model.layers.0.mlp.gate.weight") == set()
    assert c.get_dependencies("lm_head.weight") == set()
    assert FP8BlockDequantizer().get_dependencies("model.layers.0.mlp.down_proj.weight") == set()  # as the reference: no targets, no partners


def test_validate_on_meta_tensors_and_the_reference_messages():
    c = FP8BlockDequantizer(ignore=["re:lm_head.*"], targets=["re:.*proj$"])
    meta = lambda *s: torch.empty(*s, device="meta", dtype=FP8)  # noqa: E731
    ok = {"model.layers.0.mlp.down_proj.weight": meta(256, 256), "model.layers.0.mlp.down_proj.weight_scale_inv": torch.empty(2, 2, device="meta"),
          "lm_head.weight": meta(8, 8), "lm_head.weight_scale_inv": torch.empty(1, 1, device="meta"), "model.norm.weight": torch.empty(8, device="meta")}
    c.validate(ok)
    with pytest.raises(ValueError, match="Found weight without corresponding weight_scale_inv model.layers.0.mlp.down_proj.weight"):
        c.validate({"model.layers.0.mlp.down_proj.weight": meta(4, 4)})
    with pytest.raises(ValueError, match="Found weight_scale_inv without corresponding weight model.layers.0.mlp.down_proj.weight_scale_inv"):
        c.validate({"model.layers.0.mlp.down_proj.weight_scale_inv": meta(1, 1)})
    with pytest.raises(ValueError, match="Found unexpected non-targeted tensor model.embed.weight_scale_inv"):
        c.validate({"model.embed.weight": meta(4, 4), "model.embed.weight_scale_inv": meta(1, 1)})
    # the reference's quirk: a plain ignore entry names the module, not its scale tensor
    with pytest.raises(ValueError, match="non-targeted tensor lm_head.weight_scale_inv"):
        FP8BlockDequantizer(ignore=["lm_head"], targets=["re:.*proj$"]).validate({"lm_head.weight": None, "lm_head.weight_scale_inv": None})


def test_create_config_is_none():
    assert FP8BlockDequantizer().create_config() is None


def test_process_refuses_bad_weights_before_any_launch(monkeypatch):
    from compressed_tensors_amd import _lib

    monkeypatch.setattr(_lib, "require_device", lambda: pytest.fail("reached the device"))
    c = FP8BlockDequantizer(targets=["re:.*proj$"])
    s = torch.ones(1, 1)
    for w in (torch.zeros(4, 4, dtype=BF16), torch.zeros(4, 4, dtype=torch.float8_e5m2), torch.zeros(2, 4, 4, dtype=FP8), torch.zeros(16, dtype=FP8)):
        with pytest.raises(ValueError, match="m.q_proj.weight: expected a 2-D float8_e4m3fn"):
            c.process({"m.q_proj.weight": w, "m.q_proj.weight_scale_inv": s})
    with pytest.raises(ValueError, match="weight_scale_inv: expected a float32, bfloat16 or float16"):
        c.process({"m.q_proj.weight": torch.zeros(4, 4, dtype=FP8), "m.q_proj.weight_scale_inv": torch.ones(1, 1, dtype=torch.float64)})
    with pytest.raises(ValueError, match="without corresponding weight_scale_inv"):
        c.process({"m.q_proj.weight": torch.zeros(4, 4, dtype=FP8)})


def test_process_without_targets_in_the_shard_passes_everything_through():
    tensors = {"lm_head.weight": torch.ones(2, 2), "model.norm.weight": torch.ones(3)}
    out = FP8BlockDequantizer(targets=["re:.*proj$"]).process(dict(tensors))
    assert list(out) == list(tensors) and all(out[k] is tensors[k] for k in tensors)


def test_without_a_gpu_the_converter_raises(monkeypatch):
    """no GPU: the converter raises instead of dequantizing on the host"""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    t = {"m.q_proj.weight": torch.zeros(4, 4, dtype=FP8), "m.q_proj.weight_scale_inv": torch.ones(1, 1)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FP8BlockDequantizer(targets=["re:.*proj$"]).process(t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FP8BlockDequantizer()._create_dequantized_weight(t["m.q_proj.weight"], t["m.q_proj.weight_scale_inv"])


# ------------------------------------------------------------------------------------------------------------------- the C planner
def _item(rows, cols, block=(128, 128), scale_shape=None, sdt=None, base=0x100000):
    from compressed_tensors_amd import _lib

    it = _lib.Fp8BlockItem()
    it.w, it.scale, it.out = base, base + 0x1000, base + 0x2000
    it.rows, it.cols, it.block_h, it.block_w = rows, cols, block[0], block[1]
    it.scale_shape[0], it.scale_shape[1] = scale_shape or (-(-rows // max(block[0], 1)), -(-cols // max(block[1], 1)))
    it.sdt = _lib.F32 if sdt is None else sdt
    return it


def _plan(items):
    from compressed_tensors_amd import _lib

    table = (_lib.Fp8BlockItem * len(items))(*items)
    return int(_lib.load().ct_fp8block_dequant_plan(ctypes.cast(table, ctypes.c_void_p), len(items))), table


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    from compressed_tensors_amd import _lib

    return _lib


def test_plan_counts_workgroups_of_a_known_mixed_table(lib):
    assert ctypes.sizeof(lib.Fp8BlockItem) == 14 * 8 and lib.Fp8BlockItem.sdt.offset == 72 and lib.Fp8BlockItem.first_block.offset == 104
    # (rows, cols, block, scale shape): 1024 units of 16 codes of one row per workgroup
    shapes = [(576, 7168, (128, 128), None), (200, 300, (96, 80), None), (256, 256, (1, 128), (1, 2)), (7, 9, (128, 128), (1, 1)),
              (64, 256, (128, 8), None)]
    n, table = _plan([_item(r, c, b, s, base=0x100000 * (i + 1)) for i, (r, c, b, s) in enumerate(shapes)])
    expect, first = [], 0
    for r, c, b, s in shapes:
        expect.append((first, -(-c // 16)))
        first += -(-(r * -(-c // 16)) // 1024)
    assert n == first == 252 + 4 + 4 + 1 + 1
    assert [(t.first_block, t.units_per_row) for t in table] == expect
    # fast path: cols % 16 == 0 and block_w % 16 == 0 (and 16-byte aligned tensors)
    assert [t.fast for t in table] == [1, 0, 1, 0, 0]
    # scale strides in elements, 0 along a broadcast dimension
    assert [tuple(t.scale_stride) for t in table] == [(56, 1), (4, 1), (0, 1), (0, 0), (0, 1)]
    assert _plan([])[0] == 0
    misaligned = _item(256, 256)
    misaligned.w += 8
    assert _plan([misaligned])[0] == 4 and _plan([misaligned])[1][0].fast == 0


def test_plan_refuses_malformed_items_and_oversized_batches(lib):
    bad = {
        "NULL": _item(64, 64),
        "empty": _item(0, 64, scale_shape=(1, 1)),
        "block 0": _item(64, 64, (0, 128), scale_shape=(1, 1)),
        "block < 0": _item(64, 64, (128, -128), scale_shape=(1, 1)),
        "scale rows": _item(300, 64, scale_shape=(2, 1)),
        "scale cols": _item(64, 300, scale_shape=(1, 2)),
        "scale too big": _item(128, 128, scale_shape=(2, 2)),
        "scale zero": _item(128, 128, scale_shape=(0, 1)),
        "sdt": _item(64, 64, sdt=lib.F8),
        "sdt int": _item(64, 64, sdt=lib.I32),
    }
    bad["NULL"].scale = None
    for why, it in bad.items():
        assert _plan([_item(64, 64), it])[0] == -1, why
        assert lib.last_error().startswith("ct_fp8block_dequant_plan: item 1"), (why, lib.last_error())
    # every broadcast torch accepts
    for shape in ((3, 2), (1, 2), (3, 1), (1, 1)):
        assert _plan([_item(300, 200, scale_shape=shape)])[0] > 0, shape
    # one item beyond a launch (2^24 workgroups), and a batch of items that fit one by one
    assert _plan([_item(1 << 30, 1 << 20, scale_shape=(1, 1))])[0] == -1 and "split the batch" in lib.last_error()
    one, _ = _plan([_item(1 << 20, 1 << 16, scale_shape=(1, 1))])
    assert one == (1 << 20) * (1 << 12) // 1024
    assert _plan([_item(1 << 20, 1 << 16, scale_shape=(1, 1)) for _ in range(5)])[0] == -1 and "split the batch" in lib.last_error()


def test_launch_refuses_a_bad_output_dtype(lib):
    assert lib.load().ct_fp8block_dequant_batch(None, 0, 0, lib.I8, None) != 0 and "output dtype" in lib.last_error()
    assert lib.load().ct_fp8block_dequant_batch(None, 0, 0, lib.BF16, None) == 0


def test_python_splits_a_table_the_plan_refuses(lib):
    from compressed_tensors_amd.entrypoints.convert import staging

    plan = lib.load().ct_fp8block_dequant_plan
    big = [_item(1 << 20, 1 << 16, scale_shape=(1, 1), base=0x100000 * (i + 1)) for i in range(5)]
    tables = staging.plan_tables(big, [f"m{i}" for i in range(5)], lib.Fp8BlockItem, plan)
    assert len(tables) > 1 and sum(n for n, _, _ in tables) == 5 and all(0 < b < 1 << 24 for _, _, b in tables)
    with pytest.raises(ValueError, match="model.bad: ct_fp8block_dequant_plan: item 0: weight_scale_inv of shape"):
        staging.plan_tables([_item(64, 64), _item(128, 128, scale_shape=(2, 2))], ["model.good", "model.bad"], lib.Fp8BlockItem, plan)


def test_restatement_matches_the_reference_fixtures():
    """the eager restatement the DeepSeek-shaped GPU test trusts, against the reference's outputs (CPU)"""
    for case in _manifest()["cases"]:
        inp = case_inputs(case)
        names = [n for n in inp if targeted(inp, n)]
        assert names and len(case["synth"]) + len(_case_tensors(case["name"], "out")) == len(names), case["name"]
        for name in names:
            assert_reference(case, name, restated(inp[name], inp[f"{name}_scale_inv"], case["block"], getattr(torch, case["dtype"])))


# ------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_process_matches_the_reference_on_every_fixture_case():
    for case in _manifest()["cases"]:
        inp = case_inputs(case)
        conv = _conv(case)
        conv.validate(dict.fromkeys(inp))
        shard = dict(inp)
        got = conv.process(shard)
        assert list(got) == case["order"], case["name"]
        for name, t in got.items():
            if not targeted(inp, name):
                assert t is inp[name], (case["name"], name)  # untargeted entries are the same objects
                continue
            assert t.device.type == "cpu", (case["name"], name)
            assert_reference(case, name, t)
        # the reference's private entry point: host tensors in, a host tensor out
        name = next(k for k in inp if k.endswith(".weight") and not k.startswith(("lm_head", "model.norm", "model.embed")))
        one = conv._create_dequantized_weight(inp[name], inp[f"{name}_scale_inv"])
        assert one.device.type == "cpu" and torch.equal(one.view(torch.uint8), got[name].view(torch.uint8)), case["name"]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, F16, F32])
def test_every_fixture_case_of_one_block_size_in_one_shard_takes_one_launch(monkeypatch, dtype):
    from compressed_tensors_amd import _lib

    shard, singles = {}, {}
    conv = FP8BlockDequantizer(ignore=["re:lm_head.*"], targets=["re:.*proj(_with_mqa)?$"], dtype=dtype)
    for case in _manifest()["cases"]:
        if case["block"] != [128, 128]:
            continue
        inp = case_inputs(case)
        for name, t in inp.items():
            if not name.endswith(".weight") or f"{name}_scale_inv" not in inp or name.startswith("lm_head"):
                continue
            m = f"c{len(singles)}.{name[: -len('.weight')]}"
            shard[f"{m}.weight"], shard[f"{m}.weight_scale_inv"] = t, inp[f"{name}_scale_inv"]
            singles[f"{m}.weight"] = conv._create_dequantized_weight(t, inp[f"{name}_scale_inv"])
    assert len(singles) >= 6
    lib = _lib.load()
    calls = []
    real = lib.ct_fp8block_dequant_batch
    monkeypatch.setattr(lib, "ct_fp8block_dequant_batch", lambda *a: calls.append(a[1]) or real(*a))
    out = conv.process(dict(shard))
    assert calls == [len(singles)]
    assert list(out) == list(singles)
    for k, v in singles.items():
        assert_same(out[k], v, k)


DEEPSEEK_V32_LAYER = [("self_attn.q_a_proj", 1536, 7168), ("self_attn.q_b_proj", 24576, 1536), ("self_attn.kv_a_proj_with_mqa", 576, 7168),
                      ("self_attn.kv_b_proj", 32768, 512), ("self_attn.o_proj", 7168, 16384), ("self_attn.indexer.wq_b", 8192, 1536),
                      ("self_attn.indexer.wk", 128, 7168), ("mlp.experts.0.gate_proj", 2048, 7168), ("mlp.experts.0.up_proj", 2048, 7168),
                      ("mlp.experts.0.down_proj", 7168, 2048), ("mlp.experts.1.down_proj", 7168, 2048)]
DEEPSEEK_TARGETS = ["re:.*(proj|proj_with_mqa|wq_b|wk)$"]


def _deepseek_table(dev, seed, scale_dtype=F32):
    gen = torch.Generator(device=dev).manual_seed(seed)
    tensors = {}
    for name, R, C in DEEPSEEK_V32_LAYER:
        m = f"model.layers.3.{name}"
        tensors[f"{m}.weight"] = torch.randint(0, 256, (R, C), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8).view(FP8)
        tensors[f"{m}.weight_scale_inv"] = (torch.rand(-(-R // 128), -(-C // 128), generator=gen, device=dev) * 1e-3 + 1e-5).to(scale_dtype)
    tensors["model.layers.3.input_layernorm.weight"] = torch.ones(7168, device=dev, dtype=BF16)
    return tensors


@pytest.mark.gpu
def test_deepseek_layer_table_matches_the_restatement():
    dev = torch.device("cuda:0")
    tensors = _deepseek_table(dev, 7)
    conv = FP8BlockDequantizer(targets=DEEPSEEK_TARGETS, device=dev)
    conv.validate(tensors)
    want = {k: restated(v, tensors[f"{k}_scale_inv"], (128, 128), BF16).cpu() for k, v in tensors.items()
            if k.endswith(".weight") and f"{k}_scale_inv" in tensors}
    assert len(want) == len(DEEPSEEK_V32_LAYER)
    got = conv.process(dict(tensors))
    assert [k for k in got] == [k for k in tensors if not k.endswith("_scale_inv")]
    for k, v in want.items():
        assert_same(got[k], v, k)
    assert got["model.layers.3.input_layernorm.weight"] is tensors["model.layers.3.input_layernorm.weight"]


@pytest.mark.gpu
def test_deepseek_layer_table_matches_the_live_reference():
    import ref_import

    if not ref_import.available():
        pytest.skip("the reference sources are not available")
    try:
        ref_import.import_reference()
        from compressed_tensors.entrypoints.convert import FP8BlockDequantizer as RefConverter
    except ImportError as e:
        pytest.skip(f"the reference converter does not import here: {e}")
    dev = torch.device("cuda:0")
    tensors = _deepseek_table(dev, 11, scale_dtype=BF16)
    want = RefConverter(targets=DEEPSEEK_TARGETS).process(dict(tensors))  # the reference's own eager torch, on the GPU tensors
    got = FP8BlockDequantizer(targets=DEEPSEEK_TARGETS, device=dev).process(dict(tensors))
    assert list(got) == list(want)
    for k, v in want.items():
        assert_same(got[k], v, k)


def _write_fp8_checkpoint(src, inp, nested):
    """the fixture case as a two-shard checkpoint; the weight_scale_inv of the second module lives in the other shard"""
    src.mkdir()
    qcfg = {"quant_method": "fp8", "fmt": "e4m3", "activation_scheme": "dynamic", "weight_block_size": [128, 128]}
    cfg = {"architectures": ["Toy"], "text_config": {"quantization_config": qcfg}} if nested else {"architectures": ["Toy"], "quantization_config": qcfg}
    (src / "config.json").write_text(json.dumps(cfg))
    mods = sorted({k[: -len(".weight")] for k in inp if k.endswith(".weight") and f"{k}_scale_inv" in inp and not k.startswith("lm_head")})
    s1, s2 = "model-00001-of-00002.safetensors", "model-00002-of-00002.safetensors"
    shards = {s1: {}, s2: {}}
    for k, v in inp.items():
        m, _, p = k.rpartition(".")
        if m in mods:
            home = s1 if m == mods[0] else s2
            shards[(s2 if home == s1 else s1) if (m == mods[1] and p == "weight_scale_inv") else home][k] = v
        else:
            shards[s1 if k.startswith("model.") else s2][k] = v
    wm = {}
    for fn, t in shards.items():
        save_file(t, str(src / fn))
        wm.update({k: fn for k in t})
    (src / "model.safetensors.index.json").write_text(json.dumps({"metadata": {"total_size": 0}, "weight_map": wm}))
    return shards, mods


@pytest.mark.gpu
@pytest.mark.parametrize("max_workers,nested", [(1, False), (3, True)])
def test_convert_checkpoint_end_to_end(tmp_path, max_workers, nested):
    case = next(c for c in _manifest()["cases"] if c["name"] == "mixed_b128_f32_bf16")
    inp = case_inputs(case)
    inp.update({k: v for k, v in _case_tensors("sq256_b128_f32_bf16", "in").items() if not k.startswith("model.layers")})
    src, dst = tmp_path / "src", tmp_path / "dst"
    shards, mods = _write_fp8_checkpoint(src, inp, nested)
    assert f"{mods[1]}.weight_scale_inv" in shards["model-00001-of-00002.safetensors"] and f"{mods[1]}.weight" in shards["model-00002-of-00002.safetensors"]
    convert_checkpoint(src, dst, _conv(case), max_workers=max_workers)

    out = {}
    for fn in shards:
        out.update(load_file(str(dst / fn)))
    assert set(out) == {k for k in inp if not (k.endswith("_scale_inv") and k[: -len(".weight_scale_inv")] in mods)}
    for m in mods:
        assert_same(out[f"{m}.weight"], restated(inp[f"{m}.weight"], inp[f"{m}.weight_scale_inv"], (128, 128), BF16), m)
    for k in ("lm_head.weight", "lm_head.weight_scale_inv", "model.norm.weight", "model.embed_tokens.weight"):
        assert torch.equal(out[k].view(torch.uint8), inp[k].view(torch.uint8)), k
    index = json.load(open(dst / "model.safetensors.index.json"))
    assert set(index["weight_map"]) == set(out) and index["metadata"]["total_size"] == sum(t.numel() * t.element_size() for t in out.values())
    cfg = json.load(open(dst / "config.json"))
    assert "quantization_config" not in cfg and "quantization_config" not in cfg.get("text_config", {})
    assert cfg["architectures"] == ["Toy"] and ("text_config" in cfg) == nested
