"""AutoAWQConverter (reference entrypoints/convert/converters/autoawq.py): AutoAWQ GEMM checkpoints to pack-quantized through one
`ct_awq_repack_batch` launch per shard.  CPU tests: the converter's host logic against the reference tests' cases and the fixture's
config dicts, and the C planner through ctypes.  GPU tests: `process` against the reference's outputs in tests/golden/awq.safetensors
(tools/gen_golden_awq.py), one launch per shard, an 8B-shaped table against an eager int32 restatement of the format, and convert_checkpoint end to end
followed by the existing dequantizer."""
import ctypes
import json
import os
import sys

import pytest
import torch
from safetensors.torch import load_file, save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from compressed_tensors_amd.entrypoints.convert import AutoAWQConverter, CompressedTensorsDequantizer, convert_checkpoint  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
AWQ_ORDER = [0, 4, 1, 5, 2, 6, 3, 7]  # nibble position of natural column c inside an AutoAWQ word


def _manifest():
    with open(os.path.join(GOLDEN, "awq_manifest.json")) as f:
        return json.load(f)


def _case_tensors(name, side):
    blob = load_file(os.path.join(GOLDEN, "awq.safetensors"))
    pre = f"{name}.{side}."
    return {k[len(pre):]: v for k, v in blob.items() if k.startswith(pre)}


def _pack_int4(values: torch.Tensor) -> torch.Tensor:
    values = values.to(torch.int32)
    packed = torch.zeros(values.shape[0], values.shape[1] // 8, dtype=torch.int32)
    for offset in range(8):
        packed |= values[:, offset::8] << (offset * 4)
    return packed


# ------------------------------------------------------------------------------------------------------------------- host logic
def test_constructor_errors_and_defaults():
    with pytest.raises(ValueError, match="only 4-bit"):
        AutoAWQConverter(bits=8)
    with pytest.raises(ValueError, match="Unsupported AutoAWQ version"):
        AutoAWQConverter(version="gemv")
    c = AutoAWQConverter()
    assert (c.bits, c.group_size, c.zero_point, c.version, c.ignore, c.targets, c.device) == (4, 128, True, "gemm", ["lm_head"], ["Linear"], None)
    assert AutoAWQConverter(device="cuda:1").device == torch.device("cuda", 1)


def test_dependencies():
    converter = AutoAWQConverter(targets=[r"re:.*down_proj$"])
    assert converter.get_dependencies("model.layers.0.mlp.down_proj.qweight") == {"model.layers.0.mlp.down_proj.qzeros",
                                                                                  "model.layers.0.mlp.down_proj.scales"}
    assert converter.get_dependencies("model.layers.0.mlp.up_proj.qweight") == set()
    assert converter.get_dependencies("model.layers.0.mlp.down_proj.scales") == set()
    symmetric = AutoAWQConverter(targets=[r"re:.*down_proj$"], zero_point=False)
    assert symmetric.get_dependencies("model.layers.0.mlp.down_proj.qweight") == {"model.layers.0.mlp.down_proj.scales"}
    assert AutoAWQConverter().get_dependencies("lm_head.qweight") == set()


def test_validate_by_names():
    converter = AutoAWQConverter()
    with pytest.raises(ValueError, match="without corresponding"):
        converter.validate({"model.layers.0.mlp.down_proj.qweight": None})
    with pytest.raises(ValueError, match="without corresponding model.layers.0.mlp.down_proj.qzeros"):
        converter.validate({"model.layers.0.mlp.down_proj.qweight": None, "model.layers.0.mlp.down_proj.scales": None})
    with pytest.raises(ValueError, match="unexpected non-targeted tensor lm_head.qweight"):
        converter.validate({"lm_head.qweight": None})
    converter.validate({"model.layers.0.mlp.down_proj.qweight": None, "model.layers.0.mlp.down_proj.scales": None,
                        "model.layers.0.mlp.down_proj.qzeros": None, "lm_head.weight": None, "model.norm.weight": None})
    AutoAWQConverter(zero_point=False).validate({"a.qweight": None, "a.scales": None})


def test_from_autoawq_config():
    converter = AutoAWQConverter.from_autoawq_config({"bits": 4, "group_size": 64, "zero_point": True, "version": "gemm",
                                                      "modules_to_not_convert": ["vision_tower"]})
    assert converter.ignore == ["lm_head", "re:.*vision_tower.*"]
    assert (converter.group_size, converter.zero_point) == (64, True)
    d = converter.create_config().model_dump()
    scheme = d["config_groups"]["config_group_0"]
    assert d["format"] == scheme["format"] == "pack-quantized" and d["quantization_status"] == "compressed"
    assert d["ignore"] == ["lm_head", "re:.*vision_tower.*"]
    assert scheme["weights"]["num_bits"] == 4 and scheme["weights"]["group_size"] == 64 and scheme["weights"]["symmetric"] is False
    assert AutoAWQConverter.from_autoawq_config({}).group_size == 128
    with pytest.raises(ValueError, match="only 4-bit"):
        AutoAWQConverter.from_autoawq_config({"bits": 8})


@pytest.mark.parametrize("nested", [False, True])
def test_from_pretrained_reads_config_json(tmp_path, nested):
    qcfg = {"quant_method": "awq", "bits": 4, "group_size": 32, "zero_point": True, "version": "gemm", "modules_to_not_convert": ["visual"]}
    cfg = {"architectures": ["Toy"], "text_config": {"quantization_config": qcfg}} if nested else {"quantization_config": qcfg}
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    converter = AutoAWQConverter.from_pretrained(tmp_path, targets=["re:.*proj$"])
    assert (converter.bits, converter.group_size, converter.zero_point, converter.version) == (4, 32, True, "gemm")
    assert converter.ignore == ["lm_head", "re:.*visual.*"] and converter.targets == ["re:.*proj$"]


def test_from_pretrained_errors(tmp_path):
    (tmp_path / "config.json").write_text(json.dumps({"architectures": ["Toy"]}))
    with pytest.raises(ValueError, match="does not contain quantization_config"):
        AutoAWQConverter.from_pretrained(tmp_path)
    (tmp_path / "config.json").write_text(json.dumps({"quantization_config": {"quant_method": "gptq", "bits": 4}}))
    with pytest.raises(ValueError, match="not an AutoAWQ config"):
        AutoAWQConverter.from_pretrained(tmp_path)
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="config.json"):
        AutoAWQConverter.from_pretrained(empty)


def test_from_pretrained_does_not_import_transformers(tmp_path):
    import subprocess

    (tmp_path / "config.json").write_text(json.dumps({"quantization_config": {"quant_method": "awq", "group_size": 64}}))
    code = ("import sys; from compressed_tensors_amd.entrypoints.convert import AutoAWQConverter as A; "
            f"c = A.from_pretrained({str(tmp_path)!r}); assert c.group_size == 64; assert 'transformers' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, env=dict(os.environ, PYTHONPATH=ROOT))


def test_create_config_equals_the_reference_dicts():
    for name, entry in _manifest()["configs"].items():
        converter = AutoAWQConverter.from_autoawq_config(entry["autoawq_config"], targets=entry["targets"])
        assert converter.create_config().model_dump() == entry["model_dump"], name


def test_process_without_targets_passes_everything_through():
    tensors = {"lm_head.weight": torch.ones(2, 2), "model.norm.weight": torch.ones(3)}
    out = AutoAWQConverter().process(dict(tensors))
    assert set(out) == set(tensors) and all(out[k] is tensors[k] for k in tensors)


def test_process_refuses_missing_zero_points_and_bad_dtypes():
    with pytest.raises(ValueError, match="without corresponding qzeros"):
        AutoAWQConverter().process({"m.qweight": torch.zeros(8, 1, dtype=torch.int32), "m.scales": torch.ones(1, 8, dtype=torch.float16)})
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        AutoAWQConverter(zero_point=False).process({"m.qweight": torch.zeros(8, 1, dtype=torch.int32), "m.scales": torch.ones(1, 8)})


# ------------------------------------------------------------------------------------------------------------------- the C planner
def _item(K, N, G, *, zp=True, base=0x100000, scale_shape=None, zp_shape=None, dt=None):
    from compressed_tensors_amd import _lib

    it = _lib.AwqItem()
    it.qweight, it.scales, it.weight_packed, it.scale_t = base, base + 0x1000, base + 0x2000, base + 0x3000
    if zp:
        it.qzeros, it.zp_packed = base + 0x4000, base + 0x5000
        it.zp_shape[0], it.zp_shape[1] = zp_shape or (G, N // 8)
    it.K, it.N, it.G = K, N, G
    it.scale_shape[0], it.scale_shape[1] = scale_shape or (G, N)
    it.scale_dt = _lib.F16 if dt is None else dt
    return it


def _plan(items):
    from compressed_tensors_amd import _lib

    table = (_lib.AwqItem * len(items))(*items)
    return int(_lib.load().ct_awq_repack_plan(ctypes.cast(table, ctypes.c_void_p), len(items))), table


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    from compressed_tensors_amd import _lib

    return _lib


def test_plan_counts_workgroups_of_a_known_table(lib):
    assert ctypes.sizeof(lib.AwqItem) == 17 * 8 and lib.AwqItem.scale_dt.offset == 104 and lib.AwqItem.first_block.offset == 112
    # (K, N, G, zp): weight tiles of 256 rows x 32 words, 64 x 64 tiles for the zero points (G, N / 8) and the scales (G, N)
    shapes = [(4096, 4096, 32, True), (14336, 4096, 112, True), (200, 96, 5, False), (2, 8, 1, True)]
    n, table = _plan([_item(K, N, G, zp=z, base=0x100000 * (i + 1)) for i, (K, N, G, z) in enumerate(shapes)])
    expect, first = [], 0
    for K, N, G, z in shapes:
        wb = -(-K // 256) * -(-(N // 8) // 32)
        zb = -(-G // 64) * -(-(N // 8) // 64) if z else 0
        sb = -(-G // 64) * -(-N // 64)
        expect.append((first, wb, zb))
        first += wb + zb + sb
    assert n == first == (16 * 16 + 1 * 8 + 64) + (56 * 16 + 2 * 8 + 2 * 64) + (1 * 1 + 0 + 2) + (1 + 1 + 1)
    assert [(t.first_block, t.weight_blocks, t.zp_blocks) for t in table] == expect
    # 16-byte qweight rows need N / 8 % 4 == 0, 16-byte weight_packed rows ceil(K / 8) % 4 == 0 (and aligned pointers)
    assert [t.wide for t in table] == [3, 3, 1, 0]
    assert _plan([])[0] == 0


def test_plan_refuses_malformed_items_and_oversized_batches(lib):
    bad = {
        "NULL": _item(64, 64, 1),
        "zp pair": _item(64, 64, 1),
        "empty": _item(0, 64, 1),
        "N % 8": _item(64, 60, 1, scale_shape=(1, 60), zp_shape=(1, 7)),
        "no groups": _item(64, 64, 0, scale_shape=(0, 64), zp_shape=(0, 8)),
        "scales vs N": _item(64, 64, 1, scale_shape=(1, 32)),
        "scales vs G": _item(64, 64, 2, scale_shape=(1, 64), zp_shape=(2, 8)),
        "qzeros vs N": _item(64, 64, 1, zp_shape=(1, 64)),
        "scale dtype": _item(64, 64, 1, dt=lib.F32),
    }
    bad["NULL"].qweight = None
    bad["zp pair"].zp_packed = None
    for why, it in bad.items():
        assert _plan([_item(64, 64, 1), it])[0] == -1, why
        assert lib.last_error().startswith("ct_awq_repack_plan: item 1"), (why, lib.last_error())
    # without zero points the zp shape is not looked at
    assert _plan([_item(64, 64, 1, zp=False, zp_shape=(9, 9))])[0] > 0
    # one item beyond a launch (2^24 workgroups), and a batch of items that fit one by one
    assert _plan([_item(1 << 30, 8192, 1, scale_shape=(1, 8192), zp_shape=(1, 1024))])[0] == -1 and "split the batch" in lib.last_error()
    one, _ = _plan([_item(1 << 26, 8192, 1, scale_shape=(1, 8192), zp_shape=(1, 1024))])
    assert 0 < one < 1 << 24
    many = [_item(1 << 26, 8192, 1, scale_shape=(1, 8192), zp_shape=(1, 1024)) for _ in range(1 + (1 << 24) // one)]
    assert _plan(many)[0] == -1 and "split the batch" in lib.last_error()


def test_python_splits_a_batch_the_plan_refuses(lib):
    from compressed_tensors_amd.entrypoints.convert import staging

    plan = lib.load().ct_awq_repack_plan
    big = [_item(1 << 26, 8192, 1, scale_shape=(1, 8192), zp_shape=(1, 1024), base=0x100000 * (i + 1)) for i in range(5)]
    tables = staging.plan_tables(big, [f"m{i}" for i in range(5)], lib.AwqItem, plan)
    assert len(tables) > 1 and sum(n for n, _, _ in tables) == 5 and all(0 < b < 1 << 24 for _, _, b in tables)
    with pytest.raises(ValueError, match="scales of shape"):
        staging.plan_tables([_item(64, 64, 1), _item(64, 64, 1, scale_shape=(1, 32))], ["model.good", "model.bad"], lib.AwqItem, plan)
    with pytest.raises(ValueError, match="^model.bad: ct_awq_repack_plan: item 0: "):
        staging.plan_tables([_item(64, 64, 1), _item(64, 64, 1, scale_shape=(1, 32))], ["model.good", "model.bad"], lib.AwqItem, plan)


# ------------------------------------------------------------------------------------------------------------------- GPU
def awq_restated(qweight: torch.Tensor, qzeros, scales: torch.Tensor):
    """the pack-quantized tensors of one AutoAWQ module, eager int32 torch, from the format: natural nibble c of a word sits at
    AWQ position AWQ_ORDER[c]; weight_packed (N, ceil(K / 8)) packs 8 consecutive k of one output row n; the zero points
    (N / 8, G) pack 8 consecutive n of one group"""
    dev = qweight.device
    K, W = qweight.shape
    N = 8 * W
    shifts = 4 * torch.tensor(AWQ_ORDER, dtype=torch.int32, device=dev)
    place = 4 * torch.arange(8, dtype=torch.int64, device=dev)
    nib = ((qweight[:, :, None] >> shifts) & 15).reshape(K, N).t()  # (N, K) codes + 8
    KW = -(-K // 8)
    nib = torch.nn.functional.pad(nib, (0, 8 * KW - K)).reshape(N, KW, 8).to(torch.int64)
    out = {"weight_packed": (nib << place).sum(-1).to(torch.int32), "weight_scale": scales.t().contiguous(),
           "weight_shape": torch.tensor([N, K], dtype=torch.int64)}
    if qzeros is not None:
        z = ((qzeros[:, :, None] >> shifts) & 15).to(torch.int64)  # (G, W, 8), natural order
        out["weight_zero_point"] = (z << place).sum(-1).to(torch.int32).t().contiguous()
    return out


def test_restatement_matches_the_reference_fixtures():
    """the eager restatement the 8B-shaped GPU test trusts, against the reference's outputs (CPU)"""
    for case in _manifest()["cases"]:
        inp, ref = _case_tensors(case["name"], "in"), _case_tensors(case["name"], "out")
        for name in inp:
            if name.endswith(".qweight"):
                m = name[: -len(".qweight")]
                got = awq_restated(inp[name], inp.get(f"{m}.qzeros") if case["autoawq_config"]["zero_point"] else None, inp[f"{m}.scales"])
                for k, v in got.items():
                    assert torch.equal(v, ref[f"{m}.{k}"]), (case["name"], m, k)


def test_without_a_gpu_the_converter_raises(monkeypatch):
    """no GPU: the converter raises instead of converting on the host"""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    t = {"m.qweight": _pack_int4(torch.arange(16).reshape(2, 8) % 16), "m.scales": torch.ones(1, 8, dtype=torch.float16)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AutoAWQConverter(zero_point=False).process(t)


@pytest.mark.gpu
def test_process_matches_the_reference_on_every_fixture_case():
    for case in _manifest()["cases"]:
        inp, ref = _case_tensors(case["name"], "in"), _case_tensors(case["name"], "out")
        converter = AutoAWQConverter.from_autoawq_config(case["autoawq_config"], targets=case["targets"])
        converter.validate(dict.fromkeys(inp))
        got = converter.process(dict(inp))
        assert set(got) == set(ref), case["name"]
        for k, v in ref.items():
            assert got[k].device.type == "cpu" and got[k].dtype == v.dtype and got[k].shape == v.shape, (case["name"], k)
            assert torch.equal(got[k], v), (case["name"], k)


@pytest.mark.gpu
def test_every_fixture_module_of_one_case_in_one_shard_takes_one_launch(monkeypatch):
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    calls = []
    real = lib.ct_awq_repack_batch
    monkeypatch.setattr(lib, "ct_awq_repack_batch", lambda *a: calls.append(a[1]) or real(*a))
    for case in _manifest()["cases"]:
        inp, ref = _case_tensors(case["name"], "in"), _case_tensors(case["name"], "out")
        modules = [k for k in ref if k.endswith(".weight_packed")]  # one per module the reference converted
        assert modules, case["name"]
        del calls[:]
        got = AutoAWQConverter.from_autoawq_config(case["autoawq_config"], targets=case["targets"]).process(dict(inp))
        assert calls == [len(modules)], case["name"]
        assert set(got) == set(ref), case["name"]
        for k, v in ref.items():
            assert torch.equal(got[k], v), (case["name"], k)


@pytest.mark.gpu
def test_process_matches_the_reference_test_cases():
    """autoawq reference tests: two rows of codes, N = 8, K = 2 (a tail word), group size 2"""
    for zero_point in (True, False):
        converter = AutoAWQConverter(group_size=2, targets=[r"re:.*proj$"], zero_point=zero_point)
        tensors = {"model.layers.0.mlp.up_proj.qweight": _pack_int4(torch.tensor([[8, 9, 10, 11, 12, 13, 14, 15], [0, 1, 2, 3, 4, 5, 6, 7]])),
                   "model.layers.0.mlp.up_proj.qzeros": _pack_int4(torch.full((1, 8), 8)),
                   "model.layers.0.mlp.up_proj.scales": torch.ones(1, 8, dtype=torch.float16), "model.embed_tokens.weight": torch.ones(4, 4)}
        if not zero_point:
            del tensors["model.layers.0.mlp.up_proj.qzeros"]
        converter.validate(tensors)
        out = converter.process(tensors)
        p = "model.layers.0.mlp.up_proj."
        assert not any(f"{p}{k}" in out for k in ("qweight", "qzeros", "scales", "weight"))
        assert out[f"{p}weight_packed"].shape == (8, 1) and torch.equal(out[f"{p}weight_shape"], torch.tensor([8, 2]))
        assert out[f"{p}weight_scale"].shape == (8, 1) and out[f"{p}weight_scale"].is_contiguous()
        # weight_packed row n holds (k = 0, k = 1) of natural column n: the first row's AWQ nibbles are 8 + position
        want = [(8 + AWQ_ORDER[n]) | (AWQ_ORDER[n] << 4) for n in range(8)]
        assert out[f"{p}weight_packed"].flatten().tolist() == want
        assert (out[f"{p}weight_zero_point"].shape == (1, 1)) if zero_point else (f"{p}weight_zero_point" not in out)


LLAMA3_8B_LAYER = [("self_attn.q_proj", 4096, 4096), ("self_attn.k_proj", 4096, 1024), ("self_attn.v_proj", 4096, 1024),
                   ("self_attn.o_proj", 4096, 4096), ("mlp.gate_proj", 4096, 14336), ("mlp.up_proj", 4096, 14336),
                   ("mlp.down_proj", 14336, 4096)]


def _llama_table(layers, dev, gen, group=128):
    tensors = {}
    for layer in range(layers):
        for name, K, N in LLAMA3_8B_LAYER:
            m = f"model.layers.{layer}.{name}"
            G = K // group
            tensors[f"{m}.qweight"] = torch.randint(-2 ** 31, 2 ** 31 - 1, (K, N // 8), generator=gen, dtype=torch.int32, device=dev)
            tensors[f"{m}.qzeros"] = torch.randint(-2 ** 31, 2 ** 31 - 1, (G, N // 8), generator=gen, dtype=torch.int32, device=dev)
            tensors[f"{m}.scales"] = (torch.rand(G, N, generator=gen, device=dev) * 0.01 + 1e-3).to(torch.float16)
    return tensors


@pytest.mark.gpu
def test_8b_shaped_table_matches_the_restatement():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    tensors = _llama_table(2, dev, gen)
    want = {}
    for name in tensors:
        if name.endswith(".qweight"):
            m = name[: -len(".qweight")]
            for k, v in awq_restated(tensors[name], tensors[f"{m}.qzeros"], tensors[f"{m}.scales"]).items():
                want[f"{m}.{k}"] = v.cpu()
    got = AutoAWQConverter(device=dev).process(dict(tensors))
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and torch.equal(got[k], v), k


@pytest.mark.gpu
def test_8b_shaped_table_matches_the_live_reference():
    import ref_import

    if not ref_import.available():
        pytest.skip("the reference sources are not available")
    try:
        ref_import.import_reference()
        from compressed_tensors.entrypoints.convert import AutoAWQConverter as RefConverter
    except ImportError as e:  # the reference converter imports transformers
        pytest.skip(f"the reference converter does not import here: {e}")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(11)
    tensors = _llama_table(1, dev, gen)
    want = RefConverter().process(dict(tensors))  # the reference's own eager torch, on the GPU tensors
    got = AutoAWQConverter(device=dev).process(dict(tensors))
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and torch.equal(got[k], v.cpu()), k


def _write_awq_checkpoint(src, inp, case):
    """the fixture case as a two-shard AutoAWQ checkpoint; the partners of the second module live in the other shard"""
    src.mkdir()
    qcfg = dict(case["autoawq_config"], quant_method="awq", bits=4, version="gemm")
    (src / "config.json").write_text(json.dumps({"architectures": ["Toy"], "quantization_config": qcfg}))
    (src / "tokenizer.json").write_text("{}")
    mods = sorted({k.rsplit(".", 1)[0] for k in inp if k.endswith(".qweight")})
    s1, s2 = "model-00001-of-00002.safetensors", "model-00002-of-00002.safetensors"
    shards = {s1: {}, s2: {}}
    for k, v in inp.items():
        m, _, p = k.rpartition(".")
        if m in mods:
            home = s1 if m == mods[0] else s2
            other = s2 if home == s1 else s1
            shards[other if (m == mods[1] and p != "qweight") else home][k] = v
        else:
            shards[s1 if k.startswith("model.") else s2][k] = v
    wm = {}
    for fn, t in shards.items():
        save_file(t, str(src / fn))
        wm.update({k: fn for k in t})
    (src / "model.safetensors.index.json").write_text(json.dumps({"metadata": {"total_size": 0}, "weight_map": wm}))
    return shards


@pytest.mark.gpu
@pytest.mark.parametrize("max_workers", [1, 3])
def test_convert_checkpoint_end_to_end_then_dequantize(tmp_path, max_workers):
    import oracle as O

    case = next(c for c in _manifest()["cases"] if c["name"] == "g128_zp_f16")
    inp, ref = _case_tensors(case["name"], "in"), _case_tensors(case["name"], "out")
    src, dst, deq = tmp_path / "src", tmp_path / "dst", tmp_path / "deq"
    shards = _write_awq_checkpoint(src, inp, case)
    assert any(k.endswith(".qweight") for k in shards["model-00002-of-00002.safetensors"])
    convert_checkpoint(src, dst, AutoAWQConverter.from_pretrained(src), max_workers=max_workers)

    out = {}
    for fn in shards:
        out.update(load_file(str(dst / fn)))
    assert set(out) == set(ref)
    for k, v in ref.items():
        assert out[k].dtype == v.dtype and torch.equal(out[k], v), k
    for k in ("lm_head.weight", "model.norm.weight", "model.visual.proj.weight", "model.visual.proj.bias"):
        assert torch.equal(out[k], inp[k]), k
    index = json.load(open(dst / "model.safetensors.index.json"))
    assert set(index["weight_map"]) == set(out) and index["metadata"]["total_size"] == sum(t.numel() * t.element_size() for t in out.values())
    qc = json.load(open(dst / "config.json"))["quantization_config"]
    want_cfg = AutoAWQConverter.from_autoawq_config(case["autoawq_config"]).create_config().model_dump()
    assert {k: v for k, v in qc.items() if k != "version"} == want_cfg and "version" in qc
    assert (dst / "tokenizer.json").exists()

    # the converted checkpoint loads through the existing dequantizer
    convert_checkpoint(dst, deq, CompressedTensorsDequantizer(dst, dtype=torch.float16, device="cuda:0"), max_workers=max_workers)
    w = {}
    for fn in shards:
        w.update(load_file(str(deq / fn)))
    mods = sorted({k.rsplit(".", 1)[0] for k in inp if k.endswith(".qweight")})
    for m in mods:
        sd = {p: ref[f"{m}.{p}"] for p in ("weight_packed", "weight_scale", "weight_zero_point", "weight_shape")}
        want = O.pack_quantized_decompress(sd, num_bits=4, strategy="group", symmetric=False)["weight"]
        assert w[f"{m}.weight"].dtype == torch.float16 and torch.equal(w[f"{m}.weight"], want), m
        # (iw - iz) * s straight from the AWQ words, in float64
        K, N = inp[f"{m}.qweight"].shape[0], 8 * inp[f"{m}.qweight"].shape[1]
        shifts = 4 * torch.tensor(AWQ_ORDER, dtype=torch.int32)
        iw = ((inp[f"{m}.qweight"][:, :, None] >> shifts) & 15).reshape(K, N).t().double()
        iz = ((inp[f"{m}.qzeros"][:, :, None] >> shifts) & 15).reshape(-1, N).t().double()
        s = inp[f"{m}.scales"].t().double()
        exact = (iw - iz.repeat_interleave(128, dim=1)[:, :K]) * s.repeat_interleave(128, dim=1)[:, :K]
        assert torch.allclose(w[f"{m}.weight"].double(), exact, rtol=2 ** -10, atol=0), m
    for k in ("lm_head.weight", "model.norm.weight", "model.visual.proj.weight"):
        assert torch.equal(w[k], inp[k]), k
