"""The permuted Hadamard rotation (`TransformScheme.randomize=True`) without a GPU: the fixtures re-synthesise; the identity
T_{W[p][:, p]}(x) = G_p(T_W(G_q(x))) holds on the reference's recorded outputs; apply_transform_config(randomize=True, seed=S) draws
upstream's permutations; the tables, the plan, the dispatch constants, the modules, the fusions and install()'s flag."""
import inspect
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hadamard_cases as H  # noqa: E402
import _hadamard_perm_cases as C  # noqa: E402
import ref_import  # noqa: E402

import compressed_tensors_amd as cta  # noqa: E402
from compressed_tensors_amd import _lib, codec, transform  # noqa: E402
from compressed_tensors_amd.quantization import dynamic  # noqa: E402
from compressed_tensors_amd.transform import apply as tapply  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "hadamard_perm_manifest.json")) as _f:
    _M = json.load(_f)
MANIFEST = _M["cases"]


@pytest.fixture(scope="module")
def golden_tensors():
    from safetensors.torch import load_file

    g = load_file(os.path.join(GOLDEN, "hadamard_perm.safetensors"))
    g.update({f"rh.{k}": v for k, v in load_file(os.path.join(GOLDEN, "random_hadamard.safetensors")).items() if k.startswith(("signs.", "had_k."))})
    return g


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------------
def test_manifest_covers_the_case_matrix():
    cases = dict(C.case_list())
    assert sorted(cases) == sorted(MANIFEST) and all(MANIFEST[k]["recipe"] == cases[k] for k in cases)
    for n in C.GROUP_SIZES + C.BLOCK_SIZES:  # every size of both kernels in every dtype
        for dt in C.DTYPES:
            assert any(r["type"] == "hadamard" and r["tier"] == "A" and r["size"] == n and r["dtype"] == dt for r in cases.values()), (n, dt)
    assert {r["size"] for r in cases.values() if r["type"] == "random-hadamard"} == set(C.RANDOM_K1 + C.RANDOM_K)
    assert any(C.dim_of(r) == 0 and r["shape"][-1] != 1 for r in cases.values()) and any(r["shape"] == [512, 1] for r in cases.values())
    assert sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in ("hadamard_perm.safetensors", "hadamard_perm_manifest.json")) <= 512 * 1024


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_recipes_resynthesise_their_inputs(key):
    assert C.sha(C.synth(MANIFEST[key]["recipe"])) == MANIFEST[key]["x_sha256"]


def test_the_identity_gives_every_stored_reference_output(golden_tensors):
    """G_p(butterfly(G_q(x))) and G_p(structured(G_q(x), ...)) — this repository's restatements of the unpermuted rotations between
    the two gathers — equal upstream's forward with the weight W[p][:, p] in every element, for every location and inverse"""
    import math

    seen = set()
    for key, entry in MANIFEST.items():
        r = entry["recipe"]
        if math.prod(r["shape"]) > 65536:
            continue  # the large cases: the generator asserted them, the GPU tests compare their sha256
        p = golden_tensors[f"perm.{r['type']}.{r['size']}"].to(torch.int64)
        assert sorted(p.tolist()) == list(range(r["size"]))
        had_k, signs = (golden_tensors.get(f"rh.had_k.{r['size']}"), golden_tensors[f"rh.signs.{r['size']}"]) if r["type"] == "random-hadamard" else (None, None)
        got = C.restated(r, C.synth(r), p, had_k, signs)
        assert str(got.dtype).replace("torch.", "") == entry["out"]["dtype"] and C.sha(got) == entry["out"]["sha256"], key
        if entry["stored"]:
            assert torch.equal(got, golden_tensors[f"{key}.out"]), key
        seen.add((r["type"], r["module"], r["location"], r["inverse"]))
    H_, R_, L, E = "hadamard", "random-hadamard", "Linear", "Embedding"
    assert seen >= {(H_, L, "input", False), (H_, L, "output", False), (H_, L, "weight_output", False), (H_, L, "weight_input", False), (H_, L, "weight_input", True),
                    (H_, E, "weight_input", False), (R_, L, "input", False), (R_, L, "input", True), (R_, L, "weight_input", False), (R_, L, "weight_input", True),
                    (R_, L, "weight_output", False), (R_, L, "weight_output", True)}


def test_the_permutations_are_randperm_on_the_factory_seed(golden_tensors):
    for name, info in _M["perms"].items():
        kind, n = name.rsplit(".", 1)
        g = torch.Generator().manual_seed(info["seed"])
        assert info["seed"] == C.seed_of(kind, int(n))
        if kind == "random-hadamard":
            torch.randint(low=0, high=2, size=(int(n),), generator=g, dtype=torch.float32)  # the weight's signs come first
        assert torch.equal(torch.randperm(int(n), generator=g), golden_tensors[f"perm.{name}"].to(torch.int64)), name


# ---- apply_transform_config(randomize=True, seed=S) draws what upstream's factories draw ----------------------------------------------------
def _meta_model():
    with torch.device("meta"):
        return torch.nn.Sequential(torch.nn.Linear(64, 128, dtype=torch.bfloat16), torch.nn.Linear(128, 32, bias=False, dtype=torch.bfloat16))


def _drawing_config(kind="hadamard"):
    """two sizes in group a (64 online + offline on module 0's input side, 128 on its output side), a randomize=False group in
    between, then a group that starts from the same seed"""
    def scheme(apply, randomize, head_dim=None):
        return {"type": kind, "apply": [dict(targets=[t], location=loc, inverse=inv, ignore=[]) for t, loc, inv in apply], "randomize": randomize,
                "requires_grad": False, "head_dim": head_dim, "precision": "torch.float32"}

    return {"config_groups": {
        "a": scheme([("0", "input", False), ("0", "weight_input", True), ("0", "output", False), ("1", "input", False)], True),
        "b": scheme([("1", "output", False)], False),
        "c": scheme([("1", "weight_output", False), ("0", "weight_input", False)], True, head_dim=32),
    }}


def _perms_of(model):
    return {k: v.clone() for k, v in model.state_dict().items() if k.endswith(".perm")}


@pytest.mark.skipif(not ref_import.available(), reason="upstream reference sources not present on this machine")
@pytest.mark.parametrize("kind", ["hadamard", "random-hadamard"])
def test_apply_draws_upstreams_permutations(kind, monkeypatch):
    ref_import.import_reference()
    try:
        import compressed_tensors.transform as up_t
        import compressed_tensors.transform.factory.hadamard as up_h
        from compressed_tensors.transform.utils.hadamard import random_hadamard_matrix
    except ImportError as e:
        pytest.skip(f"upstream's transform package does not import here: {e}")
    seed = 11
    # the fused locations compute nothing here (no GPU is needed to compare draws): both sides leave the weights alone
    monkeypatch.setattr(up_h.HadamardTransform, "forward", lambda self, value: value)
    monkeypatch.setattr(transform.HadamardTransform, "forward", lambda self, value: value)
    monkeypatch.setattr(transform.RandomHadamardTransform, "forward", lambda self, value: value)
    cfg = _drawing_config(kind)
    theirs = torch.nn.Sequential(torch.nn.Linear(64, 128, dtype=torch.bfloat16), torch.nn.Linear(128, 32, bias=False, dtype=torch.bfloat16))
    drawn = []
    for name, scheme in up_t.TransformConfig.model_validate(cfg).config_groups.items():
        factory = up_t.TransformFactory.from_scheme(scheme, name=name, seed=seed)
        factory.apply_to_model(theirs, use_tqdm=False)
        drawn.append(list(factory.perms.values()))
    assert [len(d) for d in drawn] == [2, 0, 1]  # two sizes; randomize=False draws nothing; one size shared by two modules
    ours = torch.nn.Sequential(torch.nn.Linear(64, 128, dtype=torch.bfloat16), torch.nn.Linear(128, 32, bias=False, dtype=torch.bfloat16))
    weights = (lambda size, dtype, device, gen: random_hadamard_matrix(size, dtype, device, gen)) if kind == "random-hadamard" else None
    cta.apply_transform_config(ours, cta.TransformConfig.from_dict(cfg), hadamard_weights=weights, randomize=True, seed=seed)
    mine, want = _perms_of(ours), _perms_of(theirs)
    assert sorted(mine) == sorted(want) == ["0.a_input.perm", "0.a_output.perm", "1.a_input.perm"]  # upstream's state_dict keys, online transforms
    for k in want:
        assert mine[k].dtype == torch.int64 and mine[k].device.type == "cpu" and torch.equal(mine[k], want[k]), k
    assert not hasattr(ours[1].b_output, "perm") or ours[1].b_output.perm is None
    assert torch.equal(ours[1].a_input.perm, ours[0].a_output.perm)  # size 128 shared across modules; 64 shared online / offline (same draw)
    # another seed, another draw; no seed: nothing pinned, still permutations
    again = torch.nn.Sequential(torch.nn.Linear(64, 128, dtype=torch.bfloat16), torch.nn.Linear(128, 32, bias=False, dtype=torch.bfloat16))
    cta.apply_transform_config(again, cta.TransformConfig.from_dict(cfg), hadamard_weights=weights, randomize=True, seed=seed + 1)
    assert not torch.equal(_perms_of(again)["1.a_input.perm"], want["1.a_input.perm"])


def test_apply_on_a_meta_model_draws_on_the_cpu_and_shares_per_size():
    m = _meta_model()
    cfg = cta.TransformConfig({"r": cta.TransformScheme("hadamard", [cta.TransformArgs("Linear", "input"), cta.TransformArgs("re:0", "output")], randomize=True),
                               "s": cta.TransformScheme("hadamard", [cta.TransformArgs("re:1", "output")])})
    cta.apply_transform_config(m, cfg, randomize=True, seed=3)
    g = torch.Generator().manual_seed(3)
    p64, p128 = torch.randperm(64, generator=g), torch.randperm(128, generator=g)  # in order of first use
    assert torch.equal(m[0].r_input.perm, p64) and torch.equal(m[1].r_input.perm, p128) and m[0].r_output.perm.data_ptr() == m[1].r_input.perm.data_ptr()  # one draw, one storage
    assert m[1].s_output.perm is None and "perm" not in m[1].s_output.state_dict() and not list(m[1].s_output.buffers())
    assert sorted(k for k in m.state_dict() if k.endswith(".perm")) == ["0.r_input.perm", "0.r_output.perm", "1.r_input.perm"]
    t = m[0].r_input
    assert not list(t.parameters()) and [tuple(b.shape) for b in t.buffers()] == [(64,)]  # no n x n tensor
    assert "permuted=True" in repr(t) and "permuted=False" in repr(m[1].s_output)


def test_the_default_calls_still_raise():
    for kwargs in (dict(), dict(seed=5), dict(hadamard_weights=lambda *a: None)):
        m = _meta_model()
        cfg = cta.TransformConfig({"bad": cta.TransformScheme("hadamard", [cta.TransformArgs("Linear", "input")], randomize=True)})
        with pytest.raises(NotImplementedError, match="randomize=True needs upstream's permutation, which is not built here"):
            cta.apply_transform_config(m, cfg, **kwargs)
        assert not hasattr(m, "transform_config") and not m[0]._forward_pre_hooks
    assert inspect.signature(cta.apply_transform_config).parameters["randomize"].default is False
    assert inspect.signature(cta.apply_transform_config).parameters["seed"].default is None


@pytest.mark.parametrize("bad,match", [(dict(requires_grad=True), "requires_grad"), (dict(type="matrix-multiply"), "type"),
                                       (dict(type="random-hadamard"), "type")])
def test_with_the_opt_in_every_other_check_still_runs_first(bad, match, monkeypatch):
    drawn = []
    monkeypatch.setattr(torch, "randperm", lambda *a, **k: drawn.append(a) or torch.arange(a[0]))
    m = _meta_model()
    groups = {"ok": cta.TransformScheme("hadamard", [cta.TransformArgs("Linear", "input")], randomize=True),
              "bad": cta.TransformScheme(**{"type": "hadamard", "apply": [cta.TransformArgs("Linear", "input")], "randomize": True, **bad})}
    with pytest.raises(NotImplementedError, match=match):
        cta.apply_transform_config(m, cta.TransformConfig(groups), randomize=True, seed=1)
    assert not drawn and not hasattr(m, "transform_config") and not m[0]._forward_pre_hooks


@pytest.mark.parametrize("location", ["q_attn", "k_cache"])
def test_attention_locations_still_need_a_pretrained_model(location):
    cfg = cta.TransformConfig({"r": cta.TransformScheme("hadamard", [cta.TransformArgs("Linear", location)], randomize=True)})
    with pytest.raises(NotImplementedError, match="location"):
        cta.apply_transform_config(_meta_model(), cfg, randomize=True)


# ---- hadamard_perm_tables ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perm", [torch.tensor([0, 1, 1, 3]), torch.tensor([0, 1, 2, 4]), torch.tensor([0, -1, 2, 3]), torch.tensor([0.0, 1.0, 2.0, 3.0]),
                                  torch.tensor([[0, 1], [2, 3]]), torch.tensor([], dtype=torch.int64), torch.tensor([True, False])],
                         ids=["repeated", "out_of_range", "negative", "float", "two_dim", "empty", "bool"])
def test_tables_reject_what_is_not_a_permutation(perm):
    with pytest.raises(ValueError):
        codec.hadamard_perm_tables(perm, "cpu")


def test_tables_hold_the_inverse_and_the_permutation():
    p = torch.randperm(512, generator=torch.Generator().manual_seed(1))
    t = codec.hadamard_perm_tables(p.to(torch.int32), "cpu")
    assert t.n == 512 and t[:3] == (t.n, t.gather_in, t.gather_out)
    assert t.gather_in.dtype == t.gather_out.dtype == torch.int16 and t.gather_in.element_size() == 2
    q = t.gather_in.to(torch.int64)
    assert torch.equal(t.gather_out.to(torch.int64), p) and torch.equal(q[p], torch.arange(512)) and torch.equal(q, C.inverse_of(p))
    assert torch.equal(t.index_in.to(torch.int64), q) and torch.equal(t.index_out.to(torch.int64), p)
    big = codec.hadamard_perm_tables(torch.arange(16384).flip(0), "cpu")
    assert int(big.gather_out[0]) == 16383 and int(big.gather_in.to(torch.int64).max()) == 16383  # 14 bits: no sign trouble
    with pytest.raises(ValueError, match="wrong|entries"):  # a wrong length for the rotation
        codec.hadamard_transform(torch.zeros(2, 64, dtype=torch.bfloat16), 64, perm=codec.hadamard_perm_tables(torch.arange(32), "cpu"))
    with pytest.raises(ValueError):
        codec.hadamard_k_transform(torch.zeros(2, 64, dtype=torch.bfloat16), 64, None, None, perm=codec.hadamard_perm_tables(torch.arange(128), "cpu"))
    with pytest.raises(ValueError):
        transform.HadamardTransform(64, cta.TransformScheme("hadamard"), cta.TransformArgs("x", "input"), perm=torch.arange(32))
    with pytest.raises(ValueError):
        transform.HadamardTransform(4, cta.TransformScheme("hadamard"), cta.TransformArgs("x", "input"), perm=torch.tensor([0, 1, 1, 3]))


# ---- plan_hadamard_perm --------------------------------------------------------------------------------------------------------------------
ALL_ON = dict.fromkeys(codec.HADAMARD_PERM_MEASURED_FASTER, True)
ALL_OFF = dict.fromkeys(codec.HADAMARD_PERM_MEASURED_FASTER, False)


def test_plan_raises_the_unpermuted_plans_errors_first():
    P = codec.plan_hadamard_perm
    with pytest.raises(ValueError, match=r"Cannot construct deterministic hadamard of size != 2\^n"):
        P((4, 12), torch.bfloat16, 12)
    with pytest.raises(ValueError, match="Cannot construct deterministic hadamard of size <= 0"):
        P((4, 8), torch.bfloat16, 0)
    with pytest.raises(ValueError, match="64 must divide 96"):
        P((4, 96), torch.bfloat16, 64)
    with pytest.raises(ValueError, match="Cannot construct random hadamard matrix of size 100"):
        P((4, 100), torch.bfloat16, 100, k=3)
    for kw in (dict(device_type="cpu"), dict(contiguous=False), dict(precision=torch.bfloat16)):
        with pytest.raises(NotImplementedError):
            P((4, 64), torch.bfloat16, 64, **kw)
    with pytest.raises(NotImplementedError):
        P((2, 32768), torch.bfloat16, 32768)  # the unpermuted plan declines it: no composition either
    with pytest.raises(NotImplementedError):
        P((2, 64, 8), torch.bfloat16, 64, dim=1)
    with pytest.raises(ValueError, match="form"):
        P((4, 64), torch.bfloat16, 64, form="both")


def test_plan_forms_keys_and_launches(monkeypatch):
    P = codec.plan_hadamard_perm
    monkeypatch.setattr(codec, "HADAMARD_PERM_MEASURED_FASTER", ALL_ON)
    rows = [((65, 1024), 128, -1, torch.float32, "group"), ((3, 2), 2, -1, torch.float32, "group"), ((3, 4096), 4096, -1, torch.float32, "block"),
            ((3, 16384), 16384, -1, torch.float32, "block"), ((24, 256), 256, -1, torch.float64, "group_f64"), ((3, 8192), 8192, -1, torch.float64, "block_f64"),
            ((512, 1), 128, 0, torch.float64, "group_f64")]
    for shape, n, dim, precision, key in rows:
        p = P(shape, torch.bfloat16, n, dim, precision)
        assert (p.form, p.key, p.reason, p.launches()) == ("fused", key, None, 1), (shape, n)
        c = P(shape, torch.bfloat16, n, dim, precision, form="composed")
        assert (c.form, c.key, c.launches()) == ("composed", key, 3)
    p = P((128, 256), torch.bfloat16, 128, 0, torch.float64)
    assert (p.form, p.key, p.launches()) == ("fused", "cols", 3) and P((128, 256), torch.bfloat16, 128, 0, torch.float64, form="composed").launches() == 5
    assert P((3, 128), torch.bfloat16, 128, random=True).form == "fused" and isinstance(P((3, 128), torch.bfloat16, 128, random=True).base, codec.HadamardKPlan)
    # the composition is the only form for K > 1, for float64 at 16384 and for whatever the unpermuted plan takes beyond the kernels
    for shape, n, k in (((3, 96), 96, 96), ((3, 1792), 1792, 224), ((3, 28672), 28672, 224)):
        p = P(shape, torch.bfloat16, n, k=k)
        assert (p.form, p.key) == ("composed", None) and "k =" in p.reason and p.launches() == (4 if n == 96 else 3)  # 96: the two-launch vector form inside
        with pytest.raises(NotImplementedError, match="no fused permuted launch"):
            P(shape, torch.bfloat16, n, k=k, form="fused")
    p = P((3, 16384), torch.bfloat16, 16384, precision=torch.float64)
    assert (p.form, p.key) == ("composed", None) and "16384" in p.reason
    # every key whose flag is off: composed, and says so; form="fused" still forces the launch
    monkeypatch.setattr(codec, "HADAMARD_PERM_MEASURED_FASTER", ALL_OFF)
    for shape, n, dim, precision, key in rows + [((128, 256), 128, 0, torch.float64, "cols")]:
        p = P(shape, torch.bfloat16, n, dim, precision)
        assert (p.form, p.key) == ("composed", key) and "HADAMARD_PERM_MEASURED_FASTER" in p.reason
        assert P(shape, torch.bfloat16, n, dim, precision, form="fused").form == "fused"


def test_as_shipped_every_dispatched_form_is_measured_faster():
    """a key of HADAMARD_PERM_MEASURED_FASTER is True only if every verdict of profiles/hadamard_perm_bench.jsonl that speaks for it
    says faster, by the rule of tools/rotated_bench.py; the file holds two runs of every row"""
    consts = codec.HADAMARD_PERM_MEASURED_FASTER
    assert set(consts) == {"group", "block", "group_f64", "block_f64", "cols"} and all(isinstance(v, bool) for v in consts.values())
    with open(os.path.join(ROOT, "profiles", "hadamard_perm_bench.jsonl")) as f:
        lines = [json.loads(line) for line in f if line.strip()]
    rows, verdicts = [r for r in lines if "row" in r], [v for v in lines if "verdict" in v]
    assert {v["verdict"] for v in verdicts} == {r["row"] for r in rows} and len(verdicts) >= 7
    for v in verdicts:
        mine = [r for r in rows if r["row"] == v["verdict"]]
        assert {r["run"] for r in mine} >= {0, 1} and all(r["key"] == v["key"] for r in mine)
        assert all(k in r for r in mine for k in ("fused_median_us", "composed_median_us", "unpermuted_median_us", "eager_median_us"))
        assert v["fused_worst_us"] == max(r["fused_median_us"] for r in mine) and v["composed_best_us"] == min(r["composed_median_us"] for r in mine)
        assert v["faster"] == (v["fused_worst_us"] + v["run_spread_us"] < v["composed_best_us"])
    for key, on in consts.items():
        if on:
            speaking = [v for v in verdicts if v["key"] == key]
            assert speaking and all(v["faster"] for v in speaking), (key, speaking)
    may = lines[-1]["HADAMARD_PERM_MEASURED_FASTER_may_be"]
    assert all(not on or may[key] for key, on in consts.items())


# ---- the modules ---------------------------------------------------------------------------------------------------------------------------
def test_the_modules_carry_perm_and_pass_the_tables(monkeypatch):
    calls = []
    monkeypatch.setattr(codec, "hadamard_transform", lambda x, size, **kw: calls.append(("h", kw)) or x)
    monkeypatch.setattr(codec, "hadamard_k_transform", lambda x, n, hk, s, **kw: calls.append(("k", kw)) or x)
    scheme, args = cta.TransformScheme("hadamard"), cta.TransformArgs("x", "input")
    p = torch.randperm(64, generator=torch.Generator().manual_seed(2))
    t = transform.HadamardTransform(64, scheme, args, perm=p)
    assert list(t.state_dict()) == ["perm"] and t.state_dict()["perm"].dtype == torch.int64 and torch.equal(t.perm, p)
    x = torch.zeros(2, 64, dtype=torch.bfloat16)
    t(x), t(x), t.right_inverse(x)  # W[p][:, p] is symmetric: the inverse is the forward
    tables = [kw["perm"] for _, kw in calls]
    assert len(tables) == 3 and tables[0] is tables[1] is tables[2] and tables[0].n == 64 and torch.equal(tables[0].gather_out.to(torch.int64), p)
    flipped = p.clone().flip(0)
    t.perm.copy_(flipped)  # written in place: the tables follow
    t(x)
    assert torch.equal(calls[-1][1]["perm"].gather_out.to(torch.int64), flipped)
    plain = transform.HadamardTransform(64, scheme, args)
    plain(x)
    assert "perm" not in calls[-1][1] and plain.perm is None and plain.perm_tables("cpu") is None and not plain.state_dict()
    f = transform.HadamardFactors(64, 1, 64, None, torch.ones(64, dtype=torch.int8))
    r = transform.RandomHadamardTransform(f, cta.TransformScheme("random-hadamard"), args, perm=p)
    r(x)
    assert calls[-1][0] == "k" and calls[-1][1]["perm"].n == 64 and list(r.state_dict()) == ["perm"] and "permuted=True" in repr(r)
    transform.RandomHadamardTransform(f, cta.TransformScheme("random-hadamard"), args)(x)
    assert "perm" not in calls[-1][1]


# ---- the fusions decline a permuted transform ----------------------------------------------------------------------------------------------
ONLINE = {"config_groups": {"v": {"type": "hadamard", "apply": [{"targets": ["Linear"], "location": "input", "inverse": False, "ignore": []}],
                                  "randomize": True, "requires_grad": False, "head_dim": 16, "precision": "torch.float32"}}}


def test_fuse_input_quantization_skips_permuted_transforms(monkeypatch):
    calls = []
    monkeypatch.setattr(codec, "hadamard_transform", lambda x, size, **kw: calls.append("rotate" if kw.get("perm") is not None else "plain") or x + 1)
    monkeypatch.setattr(dynamic, "rotated_fake_quantize", lambda x, size, args, gs=None, **kw: calls.append("fused") or (x + 1) * 2)
    monkeypatch.setattr(dynamic, "plan_rotated_dynamic", lambda *a, **k: type("P", (), {"fused": True})())
    m = torch.nn.Sequential(torch.nn.Linear(32, 8, bias=False))
    cta.apply_transform_config(m, cta.TransformConfig.from_dict(ONLINE), randomize=True, seed=0)
    lin = m[0]
    lin.quantization_scheme = cta.QuantizationScheme(targets=["Linear"], input_activations=cta.QuantizationArgs(num_bits=8, type="float", strategy="token", dynamic=True))
    lin.quantization_status = "frozen"
    assert transform.fuse_input_quantization(m) == []
    hook = lin.__dict__[tapply._INPUT_ROTATIONS][0]
    hook.fuse_quantization = True  # forced on: the hook itself still returns the rotate-only result
    x = torch.ones(2, 3, 32, dtype=torch.bfloat16)
    assert torch.equal(hook(lin, (x,)), x + 1) and calls == ["rotate"]


def test_fuse_attention_quantization_skips_permuted_transforms(monkeypatch):
    calls = []
    monkeypatch.setitem(codec.ATTN_ROTATED_MEASURED_FASTER, "single", True)
    monkeypatch.setitem(codec.ATTN_ROTATED_MEASURED_FASTER, "pair", True)
    monkeypatch.setattr(codec, "_attn_rot_fusable", lambda *a, **k: True)
    monkeypatch.setattr(codec, "_attn_rot_pair_fusable", lambda *a, **k: True)
    monkeypatch.setattr(codec, "hadamard_transform", lambda x, size, **kw: calls.append("rotate") or x + 1)
    monkeypatch.setattr(codec, "attn_rotated_fake_quantize", lambda x, size, s, z=None, **kw: calls.append("rot_qdq") or (x + 1) * 2)
    monkeypatch.setattr(codec, "attn_rotated_fake_quantize_pair", lambda k, v, size, *a, **kw: calls.append("rot_pair") or ((k + 1) * 2, v * 2))
    attn = torch.nn.Module()
    attn.quantization_scheme = cta.QuantizationScheme(targets=["A"], input_activations=cta.QuantizationArgs(num_bits=8, type="float", symmetric=True, strategy="attn_head"))
    for name in ("q_scale", "k_scale", "v_scale"):
        setattr(attn, name, torch.ones(2, 1, 1))
    scheme = cta.TransformScheme("hadamard", [cta.TransformArgs("A", "q_attn")], head_dim=16)
    rot = transform.HadamardTransform(16, scheme, scheme.apply[0], torch.nn.Module, perm=torch.arange(16).flip(0))
    q, k = tapply.QueryRotation(rot), tapply.KeyRotation(rot)
    assert not q.fusable() and not k.fusable()
    assert tapply.QueryRotation(transform.HadamardTransform(16, scheme, scheme.apply[0], torch.nn.Module)).fusable()
    # fuse_attention_quantization goes by fusable(): a module whose hooks are permuted is skipped
    owner = torch.nn.Module()
    q.handle = owner.register_forward_pre_hook(lambda *a: None)
    attn.__dict__[tapply._ATTN_ROTATIONS] = {"q": q}
    setattr(attn, tapply.IMPL_ATTR, owner)
    root = torch.nn.Module()
    root.attn = attn
    assert transform.fuse_attention_quantization(root) == [] and not q.fuse_quantization
    q.fuse_quantization = k.fuse_quantization = True  # forced on: rotate only
    x = torch.ones(1, 2, 3, 16)
    assert torch.equal(q(attn, x), x + 1)
    k2, v2 = k(attn, x, x * 3)
    assert torch.equal(k2, x + 1) and torch.equal(v2, x * 3) and calls == ["rotate", "rotate"]


# ---- install() and the C ABI surface ---------------------------------------------------------------------------------------------------------
def test_install_flag_needs_patch_transforms():
    import compressed_tensors_amd.install as ct_amd

    assert inspect.signature(ct_amd.install).parameters["patch_permuted_hadamard"].default is False
    with pytest.raises(ValueError, match="patch_permuted_hadamard=True needs patch_transforms=True"):
        ct_amd.install(patch_permuted_hadamard=True)
    assert ct_amd._TR_PERMUTED == [False]


@pytest.mark.skipif(not ref_import.available(), reason="upstream reference sources not present on this machine")
def test_install_flag_is_set_and_cleared():
    ref_import.import_reference()
    try:
        import compressed_tensors.transform.factory.hadamard as up_h
    except ImportError as e:
        pytest.skip(f"upstream's transform package does not import here: {e}")
    import compressed_tensors_amd.install as ct_amd

    orig = up_h.HadamardTransform.forward
    ct_amd.install(patch_transforms=True)
    try:
        assert ct_amd._TR_PERMUTED == [False]
        ct_amd.install(patch_transforms=True, patch_permuted_hadamard=True)
        assert ct_amd._TR_PERMUTED == [True] and up_h.HadamardTransform.forward is not orig
    finally:
        ct_amd.uninstall()
    assert ct_amd._TR_PERMUTED == [False] and up_h.HadamardTransform.forward is orig


def test_the_entries_are_declared():
    rows, cols = _lib._PROTOTYPES["ct_hadamard_perm_rows"], _lib._PROTOTYPES["ct_hadamard_perm_cols"]
    assert len(rows[0]) == 11 and len(cols[0]) == 13 and rows[1] is cols[1] is _lib._PROTOTYPES["ct_hadamard_rows"][1]
    with open(os.path.join(ROOT, "include", "ct_hip.h")) as f:
        header = f.read()
    assert "int ct_hadamard_perm_rows(const void* x, void* out, int dt, int64_t numel, int64_t n, int acc64, const void* gather_in," in header
    assert "int ct_hadamard_perm_cols(const void* x, void* out, void* workspace, int dt, int64_t rows, int64_t cols, int64_t n, int acc64," in header
    with open(os.path.join(ROOT, "compressed_tensors_amd", "csrc", "ct_hadamard_perm.hip")) as f:
        src = f.read()
    assert '#include "ct_hadamard.h"' in src and all(name in src for name in ("unit_stages", "lane_stages", "had_div8", "HadScale", "launch_transpose_words"))
    for name in ("hadamard_perm_tables", "plan_hadamard_perm", "HADAMARD_PERM_MEASURED_FASTER"):
        assert name in codec.__all__
    assert inspect.signature(codec.hadamard_transform).parameters["perm"].default is None
    assert inspect.signature(codec.hadamard_k_transform).parameters["perm"].default is None
