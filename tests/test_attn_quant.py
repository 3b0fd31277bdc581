"""Host side of the attention q / k / v QDQ (codec.plan_attn_qdq, the ct_attn_qdq ABI, the modeling package's import hygiene, the
fixtures' recipes): everything here runs without a GPU."""
import inspect
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_cases as C  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "attn_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
TORCH_DT = {"bfloat16": C.BF16, "float16": C.F16, "float32": C.F32, "int8": torch.int8, "float8_e4m3fn": C.F8}


def _plan(x, scale_shape=(8, 1, 1), strategy="attn_head", **kw):
    from compressed_tensors_amd import codec

    return codec.plan_attn_qdq(x.shape, x.stride(), x.dtype, scale_shape, strategy, offset_bytes=(x.storage_offset() * x.element_size()) % 16, **kw)


def _recipe(layout, D=128, B=2, H=8, S=5, dtypes="bf16/bf16"):
    return C.normalise(dict(D=D, B=B, H=H, S=S, layout=layout, dtypes=dtypes, kind="fp8", strategy="attn_head", mode="fake", salt=1))


# ---- plan_attn_qdq ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", C.LAYOUTS)
@pytest.mark.parametrize("D", C.D_VALUES)
def test_plan_reads_every_fixture_layout_in_place(layout, D):
    r = _recipe(layout, D=D)
    x = C.make_input(r)
    p = _plan(x)
    assert p.in_place and p.reason is None
    assert (p.B, p.H, p.S, p.D) == C.logical_shape(r) and p.per_head
    # the strides the kernel reads are the tensor's own (a missing batch dimension: stride 0)
    want = tuple(x.stride()[:-1]) if x.ndim == 4 else (0,) + tuple(x.stride()[:-1])
    assert p.strides == want
    if layout == "expanded":
        assert p.strides[0] == 0
    # the vector form: whole 8-element units, and a 16-byte aligned base with strides that keep units aligned
    vector = D % 8 == 0 and layout != "misaligned"
    assert p.vector == vector, (layout, D, x.stride(), x.storage_offset())


def test_plan_vector_rule_follows_the_dtypes():
    from compressed_tensors_amd import codec

    # fp32: 8 elements are two 16-byte vectors; a base 8 bytes off a boundary is misaligned for them but fine for 1-byte codes
    assert codec.plan_attn_qdq((2, 4, 5, 64), (1280, 320, 64, 1), C.F32, (4, 1, 1), "attn_head").vector
    assert not codec.plan_attn_qdq((2, 4, 5, 64), (1280, 320, 64, 1), C.F32, (4, 1, 1), "attn_head", offset_bytes=8).vector
    assert codec.plan_attn_qdq((2, 4, 5, 64), (1280, 320, 64, 1), torch.int8, (4, 1, 1), "attn_head", out_dtype=C.BF16, offset_bytes=8).vector
    # a head stride that is not a whole number of units (bf16: 8 elements) breaks the alignment of every other head
    assert not codec.plan_attn_qdq((1, 4, 5, 64), (0, 324, 64, 1), C.BF16, (4, 1, 1), "attn_head").vector
    # ... unless that dimension has one entry: its stride is never used
    assert codec.plan_attn_qdq((1, 1, 5, 64), (0, 324, 64, 1), C.BF16, (1, 1, 1), "attn_head").vector
    # a dense permuted input keeps its strides in the output: a 1-byte input whose strides only suit bytes does not suit bf16 out
    assert not codec.plan_attn_qdq((2, 4, 5, 64), (1280, 320, 64, 1), torch.int8, (4, 1, 1), "attn_head", out_dtype=C.BF16, offset_bytes=4).vector


def test_plan_copies_what_the_kernel_does_not_read():
    x = torch.zeros(2, 8, 5, 128, dtype=C.BF16)
    assert not _plan(x.transpose(2, 3), scale_shape=(8, 1, 1)).in_place  # last stride != 1
    assert "stride" in _plan(x.transpose(2, 3)).reason
    overlapping = torch.zeros(4096, dtype=C.BF16).as_strided((2, 8, 5, 128), (64, 8, 128, 1))
    p = _plan(overlapping)
    assert not p.in_place and "overlaps" in p.reason
    # after the copy the kernel reads the dense tensor
    assert p.strides == (8 * 5 * 128, 5 * 128, 128) and p.vector
    # more than four dimensions: leading dimensions that are mutually contiguous fold into B
    five = torch.zeros(3, 2, 8, 5, 128, dtype=C.BF16)
    p = _plan(five)
    assert p.in_place and (p.B, p.H, p.S, p.D) == (6, 8, 5, 128) and p.strides == (8 * 5 * 128, 5 * 128, 128)
    p = _plan(five.transpose(2, 3), scale_shape=(5, 1, 1))
    assert p.in_place and (p.B, p.H, p.S) == (6, 5, 8)
    p = _plan(five.transpose(0, 1))
    assert not p.in_place and "fold" in p.reason and p.B == 6
    # fewer: (H, S, D) is one batch; the tensor strategy takes anything
    p = _plan(torch.zeros(8, 5, 128, dtype=C.BF16))
    assert p.in_place and (p.B, p.H, p.S, p.D) == (1, 8, 5, 128)
    p = _plan(torch.zeros(7, 24, dtype=C.BF16), scale_shape=(1,), strategy="tensor")
    assert p.in_place and (p.B, p.H, p.S, p.D) == (1, 1, 7, 24) and not p.per_head and p.vector
    assert not _plan(torch.zeros(2, 8, 5, 128, dtype=C.BF16), scale_shape=(), strategy="attn_head").per_head  # one element: index 0


def test_plan_raises_what_the_reference_raises():
    from compressed_tensors_amd import codec

    with pytest.raises(ValueError, match="Attention quant requires at least 3 observed dimensions"):
        _plan(torch.zeros(5, 128, dtype=C.BF16))
    with pytest.raises(RuntimeError, match=r"The size of tensor a \(8\) must match the size of tensor b \(3\) at non-singleton dimension 1"):
        _plan(torch.zeros(2, 8, 5, 128, dtype=C.BF16), scale_shape=(3, 1, 1))
    with pytest.raises(ValueError, match="single scale"):
        _plan(torch.zeros(2, 8, 5, 128, dtype=C.BF16), scale_shape=(8, 1, 1), strategy="tensor")
    with pytest.raises(NotImplementedError):
        _plan(torch.zeros(2, 8, 5, 128, dtype=C.BF16), strategy="channel")
    x, s = torch.zeros(2, 8, 5, 16, dtype=C.BF16), torch.ones(8, 1, 1, dtype=C.BF16)
    # FLOAT 4-bit and a global scale are left to upstream, before any device is asked for
    with pytest.raises(NotImplementedError, match="4-bit"):
        codec.attn_fake_quantize(x, s, None, num_bits=4, qtype="float")
    with pytest.raises(NotImplementedError, match="global scale"):
        codec.attn_fake_quantize(x, s, None, num_bits=8, qtype="float", global_scale=torch.ones(1))
    with pytest.raises(NotImplementedError, match="share"):
        codec.attn_fake_quantize_pair(x, x.float(), s, s, num_bits=8, qtype="float")


def test_the_layout_vocabulary_knows_attn_head():
    from compressed_tensors_amd import codec

    s = torch.ones(8, 1, 1)
    one_batch = codec.QuantLayout((1, 8, 5, 128), s, "attn_head")
    assert (one_batch.rows, one_batch.cols, one_batch.rdiv, one_batch.cdiv, one_batch.scale_cols, one_batch.heads) == (40, 128, 5, 128, 1, 8)
    assert codec.QuantLayout((8, 5, 128), s, "attn_head").rdiv == 5
    assert codec.QuantLayout((2, 8, 5, 128), torch.ones(1), "attn_head").rdiv == 80
    several = codec.QuantLayout((2, 8, 5, 128), s, "attn_head")  # (row // S) % H is not a (row // rdiv) layout
    with pytest.raises(NotImplementedError, match="attn_fake_quantize"):
        several.args(torch.device("cpu"))
    with pytest.raises(ValueError, match="at least 3"):
        codec.QuantLayout((5, 128), s, "attn_head")
    with pytest.raises(ValueError, match="8 heads"):
        codec.QuantLayout((2, 8, 5, 128), torch.ones(3, 1, 1), "attn_head")
    # without args a 3-D scale still infers nothing, as upstream
    with pytest.raises(ValueError, match="Could not infer a quantization strategy"):
        codec.infer_dequant_layout((2, 8, 5, 128), s)


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------
def test_the_case_matrix():
    cases = C.case_list()
    assert sorted(k for k, _ in cases) == sorted(MANIFEST) and 100 <= len(cases) <= 400
    for name, values in C.FACTORS.items():  # every value of every factor occurs
        assert {r[name] for _, r in cases} == set(values), name
    for a, b in (("layout", "D"), ("layout", "mode"), ("dtypes", "kind"), ("strategy", "mode"), ("kind", "mode"), ("H", "S"), ("layout", "dtypes")):
        want = {(va, vb) for va in C.FACTORS[a] for vb in C.FACTORS[b]}
        assert {(r[a], r[b]) for _, r in cases} == want, (a, b)


def test_manifest_inputs_still_synthesise():
    for key, entry in MANIFEST.items():
        x = C.make_input(entry["recipe"])
        assert C.sha(x) == entry["x_sha256"], key
        assert list(x.stride()) == entry["x_strides"], key


def test_output_strides_are_the_references():
    """the strides the wrappers allocate (asked of torch on meta tensors) against the strides the reference's CPU run left"""
    from compressed_tensors_amd import codec

    for key, entry in MANIFEST.items():
        r = entry["recipe"]
        x = C.make_input(r)
        scale, _ = C.make_qparams(r)
        rounds = C.KINDS[r["kind"]]["type"] == "int"
        sargs = (tuple(scale.shape), tuple(scale.stride()), scale.dtype)
        if r["mode"] == "dequantize":  # its input is the quantize result
            st = codec._attn_out_strides(tuple(x.shape), tuple(x.stride()), x.dtype, *sargs, "quantize", rounds)
            x = torch.empty_strided(x.shape, st, dtype=C.quantized_dtype(r))
        st = codec._attn_out_strides(tuple(x.shape), tuple(x.stride()), x.dtype, *sargs, r["mode"], rounds)
        assert list(st) == entry["out"]["strides"], key
        if codec._attn_is_dense(x.shape, x.stride()) and 1 not in x.shape:  # the wrappers' shortcut
            assert list(torch.empty_like(x).stride()) == entry["out"]["strides"], key


def test_golden_files_are_small():
    for name in ("attn_manifest.json", "attn.safetensors"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < 512 * 1024, name


# ---- ABI, imports, wiring ------------------------------------------------------------------------------------------------------------
def test_abi_symbol_is_declared_and_bound():
    import ctypes

    from compressed_tensors_amd import _lib

    argtypes, restype = _lib._PROTOTYPES["ct_attn_qdq"]
    assert len(argtypes) == 11 and restype is ctypes.c_int
    with open(os.path.join(ROOT, "include", "ct_hip.h")) as f:
        header = f.read()
    assert "int ct_attn_qdq(const ct_attn_tensor* tensors, int n, int mode, int kind, int bits, int xdt, int sdt, int zdt, int tdt, int odt," in header
    assert "} ct_attn_tensor;" in header
    assert ctypes.sizeof(_lib.AttnTensor) == 15 * 8  # "15 64-bit words"
    assert [f[0] for f in _lib.AttnTensor._fields_] == ["x", "out", "scale", "zp", "B", "H", "S", "D", "x_stride", "out_stride", "per_head"]
    with open(os.path.join(ROOT, "compressed_tensors_amd", "csrc", "ct_attn.hip")) as f:
        assert 'extern "C" int ct_attn_qdq(' in f.read()


def test_importing_the_package_does_not_import_transformers():
    code = ("import sys; import compressed_tensors_amd, compressed_tensors_amd.modeling as m; "
            "assert 'transformers' not in sys.modules, 'transformers was imported'; "
            "print(sorted(m.__all__))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    for name in ("QuantizedKVCache", "QuantizedAttentionImpl", "initialize_hooked_kv_cache", "initialize_hooked_attention", "register_query_hook",
                 "register_key_hook", "register_value_hook", "KV_CACHE_ATTR", "IMPL_ATTR"):
        assert name in r.stdout, name


def test_modeling_surface():
    from compressed_tensors_amd import modeling
    from compressed_tensors_amd.modeling import kvcache

    assert modeling.KV_CACHE_ATTR == "kv_cache" and modeling.IMPL_ATTR == "impl"
    assert isinstance(kvcache.PAIR_MEASURED_FASTER, bool)
    attn = torch.nn.Module()
    cache = modeling.QuantizedKVCache(config=None, attn_module=attn)
    k, v = torch.zeros(1, 2, 3, 4), torch.ones(1, 2, 3, 4)
    got = cache.update(k, v, 0)  # no scheme, no wrapped cache: the states come back as they are
    assert got[0] is k and got[1] is v

    class Wrapped:
        def update(self, key_states, value_states, layer_idx, cache_kwargs=None):
            return key_states + 1, value_states + layer_idx

    w = Wrapped()
    cache.add_past_key_values(w)
    out = cache.update(k, v, 3)
    assert torch.equal(out[0], k + 1) and torch.equal(out[1], v + 3) and cache.past_key_values is None  # one forward per hand-over
    attn.kv_cache = cache
    seen = []
    h1 = modeling.register_key_hook(attn, lambda m, ks: seen.append(("k", m is attn)) or ks + 10)
    h2 = modeling.register_value_hook(attn, lambda m, vs: seen.append(("v", m is attn)))
    out = cache.update(k, v, 0)
    assert seen == [("k", True), ("v", True)] and torch.equal(out[0], k + 10) and out[1] is v
    h1.remove(), h2.remove()
    assert cache.update(k, v, 0)[0] is k


def test_attention_locations_need_a_pretrained_model():
    import compressed_tensors_amd as cta
    from compressed_tensors_amd.transform.apply import AttentionHookError

    m = torch.nn.Sequential(torch.nn.Linear(16, 16))
    for location in ("q_attn", "k_cache"):
        cfg = cta.TransformConfig({"r": cta.TransformScheme("hadamard", [cta.TransformArgs("Linear", location)], head_dim=16)})
        with pytest.raises(ValueError, match="Cannot hook attention of model"):
            cta.apply_transform_config(m, cfg)
        assert not hasattr(m, "transform_config")
    assert issubclass(AttentionHookError, ValueError) and issubclass(AttentionHookError, NotImplementedError)


def test_install_keywords():
    import compressed_tensors_amd.install as ct_amd

    sig = inspect.signature(ct_amd.install)
    assert sig.parameters["patch_modeling"].default is False
    assert all(p.default in (True, False) for p in sig.parameters.values())
