"""The head-dim Hadamard rotation in the launch of the attention q / k / v QDQ (csrc/ct_attn_rot.hip) on the MI355X: the fused
launch against the composition of the existing launches bit for bit (dtype, shape, strides, the sign of zeros; NaNs canonicalised),
the pair form, one launch and no copy, the reference's outputs on the fixtures of tools/gen_golden_attn_rotated.py by value, a 2-layer
Llama under transform.fuse_attention_quantization, and graph capture."""
import collections
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_cases as A  # noqa: E402
import _attn_rotated_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "attn_rotated_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
_GOLDEN = {}


def _golden_tensors():
    if not _GOLDEN:
        from safetensors.torch import load_file

        _GOLDEN.update(load_file(os.path.join(GOLDEN, "attn_rotated.safetensors")))
    return _GOLDEN


@pytest.fixture(autouse=True)
def _seeded():
    torch.manual_seed(1234)


@pytest.fixture()
def counted():
    from compressed_tensors_amd import _lib

    counts = collections.Counter()
    orig = _lib.call

    def call(name, *a):
        counts[name] += 1
        return orig(name, *a)

    _lib.call = call
    import compressed_tensors_amd.codec as codec_mod

    saved = codec_mod.call
    codec_mod.call = call
    try:
        yield counts
    finally:
        _lib.call = orig
        codec_mod.call = saved


def _same(a, b):
    """bit for bit (the sign of a zero included), NaNs canonicalised; dtype, shape and strides too"""
    return a.dtype == b.dtype and a.shape == b.shape and a.stride() == b.stride() and A.canonical_bytes(a) == A.canonical_bytes(b)


def _diff(a, b):
    """a short description of where two results differ, for the assertion message"""
    if a.dtype != b.dtype or a.shape != b.shape or a.stride() != b.stride():
        return f"{a.dtype} {tuple(a.shape)} {a.stride()} against {b.dtype} {tuple(b.shape)} {b.stride()}"
    wa = a.contiguous().view(torch.uint8).reshape(-1).cpu().to(torch.int32)
    wb = b.contiguous().view(torch.uint8).reshape(-1).cpu().to(torch.int32)
    idx = (wa != wb).nonzero().reshape(-1)
    return f"{idx.numel()} of {wa.numel()} bytes differ, first at {idx[:8].tolist()}: {wa[idx[:8]].tolist()} against {wb[idx[:8]].tolist()}"


def _qparams(kind, strategy, H, x_dtype, scale_dtype=None):
    name = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}[scale_dtype or x_dtype]
    r = dict(H=H, dtypes=f"bf16/{name}", kind=kind, strategy=strategy)
    scale, zp = A.make_qparams(r)
    return scale.to(DEV), (None if zp is None else zp.to(DEV))


def _call(mode, x, n, scale, zp, kind, strategy, fused):
    from compressed_tensors_amd import codec

    k = C.KINDS[kind]
    kw = dict(num_bits=k["num_bits"], qtype=k["type"], strategy=strategy, fused=fused)
    if mode == "fake":
        return codec.attn_rotated_fake_quantize(x, n, scale, zp, **kw)
    return codec.attn_rotated_quantize(x, n, scale, zp, dtype=F8 if k["type"] == "float" else torch.int8, **kw)


F8 = C.F8


# ---- fused == composition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.identity_cases(), ids=C.identity_id)
def test_fused_equals_the_composition(case, counted):
    x = C.identity_input(case, DEV, seed=len(C.identity_id(case)))
    D, n = case["dn"]
    scale, zp = _qparams(case["kind"], case["strategy"], x.shape[1], x.dtype)
    before = x.clone()
    want = _call(case["mode"], x, n, scale, zp, case["kind"], case["strategy"], fused=False)
    assert counted["ct_hadamard_rows"] == 1 and counted["ct_attn_qdq"] == 1 and "ct_attn_rot_qdq" not in counted, counted
    counted.clear()
    got = _call(case["mode"], x, n, scale, zp, case["kind"], case["strategy"], fused=True)
    torch.cuda.synchronize()
    assert dict(counted) == {"ct_attn_rot_qdq": 1}, counted
    assert _same(got, want), "the fused launch differs from the composition: " + _diff(got, want)
    assert A.canonical_bytes(x) == A.canonical_bytes(before), "the input was written"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("dn", [(128, 128), (64, 8), (384, 128), (16, 2)])
def test_special_values_rotate_and_quantize_alike(dn, dtype):
    """subnormals, +-0, +-inf, NaN and a constant row: the range test of the quotient (had_div8) and the exchanges see them all"""
    D, n = dn
    x = C.place(C.special_values(D, dtype).to(DEV), "transposed")
    for kind in ("fp8", "int8_zp"):
        scale, zp = _qparams(kind, "attn_head", 2, dtype)
        for mode in ("fake", "quantize"):
            want = _call(mode, x, n, scale, zp, kind, "attn_head", fused=False)
            got = _call(mode, x, n, scale, zp, kind, "attn_head", fused=True)
            assert _same(got, want), (kind, mode)


@pytest.mark.parametrize("kind", ["fp8", "int8_zp"])
@pytest.mark.parametrize("shape_n", [((1, 2, 3, 1024), 128), ((1, 1, 3, 2048), 512)], ids=["1x2x3x1024-n128", "1x1x3x2048-n512"])
def test_wide_rows_equal_the_rotation_kernel_then_eager_torch(shape_n, kind, counted):
    """rows of two waves and of a whole workgroup: the untouched rotation kernel, then torch's own arithmetic"""
    from compressed_tensors_amd import codec

    shape, n = shape_n
    x = A.wide_input(shape, BF16, DEV)
    scale, zp = _qparams(kind, "attn_head", shape[1], BF16)
    want = A.eager_fake_quantize(codec.hadamard_transform(x.contiguous(), n), scale, zp, kind)
    assert torch.isfinite(want).all()
    counted.clear()
    got = _call("fake", x, n, scale, zp, kind, "attn_head", fused=True)
    torch.cuda.synchronize()
    assert dict(counted) == {"ct_attn_rot_qdq": 1}, counted
    assert got.dtype == want.dtype == BF16 and got.shape == want.shape
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_mixed_dtypes_and_a_0_dim_scale():
    x = C.identity_input(dict(dn=(128, 32), layout="fused_k", dtype="bf16", shape="tail", scale=1.0), DEV, 7)
    for sdt in (torch.float32, torch.bfloat16):
        scale, zp = _qparams("int8_zp", "attn_head", 2, x.dtype, sdt)
        assert _same(_call("fake", x, 32, scale, zp, "int8_zp", "attn_head", True), _call("fake", x, 32, scale, zp, "int8_zp", "attn_head", False))
    one = torch.tensor(0.0078, dtype=BF16, device=DEV)
    assert _same(_call("fake", x, 32, one, None, "fp8", "tensor", True), _call("fake", x, 32, one, None, "fp8", "tensor", False))


def test_what_the_launch_declines_is_the_composition(counted):
    """fused=True is a wish: a shape outside the plan runs the existing launches, with the same result as fused=False"""
    from compressed_tensors_amd import codec

    scale, _ = _qparams("fp8", "attn_head", 3, BF16)
    for x, n in ((torch.randn(2, 5, 3, 20, device=DEV).to(BF16).transpose(1, 2), 4),  # D % 8
                 (torch.randn(1, 2, 3, 1024, device=DEV).to(BF16).transpose(1, 2), 1024),  # n > 512
                 (torch.randn(2 * 5 * 3 * 64 + 1, device=DEV).to(BF16)[1:].view(2, 5, 3, 64).transpose(1, 2), 64)):  # misaligned
        counted.clear()
        got = codec.attn_rotated_fake_quantize(x, n, scale, None, num_bits=8, qtype="float", fused=True)
        assert "ct_attn_rot_qdq" not in counted and counted["ct_hadamard_rows"] == 1, counted
        assert _same(got, codec.attn_rotated_fake_quantize(x, n, scale, None, num_bits=8, qtype="float", fused=False))
    with pytest.raises(ValueError, match="2\\^n"):
        codec.attn_rotated_fake_quantize(torch.zeros(1, 3, 2, 24, device=DEV, dtype=BF16), 12, scale, None, num_bits=8, qtype="float", fused=True)
    with pytest.raises(ValueError, match="must divide"):
        codec.attn_rotated_fake_quantize(torch.zeros(1, 3, 2, 24, device=DEV, dtype=BF16), 16, scale, None, num_bits=8, qtype="float", fused=True)


def test_the_c_entry_rejects_what_it_does_not_serve():
    from compressed_tensors_amd import _lib

    x = torch.zeros(1, 2, 3, 64, device=DEV, dtype=BF16)
    out, scale = torch.empty_like(x), torch.ones(2, dtype=BF16, device=DEV)
    d = (_lib.AttnTensor * 1)()
    d[0].x, d[0].out, d[0].scale, d[0].zp, d[0].B, d[0].H, d[0].S, d[0].D = x.data_ptr(), out.data_ptr(), scale.data_ptr(), None, 1, 2, 3, 64
    d[0].x_stride[:], d[0].out_stride[:], d[0].per_head = (384, 192, 64), (384, 192, 64), 1
    bf = _lib.DT[BF16]
    s = _lib.stream_on(DEV)
    with pytest.raises(ValueError, match="mode"):  # dequantize
        _lib.call("ct_attn_rot_qdq", d, 1, 64, 1, 2, 1, 8, bf, bf, -1, bf, bf, s)
    with pytest.raises(ValueError, match="2\\^n"):
        _lib.call("ct_attn_rot_qdq", d, 1, 48, 1, 0, 1, 8, bf, bf, -1, bf, bf, s)
    with pytest.raises(NotImplementedError, match="2 .. 512"):
        _lib.call("ct_attn_rot_qdq", d, 1, 1024, 1, 0, 1, 8, bf, bf, -1, bf, bf, s)
    with pytest.raises(NotImplementedError, match="does not divide"):
        _lib.call("ct_attn_rot_qdq", d, 1, 128, 1, 0, 1, 8, bf, bf, -1, bf, bf, s)
    d[0].x = x.data_ptr() + 2
    with pytest.raises(NotImplementedError, match="aligned"):
        _lib.call("ct_attn_rot_qdq", d, 1, 64, 1, 0, 1, 8, bf, bf, -1, bf, bf, s)
    assert _lib.load().ct_abi_version() == 2


# ---- the pair -------------------------------------------------------------------------------------------------------------------------------
def _kernels_of(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    events = list(prof.events())
    kernels = [e.name for e in events if e.device_type == torch.autograd.DeviceType.CUDA]
    ops = [e.name for e in events if e.device_type == torch.autograd.DeviceType.CPU]
    return kernels, ops


@pytest.mark.parametrize("kind", ["fp8", "int8_zp"])
@pytest.mark.parametrize("dims", [(128, 128, 128), (128, 64, 64), (64, 384, 16)])  # (K's D, V's D, n): MLA-style different head dims
def test_pair_rotates_k_only_in_one_launch(dims, kind, counted):
    from compressed_tensors_amd import codec

    Dk, Dv, n = dims
    k = torch.randn(2, 7, 3, Dk, device=DEV).to(BF16).transpose(1, 2)
    v = torch.randn(2, 7, 3, Dv, device=DEV).to(BF16).transpose(1, 2)
    ks, kz = _qparams(kind, "attn_head", 3, BF16)
    vs = (ks.float() * 1.5).to(BF16)
    q = C.KINDS[kind]
    kw = dict(num_bits=q["num_bits"], qtype=q["type"], strategy="attn_head")
    want_k, want_v = codec.attn_fake_quantize_pair(codec.hadamard_transform(k.contiguous(), n), v, ks, vs, kz, kz, **kw)
    counted.clear()
    got_k, got_v = codec.attn_rotated_fake_quantize_pair(k, v, n, ks, vs, kz, kz, fused=True, **kw)
    torch.cuda.synchronize()
    assert dict(counted) == {"ct_attn_rot_qdq": 1}, counted
    assert _same(got_k, want_k) and _same(got_v, want_v)
    assert got_k.is_contiguous() and got_v.stride() == v.stride()
    # V is NOT rotated: it is what the unrotated QDQ gives
    assert _same(got_v, codec.attn_fake_quantize(v, vs, kz, **kw))
    counted.clear()
    off_k, off_v = codec.attn_rotated_fake_quantize_pair(k, v, n, ks, vs, kz, kz, fused=False, **kw)
    assert dict(counted) == {"ct_hadamard_rows": 1, "ct_attn_qdq": 1} and _same(off_k, want_k) and _same(off_v, want_v)


# ---- one launch, no copy -------------------------------------------------------------------------------------------------------------------
def test_transposed_view_is_rotated_and_quantized_in_one_launch():
    from compressed_tensors_amd import codec

    x = torch.randn(2, 33, 8, 128, device=DEV).to(BF16).transpose(1, 2)
    scale, _ = _qparams("fp8", "attn_head", 8, BF16)
    kw = dict(num_bits=8, qtype="float", strategy="attn_head", fused=True)
    for fn in (lambda: codec.attn_rotated_fake_quantize(x, 128, scale, None, **kw),
               lambda: codec.attn_rotated_quantize(x, 128, scale, None, dtype=F8, **kw),
               lambda: codec.attn_rotated_fake_quantize_pair(x, x, 128, scale, scale, **kw)):
        kernels, ops = _kernels_of(fn)
        assert len(kernels) == 1 and "attn_rot" in kernels[0], kernels  # exactly one device activity: no Memcpy, no copy kernel
        assert not [o for o in ops if o in ("aten::clone", "aten::copy_", "aten::_to_copy", "aten::contiguous")], ops
        torch.cuda.set_sync_debug_mode("error")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


# ---- against the reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_fused_matches_the_reference_by_value(key, counted):
    entry = MANIFEST[key]
    r = entry["recipe"]
    x = C.make_input(r, DEV)
    assert C.sha(x) == entry["x_sha256"] and list(x.stride()) == entry["x_strides"], "the recipe no longer synthesises the reference's input"
    scale, zp = C.make_qparams(r)
    scale, zp = scale.to(DEV), (None if zp is None else zp.to(DEV))
    out = _call(r["mode"], x, r["n"], scale, zp, r["kind"], A.strategy_of(r), fused=True)
    torch.cuda.synchronize()
    assert dict(counted) == {"ct_attn_rot_qdq": 1}, counted
    want = entry["out"]
    assert str(out.dtype).replace("torch.", "") == want["dtype"] and list(out.shape) == want["shape"]
    # the stride of a size-1 dimension is never multiplied by an index: the composition keeps the view's there (S = 1), the reference's GEMM does not
    assert [st for st, sz in zip(out.stride(), out.shape) if sz > 1] == [st for st, sz in zip(want["strides"], want["shape"]) if sz > 1]
    assert C.sha(out) == want["sha256"], "the output differs from the reference"
    if entry["stored"]:
        ref = _golden_tensors()[f"{key}.out"]
        ref = ref.view(F8) if out.dtype == F8 else ref
        assert C.equal_by_value(out, ref), "the output differs from the stored reference"


# ---- a 2-layer Llama -----------------------------------------------------------------------------------------------------------------------
LAYERS, HEADS, KV_HEADS, HEAD_DIM = 2, 4, 2, 16


def _model(attn_implementation=None, seed=0):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                      num_key_value_heads=KV_HEADS, head_dim=HEAD_DIM, max_position_embeddings=64)
    m = LlamaForCausalLM(cfg).to(BF16).to(DEV).eval()
    if attn_implementation is not None:
        m.set_attn_implementation(attn_implementation)
    return m


def _ids():
    return (torch.arange(10, device=DEV).reshape(2, 5) * 7 + 3) % 64


def _attentions(m):
    return [mod for name, mod in m.named_modules() if name.endswith("self_attn")]


def _rotated_quantized_model(impl):
    import compressed_tensors_amd as cta

    m = _model(impl)
    cfg = cta.TransformConfig({"r": cta.TransformScheme("hadamard", [cta.TransformArgs("LlamaAttention", "q_attn"), cta.TransformArgs("LlamaAttention", "k_cache")],
                                                        head_dim=HEAD_DIM)})
    cta.apply_transform_config(m, cfg)
    args = cta.QuantizationArgs(num_bits=8, type="float", symmetric=True, strategy="attn_head")
    for layer, attn in enumerate(_attentions(m)):
        attn.quantization_scheme = cta.QuantizationScheme(targets=["LlamaAttention"], input_activations=args)
        for name, heads, base in (("q_scale", HEADS, 0.011), ("k_scale", KV_HEADS, 0.017), ("v_scale", KV_HEADS, 0.007)):
            value = (base * (layer + 1) * (1.0 + 0.5 * torch.arange(heads, dtype=torch.float32))).to(BF16).reshape(heads, 1, 1).to(DEV)
            attn.register_parameter(name, torch.nn.Parameter(value, requires_grad=False))
    return m


@pytest.fixture()
def dispatched(monkeypatch):
    """the fused launches dispatched, whatever ROTATED_MEASURED_FASTER ships (tests/test_attn_rotated.py holds that to the measurement)"""
    from compressed_tensors_amd import codec

    monkeypatch.setitem(codec.ATTN_ROTATED_MEASURED_FASTER, "single", True)
    monkeypatch.setitem(codec.ATTN_ROTATED_MEASURED_FASTER, "pair", True)


@pytest.mark.parametrize("impl", ["sdpa", "eager"])
def test_llama_logits_under_fuse_attention_quantization(impl, counted, dispatched):
    from compressed_tensors_amd import modeling, transform

    ids = _ids()
    plain = _rotated_quantized_model(impl)
    counted.clear()
    with torch.no_grad():
        want = plain(ids).logits
    qdq = 1 + (1 if modeling.PAIR_MEASURED_FASTER else 2)  # q; K + V: one launch (pair) or two
    assert counted["ct_hadamard_rows"] == 2 * LAYERS and counted["ct_attn_qdq"] == qdq * LAYERS and "ct_attn_rot_qdq" not in counted, counted
    m = _rotated_quantized_model(impl)
    names = transform.fuse_attention_quantization(m)
    assert names == [f"model.layers.{i}.self_attn" for i in range(LAYERS)]
    counted.clear()
    with torch.no_grad():
        got = m(ids).logits
    assert dict(counted) == {"ct_attn_rot_qdq": 2 * LAYERS}, counted  # per layer: one for q, one for k + v; no rotation, no plain QDQ
    assert torch.equal(got, want) and torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert all(not any(k.startswith("_ct_prequantized") for k in attn.__dict__) for attn in _attentions(m))  # every hand-off was taken
    # quantization disabled: the hooks rotate only
    for mod in _attentions(m) + _attentions(plain):
        mod.quantization_enabled = False
    counted.clear()
    with torch.no_grad():
        off, off_want = m(ids).logits, plain(ids).logits
    assert dict(counted) == {"ct_hadamard_rows": 4 * LAYERS}, counted
    assert torch.equal(off.view(torch.int16), off_want.view(torch.int16))
    for mod in _attentions(m) + _attentions(plain):
        mod.quantization_enabled = True
    # a hook registered after the opt-in that REPLACES K: the replacement is not the remembered tensor and is quantized as always
    for mod in _attentions(m):
        modeling.register_key_hook(mod, lambda _mod, k: k * 0.5)
    counted.clear()
    with torch.no_grad():
        got2 = m(ids).logits
    assert dict(counted) == {"ct_attn_rot_qdq": 2 * LAYERS, "ct_attn_qdq": LAYERS}, counted  # K again, on the ordinary path; V was handed off
    # (the same model without the opt-in quantizes 0.5 * rotated K: a different computation — the precondition the opt-in documents)
    assert torch.isfinite(got2).all()


def test_without_the_dispatch_constants_the_opt_in_changes_no_launch(counted, monkeypatch):
    from compressed_tensors_amd import codec, transform

    monkeypatch.setitem(codec.ATTN_ROTATED_MEASURED_FASTER, "single", False)
    monkeypatch.setitem(codec.ATTN_ROTATED_MEASURED_FASTER, "pair", False)
    m = _rotated_quantized_model("sdpa")
    with torch.no_grad():
        want = m(_ids()).logits
    transform.fuse_attention_quantization(m)
    counted.clear()
    with torch.no_grad():
        got = m(_ids()).logits
    assert "ct_attn_rot_qdq" not in counted and counted["ct_hadamard_rows"] == 2 * LAYERS, counted
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


# ---- graph capture -------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_to_the_same_bytes():
    from compressed_tensors_amd import codec

    x = torch.randn(2, 9, 4, 128, device=DEV).to(BF16).transpose(1, 2)
    v = torch.randn(2, 9, 4, 64, device=DEV).to(BF16).transpose(1, 2)
    scale, _ = _qparams("fp8", "attn_head", 4, BF16)
    kw = dict(num_bits=8, qtype="float", strategy="attn_head", fused=True)
    want_q = codec.attn_rotated_fake_quantize(x, 128, scale, None, **kw)
    want_k, want_v = codec.attn_rotated_fake_quantize_pair(x, v, 64, scale, scale, **kw)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        codec.attn_rotated_fake_quantize(x, 128, scale, None, **kw)  # warm-up on the capture stream
        codec.attn_rotated_fake_quantize_pair(x, v, 64, scale, scale, **kw)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got_q = codec.attn_rotated_fake_quantize(x, 128, scale, None, **kw)
        got_k, got_v = codec.attn_rotated_fake_quantize_pair(x, v, 64, scale, scale, **kw)
    for t in (got_q, got_k, got_v):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(got_q, want_q) and _same(got_k, want_k) and _same(got_v, want_v)
