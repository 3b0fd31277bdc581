"""The strided q / k / v QDQ (csrc/ct_attn.hip) on the MI355X: against the reference's outputs on every fixture case
(tests/golden/attn*, tools/gen_golden_attn.py) with dtype, shape AND strides, against today's contiguous kernels on the same
values, the pair form against the two single calls, launch counts, no copies and no host synchronisation, and every bf16 bit
pattern against an eager restatement.  Every comparison is bit-exact (NaN payload and sign canonicalised)."""
import collections
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "attn_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
DEV = torch.device("cuda:0")
_GOLDEN = {}


def _golden_tensors():
    if not _GOLDEN:
        from safetensors.torch import load_file

        _GOLDEN.update(load_file(os.path.join(GOLDEN, "attn.safetensors")))
    return _GOLDEN


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


def _kw(r):
    k = C.KINDS[r["kind"]]
    return dict(num_bits=k["num_bits"], qtype=k["type"], strategy=C.strategy_of(r))


def _run(r, x, scale, zp):
    from compressed_tensors_amd import codec

    kw = _kw(r)
    if r["mode"] == "fake":
        return codec.attn_fake_quantize(x, scale, zp, **kw)
    q = codec.attn_quantize(x, scale, zp, dtype=C.quantized_dtype(r), **kw)
    if r["mode"] == "quantize":
        return q
    return codec.attn_dequantize(q, scale, zp, strategy=kw["strategy"])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and C.canonical_bytes(a) == C.canonical_bytes(b)


def _contiguous_kernels(mode, kw, x, scale, zp, shape, qdtype):
    """today's kernels on the same values, made contiguous: ct_fake_quantize{,_fp8} / ct_quantize{,_fp8} / ct_dequantize"""
    from compressed_tensors_amd import codec

    xc = x.contiguous()
    if kw["strategy"] == "tensor":
        layout = dict(strategy="tensor")
        old_x, old_s, old_z = xc, scale, zp
    else:  # one batch at a time, a head per row: the channel strategy on (H, S * D)
        layout = dict(strategy="channel")
        B, H, S, D = shape
        old_x, old_s, old_z = xc.reshape(B, H, S * D), scale.reshape(H, 1), (None if zp is None else zp.reshape(H, 1))
    old_kw = dict(num_bits=kw["num_bits"], qtype=kw["qtype"], **layout)

    def old(xb):
        if mode == "fake":
            return codec.fake_quantize_tensor(xb, old_s, old_z, **old_kw)
        q = codec.quantize_tensor(xb, old_s, old_z, dtype=qdtype, **old_kw)
        return q if mode == "quantize" else codec.dequantize_tensor(q, old_s, old_z, **layout)

    return old(old_x) if kw["strategy"] == "tensor" else torch.stack([old(old_x[b]) for b in range(old_x.shape[0])])


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_attn_qdq_matches_the_reference(key, counted):
    entry = MANIFEST[key]
    r = entry["recipe"]
    x = C.make_input(r, DEV)
    assert C.sha(x) == entry["x_sha256"] and list(x.stride()) == entry["x_strides"], "the recipe no longer synthesises the reference's input"
    scale, zp = C.make_qparams(r)
    scale, zp = scale.to(DEV), (None if zp is None else zp.to(DEV))
    before = x.clone()
    out = _run(r, x, scale, zp)
    torch.cuda.synchronize()
    want = entry["out"]
    assert str(out.dtype).replace("torch.", "") == want["dtype"], out.dtype
    assert list(out.shape) == want["shape"] and list(out.stride()) == want["strides"], (out.shape, out.stride(), want["strides"])
    assert C.sha(out) == want["sha256"], "the output differs from the reference"
    if entry["stored"]:
        ref = _golden_tensors()[f"{key}.out"]
        ref = ref.view(C.F8) if out.dtype == C.F8 else ref  # stored as bytes; compared as float8 (one canonical NaN)
        assert C.canonical_bytes(out) == C.canonical_bytes(ref), "the output differs from the stored reference"
    assert dict(counted) == {"ct_attn_qdq": 2 if r["mode"] == "dequantize" else 1}, counted
    assert C.canonical_bytes(x) == C.canonical_bytes(before), "the input was written"
    ref = _contiguous_kernels(r["mode"], _kw(r), x, scale, zp, C.logical_shape(r), C.quantized_dtype(r))
    assert _same(out.contiguous().reshape(ref.shape), ref), "the strided entry differs from the contiguous kernels"


# ---- the pair form -------------------------------------------------------------------------------------------------------------------
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


def _pair_inputs(kind):
    rk = C.normalise(dict(D=16, B=2, H=2, S=5, layout="transposed", dtypes="bf16/bf16", kind=kind, strategy="attn_head", mode="fake", salt=3))
    rv = C.normalise(dict(D=80, B=2, H=2, S=7, layout="fused_v", dtypes="bf16/bf16", kind=kind, strategy="attn_head", mode="fake", salt=4))
    k, v = C.make_input(rk, DEV), C.make_input(rv, DEV)
    (ks, kz), (vs, vz) = C.make_qparams(rk), C.make_qparams(rv)
    vs = vs * 1.5  # K and V carry different scales
    to = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    return rk, k, v, to(ks), to(vs.to(ks.dtype)), to(kz), to(vz)


@pytest.mark.parametrize("kind", ["fp8", "int8_zp"])
def test_pair_equals_the_two_single_calls_in_one_launch(kind, counted):
    from compressed_tensors_amd import codec

    rk, k, v, ks, vs, kz, vz = _pair_inputs(kind)
    kw = _kw(rk)
    want_k, want_v = codec.attn_fake_quantize(k, ks, kz, **kw), codec.attn_fake_quantize(v, vs, vz, **kw)
    counted.clear()
    got_k, got_v = codec.attn_fake_quantize_pair(k, v, ks, vs, kz, vz, **kw)
    torch.cuda.synchronize()
    assert dict(counted) == {"ct_attn_qdq": 1}, counted  # one C-ABI call ...
    assert _same(got_k, want_k) and _same(got_v, want_v)
    assert got_k.stride() == want_k.stride() and got_v.stride() == want_v.stride()
    kernels, _ = _kernels_of(lambda: codec.attn_fake_quantize_pair(k, v, ks, vs, kz, vz, **kw))
    assert len(kernels) == 1 and "attn_qdq" in kernels[0], kernels  # ... and one kernel launch


# ---- no copies, no synchronisation -------------------------------------------------------------------------------------------------------
def test_transposed_view_is_read_in_place():
    from compressed_tensors_amd import codec

    r = C.normalise(dict(D=128, B=2, H=8, S=33, layout="transposed", dtypes="bf16/bf16", kind="fp8", strategy="attn_head", mode="fake", salt=5))
    x = C.make_input(r, DEV)
    scale, _ = C.make_qparams(r)
    scale = scale.to(DEV)
    kw = _kw(r)
    for fn in (lambda: codec.attn_fake_quantize(x, scale, None, **kw),
               lambda: codec.attn_quantize(x, scale, None, dtype=C.F8, **kw),
               lambda: codec.attn_fake_quantize_pair(x, x, scale, scale, **kw)):
        kernels, ops = _kernels_of(fn)
        assert len(kernels) == 1 and "attn_qdq" in kernels[0], kernels
        # (every device activity is in `kernels`: an aten::contiguous / aten::clone / aten::copy_ would be a second one, or a Memcpy)
        assert not [o for o in ops if o in ("aten::clone", "aten::copy_", "aten::_to_copy")], ops
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
        out = out[0] if isinstance(out, tuple) else out
        assert out.stride() == x.stride()
    torch.cuda.synchronize()


# ---- every bf16 bit pattern ---------------------------------------------------------------------------------------------------------------
_eager = C.eager_fake_quantize


@pytest.mark.parametrize("kind", ["fp8", "int8", "int8_zp"])
def test_every_bf16_bit_pattern(kind):
    from compressed_tensors_amd import codec

    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(C.BF16)
    x = pats.reshape(2, 64, 4, 128).to(DEV).transpose(1, 2)  # (2, 4, 64, 128), strided as a Llama's states are
    r = dict(H=4, dtypes="bf16/bf16", kind=kind, strategy="attn_head")
    scale, zp = C.make_qparams(r)
    scale, zp = scale.to(DEV), (None if zp is None else zp.to(DEV))
    out = codec.attn_fake_quantize(x, scale, zp, **_kw(r))
    ref = _eager(x, scale, zp, kind)
    assert out.dtype == ref.dtype == C.BF16 and out.stride() == x.stride()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(out), nan)
    assert torch.equal(out[~nan].view(torch.int16), ref[~nan].view(torch.int16))


# ---- rows wider than the fixtures' 256 elements: several waves per row, a workgroup per row, the unit loop ----------------------------------
def _wide(shape, kind):
    x = C.wide_input(shape, C.BF16, DEV)
    r = dict(H=shape[1], dtypes="bf16/bf16", kind=kind, strategy="attn_head")
    scale, zp = C.make_qparams(r)
    return x, scale.to(DEV), (None if zp is None else zp.to(DEV)), _kw(r)


@pytest.mark.parametrize("kind", ["fp8", "int8_zp"])
@pytest.mark.parametrize("shape", C.WIDE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wide_rows_fake_quantize_like_eager_torch(shape, kind):
    from compressed_tensors_amd import codec

    x, scale, zp, kw = _wide(shape, kind)
    out = codec.attn_fake_quantize(x, scale, zp, **kw)
    ref = _eager(x, scale, zp, kind)
    assert torch.isfinite(ref).all()
    assert out.dtype == ref.dtype == C.BF16 and out.shape == ref.shape
    # (the stride of a size-1 dimension — H = 1 — is never multiplied by an index; torch's ops place it by rules of their own)
    assert [st for st, sz in zip(out.stride(), out.shape) if sz > 1] == [st for st, sz in zip(x.stride(), x.shape) if sz > 1]
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("shape", C.WIDE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wide_rows_quantize_and_dequantize_like_the_contiguous_kernels(shape):
    from compressed_tensors_amd import codec

    x, scale, zp, kw = _wide(shape, "int8_zp")
    q = codec.attn_quantize(x, scale, zp, dtype=torch.int8, **kw)
    back = codec.attn_dequantize(q, scale, zp, strategy=kw["strategy"])
    for mode, got in (("quantize", q), ("dequantize", back)):
        ref = _contiguous_kernels(mode, kw, x, scale, zp, shape, torch.int8)
        assert _same(got.contiguous().reshape(ref.shape), ref), f"{mode}: the strided entry differs from the contiguous kernels"
