"""The strided min-max observer (csrc/ct_attn_observe.hip) on the MI355X: against the reference observer's results on every fixture
case (tests/golden/attn_observe*, tools/gen_golden_attn_observe.py), launch counts and no copies, the pair form against two single
calls, the running state against the union of two memoryless calls, extremes planted where the row loop and the last partial
workgroup read them, every finite bf16 bit pattern through the key map, and results written into module parameters.  Scale and
zero point are compared byte for byte (one canonical NaN); minima and maxima with torch.equal, NaNs at equal positions."""
import collections
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_observe_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "attn_observe_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
DEV = torch.device("cuda:0")
TORCH_DT = {"bfloat16": C.BF16, "float16": C.F16, "float32": C.F32, "int8": torch.int8, "float8_e4m3fn": C.F8}
_GOLDEN = {}
FP8 = dict(num_bits=8, qtype="float", symmetric=True)


def _golden(key, name):
    if not _GOLDEN:
        from safetensors.torch import load_file

        _GOLDEN.update(load_file(os.path.join(GOLDEN, "attn_observe.safetensors")))
    t = _GOLDEN[f"{key}.{name}"]
    return t.view(C.F8) if MANIFEST[key]["out"][name]["dtype"] == "float8_e4m3fn" else t


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


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and C.canonical_bytes(a) == C.canonical_bytes(b)


def _same_values(a, b):
    """torch.equal with NaNs at equal positions (-0.0 == +0.0: no quantization parameter can tell them apart)"""
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.isnan(a), nan) and torch.equal(a[~nan], b[~nan])


def _kw(r):
    k = C.KINDS[r["kind"]]
    return dict(num_bits=k["num_bits"], qtype=k["type"], symmetric=k["symmetric"], strategy=r["strategy"])


def _state(x, strategy="attn_head"):
    from compressed_tensors_amd import codec

    return codec.attn_observe_state(x.shape[-3] if strategy == "attn_head" else 1, x.device)


def _armed(state):
    return state.cpu().tolist() == [[0x7FFFFFFF] * state.shape[1], [-0x80000000] * state.shape[1]]


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_observer_matches_the_reference(key, counted):
    import compressed_tensors_amd as cta
    from compressed_tensors_amd.quantization import MinMaxObserver

    entry = MANIFEST[key]
    r = entry["recipe"]
    x = C.make_observed(r, DEV)
    assert C.sha(x) == entry["x_sha256"] and list(x.stride()) == entry["x_strides"], "the recipe no longer synthesises the reference's input"
    before = x.clone()
    observer = MinMaxObserver(r["base"], cta.QuantizationArgs(**C.args_of(r)), torch.nn.Module())
    counted.clear()
    scale, zero_point = observer(x)
    torch.cuda.synchronize()
    assert dict(counted) == {"ct_attn_observe": 1}, counted
    got = dict(scale=scale, zero_point=zero_point, min_vals=observer.min_vals, max_vals=observer.max_vals)
    for name, t in got.items():
        want = _golden(key, name)
        assert t.dtype == want.dtype == TORCH_DT[entry["out"][name]["dtype"]] and list(t.shape) == entry["out"][name]["shape"], (name, t.dtype, t.shape)
        print(name, t.flatten().tolist()[:8], want.flatten().tolist()[:8])
        if name in ("scale", "zero_point"):
            assert _same_bytes(t, want.to(DEV)), f"{name} differs from the reference"
        else:
            assert _same_values(t, want), f"{name} differs from the reference"
    assert C.canonical_bytes(x) == C.canonical_bytes(before), "the input was written"
    assert _armed(observer._state), "a memoryless call leaves the state armed"


# ---- launches, copies, synchronisation ---------------------------------------------------------------------------------------------
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


def _transposed(B, H, S, D, dtype=C.BF16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, H, D, generator=g).to(dtype).to(DEV).transpose(1, 2)


def test_a_transposed_view_is_observed_in_place_in_two_launches(counted):
    from compressed_tensors_amd import codec

    k, v = _transposed(2, 8, 33, 128), _transposed(2, 8, 33, 64, seed=1)
    ks, vs = _state(k), _state(v)
    counted.clear()
    codec.attn_observe(k, ks, **FP8)
    assert dict(counted) == {"ct_attn_observe": 1}, counted  # and nothing else: no fill, no copy
    counted.clear()
    codec.attn_observe_pair(k, v, ks, vs, **FP8)
    assert dict(counted) == {"ct_attn_observe": 1}, counted  # one call for a pair
    for fn in (lambda: codec.attn_observe(k, ks, **FP8), lambda: codec.attn_observe_pair(k, v, ks, vs, **FP8),
               lambda: codec.attn_observe(k, ks, keep=True, **FP8)):
        kernels, ops = _kernels_of(fn)
        assert len(kernels) == 2 and sum("attn_observe_fold" in k for k in kernels) == sum("attn_observe_finalize" in k for k in kernels) == 1, kernels
        # (every device activity is in `kernels`: a `.contiguous()`, a fill of the state or a Memcpy would be a third)
        assert not [o for o in ops if o in ("aten::clone", "aten::copy_", "aten::_to_copy", "aten::contiguous", "aten::fill_")], ops
        torch.cuda.set_sync_debug_mode("error")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


# ---- the pair form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fp8", "int8_zp"])
def test_pair_equals_the_two_single_calls(kind):
    from compressed_tensors_amd import codec

    k, v = _transposed(2, 8, 5, 64, seed=2), _transposed(2, 4, 7, 128, seed=3) * 3  # K and V: their own heads, rows and head dims
    kw = dict(_kw(dict(kind=kind, strategy="attn_head")), want_minmax=True)
    want_k, want_v = codec.attn_observe(k, _state(k), **kw), codec.attn_observe(v, _state(v), **kw)
    ks, vs = _state(k), _state(v)
    got_k, got_v = codec.attn_observe_pair(k, v, ks, vs, **kw)
    for got, want in ((got_k, want_k), (got_v, want_v)):
        assert len(got) == len(want) == 4 and all(_same_bytes(a, b) for a, b in zip(got, want))
    assert _armed(ks) and _armed(vs)


# ---- the running state -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fp8", "int8_zp"])
def test_static_equals_memoryless_on_the_union(kind):
    from compressed_tensors_amd import codec

    a, b = _transposed(2, 8, 5, 64, seed=4), _transposed(1, 8, 7, 64, seed=5) * 2
    kw = dict(_kw(dict(kind=kind, strategy="attn_head")), want_minmax=True)
    state = _state(a)
    _, _, mn_a, mx_a = codec.attn_observe(a, state, **kw)
    assert _armed(state)  # after a memoryless call the state equals a freshly armed one
    _, _, mn_b, mx_b = codec.attn_observe(b, _state(b), **kw)
    first = codec.attn_observe(a, state, keep=True, **kw)
    assert not _armed(state) and _same_bytes(first[2], mn_a) and _same_bytes(first[3], mx_a)
    scale, zp, mn, mx = codec.attn_observe(b, state, keep=True, **kw)
    assert torch.equal(mn, torch.minimum(mn_a, mn_b)) and torch.equal(mx, torch.maximum(mx_a, mx_b))
    # ... and its scale is calculate_qparams of those extremes: the memoryless observer on a tensor that holds exactly them
    union = torch.stack([mn, mx], dim=-1).reshape(1, 8, 1, 2).repeat(1, 1, 1, 8)
    want_scale, want_zp = codec.attn_observe(union, _state(union), **_kw(dict(kind=kind, strategy="attn_head")))
    assert _same_bytes(scale, want_scale) and _same_bytes(zp, want_zp)
    # the same through the observer module: static_minmax keeps, reset() forgets
    import compressed_tensors_amd as cta
    from compressed_tensors_amd.quantization import MinMaxObserver

    k = C.KINDS[kind]
    observer = MinMaxObserver("k", cta.QuantizationArgs(strategy="attn_head", observer="static_minmax", **k), torch.nn.Module())
    observer(a)
    s2, z2 = observer(b)
    assert _same_bytes(s2, scale) and _same_bytes(z2, zp) and _same_bytes(observer.min_vals, mn) and _same_bytes(observer.max_vals, mx)
    observer.reset()
    observer(b)
    assert _same_bytes(observer.min_vals, mn_b) and _same_bytes(observer.max_vals, mx_b)


# ---- planted extremes: the row loop, the last partial workgroup, both forms ----------------------------------------------------------------
# (2, 8, 4100, 16): the vector form, 65600 rows of two lanes; (1, 2, 257, 20): the element form, 514 rows of four lanes — a workgroup
# owns several steps and the last step is partial; (1, 8, 8200, 256): 65600 rows of 32 lanes, enough steps for the grid to stop at its cap;
# C.WIDE_SHAPES: rows of several waves, of a whole workgroup, and of more units than a workgroup has lanes (both forms)
@pytest.mark.parametrize("shape", [(2, 8, 4100, 16), (1, 2, 257, 20), (1, 8, 8200, 256), *C.WIDE_SHAPES])
@pytest.mark.parametrize("where", ["first", "last", "middle"])
def test_planted_extremes_are_found(shape, where):
    from compressed_tensors_amd import codec

    B, H, S, D = shape
    g = torch.Generator().manual_seed(S)
    base = (torch.rand(B, S, H, D, generator=g) * 2 - 1).to(C.BF16)  # |x| <= 1
    lo = -(2.0 + torch.arange(H, dtype=torch.float32)).to(C.BF16)  # distinct per head
    hi = (3.0 + torch.arange(H, dtype=torch.float32) * 0.5).to(C.BF16)
    at = {"first": ((0, 0, 0), (0, 0, 1)), "last": ((B - 1, S - 1, D - 1), (B - 1, S - 1, D - 2)), "middle": ((B - 1, S // 2, D - 1), (0, S // 2 + 1, D - 1))}[where]
    for h in range(H):
        (b0, s0, d0), (b1, s1, d1) = at
        base[b0, s0, h, d0] = lo[h]
        base[b1, s1, h, d1] = hi[h]
    x = base.to(DEV).transpose(1, 2)
    _, _, mn, mx = codec.attn_observe(x, _state(x), want_minmax=True, **FP8)
    assert torch.equal(mn.cpu().flatten(), lo) and torch.equal(mx.cpu().flatten(), hi), (mn.flatten().tolist(), mx.flatten().tolist())
    _, _, mn, mx = codec.attn_observe(x, _state(x, "tensor"), want_minmax=True, strategy="tensor", **FP8)
    assert torch.equal(mn.cpu(), lo.min().reshape(1)) and torch.equal(mx.cpu(), hi.max().reshape(1))


def test_a_wide_float32_row_matches_torch():
    """(1, 2, 3, 1024) float32: 128 units, a row of two waves, every wave of a row posting its own extremes"""
    from compressed_tensors_amd import codec

    x = C.wide_input((1, 2, 3, 1024), C.F32, DEV)
    _, _, mn, mx = codec.attn_observe(x, _state(x), want_minmax=True, **FP8)
    assert torch.equal(mn, torch.amin(x, dim=(0, 2, 3)).reshape(2, 1, 1)) and torch.equal(mx, torch.amax(x, dim=(0, 2, 3)).reshape(2, 1, 1))
    _, _, mn, mx = codec.attn_observe(x, _state(x, "tensor"), want_minmax=True, strategy="tensor", **FP8)
    assert torch.equal(mn, torch.amin(x).reshape(1)) and torch.equal(mx, torch.amax(x).reshape(1))


# ---- the key map: every finite bf16 bit pattern -------------------------------------------------------------------------------------------
def test_every_finite_bf16_bit_pattern():
    from compressed_tensors_amd import codec

    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(C.BF16)
    finite = pats[torch.isfinite(pats.float())]
    order = torch.argsort(finite.float(), stable=True)  # -0.0 and +0.0 stay neighbours: they compare equal
    values = finite[order]
    assert values.numel() == 65280 == 8 * 510 * 16
    heads = values.reshape(8, 510, 16)  # sorted and cut into 8 heads: head h holds one interval, subnormals and both zeros included
    perm = torch.randperm(510 * 16, generator=torch.Generator().manual_seed(0))
    x = heads.reshape(8, -1)[:, perm].reshape(1, 8, 510, 16).to(DEV)
    _, _, mn, mx = codec.attn_observe(x, _state(x), want_minmax=True, **FP8)
    want_mn, want_mx = heads[:, 0, 0], heads[:, -1, -1]
    got_mn, got_mx = mn.cpu().flatten(), mx.cpu().flatten()
    for got, want in ((got_mn, want_mn), (got_mx, want_mx)):
        zero = want == 0
        assert torch.equal(got[zero], want[zero])  # by value: the sign of a zero is not told apart
        assert torch.equal(got[~zero].view(torch.int16), want[~zero].view(torch.int16)), (got.tolist(), want.tolist())
    # the same patterns as fp16 and fp32 values: the keys are exact for every observed dtype
    for dt in (C.F16, C.F32):
        sub = heads[3:5].to(dt)  # the heads around zero: bf16 subnormals are fp32 subnormals (fp16: they round, identically on both sides)
        xs = sub.reshape(1, 2, 510, 16).to(DEV)
        _, _, mn, mx = codec.attn_observe(xs, _state(xs), want_minmax=True, **FP8)
        assert torch.equal(mn.cpu().flatten(), sub.reshape(2, -1).amin(dim=1)) and torch.equal(mx.cpu().flatten(), sub.reshape(2, -1).amax(dim=1))


# ---- results written into module parameters ---------------------------------------------------------------------------------------------------
def test_parameters_are_written_in_place():
    from compressed_tensors_amd import codec

    x = _transposed(2, 8, 33, 128, seed=6)
    kw = _kw(dict(kind="int8_zp", strategy="attn_head"))
    want_scale, want_zp = codec.attn_observe(x, _state(x), **kw)
    scale = torch.nn.Parameter(torch.full((8, 1, 1), -1.0, dtype=C.BF16, device=DEV), requires_grad=False)
    zp = torch.nn.Parameter(torch.full((8, 1, 1), 99, dtype=torch.int8, device=DEV), requires_grad=False)
    ptrs = scale.data_ptr(), zp.data_ptr()
    got_scale, got_zp = codec.attn_observe(x, _state(x), scale=scale, zero_point=zp, **kw)
    assert got_scale is scale and got_zp is zp and (scale.data_ptr(), zp.data_ptr()) == ptrs
    assert _same_bytes(scale.data, want_scale) and _same_bytes(zp.data, want_zp)
    # a float32 parameter over bfloat16 states: the bfloat16 result, widened
    wide = torch.nn.Parameter(torch.empty(8, 1, 1, dtype=C.F32, device=DEV), requires_grad=False)
    codec.attn_observe(x, _state(x), scale=wide, **kw)
    assert torch.equal(wide.data, want_scale.float())
    with pytest.raises(ValueError, match="scale must be"):
        codec.attn_observe(x, _state(x), scale=torch.empty(4, 1, 1, dtype=C.BF16, device=DEV), **kw)
    with pytest.raises(ValueError, match="observer state"):
        codec.attn_observe(x, codec.attn_observe_state(4, DEV), **kw)


# ---- what the entry refuses, without a launch ---------------------------------------------------------------------------------------------------
def test_rejections():
    from compressed_tensors_amd import codec

    unit = torch.zeros(1, 1, 1, 8, dtype=C.BF16, device=DEV)
    huge = unit.expand(1 << 16, 1 << 15, 1, 8)  # 2^31 rows of one stored row: the rows are indexed in 32 bits
    with pytest.raises(ValueError, match="rows"):
        codec.attn_observe(huge, codec.attn_observe_state(1, DEV), strategy="tensor", **FP8)
    with pytest.raises(ValueError, match="empty"):
        codec.attn_observe(unit[:, :, :0], codec.attn_observe_state(1, DEV), **FP8)
    many = unit.expand(1, codec.ATTN_OBSERVE_MAX_ENTRIES + 1, 1, 8)
    with pytest.raises(NotImplementedError, match="heads"):
        codec.attn_observe(many, codec.attn_observe_state(codec.ATTN_OBSERVE_MAX_ENTRIES + 1, DEV), **FP8)
    # the table's last entry is served
    full = torch.arange(codec.ATTN_OBSERVE_MAX_ENTRIES, dtype=torch.float32, device=DEV).to(C.BF16).reshape(1, -1, 1, 1).expand(1, -1, 3, 8)
    _, _, mn, mx = codec.attn_observe(full, _state(full), want_minmax=True, **FP8)
    assert torch.equal(mn.flatten(), full[0, :, 0, 0]) and torch.equal(mx.flatten(), full[0, :, 0, 0])
    torch.cuda.synchronize()
