"""The table form of the one-pass NVFP4 round-to-nearest compress, generate_gparam of every weight included (ct_rtn_nvfp4_amax_batch +
ct_rtn_nvfp4_quant_pack_batch), against the single-tensor entry and the CPU oracle, up to ModelCompressor.compress_model_rtn(batched=True) against
its per-module loop.  Everything is bit-exact.  Every test here needs an MI355X:  python -m pytest tests -m gpu"""
import copy

import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

BF16, F16, F32, F8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
# a lane is 32 elements: (5, 96) has 15 lanes, a partial workgroup in front of the next item; (64, 4096) spans 32 workgroups, so its maximum crosses them
SHAPES = [(1, 32), (5, 96), (3, 64), (64, 4096), (7, 1024), (2, 32)]
WG = 256 * 32  # elements per workgroup


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cta():
    import compressed_tensors_amd as m
    from compressed_tensors_amd import _lib

    _lib.load()  # fail loudly if the HIP extension is missing
    return m


def weight(shape, dtype, seed=23):
    """the data of test_rtn_nvfp4_one_pass: group maxima from 2^-12 to 2^3 with alternating signs, an all-zero first group"""
    g = torch.Generator().manual_seed(seed + shape[0] * 7 + shape[1])
    x = (torch.randn(shape, generator=g) * 0.3).to(dtype)
    ngroups = x.numel() // 16
    mags = (2.0 ** torch.linspace(-12, 3, ngroups)) * (1 + 0.25 * (torch.arange(ngroups) % 5))
    xv = x.view(-1, 16)
    xv[:, 0] = torch.where(torch.arange(ngroups) % 2 == 0, mags, -mags).to(dtype)
    xv[:, 1:] = (xv[:, 1:].float().clamp(-1, 1) * mags[:, None] * 0.9).to(dtype)
    xv[0] = 0
    return x


def bits(t):
    return t.view(torch.uint8) if t.dtype.itemsize == 1 else (t.view(torch.int16) if t.dtype in (BF16, F16) else t.view(torch.int32) if t.dtype == F32 else t)


def same_triple(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def check_against_oracle(x, got, what):
    packed, s8, gs = got
    gs_ref = O.generate_gparam(x)
    s_ref = O.calculate_qparams_float(x, kind="nvfp4", group_size=16, global_scale=gs_ref)
    ref = O.fp4_compress(x, s_ref, gs_ref, fmt="nvfp4-pack-quantized")
    assert torch.equal(bits(gs.cpu()), bits(gs_ref)), (what, gs, gs_ref)
    assert torch.equal(s8.cpu().view(torch.uint8), ref["weight_scale"].view(torch.uint8)) and torch.equal(packed.cpu(), ref["weight_packed"]), what


def check_table(cta, dev, xs, oracle=True):
    got = cta.codec.rtn_nvfp4_quantize_and_pack_many([x.to(dev) for x in xs])
    assert len(got) == len(xs)
    for i, (x, t) in enumerate(zip(xs, got)):
        packed, s8, gs = t
        assert packed.is_cuda and packed.dtype == torch.uint8 and packed.shape == (x.shape[0], x.shape[1] // 2)
        assert s8.dtype == F8 and s8.shape == (x.shape[0], x.shape[1] // 16) and gs.dtype == F32 and gs.shape == (1,)
        assert same_triple(t, cta.codec.rtn_nvfp4_quantize_and_pack(x.to(dev))), (i, tuple(x.shape), gs)
        if oracle:
            check_against_oracle(x, t, (i, tuple(x.shape)))
    return got


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_table_equals_single_entry_and_oracle(cta, dev, dtype):
    got = check_table(cta, dev, [weight(shape, dtype) for shape in SHAPES])
    assert len({float(gs) for _, _, gs in got}) > 1  # (the items do have different global scales)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("where", ["first", "last", "wg17"])
def test_planted_maximum_crosses_the_workgroups(cta, dev, dtype, where):
    """the one element that decides the global scale of (64, 4096) sits in the first lane, the last lane, or inside the 17th of its 32 workgroups"""
    at = {"first": 0, "last": 64 * 4096 - 1, "wg17": 16 * WG + 4321}[where]
    assert where != "wg17" or at // WG == 16
    for sign in (1.0, -1.0):
        xs = [weight(shape, dtype) for shape in SHAPES]
        xs[3].view(-1)[at] = sign * 1000.0
        got = check_table(cta, dev, xs)
        assert float(got[3][2]) == float(O.generate_gparam(torch.tensor([1000.0], dtype=dtype).reshape(1, 1)))


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_an_item_between_large_neighbours_gets_its_own_global_scale(cta, dev, dtype):
    g = torch.Generator().manual_seed(5)
    big0, small, big1 = (torch.randn(s, generator=g).clamp(-1, 1) for s in ((5, 96), (3, 64), (7, 1024)))
    big0, small, big1 = (big0 * 1e3).to(dtype), (small * 1e-3).to(dtype), (big1 * 1e3).to(dtype)
    big0[0, 0], small[1, 7], big1[6, 1023] = 1e3, 1e-3, -1e3
    got = check_table(cta, dev, [big0, small, big1])  # (each against generate_gparam of that tensor alone)
    assert float(got[0][2]) == float(got[2][2]) != float(got[1][2])
    if dtype == BF16:  # (in float16 2688 / 1e-3 overflows: generate_gparam's nan_to_num makes it 1)
        assert float(got[1][2]) > 1e5 * float(got[0][2])


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_degenerate_items(cta, dev, dtype):
    """all-zero, one NaN, one +inf: global scales 1, 1 and 0 (generate_gparam's clamp and nan_to_num), bytes those of the single-tensor entry"""
    plain0, plain1 = weight((5, 96), dtype), weight((3, 64), dtype)
    zero = torch.zeros((4, 64), dtype=dtype)
    nan, inf = weight((7, 1024), dtype), weight((2, 2048), dtype)
    nan[3, 517] = float("nan")
    inf[1, 100] = float("inf")
    xs = [plain0, zero, nan, plain1, inf]
    got = check_table(cta, dev, xs, oracle=False)
    assert [float(got[i][2]) for i in (1, 2, 4)] == [1.0, 1.0, 0.0]
    for i in (0, 3):  # the finite items between them are untouched by their neighbours
        check_against_oracle(xs[i], got[i], i)
    for x, i in ((zero, 1), (nan, 2), (inf, 4)):  # generate_gparam itself agrees on the degenerate cases
        assert torch.equal(bits(got[i][2].cpu()), bits(O.generate_gparam(x)))


def test_keys_of_an_earlier_call_do_not_leak_into_the_next(cta, dev):
    """the same shapes twice, large values first: the allocator hands the second call the first call's key buffer"""
    first = [(weight(shape, BF16) * 64).to(BF16) for shape in SHAPES]
    second = [(weight(shape, BF16, seed=99) * 0.01).to(BF16) for shape in SHAPES]
    a = check_table(cta, dev, first)
    b = check_table(cta, dev, second)
    assert all(float(y[2]) > 100 * float(x[2]) for x, y in zip(a, b))


def test_one_table_is_one_fold_and_one_quantize_launch(cta, dev, monkeypatch):
    from compressed_tensors_amd import codec

    names, real = [], codec.call
    monkeypatch.setattr(codec, "call", lambda name, *a: names.append(name) or real(name, *a))
    xs = [weight(shape, BF16).to(dev) for shape in SHAPES]
    codec.rtn_nvfp4_quantize_and_pack_many(xs)
    assert names == ["ct_rtn_nvfp4_amax_batch", "ct_rtn_nvfp4_quant_pack_batch"]
    names.clear()
    codec.rtn_nvfp4_quantize_and_pack(xs[0])
    assert names == ["ct_generate_gparam", "ct_rtn_nvfp4_quant_pack"]  # what the table replaces, per module
    # a list of two dtypes: the table is the first eligible tensor's, the others go one by one
    names.clear()
    mixed = [xs[0], weight((3, 64), F16).to(dev), xs[1], torch.randn(4, 48).to(BF16).to(dev)]
    with pytest.raises(NotImplementedError):
        codec.rtn_nvfp4_quantize_and_pack_many(mixed)  # cols % 32: as the single call
    names.clear()
    got = codec.rtn_nvfp4_quantize_and_pack_many(mixed[:3])
    assert sorted(names) == ["ct_generate_gparam", "ct_rtn_nvfp4_amax_batch", "ct_rtn_nvfp4_quant_pack", "ct_rtn_nvfp4_quant_pack_batch"]
    for x, t in zip(mixed[:3], got):
        assert same_triple(t, codec.rtn_nvfp4_quantize_and_pack(x))


def _model(cta, dev, dtype):
    from compressed_tensors_amd.quantization import QuantizationArgs, QuantizationScheme

    torch.manual_seed(11)
    nv = QuantizationArgs(num_bits=4, type="float", strategy="tensor_group", symmetric=True, group_size=16, scale_dtype=F8)
    w4 = QuantizationArgs(num_bits=4, group_size=32, symmetric=True)
    mx = QuantizationArgs(num_bits=4, type="float", strategy="group", symmetric=True, group_size=32, scale_dtype=torch.uint8)
    kinds = [nv, nv, w4, nv, mx, nv] * 6
    kinds = kinds[:34]
    layers = []
    for k, args in enumerate(kinds):
        cols = 48 if k == 9 else 64  # module 9: NVFP4 with cols % 32 != 0 — not a table item
        layers.append(torch.nn.Linear(cols, 32, bias=(k == 1)))
    model = torch.nn.Sequential(*layers).to(dev).to(dtype)
    for k, (m, args) in enumerate(zip(model, kinds)):
        m.weight.data.mul_(1.0 + 0.5 * k)  # every module its own amax
        m.quantization_scheme = QuantizationScheme(targets=["Linear"], weights=args)
    assert kinds[1] is nv and kinds[9] is nv and sum(a is nv for a in kinds) > 16
    return model, [a is nv for a in kinds]


@pytest.mark.parametrize("window", [32, 8], ids=["window32", "window8"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_compress_model_rtn_batched_equals_per_module(cta, dev, dtype, window, monkeypatch):
    """34 modules, two windows of the model; NVFP4 (one with a bias, one the table does not take) mixed with W4 g32 and MXFP4.  The windows are cut
    per codec: the 23 NVFP4 modules are one window of 32 and three windows of 8"""
    from compressed_tensors_amd import codec
    from compressed_tensors_amd.compressors import base

    monkeypatch.setattr(cta.NVFP4PackedCompressor, "RTN_TABLE_MEASURED_FASTER", True)  # the hook itself is under test, whatever the dispatch rule holds
    monkeypatch.setattr(base, "RTN_WINDOW", window)
    model, is_nv = _model(cta, dev, dtype)
    dense = [m.weight.data.clone() for m in model]
    bias1 = model[1].bias.data.clone()
    loop = copy.deepcopy(model)
    cta.ModelCompressor().compress_model_rtn(loop, batched=False)
    names, real = [], codec.call
    monkeypatch.setattr(codec, "call", lambda name, *a: names.append(name) or real(name, *a))
    cta.ModelCompressor().compress_model_rtn(model, batched=True)
    monkeypatch.undo()
    # a fold and a quantize launch per window, and the two-kernel composition once, for module 9
    windows = -(-sum(is_nv) // window)
    assert sum(is_nv) == 23 and names.count("ct_rtn_nvfp4_amax_batch") == windows and names.count("ct_rtn_nvfp4_quant_pack_batch") == windows
    assert names.count("ct_generate_gparam") == 1 and names.count("ct_rtn_nvfp4_quant_pack") == 0  # ((32, 48) takes the two-kernel composition)
    storages = set()
    for k, (a, b) in enumerate(zip(model, loop)):
        assert list(a._parameters) == list(b._parameters) and list(a._buffers) == list(b._buffers), k
        for name in a._parameters:
            p, q = a._parameters[name], b._parameters[name]
            if p is None or q is None:
                assert p is None and q is None, (k, name)
                continue
            assert type(p) is type(q) and p.dtype == q.dtype and p.device == q.device and p.shape == q.shape and p.requires_grad == q.requires_grad, (k, name)
            assert torch.equal(bits(p.data), bits(q.data)), (k, name)
        assert a.quantization_status == b.quantization_status == cta.QuantizationStatus.COMPRESSED
        assert a.quantization_scheme.format == b.quantization_scheme.format
        if is_nv[k]:
            if k != 9:  # (module 9 takes `compress`, which keeps the global scale in front; its order is the per-module loop's, checked above)
                assert list(a._parameters)[-3:] == ["weight_packed", "weight_scale", "weight_global_scale"], k
            gs = a.weight_global_scale
            assert gs.numel() == 1 and gs.dtype == F32 and gs.untyped_storage().nbytes() == 4 and gs.storage_offset() == 0, k  # no view into a shared buffer
            storages.add(gs.untyped_storage().data_ptr())
    assert len(storages) == sum(is_nv)
    assert list(model[1]._parameters)[0] == "bias" and torch.equal(model[1].bias.data, bias1)
    cta.ModelCompressor().decompress_model(model)
    for k, (m, w) in enumerate(zip(model, dense)):
        if is_nv[k]:
            assert float((m.weight.data.float() - w.float()).abs().max()) <= float(w.float().abs().max()) * 0.26, k
