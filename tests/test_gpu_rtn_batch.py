"""The table form of the one-pass round-to-nearest compress (ct_rtn_quant_pack_w4_batch / ct_rtn_mxfp4_quant_pack_batch) against the single-tensor
entries and the CPU oracle, up to ModelCompressor.compress_model_rtn(batched=True) against its per-module loop.  Everything is bit-exact.
Every test here needs an MI355X:  python -m pytest tests -m gpu"""
import array
import copy

import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
# (shape, group_size) of one table: (5, 256) g32 has 40 lanes, a partial last workgroup in front of the next item; (64, 4096) g128 spans 32 workgroups
W4_ITEMS = [((5, 256), 32), ((8, 512), 128), ((3, 2048), None), ((16, 64), 64), ((64, 4096), 128), ((7, 1024), None), ((1, 32), 32)]
MX_SHAPES = [(4, 64), (5, 96), (64, 4096), (1, 32)]


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


def special_values(dtype):
    v = [0.0, -0.0, 1e30, -1e30, 1e-30, 2.498, 3.496, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 6.5, 7.5, -7.5, -8.5, 127.5, -128.5, 65504.0, 1e-8]
    sp = torch.tensor(v, dtype=torch.float32).to(dtype)
    return sp[torch.isfinite(sp.float())]


def weight(shape, group, dtype):
    """the data of test_rtn_one_pass_equals_observer_plus_compress: finite special values, an all-zero group, a strictly positive group"""
    g = torch.Generator().manual_seed(shape[0] * 7 + shape[1])
    x = (torch.randn(shape, generator=g) * 0.05).to(dtype)
    sp = special_values(dtype)
    x.view(-1)[: min(sp.numel(), x.numel())] = sp[: x.numel()]
    if shape[0] > 2:
        x[1, :group] = 0
        x[2, :group] = x[2, :group].abs() + 0.01
    return x


def same(a, b):
    """0 ulp: 16-bit floats through their bit patterns"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype in (BF16, F16):
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a, b)


def same_triple(a, b):
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
def test_w4_table_equals_single_entry_and_oracle(cta, dev, dtype, symmetric):
    """one table of seven tensors with group and channel items mixed — against rtn_quantize_and_pack of each tensor and against the oracle's
    calculate_qparams + quantize + pack_to_int32"""
    xs = [weight(shape, gs or shape[1], dtype) for shape, gs in W4_ITEMS]
    groups = [gs for _, gs in W4_ITEMS]
    got = cta.codec.rtn_quantize_and_pack_many([x.to(dev) for x in xs], group_size=groups, symmetric=symmetric)
    assert len(got) == len(xs)
    for x, gs, (packed, scale, zp) in zip(xs, groups, got):
        assert packed.is_cuda and packed.dtype == torch.int32 and scale.dtype == dtype and zp.dtype == torch.int8
        one = cta.codec.rtn_quantize_and_pack(x.to(dev), group_size=gs, symmetric=symmetric)
        assert same_triple((packed, scale, zp), one), (tuple(x.shape), gs)
        s_ref, z_ref = O.calculate_qparams_minmax(x, num_bits=4, group_size=gs, symmetric=symmetric)
        assert same(scale.cpu(), s_ref) and torch.equal(zp.cpu(), z_ref), (tuple(x.shape), gs)
        q = O.quantize(x, s_ref, z_ref, num_bits=4, strategy="group" if gs else "channel", group_size=gs, dtype=torch.int8)
        assert torch.equal(packed.cpu(), O.pack_to_int32(q, 4).contiguous()), (tuple(x.shape), gs)
    # one group size for the whole call, and None (channel) for the whole call
    for gs in (32, None):
        sub = [x.to(dev) for x in xs[:4]]
        many = cta.codec.rtn_quantize_and_pack_many(sub, group_size=gs, symmetric=symmetric)
        for x, t in zip(sub, many):
            assert same_triple(t, cta.codec.rtn_quantize_and_pack(x, group_size=gs, symmetric=symmetric)), (tuple(x.shape), gs)


@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
def test_w4_table_of_one_item_with_a_nan(cta, dev, symmetric):
    x = torch.randn((4, 256), generator=torch.Generator().manual_seed(5)).to(BF16)
    x[0, 3] = float("nan")
    (packed, scale, zp), = cta.codec.rtn_quantize_and_pack_many([x.to(dev)], group_size=128, symmetric=symmetric)
    assert same_triple((packed, scale, zp), cta.codec.rtn_quantize_and_pack(x.to(dev), group_size=128, symmetric=symmetric))
    s_ref, z_ref = O.calculate_qparams_minmax(x, num_bits=4, group_size=128, symmetric=symmetric)
    assert same(scale.cpu(), s_ref) and torch.equal(zp.cpu(), z_ref)
    q = O.quantize(x, s_ref, z_ref, num_bits=4, strategy="group", group_size=128, dtype=torch.int8)
    assert torch.equal(packed.cpu(), O.pack_to_int32(q, 4).contiguous())


def test_w4_table_of_twenty_items(cta, dev):
    """20 small items of alternating shapes: the workgroups' binary search over the table is several levels deep"""
    shapes = [((3, 512), 128), ((9, 1024), None), ((2, 64), 32), ((33, 256), 64)] * 5
    g = torch.Generator().manual_seed(20)
    xs = [(torch.randn(shape, generator=g) * (0.02 * (i + 1))).to(BF16).to(dev) for i, (shape, _) in enumerate(shapes)]
    groups = [gs for _, gs in shapes]
    for symmetric in (True, False):
        got = cta.codec.rtn_quantize_and_pack_many(xs, group_size=groups, symmetric=symmetric)
        for i, (x, gs, t) in enumerate(zip(xs, groups, got)):
            assert same_triple(t, cta.codec.rtn_quantize_and_pack(x, group_size=gs, symmetric=symmetric)), (i, symmetric)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_mxfp4_table_equals_single_entry(cta, dev, dtype):
    xs = [weight(shape, 32, dtype).to(dev) for shape in MX_SHAPES]
    xs[2][5, 64:96] = 0  # an all-zero MX group
    got = cta.codec.rtn_mxfp4_quantize_and_pack_many(xs)
    assert len(got) == len(xs)
    for x, (packed, code) in zip(xs, got):
        assert packed.dtype == torch.uint8 and code.dtype == torch.uint8 and packed.shape == (x.shape[0], x.shape[1] // 2)
        assert same_triple((packed, code), cta.codec.rtn_mxfp4_quantize_and_pack(x)), tuple(x.shape)


def test_ineligible_tensors_keep_their_place(cta, dev):
    """a float32 weight, group 48 at 96 columns and a non-contiguous view mixed into a list of table tensors: the results come back in input
    order and equal the single-tensor call resp. the observer + compress composition"""
    g = torch.Generator().manual_seed(7)
    a, b, c = (torch.randn(s, generator=g).to(BF16).to(dev) for s in ((8, 512), (16, 256), (4, 128)))
    f32 = torch.randn((8, 256), generator=g).to(dev)
    g48 = torch.randn((8, 96), generator=g).to(BF16).to(dev)
    view = torch.randn((256, 8), generator=g).to(BF16).to(dev).t()
    assert not view.is_contiguous()
    xs, groups = [a, f32, b, g48, view, c], [128, 128, 128, 48, 128, 128]
    for symmetric in (True, False):
        got = cta.codec.rtn_quantize_and_pack_many(xs, group_size=groups, symmetric=symmetric)
        for i in (0, 2, 4, 5):
            assert same_triple(got[i], cta.codec.rtn_quantize_and_pack(xs[i], group_size=128, symmetric=symmetric)), i
        for i in (1, 3):
            s, z = cta.codec.minmax_qparams(xs[i], num_bits=4, group_size=groups[i], symmetric=symmetric)
            p = cta.codec.quantize_and_pack(xs[i], s, z, num_bits=4, strategy="group", group_size=groups[i])
            assert same_triple(got[i], (p, s, z)), i
    mx = [a, view, b]
    got = cta.codec.rtn_mxfp4_quantize_and_pack_many(mx)
    for x, t in zip(mx, got):
        assert same_triple(t, cta.codec.rtn_mxfp4_quantize_and_pack(x))
    with pytest.raises(NotImplementedError):
        cta.codec.rtn_mxfp4_quantize_and_pack_many([a, f32])  # as the single call


def _model_and_schemes(cta, dev):
    from compressed_tensors_amd.quantization import QuantizationArgs, QuantizationScheme

    torch.manual_seed(3)
    dims = [(256, 512), (512, 256), (256, 1024), (1024, 128), (128, 384), (384, 128)]
    model = torch.nn.Sequential(*[torch.nn.Linear(i, o, bias=(k == 0)) for k, (i, o) in enumerate(dims)]).to(dev).to(BF16)
    act = QuantizationArgs(num_bits=8, type="float", strategy="tensor")
    weights = [QuantizationArgs(num_bits=4, group_size=128, symmetric=True), QuantizationArgs(num_bits=4, group_size=128, symmetric=False),
               QuantizationArgs(num_bits=4, strategy="channel", symmetric=True),
               QuantizationArgs(num_bits=4, type="float", strategy="group", symmetric=True, group_size=32, scale_dtype=torch.uint8),
               QuantizationArgs(num_bits=4, type="float", strategy="tensor_group", symmetric=True, group_size=16, scale_dtype=torch.float8_e4m3fn),
               QuantizationArgs(num_bits=8, type="float", strategy="channel")]
    for k, (m, w) in enumerate(zip(model, weights)):
        m.quantization_scheme = QuantizationScheme(targets=["Linear"], weights=w, input_activations=act if k == 5 else None)
    return model


def _bits(t):
    return t.view(torch.uint8) if t.dtype.itemsize == 1 else (t.view(torch.int16) if t.dtype in (BF16, F16) else t)


def test_compress_model_rtn_batched_equals_per_module(cta, dev):
    """W4 g128 symmetric (with a bias), W4 g128 asymmetric, W4 channel, MXFP4, NVFP4 and FP8 channel in one model: batched=True leaves every module
    in exactly the state batched=False does — names and their order, tensors (the packed zero points and weight_shape included), status, format —
    and the first forward decompresses both to the same weights"""
    model = _model_and_schemes(cta, dev)
    loop = copy.deepcopy(model)
    bias0 = model[0].bias.data.clone()
    cta.ModelCompressor().compress_model_rtn(loop, batched=False)
    cta.ModelCompressor().compress_model_rtn(model, batched=True)
    assert [m.quantization_scheme.format.value for m in model] == ["pack-quantized"] * 3 + ["mxfp4-pack-quantized", "nvfp4-pack-quantized", "float-quantized"]
    assert list(model[0]._parameters) == ["bias", "weight_packed", "weight_scale", "weight_shape"]
    assert list(model[1]._parameters)[-4:] == ["weight_packed", "weight_scale", "weight_shape", "weight_zero_point"]
    assert model[1].weight_zero_point.dtype == torch.int32 and model[1].weight_zero_point.shape == (256 // 8, 512 // 128)
    for k, (a, b) in enumerate(zip(model, loop)):
        assert list(a._parameters) == list(b._parameters) and list(a._buffers) == list(b._buffers), k
        for name in a._parameters:
            p, q = a._parameters[name], b._parameters[name]
            if p is None or q is None:  # the `bias` slot of a Linear without one
                assert p is None and q is None, (k, name)
                continue
            assert type(p) is type(q) and p.dtype == q.dtype and p.device == q.device and p.shape == q.shape and p.requires_grad == q.requires_grad, (k, name)
            assert torch.equal(_bits(p.data), _bits(q.data)), (k, name)
        assert a.quantization_status == b.quantization_status == cta.QuantizationStatus.COMPRESSED
        assert a.quantization_scheme.format == b.quantization_scheme.format
    assert torch.equal(model[0].bias.data, bias0)
    x = torch.randn(4, 256, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(BF16)
    ya, yb = model(x), loop(x)  # the first forward decompresses (the hook)
    assert ya.shape == (4, 128) and same(ya, yb)
    for k, (a, b) in enumerate(zip(model, loop)):
        assert list(a._parameters) == list(b._parameters) and same(a.weight.data, b.weight.data), k


def test_table_entries_are_hip_graph_capturable(cta, dev):
    """the two table entries (and the zero-point packing behind the asymmetric W4 table) allocate nothing and never synchronise: captured as one
    sequential chain and replayed once on new data"""
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(12)
    shapes = [(64, 1024), (128, 512), (8, 4096)]
    ws = [torch.randn(s, device=dev, generator=g).to(BF16) for s in shapes]
    packed = [torch.empty(r, c // 8, dtype=torch.int32, device=dev) for r, c in shapes]
    scale = [torch.empty(r, c // 128, dtype=BF16, device=dev) for r, c in shapes]
    zp = [torch.empty(r, c // 128, dtype=torch.int8, device=dev) for r, c in shapes]
    zpp = [torch.empty(r // 8, c // 128, dtype=torch.int32, device=dev) for r, c in shapes]
    mxp = [torch.empty(r, c // 2, dtype=torch.uint8, device=dev) for r, c in shapes]
    code = [torch.empty(r, c // 32, dtype=torch.uint8, device=dev) for r, c in shapes]
    row = cta.codec.item_row

    def planned(rows, plan):
        words = array.array("q", [v for r in rows for v in r])
        blocks = int(getattr(lib, plan)(words.buffer_info()[0], len(rows)))
        assert blocks > 0, _lib.last_error()
        return torch.tensor(list(words), dtype=torch.int64).to(dev), blocks

    n = len(shapes)
    t_w4, b_w4 = planned([row(w, s, z, p, r, c, 128) for w, s, z, p, (r, c) in zip(ws, scale, zp, packed, shapes)], "ct_rtn_w4_batch_plan")
    t_zp, b_zp = planned([row(z, dst=q, rows=r, cols=c // 128) for z, q, (r, c) in zip(zp, zpp, shapes)], "ct_zp4_batch_plan")
    t_mx, b_mx = planned([row(w, dst=p, rows=r, cols=c, group=32, zp_packed=k) for w, p, k, (r, c) in zip(ws, mxp, code, shapes)], "ct_rtn_mxfp4_batch_plan")
    torch.cuda.synchronize()

    def launches(stream):
        rcs = [lib.ct_rtn_quant_pack_w4_batch(t_w4.data_ptr(), n, b_w4, _lib.BF16, 0, stream),
               lib.ct_zp4_pack_dim0_batch(t_zp.data_ptr(), n, b_zp, 0, stream),
               lib.ct_rtn_mxfp4_quant_pack_batch(t_mx.data_ptr(), n, b_mx, _lib.BF16, stream)]
        assert not any(rcs), (rcs, _lib.last_error())

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        launches(_lib.stream_on(dev, side.cuda_stream))  # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches(_lib.stream_on(dev, torch.cuda.current_stream(dev).cuda_stream))
    for w in ws:
        w.copy_(torch.randn(w.shape, device=dev, generator=g).to(BF16))
    for t in (*packed, *scale, *zp, *zpp, *mxp, *code):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for i, w in enumerate(ws):
        p, s, z = cta.codec.rtn_quantize_and_pack(w, group_size=128, symmetric=False)
        assert same_triple((packed[i], scale[i], zp[i]), (p, s, z)) and torch.equal(zpp[i], cta.codec.pack_to_int32(z, 4, packed_dim=0)), i
        assert same_triple((mxp[i], code[i]), cta.codec.rtn_mxfp4_quantize_and_pack(w)), i
