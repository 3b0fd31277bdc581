"""The data-free window hooks of the three table codecs (pack-quantized W4, MXFP4, NVFP4) in ONE model whose windows mix two weight dtypes: the
tables are keyed by (device, dtype[, symmetric]), and a wrong key would read float16 words as bfloat16 without any error.  Everything is
bit-exact against the per-module path, which tests/test_gpu_rtn_batch.py and tests/test_gpu_nvfp4_rtn_table.py hold to the oracle.
Every test here needs an MI355X:  python -m pytest tests -m gpu"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F16, F32, F8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn


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


def bits(t):
    return t.view(torch.uint8) if t.dtype.itemsize == 1 else (t.view(torch.int16) if t.dtype in (BF16, F16) else t.view(torch.int32) if t.dtype == F32 else t)


def _schemes():
    from compressed_tensors_amd.quantization import QuantizationArgs, QuantizationScheme

    args = {"g32": QuantizationArgs(num_bits=4, group_size=32, symmetric=True),
            "g128a": QuantizationArgs(num_bits=4, group_size=128, symmetric=False),
            "chan": QuantizationArgs(num_bits=4, strategy="channel", symmetric=True),
            "mx": QuantizationArgs(num_bits=4, type="float", strategy="group", symmetric=True, group_size=32, scale_dtype=torch.uint8),
            "nv": QuantizationArgs(num_bits=4, type="float", strategy="tensor_group", symmetric=True, group_size=16, scale_dtype=F8)}
    return {name: QuantizationScheme(targets=["Linear"], weights=a) for name, a in args.items()}  # one scheme object per kind, shared by its modules


# (scheme, weight dtype, out x in): bfloat16 and float16 interleaved within every codec's window.  5 x 64: less than one workgroup; 32 x 256; 3 x 2048:
# one 2048-element group per row, the DPP reduction's widest; 33 x 128: a partial last workgroup, and rows that are no multiple of 8 for the stored
# zero points.  The last three are the ones a table refuses — a float32 weight (W4, MXFP4), in_features = 48 (NVFP4) — and module 8 has a bias.
MODULES = [("g32", BF16, 5, 64), ("mx", F16, 5, 64), ("nv", BF16, 32, 256), ("g128a", F16, 33, 128), ("chan", BF16, 3, 2048), ("nv", F16, 33, 128),
           ("mx", BF16, 32, 256), ("g32", F16, 32, 256), ("g128a", BF16, 32, 256), ("chan", F16, 3, 2048), ("mx", BF16, 33, 128), ("nv", BF16, 5, 64),
           ("g128a", BF16, 33, 128), ("nv", F16, 3, 2048), ("mx", F16, 3, 2048), ("g32", F32, 5, 64), ("mx", F32, 5, 64), ("nv", BF16, 5, 48)]
REFUSED = (15, 16, 17)


def _model(dev):
    torch.manual_seed(17)
    schemes = _schemes()
    layers = []
    for k, (name, dtype, rows, cols) in enumerate(MODULES):
        m = torch.nn.Linear(cols, rows, bias=(k == 8)).to(dev).to(dtype)
        m.weight.data.mul_(1.0 + 0.5 * k)  # every module its own range
        m.quantization_scheme = schemes[name]
        layers.append(m)
    return torch.nn.Sequential(*layers)


def test_two_dtypes_in_one_window_of_every_table_codec(cta, dev, monkeypatch):
    """18 Linears, one window per codec: W4 g32 symmetric, W4 g128 asymmetric, W4 channel-wise, MXFP4 and NVFP4, bfloat16 and float16 interleaved,
    one refused module per codec family, one bias.  compress_model_rtn(batched=True) leaves every module bit-identical to batched=False — names and
    order, dtypes, shapes, requires_grad, bits, status, format — and every table launch ran exactly once per (codec, dtype, symmetric) group, with
    that group's dtype code and item count"""
    from compressed_tensors_amd import _lib, codec

    monkeypatch.setattr(cta.NVFP4PackedCompressor, "RTN_TABLE_MEASURED_FASTER", True)  # the hook itself is under test, whatever the dispatch rule holds
    model = _model(dev)
    loop = copy.deepcopy(model)
    bias8 = model[8].bias.data.clone()
    cta.ModelCompressor().compress_model_rtn(loop, batched=False)
    calls, real = [], codec.call
    monkeypatch.setattr(codec, "call", lambda name, *a: calls.append((name, a)) or real(name, *a))
    cta.ModelCompressor().compress_model_rtn(model, batched=True)
    monkeypatch.undo()

    # a table launch is (table, n, workgroups, scalars..., stream): the dtype code — and W4's `symmetric` — of each launch against the groups present
    def group(names, dtype, skip=REFUSED):
        return sum(1 for k, (name, dt, _, _) in enumerate(MODULES) if name in names and dt is dtype and k not in skip)

    def launched(symbol):
        return sorted((a[3:-1], a[1]) for name, a in calls if name == symbol)

    code = {BF16: _lib.BF16, F16: _lib.F16}
    sym, asym = ("g32", "chan"), ("g128a",)
    assert launched("ct_rtn_quant_pack_w4_batch") == sorted(((code[dt], s), group(names, dt)) for dt in (BF16, F16) for names, s in ((sym, 1), (asym, 0)))
    assert launched("ct_zp4_pack_dim0_batch") == sorted(((0,), group(asym, dt)) for dt in (BF16, F16))  # behind each asymmetric table, never a symmetric one
    for symbol, names in (("ct_rtn_mxfp4_quant_pack_batch", ("mx",)), ("ct_rtn_nvfp4_amax_batch", ("nv",)), ("ct_rtn_nvfp4_quant_pack_batch", ("nv",))):
        assert launched(symbol) == sorted(((code[dt],), group(names, dt)) for dt in (BF16, F16)), symbol
    assert [group(sym, dt) for dt in (BF16, F16)] == [2, 2] and [group(asym, dt) for dt in (BF16, F16)] == [2, 1]
    order = [name for name, _ in calls]
    for k, name in enumerate(order):  # the stored zero points directly behind their own table; the fold directly in front of its quantize pass
        if name == "ct_zp4_pack_dim0_batch":
            assert order[k - 1] == "ct_rtn_quant_pack_w4_batch" and calls[k - 1][1][4] == 0
        if name == "ct_rtn_nvfp4_quant_pack_batch":
            assert order[k - 1] == "ct_rtn_nvfp4_amax_batch" and calls[k - 1][1][0] == calls[k][1][0]
    # the refused modules ran per module: no single-tensor one-pass launch for anything a table took
    assert order.count("ct_rtn_quant_pack_w4") == 0 and order.count("ct_rtn_mxfp4_quant_pack") == 0 and order.count("ct_rtn_nvfp4_quant_pack") == 0
    assert order.count("ct_minmax_qparams") == 1 and order.count("ct_minmax_qparams_float") == 2 and order.count("ct_generate_gparam") == 1

    for k, (a, b) in enumerate(zip(model, loop)):
        assert list(a._parameters) == list(b._parameters) and list(a._buffers) == list(b._buffers), k
        for name in a._parameters:
            p, q = a._parameters[name], b._parameters[name]
            if p is None or q is None:  # the `bias` slot of a Linear without one
                assert p is None and q is None, (k, name)
                continue
            assert type(p) is type(q) and p.dtype == q.dtype and p.device == q.device and p.shape == q.shape and p.requires_grad == q.requires_grad, (k, name)
            assert torch.equal(bits(p.data), bits(q.data)), (k, name)
        assert a.quantization_status == b.quantization_status == cta.QuantizationStatus.COMPRESSED
        assert a.quantization_scheme.format == b.quantization_scheme.format
        assert "weight" not in a._parameters and "weight_packed" in a._parameters, k
    assert list(model[8]._parameters) == ["bias", "weight_packed", "weight_scale", "weight_shape", "weight_zero_point"] and torch.equal(model[8].bias.data, bias8)
    assert model[3].weight_zero_point.shape == (5, 1) and model[3].weight_scale.dtype == F16 and model[12].weight_scale.dtype == BF16  # ceil(33 / 8) words
    assert model[2].weight_global_scale.dtype == F32 and model[1].weight_scale.dtype == torch.uint8 and model[5].weight_scale.dtype == F8


def test_an_mxfp4_weight_of_48_columns_fails_the_same_way_on_both_paths(cta, dev):
    """in_features = 48 is no MXFP4 weight at all (groups of 32): the table refuses it, and `compress_rtn` — reached through the hook's rest or per
    module — raises the codec's ValueError about the scale shape either way, so such a module cannot sit in the model above"""
    errors = []
    for batched in (True, False):
        m = torch.nn.Linear(48, 5, bias=False).to(dev).to(BF16)
        m.quantization_scheme = _schemes()["mx"]
        with pytest.raises(ValueError, match="scale shape") as err:
            cta.ModelCompressor().compress_model_rtn(torch.nn.Sequential(m), batched=batched)
        errors.append(str(err.value))
        assert "weight" in m._parameters and not hasattr(m, "quantization_status")
    assert errors[0] == errors[1]
