"""The two kernels behind ct_quant_pack's lean W4 branch — four plain 16-byte loads per lane (CT_W4_COMPRESS=plain) and the wave's 4 KiB
brought in by non-temporal LDS-DMA and read back at the lane's own 64 bytes (CT_W4_COMPRESS=lds; the variable is read by the
diagnostics build of the library, the product chooses by size alone) — leave the same packed words: equal to
each other, to the CPU oracle's pack_quantized_compress, and ct_unpack_dequant of them equals fake_quantize_tensor.  The shapes are the
smallest that reach each way the LDS form can go wrong (csrc/ct_quant.hip, w4_quant_pack_lds_kernel)."""
import functools

import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
VARIANTS = ("plain", "lds")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def diag_lib():
    """the diagnostics build of the library (-DCT_DIAG): the only one that reads CT_W4_COMPRESS"""
    import ctypes

    from compressed_tensors_amd import _lib

    _lib.load()  # fail loudly if the HIP extension is missing
    lib = ctypes.CDLL(_lib.DIAG_LIB_PATH)
    for name, (argtypes, restype) in _lib._PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    return lib


@pytest.fixture
def codec(diag_lib, monkeypatch):
    """the codec's entry points over the diagnostics library for the duration of one test"""
    from compressed_tensors_amd import _lib, codec

    monkeypatch.setattr(_lib, "_lib", diag_lib)
    return codec


def _pack(codec, monkeypatch, variant, w, s, z, kw):
    monkeypatch.setenv("CT_W4_COMPRESS", variant)
    return codec.quantize_and_pack(w, s, z, **kw)


# (rows, cols, group or None for channel-wise, what): see the module docstring
SHAPES = [
    (8, 256, 128, "one_full_wave"),
    (9, 256, 128, "full_wave_plus_8_lane_tail"),
    (5, 416, 32, "one_lane_tail_group_is_a_lane"),
    (257, 8192, 128, "many_workgroups_last_has_one_wave"),
    (64, 2048, None, "channel_wise"),
    (33, 4096, 128, "zero_points_in_some_waves"),
    (16, 2048, 128, "nan_inf_and_slow_scales"),
]


@functools.lru_cache(maxsize=None)
def _case(rows, cols, group, what, dtype):
    """inputs and the oracle's packed words, built once per (shape, dtype) and left unchanged"""
    gen = torch.Generator().manual_seed(rows * 131 + cols + (1 if dtype is F16 else 0))
    w = torch.randn(rows, cols, generator=gen).to(dtype)
    sym = what != "zero_points_in_some_waves"
    if what == "nan_inf_and_slow_scales":
        # lane 3 and lane 70 (another wave) hold non-finite values: the data test fails there and the exact-division path runs
        w.view(-1)[3 * 32: 3 * 32 + 3] = torch.tensor([float("nan"), float("inf"), float("-inf")]).to(dtype)
        w.view(-1)[70 * 32 + 31] = float("nan")
    s, z = O.calculate_qparams_minmax(w.masked_fill(~torch.isfinite(w.float()), 0), num_bits=4, group_size=group, symmetric=sym)
    if what == "nan_inf_and_slow_scales":
        # scales outside fast_scale_ok in groups of waves 2 and 5 only (a group = 4 lanes, a row = 16 groups = one wave)
        s[2, 1], s[5, 7] = torch.tensor(2.0 ** -20).to(dtype), torch.tensor(3.0e4).to(dtype)
    if not sym:
        # int8 zero points, non-zero in the groups of rows 0 - 1 and 20 only: waves 0 - 3 and 40 - 41 add them, the other 60 waves skip the add
        z = torch.zeros_like(z)
        z[0:2] = torch.randint(-8, 8, z[0:2].shape, generator=gen, dtype=torch.int8)
        z[20] = torch.randint(-8, 8, z[20].shape, generator=gen, dtype=torch.int8)
        z[20, 0] = 3
    kw = dict(num_bits=4, strategy="group" if group else "channel", group_size=group)
    ref = O.pack_quantized_compress({"weight": w, "weight_scale": s, "weight_zero_point": z}, symmetric=sym, **kw)["weight_packed"]
    return w, s, z, kw, sym, ref


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows,cols,group,what", SHAPES, ids=[c[3] for c in SHAPES])
def test_both_variants_equal_each_other_and_the_oracle(codec, dev, monkeypatch, rows, cols, group, what, dtype):
    w, s, z, kw, sym, ref = _case(rows, cols, group, what, dtype)
    wd, sd, zd = w.to(dev), s.to(dev), z.to(dev)
    got = {v: _pack(codec, monkeypatch, v, wd, sd, zd, kw) for v in VARIANTS}
    assert torch.equal(got["plain"], got["lds"])
    for v in VARIANTS:
        assert got[v].shape == ref.shape and torch.equal(got[v].cpu(), ref), v
        back = codec.unpack_and_dequantize(got[v], (rows, cols), sd, None if sym else zd, num_bits=4)
        fq = codec.fake_quantize_tensor(wd, sd, zd, **kw)
        # a NaN weight stays NaN through fake_quantize (no integer cast) and is code 0 in the packed words (the cast): compared elsewhere
        keep = ~torch.isnan(wd)
        assert torch.equal(back[keep], fq[keep]), v
        assert int((~keep).sum()) == (2 if what == "nan_inf_and_slow_scales" else 0)
    if sym:  # the kernels without a zero-point operand
        nz = {v: _pack(codec, monkeypatch, v, wd, sd, None, kw) for v in VARIANTS}
        assert torch.equal(nz["plain"].cpu(), ref) and torch.equal(nz["lds"].cpu(), ref)


def test_unknown_variant_is_an_error(codec, dev, monkeypatch):
    w, s, z, kw, _, _ = _case(8, 256, 128, "one_full_wave", BF16)
    with pytest.raises(Exception, match="CT_W4_COMPRESS"):
        _pack(codec, monkeypatch, "fastest", w.to(dev), s.to(dev), z.to(dev), kw)


def test_input_at_an_offset_that_is_16_byte_but_not_4_kib_aligned(codec, dev, monkeypatch):
    """the weight starts inside a larger allocation at an address that is 16 mod 4096: so does every wave's 4 KiB run"""
    rows, cols = 9, 256
    w, s, z, kw, _, ref = _case(rows, cols, 128, "full_wave_plus_8_lane_tail", BF16)
    big = torch.full((rows * cols + 4096,), 777.0, dtype=BF16, device=dev)
    first = ((16 - big.data_ptr()) % 4096) // 2  # the allocator promises 512-byte alignment only
    view = big[first: first + rows * cols].view(rows, cols)
    view.copy_(w)
    assert view.data_ptr() % 4096 == 16 and view.is_contiguous()
    for v in VARIANTS:
        assert torch.equal(_pack(codec, monkeypatch, v, view, s.to(dev), z.to(dev), kw).cpu(), ref), v
    assert bool((big[:first] == 777.0).all()) and bool((big[first + rows * cols:] == 777.0).all())


def test_last_wave_ends_at_the_last_byte_of_the_allocation(codec, dev, monkeypatch):
    """the input's last byte is the allocation's last byte, for a whole last wave (8 x 256) and for a tail wave (9 x 256): the address range
    the kernel may read is [data_ptr, data_ptr + rows * cols * 2), checked here against the storage, and the result against the oracle"""
    for rows, what in ((8, "one_full_wave"), (9, "full_wave_plus_8_lane_tail")):
        cols = 256
        w, s, z, kw, _, ref = _case(rows, cols, 128, what, BF16)
        store = torch.empty(4096 // 2 + rows * cols, dtype=BF16, device=dev)
        view = store[4096 // 2:].view(rows, cols)
        view.copy_(w)
        end = view.data_ptr() + rows * cols * 2
        assert end == store.data_ptr() + store.untyped_storage().nbytes() == store.untyped_storage().data_ptr() + store.untyped_storage().nbytes()
        lanes = rows * cols // 32
        whole = lanes // 64 * 64  # the lanes that the LDS-DMA serves: whole waves only, 64 bytes per lane
        assert view.data_ptr() + whole * 64 <= end and view.data_ptr() + lanes * 64 == end
        for v in VARIANTS:
            assert torch.equal(_pack(codec, monkeypatch, v, view, s.to(dev), z.to(dev), kw).cpu(), ref), v


def test_two_streams_at_once_equal_one_after_the_other(codec, dev, monkeypatch):
    """two launches of the LDS form on two streams with different inputs (their workgroups share CUs, each with its own LDS) leave what
    the same two launches leave one after the other"""
    monkeypatch.setenv("CT_W4_COMPRESS", "lds")
    kw = dict(num_bits=4, strategy="group", group_size=128)
    gen = torch.Generator(device=dev).manual_seed(7)
    ws = [torch.randn(1025, 4096, device=dev, generator=gen).to(BF16) for _ in range(2)]
    qp = [codec.minmax_qparams(w, num_bits=4, group_size=128, symmetric=True) for w in ws]
    serial = [codec.quantize_and_pack(w, s, z, **kw) for w, (s, z) in zip(ws, qp)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    both = [None, None]
    for rep in range(4):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                both[i] = codec.quantize_and_pack(ws[i], *qp[i], **kw)
    torch.cuda.synchronize()
    assert torch.equal(both[0], serial[0]) and torch.equal(both[1], serial[1])
    assert not torch.equal(serial[0], serial[1])
