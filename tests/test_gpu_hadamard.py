"""The fast Walsh-Hadamard kernels (csrc/ct_hadamard.hip) on the MI355X against the reference's outputs (tests/golden/hadamard*,
tools/gen_golden_hadamard.py): tier A (online float32, integer-valued inputs) and tier C (offline float64) equal in EVERY element
by value, tier B (online float32, random inputs) inside the derived bound in every element; apply_transform_config on a CUDA
model; launch discipline; install(patch_transforms=True) against the staged reference.

Figures of the first run on an MI355X (tests/_hadamard_cases.py::bound, worst |y - exact| / tolerance over all tier B cases):
see DESIGN.md 5.11."""
import collections
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hadamard_cases as C  # noqa: E402
import ref_import  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "hadamard_manifest.json")) as _f:
    MANIFEST = json.load(_f)["cases"]
DEV = torch.device("cuda:0")
EXACT = sorted(k for k, e in MANIFEST.items() if e["recipe"]["tier"] in ("A", "C"))
BOUNDED = sorted(k for k, e in MANIFEST.items() if e["recipe"]["tier"] == "B")


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


@pytest.fixture(scope="module")
def golden_tensors():
    from safetensors.torch import load_file

    return load_file(os.path.join(GOLDEN, "hadamard.safetensors"))


def _transform(recipe, head_dim=None):
    """our HadamardTransform for a recipe: location and module type select the dimension and the accumulator"""
    import compressed_tensors_amd as cta

    scheme = cta.TransformScheme("hadamard", head_dim=head_dim, precision=torch.float32)
    args = cta.TransformArgs(["x"], recipe["location"], inverse=recipe["inverse"])
    return cta.HadamardTransform(recipe["size"], scheme, args, getattr(torch.nn, recipe["module"]))


@pytest.mark.parametrize("key", EXACT)
def test_exact_tiers_equal_the_reference_in_every_element(key, counted, golden_tensors):
    entry = MANIFEST[key]
    r = entry["recipe"]
    x = C.synth(r)
    assert C.sha(x) == entry["x_sha256"], "the recipe no longer synthesises the reference's input"
    t = _transform(r)
    assert t.precision is C.precision_of(r) and t.dim == C.dim_of(r)
    out = t(x.to(DEV))
    torch.cuda.synchronize()
    assert str(out.dtype).replace("torch.", "") == entry["out"]["dtype"] and list(out.shape) == entry["out"]["shape"]
    if entry["stored"]:
        ref = golden_tensors[f"{key}.out"]
        bad = (out.cpu() != ref).nonzero()
        assert bad.numel() == 0, f"{bad.shape[0]} elements differ from the stored reference, first at {bad[0].tolist()}"
    assert C.sha(out) == entry["out"]["sha256"], "differs from the reference (compared by value, every element)"
    form = "ct_hadamard_cols" if (t.dim == 0 and x.shape[-1] != 1 and x.dim() > 1) else "ct_hadamard_rows"
    assert dict(counted) == {form: 1}, counted  # ONE library call per transform, nothing else


@pytest.mark.parametrize("key", BOUNDED)
def test_random_inputs_stay_inside_the_derived_bound(key):
    from compressed_tensors_amd import codec

    entry = MANIFEST[key]
    r = entry["recipe"]
    x = C.synth(r)
    assert C.sha(x) == entry["x_sha256"], "the recipe no longer synthesises the generator's input"
    out = codec.hadamard_transform(x.to(DEV), r["size"], dim=C.dim_of(r), precision=torch.float32).cpu()
    exact, tol = C.bound(x, r["size"], C.dim_of(r))
    err = (out.to(C.F64) - exact).abs()
    print(f"{key}: worst |y - exact| / tolerance = {(err / tol).max().item():.4f}")
    bad = (err > tol).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} of {x.numel()} elements outside the bound, first at {bad[0].tolist()}"


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("n,precision", [(16384, torch.float32), (16384, torch.float64)])
def test_sizes_beyond_8192(n, precision, dtype):
    """16384 (32768 is declined: DESIGN.md 10): against the butterfly restatement (tests/test_hadamard.py shows it equals the reference), on
    integer-valued inputs, where every order of summation is exact"""
    from compressed_tensors_amd import codec

    x = C.synth(dict(gen="ints", dtype=dtype, shape=[3, n], salt=n % 251))
    out = codec.hadamard_transform(x.to(DEV), n, precision=precision).cpu()
    assert torch.equal(out, C.butterfly(x, n, -1, precision))


def test_declined_sizes_and_tensors():
    from compressed_tensors_amd import codec

    x = torch.zeros(2, 65536, dtype=C.BF16, device=DEV)
    with pytest.raises(NotImplementedError):
        codec.hadamard_transform(x, 32768)
    with pytest.raises(NotImplementedError):
        codec.hadamard_transform(x[:, :16384], 16384)  # not contiguous
    with pytest.raises(NotImplementedError):
        codec.hadamard_transform(x, 32768, precision=torch.float64)
    with pytest.raises(NotImplementedError):
        codec.hadamard_transform(x.reshape(-1)[1:129], 128)  # not 16-byte aligned
    with pytest.raises(NotImplementedError):
        codec.hadamard_transform(x.cpu(), 64)
    assert codec.hadamard_transform(x[:0], 64).shape == (0, 65536)
    ones = torch.ones(5, 3, dtype=C.F32, device=DEV)
    assert torch.equal(codec.hadamard_transform(ones, 1), ones)  # H_1 = [[1]]
    assert torch.equal(codec.hadamard_transform(ones, 1, dim=0, precision=torch.float64), ones)


@pytest.mark.parametrize("n,stride", [(2, 1), (128, 8), (8192, 512)])
def test_division_by_sqrt_n_is_the_ieee_quotient(n, stride):
    """rows (x, 0, ..., 0) rotate to x / sqrt(n) in every element.  n = 2: ALL 2^24 float32 values of two binades (every
    significand); the larger sizes (the same quotient code behind the other kernels, sqrt(n) scaled by a power of two) every
    `stride`-th of them; always both signs and the values the fast quotient hands to the IEEE division (zeros, tiny, huge, inf).
    Against torch's float32 division on the same device."""
    from compressed_tensors_amd import codec

    bits = torch.arange(0, 1 << 24, stride, dtype=torch.int32) + (127 << 23)  # [1, 4)
    edge = torch.tensor([0.0, -0.0, 1e-45, 3e-39, 2.0 ** -91, 2.0 ** -90, 1.5e-27, 2.0 ** 100, 1.1 * 2.0 ** 100, 3e38, float("inf"), -float("inf")])
    xs = torch.cat([bits.view(torch.float32), -bits[:: 4097].view(torch.float32), edge])
    sn = torch.tensor(n, dtype=torch.float64).sqrt().to(torch.float32)
    x = torch.zeros(len(xs), n, dtype=torch.float32, device=DEV)
    x[:, 0] = xs.to(DEV)
    out = codec.hadamard_transform(x, n)
    del x
    want = xs.to(DEV) / sn.to(DEV)
    bad = (out != want.unsqueeze(1)).nonzero()
    assert bad.numel() == 0, (n, bad.shape[0], xs[bad[0, 0]].item())
    # a unit that mixes fast and slow values (a zero next to ordinary ones) takes the IEEE division as a whole
    mixed = torch.zeros(8, n, dtype=torch.float32, device=DEV)
    mixed[:, 0] = torch.tensor([1.0, 0.0, 3.0, -5.0, 2.0 ** -100, 7.0, 1e30, 1e38], device=DEV)
    assert torch.equal(codec.hadamard_transform(mixed, n)[:, 0], mixed[:, 0] / sn.to(DEV))


def test_negative_zero_rows_compare_by_value():
    from compressed_tensors_amd import codec

    x = torch.full((3, 256), -0.0, dtype=C.BF16, device=DEV)
    out = codec.hadamard_transform(x, 256)
    assert torch.equal(out, torch.zeros_like(out)) and C.sha(out) == C.sha(torch.zeros(3, 256, dtype=C.BF16))


def test_apply_transform_config_on_a_cuda_model(golden_tensors, counted, tmp_path):
    import compressed_tensors_amd as cta

    m = C.model().to(DEV)
    cfg = cta.TransformConfig.from_dict(C.MODEL_CONFIG)
    cta.apply_transform_config(m, cfg)
    torch.cuda.synchronize()
    # weight_output of the first Linear: the column form for the weight, the row form for the bias; weight_input of the second: rows
    assert dict(counted) == {"ct_hadamard_cols": 1, "ct_hadamard_rows": 2}, counted
    for name, t in (("model.0.weight", m[0].weight), ("model.0.bias", m[0].bias), ("model.1.weight", m[1].weight)):
        assert torch.equal(t.data.cpu(), golden_tensors[name]), f"{name} differs from upstream's fused tensor"
    assert m.transform_config is cfg and isinstance(m[1].v_input, cta.HadamardTransform) and not hasattr(m[0], "u_weight_output")
    seen = []
    m[1].register_forward_pre_hook(lambda _, inputs: seen.append(inputs[0]))  # after the prepended rotation
    x = C.synth(dict(gen="ints", dtype="bf16", shape=[2, 5, 128], salt=77))
    m[1](x.to(DEV))
    assert len(seen) == 1 and torch.equal(seen[0].cpu(), C.butterfly(x, 64)), "the second Linear does not receive the rotated input"
    assert counted["ct_hadamard_rows"] == 3
    # a model rotated here and then compressed writes upstream's own dump of the config
    cta.ModelCompressor.from_pretrained_model(m).update_config(str(tmp_path))
    with open(tmp_path / "config.json") as f, open(os.path.join(GOLDEN, "hadamard_transform_config.json")) as g:
        assert json.load(f)["quantization_config"]["transform_config"] == json.load(g)


def _kernels_of(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@pytest.mark.parametrize("shape,n,precision", [((2, 64, 4096), 4096, torch.float32), ((65, 8192), 128, torch.float32), ((3, 8192), 8192, torch.float32),
                                               ((512, 1024), 1024, torch.float64), ((7, 16), 2, torch.float32)])
def test_row_form_is_one_launch_and_nothing_else(shape, n, precision, counted):
    from compressed_tensors_amd import codec

    x = torch.randn(shape, device=DEV).to(C.BF16)
    codec.hadamard_transform(x, n, precision=precision)
    assert dict(counted) == {"ct_hadamard_rows": 1}
    kernels = _kernels_of(lambda: codec.hadamard_transform(x, n, precision=precision))
    assert len(kernels) == 1 and "had_" in kernels[0], kernels  # no memset, no copy, no cast


def test_column_form_launches(counted):
    from compressed_tensors_amd import codec

    x = torch.randn(1024, 520, device=DEV).to(C.BF16)
    kernels = _kernels_of(lambda: codec.hadamard_transform(x, 1024, dim=0, precision=torch.float64))
    assert len(kernels) == 3 and sum("transpose" in k for k in kernels) == 2 and sum("had_" in k for k in kernels) == 1, kernels
    assert dict(counted) == {"ct_hadamard_cols": 2}


def test_no_host_synchronisation():
    from compressed_tensors_amd import codec

    x = torch.randn(16, 4096, device=DEV).to(C.BF16)
    calls = [lambda: codec.hadamard_transform(x, 4096), lambda: codec.hadamard_transform(x, 128), lambda: codec.hadamard_transform(x, 16, dim=0, precision=torch.float64)]
    for fn in calls:
        fn()  # warm: the first call loads the library
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fn in calls:
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_c_abi_entries_are_graph_capturable():
    """the entries allocate nothing and never synchronise: captured once, replayed on changing inputs"""
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    x = torch.zeros(64, 4096, dtype=C.BF16, device=DEV)
    outs = [torch.empty_like(x) for _ in range(4)]
    ws = torch.empty_like(x)
    B = _lib.BF16

    def launches(stream):
        rcs = [lib.ct_hadamard_rows(x.data_ptr(), outs[0].data_ptr(), B, x.numel(), 4096, 0, stream),
               lib.ct_hadamard_rows(x.data_ptr(), outs[1].data_ptr(), B, x.numel(), 128, 0, stream),
               lib.ct_hadamard_rows(x.data_ptr(), outs[2].data_ptr(), B, x.numel(), 2048, 1, stream),
               lib.ct_hadamard_cols(x.data_ptr(), outs[3].data_ptr(), ws.data_ptr(), B, 64, 4096, 64, 1, stream)]
        assert not any(rcs), (rcs, _lib.last_error())

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        launches(_lib.stream_on(DEV, side.cuda_stream))  # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches(_lib.stream_on(DEV, torch.cuda.current_stream(DEV).cuda_stream))
    for rep in range(3):
        xc = C.synth(dict(gen="ints", dtype="bf16", shape=[64, 4096], salt=rep))
        x.copy_(xc.to(DEV))
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[0].cpu(), C.butterfly(xc, 4096)) and torch.equal(outs[1].cpu(), C.butterfly(xc, 128))
        assert torch.equal(outs[2].cpu(), C.butterfly(xc, 2048, -1, C.F64)) and torch.equal(outs[3].cpu(), C.butterfly(xc, 64, 0, C.F64))


# ---- install(patch_transforms=True) against the staged reference ----------------------------------------------------------------
def _upstream_transform():
    if not ref_import.available():
        pytest.skip("no reference on this machine (neither the live tree nor the staged archive)")
    ref_import.import_reference()
    try:
        import compressed_tensors.transform as up_t
        import compressed_tensors.transform.factory.hadamard as up_h
    except ImportError as e:
        pytest.skip(f"upstream's transform package cannot be imported on this machine: {e!r}")
    return up_t, up_h


def _count_lib(names):
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    counts = collections.Counter()
    saved = {n: getattr(lib, n) for n in names}
    for n in saved:
        def counted(*a, _o=saved[n], _n=n):
            counts[_n] += 1
            return _o(*a)
        setattr(lib, n, counted)

    def restore():
        for n, f in saved.items():
            setattr(lib, n, f)

    return counts, restore


def test_upstream_apply_transform_config_under_install(golden_tensors):
    up_t, up_h = _upstream_transform()
    import compressed_tensors_amd.install as ct_amd

    orig_create, orig_forward = up_h.HadamardFactory.create_transform, up_h.HadamardTransform.forward
    counts, restore = _count_lib(("ct_hadamard_rows", "ct_hadamard_cols"))
    ct_amd.install(patch_transforms=True)
    try:
        m = C.model().to(DEV)
        up_t.apply_transform_config(m, up_t.TransformConfig.model_validate(C.MODEL_CONFIG))
        torch.cuda.synchronize()
        assert dict(counts) == {"ct_hadamard_cols": 1, "ct_hadamard_rows": 2}, counts  # upstream's own loop reached the kernels
        for name, t in (("model.0.weight", m[0].weight), ("model.0.bias", m[0].bias), ("model.1.weight", m[1].weight)):
            assert torch.equal(t.data.cpu(), golden_tensors[name]), f"{name}: tier C result expected"
        seen = []
        m[1].register_forward_pre_hook(lambda _, inputs: seen.append(inputs[0]))
        x = C.synth(dict(gen="ints", dtype="bf16", shape=[2, 5, 128], salt=77))
        m[1](x.to(DEV))
        assert counts["ct_hadamard_rows"] == 3 and torch.equal(seen[0].cpu(), C.butterfly(x, 64))  # tier A result
        # randomize=True stays upstream's: zero counted calls, upstream's own result
        counts.clear()
        lin = torch.nn.Linear(128, 128, bias=False, dtype=C.BF16).to(DEV)
        scheme = up_t.TransformScheme(type="hadamard", randomize=True)
        t = up_t.TransformFactory.from_scheme(scheme, name="p", seed=3).create_transform(lin, up_t.TransformArgs(targets=["Linear"], location="input"))
        xr = C.synth(dict(gen="ints", dtype="bf16", shape=[4, 128], salt=9)).to(DEV)
        got = t(xr)
        assert sum(counts.values()) == 0 and torch.equal(got, orig_forward(t, xr))
        # a CPU value on a tagged transform too
        plain = up_t.TransformFactory.from_scheme(up_t.TransformScheme(type="hadamard"), name="q").create_transform(
            torch.nn.Linear(128, 128, bias=False, dtype=C.BF16), up_t.TransformArgs(targets=["Linear"], location="input"))
        assert torch.equal(plain(xr.cpu()), C.butterfly(xr.cpu(), 128)) and sum(counts.values()) == 0
    finally:
        ct_amd.uninstall()
        restore()
    assert up_h.HadamardFactory.create_transform is orig_create and up_h.HadamardTransform.forward is orig_forward
