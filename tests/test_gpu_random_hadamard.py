"""The random-hadamard kernels (csrc/ct_hadamard_k.hip) on the MI355X against the reference's outputs (tests/golden/random_hadamard*,
tools/gen_golden_random_hadamard.py): tier A (online float32, integer-valued inputs) and tier C (offline float64) equal in EVERY
element by value, tier B (online float32, random inputs) inside the derived bound in every element; non-finite rows stay in their
block; plain followed by transposed is the identity; apply_transform_config(hadamard_weights=...) on a CUDA model; graph capture;
install(patch_transforms=True, patch_random_hadamard=True) against the staged reference.  Everything here reads fixtures only.

Figures of the first run on an MI355X (worst |y - exact| / tolerance over the tier B cases): see DESIGN.md 5.13."""
import collections
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _random_hadamard_cases as C  # noqa: E402
import ref_import  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "random_hadamard_manifest.json")) as _f:
    _M = json.load(_f)
MANIFEST, MODEL = _M["cases"], _M["model"]
DEV = torch.device("cuda:0")
EXACT = sorted(k for k, e in MANIFEST.items() if e["recipe"]["tier"] in ("A", "C"))
BOUNDED = sorted(k for k, e in MANIFEST.items() if e["recipe"]["tier"] == "B")


@pytest.fixture()
def counted():
    import compressed_tensors_amd.codec as codec_mod

    counts = collections.Counter()
    saved = codec_mod.call

    def call(name, *a):
        counts[name] += 1
        return saved(name, *a)

    codec_mod.call = call
    try:
        yield counts
    finally:
        codec_mod.call = saved


@pytest.fixture(scope="module")
def golden_tensors():
    from safetensors.torch import load_file

    return load_file(os.path.join(GOLDEN, "random_hadamard.safetensors"))


def _factors(golden_tensors, n, device=DEV):
    had_k = golden_tensors.get(f"had_k.{n}")
    return (None if had_k is None else had_k.to(device)), golden_tensors[f"signs.{n}"].to(device)


def _transform(recipe, golden_tensors):
    """our RandomHadamardTransform for a recipe: location, module type and inverse select dimension, form and accumulator"""
    import compressed_tensors_amd as cta
    from compressed_tensors_amd.transform import HadamardFactors, RandomHadamardTransform

    n = recipe["size"]
    had_k, signs = _factors(golden_tensors, n)
    scheme = cta.TransformScheme("random-hadamard", precision=torch.float32)
    args = cta.TransformArgs(["x"], recipe["location"], inverse=recipe["inverse"])
    return RandomHadamardTransform(HadamardFactors(n, *C.SIZES[n], had_k, signs), scheme, args, getattr(torch.nn, recipe["module"]))


@pytest.mark.parametrize("key", EXACT)
def test_exact_tiers_equal_the_reference_in_every_element(key, counted, golden_tensors):
    entry = MANIFEST[key]
    r = entry["recipe"]
    x = C.synth(r)
    assert C.sha(x) == entry["x_sha256"], "the recipe no longer synthesises the reference's input"
    t = _transform(r, golden_tensors)
    assert t.precision is C.precision_of(r) and t.dim == C.dim_of(r) and t.transposed == C.transposed_of(r)
    out = t(x.to(DEV))
    torch.cuda.synchronize()
    assert str(out.dtype).replace("torch.", "") == entry["out"]["dtype"] and list(out.shape) == entry["out"]["shape"]
    if entry["stored"]:
        ref = golden_tensors[f"{key}.out"]
        bad = (out.cpu() != ref).nonzero()
        assert bad.numel() == 0, f"{bad.shape[0]} elements differ from the stored reference, first at {bad[0].tolist()}"
    assert C.sha(out) == entry["out"]["sha256"], "differs from the reference (compared by value, every element)"
    form = "ct_hadamard_k_cols" if (t.dim == 0 and x.shape[-1] != 1 and x.dim() > 1) else "ct_hadamard_k_rows"
    assert dict(counted) == {form: 1}, counted  # ONE library call per transform, nothing else


@pytest.mark.parametrize("key", BOUNDED)
def test_random_inputs_stay_inside_the_derived_bound(key, golden_tensors):
    from compressed_tensors_amd import codec

    entry = MANIFEST[key]
    r = entry["recipe"]
    x = C.synth(r)
    assert C.sha(x) == entry["x_sha256"], "the recipe no longer synthesises the generator's input"
    had_k, signs = _factors(golden_tensors, r["size"])
    tr = C.transposed_of(r)
    out = codec.hadamard_k_transform(x.to(DEV), r["size"], had_k, signs, dim=C.dim_of(r), precision=torch.float32, transposed=tr).cpu()
    exact, tol = C.bound(x, r["size"], None if had_k is None else had_k.cpu(), signs.cpu(), tr, C.dim_of(r))
    err = (out.to(C.F64) - exact).abs()
    print(f"{key}: worst |y - exact| / tolerance = {(err / tol).max().item():.4f}")
    bad = (err > tol).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} of {x.numel()} elements outside the bound, first at {bad[0].tolist()}"


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("transposed", [False, True])
def test_a_non_finite_row_stays_in_its_block(dtype, transposed, golden_tensors):
    """K = 172 is padded to 176 in the matrix-core form: the pad rows of the staged operand must be real zeros, and a NaN / inf in
    one block must not reach its neighbours (a group of 4 blocks shares a workgroup at M = 8)"""
    from compressed_tensors_amd import codec

    n = 1376
    had_k, signs = _factors(golden_tensors, n)
    x = C.synth(dict(gen="ints", dtype=dtype, shape=[9, n], salt=5))
    clean = codec.hadamard_k_transform(x.to(DEV), n, had_k, signs, transposed=transposed).cpu()
    assert bool(torch.isfinite(clean).all())
    dirty = x.clone()
    dirty[1, 1375] = float("nan")
    dirty[2, 0] = float("inf")
    dirty[6, 700] = float("-inf")
    out = codec.hadamard_k_transform(dirty.to(DEV), n, had_k, signs, transposed=transposed).cpu()
    for row in (0, 3, 4, 5, 7, 8):
        assert torch.equal(out[row], clean[row]), f"row {row} changed"
    assert bool(torch.isnan(out[1]).all())  # a NaN reaches every output of ITS block
    assert not bool(torch.isfinite(out[2]).any()) and not bool(torch.isfinite(out[6]).any())


@pytest.mark.parametrize("n", [1376, 5120, 14336, 96, 4096])
def test_plain_then_transposed_is_the_identity(n, golden_tensors):
    """W W^T = n I: float32 values through both forms come back.  y carries one float32 rounding per element, which the second
    rotation (orthogonal: |sum_j W_ij e_j| / sqrt(n) <= sum|e_j| / sqrt(n)) spreads; then the second call's own tier B tolerance."""
    from compressed_tensors_amd import codec

    had_k, signs = _factors(golden_tensors, n)
    x = C.synth(dict(gen="ints", dtype="f32", shape=[3, n], salt=n % 97))
    y = codec.hadamard_k_transform(x.to(DEV), n, had_k, signs)
    back = codec.hadamard_k_transform(y, n, had_k, signs, transposed=True).cpu()
    _, tol = C.bound(y.cpu(), n, None if had_k is None else had_k.cpu(), signs.cpu(), True)
    tol = tol + 2.0 ** -24 * y.cpu().to(C.F64).abs().sum(-1, keepdim=True) / n ** 0.5
    err = (back.to(C.F64) - x.to(C.F64)).abs()
    print(f"n = {n}: worst |back - x| / tolerance = {(err / tol).max().item():.4f}")
    assert bool((err <= tol).all())


def test_declined_on_the_device(golden_tensors):
    from compressed_tensors_amd import codec

    had_k, signs = _factors(golden_tensors, 1376)
    x = torch.zeros(2, 1376, dtype=C.BF16, device=DEV)
    with pytest.raises(NotImplementedError, match="GPU tensors"):
        codec.hadamard_k_transform(x.cpu(), 1376, had_k.cpu(), signs.cpu())
    with pytest.raises(NotImplementedError, match="contiguous"):
        codec.hadamard_k_transform(torch.zeros(1376, 2, dtype=C.BF16, device=DEV).t(), 1376, had_k, signs)
    with pytest.raises(NotImplementedError, match="aligned"):
        codec.hadamard_k_transform(torch.zeros(2 * 1376 + 8, dtype=C.BF16, device=DEV)[4:-4].view(2, 1376), 1376, had_k, signs)
    with pytest.raises(ValueError, match="had_k must be"):
        codec.hadamard_k_transform(x, 1376, had_k.to(torch.int32), signs)
    with pytest.raises(ValueError, match="signs must be"):
        codec.hadamard_k_transform(x, 1376, had_k, signs[:-8])
    assert codec.hadamard_k_transform(x[:0], 1376, had_k, signs).shape == (0, 1376)


def test_without_factors_it_is_the_sylvester_rotation():
    from compressed_tensors_amd import codec

    x = C.synth(dict(gen="ints", dtype="bf16", shape=[5, 512], salt=3)).to(DEV)
    assert torch.equal(codec.hadamard_k_transform(x, 512), codec.hadamard_transform(x, 512))


def _model_weights(golden_tensors, device):
    """a stand-in for upstream's random_hadamard_matrix: the three weights upstream drew for the fixture model, rebuilt from their
    factors in the order apply_transform_config asks for them (one per config group)"""
    order = list(C.MODEL_CONFIG["config_groups"])
    calls = []

    def hadamard_weights(size, dtype, dev, gen):
        assert size == C.MODEL_SIZE and isinstance(gen, torch.Generator)
        group = order[len(calls)]
        calls.append((group, dtype))
        w = C.weight_from_factors(size, golden_tensors[f"had_k.{size}"], golden_tensors[f"model.signs.{group}"], torch.float32)
        return w.to(device=dev, dtype=dtype)

    return hadamard_weights, calls


def test_apply_transform_config_on_a_cuda_model(golden_tensors, counted):
    import compressed_tensors_amd as cta
    from compressed_tensors_amd.transform import RandomHadamardTransform, match_named_modules

    m = C.model().to(DEV)
    with pytest.raises(NotImplementedError, match="random-hadamard"):
        cta.apply_transform_config(m, C.MODEL_CONFIG)  # without the constructor: as before
    assert C.sha(m[0].weight.data) == C.sha(C.model()[0].weight.data)  # nothing was changed
    hadamard_weights, calls = _model_weights(golden_tensors, DEV)
    cta.apply_transform_config(m, C.MODEL_CONFIG, hadamard_weights=hadamard_weights)
    torch.cuda.synchronize()
    assert calls == [("u", torch.float64), ("v", torch.float32), ("w", torch.float64)]  # one draw per (group, size), at the first use's precision
    assert dict(counted) == {"ct_hadamard_k_cols": 1, "ct_hadamard_k_rows": 2}, counted  # weight + bias of 0, weight of 1
    for name, t in (("0.weight", m[0].weight), ("0.bias", m[0].bias), ("1.weight", m[1].weight)):
        assert list(t.shape) == MODEL[name]["shape"] and C.sha(t.data) == MODEL[name]["sha256"], f"{name}: tier C result expected"
    transforms = [mod for mod in m.modules() if isinstance(mod, RandomHadamardTransform)]
    assert len(transforms) == 1 and transforms[0].had_k.dtype is torch.int8 and transforms[0].signs.numel() == C.MODEL_SIZE
    assert [n for n, _ in match_named_modules(m, ["re:.*"])] == ["", "0", "1"]  # the transform submodule (1.v_input) is internal
    seen = []
    m[1].register_forward_pre_hook(lambda _, inputs: seen.append(inputs[0]))
    x = C.synth(dict(gen="ints", dtype="bf16", shape=[2, 5, C.MODEL_SIZE], salt=77))
    m[1](x.to(DEV))
    assert C.sha(seen[0]) == MODEL["1.input"]["sha256"]  # tier A result
    assert cta.transform.fuse_input_quantization(m) == []  # not a Sylvester rotation: left alone


def test_the_online_form_is_one_launch_and_does_not_synchronise(golden_tensors, counted):
    from compressed_tensors_amd import codec

    had_k, signs = _factors(golden_tensors, 14336)
    x = torch.randn(8, 14336, device=DEV).to(C.BF16)
    assert codec.plan_hadamard_k(x.shape, x.dtype, 14336, 224).form == "mfma"
    codec.hadamard_k_transform(x, 14336, had_k, signs)  # warm
    counted.clear()
    torch.cuda.set_sync_debug_mode("error")
    try:
        codec.hadamard_k_transform(x, 14336, had_k, signs)
        codec.hadamard_k_transform(x.float(), 14336, had_k, signs, transposed=True)  # the vector form: two launches, one entry
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert dict(counted) == {"ct_hadamard_k_rows": 2}


def test_c_abi_entries_are_graph_capturable(golden_tensors):
    """the entries allocate nothing and never synchronise: captured once, replayed on changing inputs"""
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    n, rows = 1376, 12
    had_k, signs = _factors(golden_tensors, n)
    s64 = golden_tensors["signs.64"].to(DEV)
    x = torch.zeros(rows, n, dtype=C.BF16, device=DEV)
    xc = torch.zeros(n, 16, dtype=C.BF16, device=DEV)
    outs = [torch.empty_like(x) for _ in range(3)] + [torch.empty_like(xc)]
    B = _lib.BF16
    ws_rows = torch.empty(lib.ct_hadamard_k_workspace_bytes(B, x.numel(), n, 172, 1, 0), dtype=torch.uint8, device=DEV)
    ws_cols = torch.empty(lib.ct_hadamard_k_workspace_bytes(B, xc.numel(), n, 172, 1, 1), dtype=torch.uint8, device=DEV)
    assert lib.ct_hadamard_k_workspace_bytes(B, x.numel(), n, 172, 0, 0) == 0

    def launches(stream):
        rcs = [lib.ct_hadamard_k_rows(x.data_ptr(), outs[0].data_ptr(), B, x.numel(), n, 172, had_k.data_ptr(), signs.data_ptr(), 0, 0, None, stream),
               lib.ct_hadamard_k_rows(x.data_ptr(), outs[1].data_ptr(), B, x.numel(), n, 172, had_k.data_ptr(), signs.data_ptr(), 1, 1, ws_rows.data_ptr(), stream),
               lib.ct_hadamard_k_rows(x.data_ptr(), outs[2].data_ptr(), B, x.numel(), 64, 1, None, s64.data_ptr(), 0, 0, None, stream),
               lib.ct_hadamard_k_cols(xc.data_ptr(), outs[3].data_ptr(), B, n, 16, n, 172, had_k.data_ptr(), signs.data_ptr(), 0, 1, ws_cols.data_ptr(), stream)]
        assert not any(rcs), (rcs, _lib.last_error())

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        launches(_lib.stream_on(DEV, side.cuda_stream))  # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches(_lib.stream_on(DEV, torch.cuda.current_stream(DEV).cuda_stream))
    hk, sg = had_k.cpu(), signs.cpu()
    for rep in range(3):
        a = C.synth(dict(gen="ints", dtype="bf16", shape=[rows, n], salt=rep))
        b = C.synth(dict(gen="grid", dtype="bf16", shape=[n, 16], salt=rep))
        x.copy_(a.to(DEV))
        xc.copy_(b.to(DEV))
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[0].cpu(), C.structured(a, n, hk, sg, False, -1, C.F32))
        assert torch.equal(outs[1].cpu(), C.structured(a, n, hk, sg, True, -1, C.F64))
        assert torch.equal(outs[2].cpu(), C.structured(a, 64, None, s64.cpu(), False, -1, C.F32))
        assert torch.equal(outs[3].cpu(), C.structured(b, n, hk, sg, False, 0, C.F64))


# ---- install(patch_transforms=True, patch_random_hadamard=True) against the staged reference -------------------------------------------
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
    if not ref_import.available():
        pytest.skip("no reference on this machine (neither the live tree nor the staged archive)")
    ref_import.import_reference()
    try:
        import compressed_tensors.transform as up_t
        import compressed_tensors.transform.factory.hadamard as up_h
        import compressed_tensors.transform.factory.random_hadamard as up_r
    except ImportError as e:
        pytest.skip(f"upstream's transform package cannot be imported on this machine: {e!r}")
    import compressed_tensors_amd.install as ct_amd

    names = ("ct_hadamard_k_rows", "ct_hadamard_k_cols", "ct_hadamard_rows", "ct_hadamard_cols")
    orig_forward = up_h.HadamardTransform.forward
    # the table of known matrices does not travel with the staged reference: the factory draws the fixture's weights instead
    saved_matrix = up_r.random_hadamard_matrix
    counts, restore = _count_lib(names)
    try:
        for flag, want in ((False, {}), (True, {"ct_hadamard_k_cols": 1, "ct_hadamard_k_rows": 2})):
            up_r.random_hadamard_matrix, _ = _model_weights(golden_tensors, DEV)
            ct_amd.install(patch_transforms=True, patch_random_hadamard=flag)
            try:
                counts.clear()
                m = C.model().to(DEV)
                up_t.apply_transform_config(m, up_t.TransformConfig.model_validate(C.MODEL_CONFIG))
                torch.cuda.synchronize()
                assert dict(counts) == want, (flag, counts)  # patch_transforms alone behaves as before: upstream's eager forward
                for name, t in (("0.weight", m[0].weight), ("0.bias", m[0].bias), ("1.weight", m[1].weight)):
                    assert C.sha(t.data) == MODEL[name]["sha256"], f"{name}: tier C result expected (flag {flag})"
                seen = []
                m[1].register_forward_pre_hook(lambda _, inputs: seen.append(inputs[0]))
                x = C.synth(dict(gen="ints", dtype="bf16", shape=[2, 5, C.MODEL_SIZE], salt=77))
                m[1](x.to(DEV))
                m[1](x.to(DEV))  # the factors are cached on the transform
                assert counts["ct_hadamard_k_rows"] == (4 if flag else 0) and C.sha(seen[0]) == MODEL["1.input"]["sha256"] == C.sha(seen[1])
                if flag:
                    online = [t for t in m.modules() if isinstance(t, up_h.HadamardTransform)][0]
                    assert online._ct_factors[0].k == 172 and online._ct_factors[0].signs.is_cuda
                    # a CPU value on a tagged transform stays upstream's
                    counts.clear()
                    xc = x[0, :2].float()
                    online_cpu = up_h.HadamardTransform(torch.nn.Parameter(online.weight.data.cpu(), requires_grad=False), None, online.scheme, online.args, online.module_type)
                    online_cpu._ct_random = True
                    assert torch.equal(online_cpu(xc), orig_forward(online_cpu, xc)) and sum(counts.values()) == 0
            finally:
                ct_amd.uninstall()
    finally:
        up_r.random_hadamard_matrix = saved_matrix
        restore()
    assert up_h.HadamardTransform.forward is orig_forward
