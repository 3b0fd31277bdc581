"""The permuted Hadamard rotation (`randomize=True`; csrc/ct_hadamard_perm.hip) on the MI355X: the one launch and the composition
index_select -> unpermuted entry -> index_select against the reference's recorded outputs (tests/golden/hadamard_perm*,
tools/gen_golden_hadamard_perm.py) in every element; the one launch against the composition bit for bit on random inputs;
apply_transform_config(randomize=True) on a CUDA model; launch discipline; install(patch_permuted_hadamard=True) against the staged
reference.  The fused form is forced with form="fused" whatever HADAMARD_PERM_MEASURED_FASTER dispatches."""
import collections
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hadamard_cases as H  # noqa: E402
import _hadamard_perm_cases as C  # noqa: E402
import ref_import  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "hadamard_perm_manifest.json")) as _f:
    _M = json.load(_f)
MANIFEST, MODEL = _M["cases"], _M["model"]
DEV = torch.device("cuda:0")
ALL_N = C.GROUP_SIZES + C.BLOCK_SIZES


@pytest.fixture(scope="module")
def golden_tensors():
    from safetensors.torch import load_file

    g = load_file(os.path.join(GOLDEN, "hadamard_perm.safetensors"))
    g.update({f"rh.{k}": v for k, v in load_file(os.path.join(GOLDEN, "random_hadamard.safetensors")).items() if k.startswith(("signs.", "had_k."))})
    return g


@pytest.fixture()
def counted():
    """calls of the library per entry, counted where codec makes them"""
    import compressed_tensors_amd.codec as codec_mod

    counts, saved = collections.Counter(), codec_mod.call

    def call(name, *a):
        counts[name] += 1
        return saved(name, *a)

    codec_mod.call = call
    try:
        yield counts
    finally:
        codec_mod.call = saved


def _perm(golden_tensors, kind, n):
    return golden_tensors[f"perm.{kind}.{n}"].to(torch.int64)


def _factors(golden_tensors, r):
    if r["type"] == "hadamard":
        return None, None
    hk = golden_tensors.get(f"rh.had_k.{r['size']}")
    return (None if hk is None else hk.to(DEV)), golden_tensors[f"rh.signs.{r['size']}"].to(DEV)


def _run(x, r, tables, had_k, signs, form):
    from compressed_tensors_amd import codec

    kw = dict(dim=C.dim_of(r), precision=C.precision_of(r), perm=tables, form=form)
    if r["type"] == "hadamard":
        return codec.hadamard_transform(x, r["size"], **kw)
    return codec.hadamard_k_transform(x, r["size"], had_k, signs, transposed=C.transposed_of(r), **kw)


def _has_fused(r):
    from compressed_tensors_amd import codec

    k = C.SIZES[r["size"]][0] if r["type"] == "random-hadamard" else 1
    return k == 1 and r["size"] <= codec.HADAMARD_PERM_MAX_SIZE[C.precision_of(r)]


def _bits(t):
    t = t + 0.0
    return t.view(torch.int32 if t.dtype is torch.float32 else torch.int16)


# ---- the reference's recorded outputs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_exact_tiers_equal_the_reference_in_every_element(key, golden_tensors, counted):
    from compressed_tensors_amd import codec

    entry = MANIFEST[key]
    r = entry["recipe"]
    x = C.synth(r)
    assert C.sha(x) == entry["x_sha256"], "the recipe no longer synthesises the reference's input"
    tables = codec.hadamard_perm_tables(_perm(golden_tensors, r["type"], r["size"]), DEV)
    had_k, signs = _factors(golden_tensors, r)
    forms = (["fused"] if _has_fused(r) else []) + ["composed"]
    for form in forms:
        counted.clear()
        out = _run(x.to(DEV), r, tables, had_k, signs, form)
        torch.cuda.synchronize()
        assert str(out.dtype).replace("torch.", "") == entry["out"]["dtype"] and list(out.shape) == entry["out"]["shape"]
        if entry["stored"]:
            bad = (out.cpu() != golden_tensors[f"{key}.out"]).nonzero()
            assert bad.numel() == 0, f"{form}: {bad.shape[0]} elements differ from the stored reference, first at {bad[0].tolist()}"
        assert C.sha(out) == entry["out"]["sha256"], f"{form}: differs from the reference (compared by value, every element)"
        cols = C.dim_of(r) == 0 and x.shape[-1] != 1
        if form == "fused":
            assert dict(counted) == {"ct_hadamard_perm_cols" if cols else "ct_hadamard_perm_rows": 1}, counted
        else:
            assert not any("perm" in name for name in counted) and sum(counted.values()) == 1, counted
    if not _has_fused(r):
        with pytest.raises(NotImplementedError):
            _run(x.to(DEV), r, tables, had_k, signs, "fused")


@pytest.mark.parametrize("n", ALL_N)
@pytest.mark.parametrize("which", ["identity", "reversal"])
def test_identity_and_reversal(n, which):
    """integer inputs: every order of summation is exact, so the restatement G_p(butterfly(G_q(x))) is the one result; the identity
    permutation gives the unpermuted launch itself"""
    from compressed_tensors_amd import codec

    p = torch.arange(n) if which == "identity" else torch.arange(n - 1, -1, -1)
    tables = codec.hadamard_perm_tables(p, DEV)
    for dt, rows in (("bf16", 3), ("f32", 2)):
        r = dict(type="hadamard", size=n, module="Linear", location="input", inverse=False)
        x = C.synth(dict(gen="ints", dtype=dt, shape=[rows, 2 * n], salt=n % 97))
        out = codec.hadamard_transform(x.to(DEV), n, perm=tables, form="fused")
        assert torch.equal(out.cpu(), C.restated(r, x, p))
        if which == "identity":
            assert torch.equal(_bits(out), _bits(codec.hadamard_transform(x.to(DEV), n)))


# ---- the one launch computes the bits of the composition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ALL_N)
@pytest.mark.parametrize("precision", [torch.float32, torch.float64], ids=["acc32", "acc64"])
def test_fused_equals_the_composition_bit_for_bit(n, precision, golden_tensors):
    from compressed_tensors_amd import codec

    if n > codec.HADAMARD_PERM_MAX_SIZE[precision]:
        plan = codec.plan_hadamard_perm((3, n), C.BF16, n, precision=precision)
        assert plan.form == "composed" and plan.key is None  # declined to the composition, not an error
        with pytest.raises(NotImplementedError):
            codec.plan_hadamard_perm((3, n), C.BF16, n, precision=precision, form="fused")
        return
    p = _perm(golden_tensors, "hadamard", n)
    tables = codec.hadamard_perm_tables(p, DEV)
    q = C.inverse_of(p)
    for i, (dt, scale) in enumerate((("bf16", 0.02), ("f16", 1.0), ("f32", 30.0), ("bf16", 30.0))):
        rows = (1, 3, 65)[i % 3] if n <= 4096 else (1, 3, 5)[i % 3]
        shape = [rows, n] if i < 3 else [rows, 2 * n]  # two blocks per row in the last round
        x = C.synth(dict(gen="randn", dtype=dt, shape=shape, salt=500 + n + i, scale=scale))
        fused = codec.hadamard_transform(x.to(DEV), n, precision=precision, perm=tables, form="fused")
        composed = codec.hadamard_transform(x.to(DEV), n, precision=precision, perm=tables, form="composed")
        by_hand = C.gather(codec.hadamard_transform(C.gather(x, q, n).to(DEV), n, precision=precision).cpu(), p, n)
        assert torch.equal(_bits(fused), _bits(composed)) and torch.equal(_bits(fused.cpu()), _bits(by_hand)), (n, dt, scale)
        exact, tol = C.bound(C.gather(x, q, n), n)
        err = (C.gather(fused.cpu().to(C.F64), q, n) - exact).abs()  # z = G_q(out): the rotation of the gathered input
        assert bool((err <= tol).all()), (n, dt, scale, (err / tol).max().item())


@pytest.mark.parametrize("n", C.RANDOM_K1)
@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("precision", [torch.float32, torch.float64], ids=["acc32", "acc64"])
def test_fused_with_signs_equals_the_composition_bit_for_bit(n, transposed, precision, golden_tensors):
    from compressed_tensors_amd import codec

    p = _perm(golden_tensors, "random-hadamard", n)
    tables, signs = codec.hadamard_perm_tables(p, DEV), golden_tensors[f"rh.signs.{n}"].to(DEV)
    for i, (dt, scale) in enumerate((("bf16", 1.0), ("f16", 0.02), ("f32", 30.0))):
        x = C.synth(dict(gen="randn", dtype=dt, shape=[(3, 1, 5)[i], n], salt=600 + n + i, scale=scale)).to(DEV)
        kw = dict(precision=precision, transposed=transposed, perm=tables)
        fused = codec.hadamard_k_transform(x, n, None, signs, form="fused", **kw)
        composed = codec.hadamard_k_transform(x, n, None, signs, form="composed", **kw)
        assert torch.equal(_bits(fused), _bits(composed)), (n, dt, scale)


def test_column_form_equals_the_composition_bit_for_bit(golden_tensors):
    from compressed_tensors_amd import codec

    for shape, n in (((128, 256), 128), ((256, 24), 64), ((2048, 40), 2048)):
        tables = codec.hadamard_perm_tables(_perm(golden_tensors, "hadamard", n), DEV)
        x = C.synth(dict(gen="randn", dtype="bf16", shape=list(shape), salt=700 + n, scale=0.02)).to(DEV)
        kw = dict(dim=0, precision=torch.float64, perm=tables)
        assert torch.equal(_bits(codec.hadamard_transform(x, n, form="fused", **kw)), _bits(codec.hadamard_transform(x, n, form="composed", **kw)))


# ---- K > 1 takes the composition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.RANDOM_K)
def test_mixed_sizes_take_the_composed_form(n, golden_tensors):
    from compressed_tensors_amd import _lib, codec

    names = ("ct_hadamard_k_rows", "ct_hadamard_k_cols", "ct_hadamard_perm_rows", "ct_hadamard_perm_cols")
    key = next(k for k, e in sorted(MANIFEST.items()) if e["recipe"]["type"] == "random-hadamard" and e["recipe"]["size"] == n
               and e["recipe"]["tier"] == "A" and not e["recipe"]["inverse"] and e["recipe"]["dtype"] == "bf16")
    r = MANIFEST[key]["recipe"]
    tables = codec.hadamard_perm_tables(_perm(golden_tensors, "random-hadamard", n), DEV)
    had_k, signs = _factors(golden_tensors, r)
    assert had_k is not None and codec.plan_hadamard_perm(r["shape"], C.BF16, n, k=had_k.shape[0]).form == "composed"
    x = C.synth(r).to(DEV)
    codec.hadamard_k_transform(x, n, had_k, signs, perm=tables)  # warm: loads the library
    lib = _lib.load()
    counts, saved = collections.Counter(), {name: getattr(lib, name) for name in names}
    for name in names:
        def entry(*a, _o=saved[name], _n=name):
            counts[_n] += 1
            return _o(*a)
        setattr(lib, name, entry)
    try:
        out = codec.hadamard_k_transform(x, n, had_k, signs, perm=tables)
    finally:
        for name, f in saved.items():
            setattr(lib, name, f)
    assert dict(counts) == {"ct_hadamard_k_rows": 1}, counts
    assert C.sha(out) == MANIFEST[key]["out"]["sha256"]


# ---- the C ABI: in place, launches, capture, the mask ---------------------------------------------------------------------------------------
def _tables16(p):
    return C.inverse_of(p).to(torch.int16).to(DEV), p.to(torch.int16).to(DEV)


@pytest.mark.parametrize("n,rows", [(128, 3), (4096, 2)])
def test_in_place_equals_out_of_place(n, rows, golden_tensors):
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    q, p = _tables16(_perm(golden_tensors, "hadamard", n))
    x = C.synth(dict(gen="randn", dtype="bf16", shape=[rows, n], salt=800 + n, scale=1.0)).to(DEV)
    out, stream = torch.empty_like(x), _lib.stream_of(x)
    assert lib.ct_hadamard_perm_rows(x.data_ptr(), out.data_ptr(), _lib.BF16, x.numel(), n, 0, q.data_ptr(), p.data_ptr(), None, 0, stream) == 0
    assert lib.ct_hadamard_perm_rows(x.data_ptr(), x.data_ptr(), _lib.BF16, x.numel(), n, 0, q.data_ptr(), p.data_ptr(), None, 0, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(out))


def _kernels_of(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@pytest.mark.parametrize("shape,n,precision", [((65, 1024), 128, torch.float32), ((3, 4096), 4096, torch.float32), ((7, 16), 2, torch.float32),
                                               ((24, 1024), 1024, torch.float64)])
def test_fused_row_form_is_one_launch_and_nothing_else(shape, n, precision, golden_tensors, counted):
    from compressed_tensors_amd import codec

    tables = codec.hadamard_perm_tables(_perm(golden_tensors, "hadamard", n), DEV)
    x = torch.randn(shape, device=DEV).to(C.BF16)
    kernels = _kernels_of(lambda: codec.hadamard_transform(x, n, precision=precision, perm=tables, form="fused"))
    assert len(kernels) == 1 and "hadp_" in kernels[0], kernels  # no gather, no memset, no copy
    assert dict(counted) == {"ct_hadamard_perm_rows": 2}
    assert codec.plan_hadamard_perm(shape, C.BF16, n, precision=precision, form="fused").launches() == 1


def test_fused_column_form_is_three_launches(golden_tensors):
    from compressed_tensors_amd import codec

    tables = codec.hadamard_perm_tables(_perm(golden_tensors, "hadamard", 1024), DEV)
    x = torch.randn(1024, 520, device=DEV).to(C.BF16)
    kernels = _kernels_of(lambda: codec.hadamard_transform(x, 1024, dim=0, precision=torch.float64, perm=tables, form="fused"))
    assert len(kernels) == 3 and sum("transpose" in k for k in kernels) == 2 and sum("hadp_" in k for k in kernels) == 1, kernels


def test_no_host_synchronisation(golden_tensors):
    from compressed_tensors_amd import codec

    x = torch.randn(16, 4096, device=DEV).to(C.BF16)
    t4096, t128 = (codec.hadamard_perm_tables(_perm(golden_tensors, "hadamard", n), DEV) for n in (4096, 128))
    calls = [lambda: codec.hadamard_transform(x, 4096, perm=t4096, form="fused"), lambda: codec.hadamard_transform(x, 128, perm=t128, form="fused"),
             lambda: codec.hadamard_transform(x.view(128, 512), 128, dim=0, precision=torch.float64, perm=t128, form="fused"),
             lambda: codec.hadamard_transform(x, 128, perm=t128, form="composed")]
    for fn in calls:
        fn()  # warm
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fn in calls:
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_c_abi_entries_are_graph_capturable(golden_tensors):
    """the entries allocate nothing and never synchronise: captured once, replayed on changing inputs, the same bits as eager calls"""
    from compressed_tensors_amd import _lib, codec

    lib = _lib.load()
    x = torch.zeros(64, 4096, dtype=C.BF16, device=DEV)
    outs, ws, B = [torch.empty_like(x) for _ in range(3)], torch.empty_like(x), _lib.BF16
    p4096, p64 = _perm(golden_tensors, "hadamard", 4096), _perm(golden_tensors, "hadamard", 64)
    (q1, p1), (q2, p2) = _tables16(p4096), _tables16(p64)
    signs = golden_tensors["rh.signs.4096"].to(DEV)

    def launches(stream):
        rcs = [lib.ct_hadamard_perm_rows(x.data_ptr(), outs[0].data_ptr(), B, x.numel(), 4096, 0, q1.data_ptr(), p1.data_ptr(), None, 0, stream),
               lib.ct_hadamard_perm_rows(x.data_ptr(), outs[1].data_ptr(), B, x.numel(), 4096, 1, q1.data_ptr(), p1.data_ptr(), signs.data_ptr(), 1, stream),
               lib.ct_hadamard_perm_cols(x.data_ptr(), outs[2].data_ptr(), ws.data_ptr(), B, 64, 4096, 64, 1, q2.data_ptr(), p2.data_ptr(), None, 0, stream)]
        assert not any(rcs), (rcs, _lib.last_error())

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        launches(_lib.stream_on(DEV, side.cuda_stream))  # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches(_lib.stream_on(DEV, torch.cuda.current_stream(DEV).cuda_stream))
    t4096, t64 = codec.hadamard_perm_tables(p4096, DEV), codec.hadamard_perm_tables(p64, DEV)
    for rep in range(2):
        x.copy_(C.synth(dict(gen="randn", dtype="bf16", shape=[64, 4096], salt=900 + rep, scale=1.0)).to(DEV))
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = [codec.hadamard_transform(x, 4096, perm=t4096, form="composed"),
                codec.hadamard_k_transform(x, 4096, None, signs, precision=torch.float64, transposed=True, perm=t4096, form="composed"),
                codec.hadamard_transform(x, 64, dim=0, precision=torch.float64, perm=t64, form="composed")]
        assert all(torch.equal(_bits(o), _bits(w)) for o, w in zip(outs, want))


def test_a_corrupted_table_cannot_escape_the_block():
    """every entry of both tables 0xFFFF at n = 128: the kernel masks it to 127, so each output element is its own block's z[127]
    with g[k] = x[127] for every k — the composition over the masked table.  Valid memory only; nothing is provoked."""
    from compressed_tensors_amd import _lib, codec

    lib, n = _lib.load(), 128
    x = C.synth(dict(gen="randn", dtype="bf16", shape=[5, 3 * n], salt=990, scale=1.0)).to(DEV)
    bad = torch.full((n,), -1, dtype=torch.int16, device=DEV)  # 0xFFFF
    guard = torch.full_like(x, 7.0)
    buf = torch.cat([guard, x, guard])  # neighbours that must stay untouched
    out = torch.cat([guard, torch.empty_like(x), guard])
    rows = x.shape[0]
    src, dst = buf[rows:2 * rows], out[rows:2 * rows]
    assert lib.ct_hadamard_perm_rows(src.data_ptr(), dst.data_ptr(), _lib.BF16, src.numel(), n, 0, bad.data_ptr(), bad.data_ptr(), None, 0, _lib.stream_of(x)) == 0
    torch.cuda.synchronize()
    masked = torch.full((n,), n - 1, dtype=torch.int64, device=DEV)
    want = C.gather(codec.hadamard_transform(C.gather(x, masked, n), n), masked, n)
    assert bool(torch.isfinite(dst).all()) and torch.equal(_bits(dst), _bits(want))
    assert torch.equal(out[:rows], guard) and torch.equal(out[2 * rows:], guard) and torch.equal(buf[rows:2 * rows], x)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _check_model(m, seen):
    for name, t in (("0.weight", m[0].weight.data), ("0.bias", m[0].bias.data), ("1.weight", m[1].weight.data), ("1.input", seen[0])):
        assert list(t.shape) == MODEL[name]["shape"] and C.sha(t) == MODEL[name]["sha256"], f"{name} differs from the reference's result"


def test_apply_transform_config_randomize_on_a_cuda_model(golden_tensors):
    import compressed_tensors_amd as cta

    m = H.model().to(DEV)
    cfg = cta.TransformConfig.from_dict(C.model_config())
    cta.apply_transform_config(m, cfg, randomize=True, seed=MODEL["seed"])
    torch.cuda.synchronize()
    t = m[1].v_input
    assert isinstance(t, cta.HadamardTransform) and torch.equal(t.perm.cpu(), golden_tensors["model.perm.v.64"].to(torch.int64))
    assert [k for k in m.state_dict() if k.endswith(".perm")] == ["1.v_input.perm"] and "permuted=True" in repr(t)
    seen = []
    m[1].register_forward_pre_hook(lambda _, inputs: seen.append(inputs[0]))
    m[1](C.synth(dict(gen="ints", dtype="bf16", shape=[2, 5, 128], salt=77)).to(DEV))
    _check_model(m, seen)
    m2 = H.model().to(DEV)  # no seed: another draw, still a rotation (orthogonal: applying it twice with the inverse gives the weights back)
    cta.apply_transform_config(m2, cfg, randomize=True)
    assert m2[1].v_input.perm.numel() == 64


def test_upstream_apply_under_install_patch_permuted_hadamard(golden_tensors):
    if not ref_import.available():
        pytest.skip("no reference on this machine (neither the live tree nor the staged archive)")
    ref_import.import_reference()
    try:
        import compressed_tensors.transform as up_t
        import compressed_tensors.transform.factory.hadamard as up_h
    except ImportError as e:
        pytest.skip(f"upstream's transform package cannot be imported on this machine: {e!r}")
    import compressed_tensors_amd.install as ct_amd
    from compressed_tensors_amd import _lib

    lib = _lib.load()
    names = ("ct_hadamard_rows", "ct_hadamard_cols", "ct_hadamard_perm_rows", "ct_hadamard_perm_cols")
    orig_create, orig_forward = up_h.HadamardFactory.create_transform, up_h.HadamardTransform.forward

    def run(flag):
        counts, saved = collections.Counter(), {name: getattr(lib, name) for name in names}
        for name in names:
            def entry(*a, _o=saved[name], _n=name):
                counts[_n] += 1
                return _o(*a)
            setattr(lib, name, entry)
        ct_amd.install(patch_transforms=True, patch_permuted_hadamard=flag)
        try:
            m = H.model().to(DEV)
            config = up_t.TransformConfig.model_validate(C.model_config())
            for name, scheme in config.config_groups.items():  # upstream's apply_transform_config loop, with the seed its factories take
                up_t.TransformFactory.from_scheme(scheme, name=name, seed=MODEL["seed"]).apply_to_model(m, use_tqdm=False)
            seen = []
            m[1].register_forward_pre_hook(lambda _, inputs: seen.append(inputs[0]))
            m[1](C.synth(dict(gen="ints", dtype="bf16", shape=[2, 5, 128], salt=77)).to(DEV))
            torch.cuda.synchronize()
            _check_model(m, seen)
        finally:
            ct_amd.uninstall()
            for name, f in saved.items():
                setattr(lib, name, f)
        return counts

    assert sum(run(False).values()) == 0  # without the flag a permuted transform is upstream's
    counts = run(True)
    assert sum(counts.values()) == 4 and not (set(counts) - set(names)), counts  # weight + bias of 0, weight of 1, the hooked input
    assert up_h.HadamardFactory.create_transform is orig_create and up_h.HadamardTransform.forward is orig_forward
