"""The random-hadamard rotation fused into the dynamic QDQ launch (csrc/ct_rotated_k.hip) on the MI355X: bit-identity with the two
launches it replaces, a float64 reference on exact inputs, declined shapes, scales only, graph capture, modules."""
import collections
import functools
import os
import sys

import pytest
import torch
from safetensors import safe_open

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dynamic_cases as D  # noqa: E402
import _random_hadamard_cases as C  # noqa: E402

import compressed_tensors_amd as cta  # noqa: E402
from compressed_tensors_amd import codec, transform  # noqa: E402
from compressed_tensors_amd.quantization import QuantizationArgs, QuantizationScheme, dynamic  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = ["fp8_token", "int8_token", "fp8_group128", "mxfp4", "mxfp8", "nvfp4", "nvfp4_nogs", "int4_group32_asym"]
ROWS = {4480: 3, 5120: 3, 1376: 5, 2368: 5, 14336: 3, 28672: 3}  # 5: a ragged last group of G = 4 / 2 blocks


@pytest.fixture(autouse=True)
def every_form_enabled(monkeypatch):
    monkeypatch.setattr(dynamic, "ROTATED_K_MEASURED_FASTER", dynamic.ROTATED_K_ALL_FORMS)


@pytest.fixture()
def counted(monkeypatch):
    counts, orig = collections.Counter(), codec.call
    monkeypatch.setattr(codec, "call", lambda name, *a: counts.update([name]) or orig(name, *a))
    return counts


@functools.lru_cache(None)
def _factors(n):
    with safe_open(os.path.join(ROOT, "tests", "golden", "random_hadamard.safetensors"), "pt") as f:
        return (f.get_tensor(f"had_k.{n}").to(DEV) if f"had_k.{n}" in f.keys() else None), f.get_tensor(f"signs.{n}").to(DEV)


def _args(kind):
    return QuantizationArgs(**D.PRESETS[kind.replace("_nogs", "")]), (D.global_scale_of("gs").to(DEV) if kind == "nvfp4" else None)


def _eager(x, n, args, gs):
    rot = codec.hadamard_k_transform(x, n, *_factors(n))
    return dynamic.dynamic_fake_quantize(rot, args, gs, return_qparams=True) + (rot,)


def _both(x, n, kind, counted=None):
    args, gs = _args(kind)
    if counted is not None:
        counted.clear()
    fused = dynamic.random_rotated_fake_quantize(x, n, *_factors(n), args, gs, return_qparams=True, return_rotated=True, fused=True)
    calls = dict(counted) if counted is not None else None
    comp = _eager(x, n, args, gs)
    torch.cuda.synchronize()
    return fused, comp, calls


def _assert_same_bits(fused, comp, what):
    for name, a, b in zip(("out", "scale", "zp", "rotated"), fused, comp):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        assert D.canonical_bytes(a) == D.canonical_bytes(b), f"{what}: {name} differs from the two-launch composition"


def _inputs(rows, n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    for s in (0.02, 1.0, 30.0):
        yield f"randn*{s}", (torch.randn((1, rows, n), generator=g, dtype=torch.float32) * s).to(dtype)
    # edge rows — all zero, one non-zero, -0.0, +inf, a NaN — next to ordinary ones that share their workgroups (G = 4 at n = 1376)
    x = torch.randn((1, 8, n), generator=g, dtype=torch.float32)
    x[0, :2] = 0.0
    x[0, 1, n // 3] = 2.5
    x[0, 2] = -0.0
    x[0, 3, n // 2] = float("inf")
    x[0, 4, n - 1] = float("nan")
    yield "edge rows", x.to(dtype)


# one item per size and dtype, every kind the size is served for inside it (the GPU suite keeps its item count down): 1376 and 2368
# (M = 8 / 16: G > 1, and 128 does not divide them) are served for the groups of 32 and 16 only, KINDS[3:]
IDENTITY = [pytest.param(n, KINDS[3 * (ROWS[n] == 5):], dt, ROWS[n], id=f"n{n}-{dt}") for n in ROWS for dt in ("bf16", "f16")]
# 1100 rows: more groups than the launch's 512 workgroups, so later grid-stride rounds rewrite the LDS image and the reduction area
IDENTITY += [pytest.param(4480, ("fp8_token", "mxfp4"), "bf16", rows, id=f"n4480-{rows}rows") for rows in (300, 1100)]


@pytest.mark.parametrize("n,kinds,dt,rows", IDENTITY)
def test_fused_equals_the_composition(n, kinds, dt, rows, counted):
    """out, scale, zero point and the rotated tensor, NaNs canonicalised, the sign of zeros included; a NaN / inf row leaves the
    other blocks of its workgroup what the composition makes them.  Fails without the feature."""
    for kind in kinds:
        for what, x in _inputs(rows, n, D.DTYPES[dt], seed=n + len(kind)):
            fused, comp, calls = _both(x.to(DEV), n, kind, counted)
            assert calls == {"ct_hadamard_k_dynamic_qdq": 1}, (kind, calls)
            _assert_same_bits(fused, comp, f"{kind}, {what}")


@pytest.mark.parametrize("n,dt", [(4480, "bf16"), (4480, "f16"), (14336, "bf16"), (14336, "f16")])
def test_against_a_float64_reference(n, dt):
    """Tier A inputs (integers |x| <= 128: n * 128 < 2^24, every summation order is exact): the rotated tensor equals the float32
    evaluation from the factors in every element.  For the FP8 kinds `out` is compared with a float64 evaluation on that rotated
    tensor r: s = amax / 448 per segment, q = float8_e4m3fn(r / s), q * s.  Derived tolerance, u one rounding of the activation dtype
    (2^-8 bf16, 2^-11 fp16): the kernel's scale is s (1 + d1), its quotient (r / s)(1 + d2)(1 + d3) / (1 + d1) (reciprocal and
    product), all |d| <= u, so the quotient moves by less than 4 u |t| < one E4M3 step (>= |t| / 16) and rounds to q or a neighbour:
    |q' - q| <= step, taken at |t| (1 + 4 u), at least the subnormal step 2^-9.  The product q' s (1 + d1)(1 + d4) adds
    3 u (|q| + step) s: tol = s (step + 3 u (|q| + step)), asserted of the composition first.  First run: worst ratio 0.89-0.99."""
    u = C.ULP[D.DTYPES[dt]]
    x = C.synth(dict(gen="ints", dtype=dt, shape=[1, 3, n], salt=n % 89))
    want_rot = C.structured(x, n, *(t.cpu() for t in _factors(n)), acc=C.F32)
    for kind, L in (("fp8_token", n), ("fp8_group128", 128)):
        fused, comp, _ = _both(x.to(DEV), n, kind)
        assert torch.equal(fused[3].cpu(), want_rot) and torch.equal(comp[3].cpu(), want_rot)
        seg = want_rot.to(C.F64).reshape(-1, L)
        s = seg.abs().amax(-1, keepdim=True) / 448.0
        t = seg / s
        q = t.to(torch.float32).clamp(-448, 448).to(torch.float8_e4m3fn).to(C.F64)
        step = torch.exp2(torch.floor(torch.log2((t.abs() * (1 + 4 * u)).clamp(2.0 ** -6, 448.0))) - 3)
        tol = s * (step + 3 * u * (q.abs() + step))
        for name, got in (("composition", comp[0]), ("fused", fused[0])):
            err = (got.cpu().to(C.F64).reshape(-1, L) - q * s).abs()
            assert bool((err <= tol).all()), (name, kind)


@pytest.mark.parametrize("kind,shape,n,dt,reason", [
    ("fp8_group128", (1, 2, 8 * 1376), 1376, "bf16", "is not fused"),  # 128 divides the row of 8 blocks, not the block
    ("fp8_token", (1, 5, 1376), 1376, "bf16", "shares its workgroup"), ("fp8_token", (1, 3, 4096), 4096, "bf16", "k == 1"),
    ("fp8_token", (1, 3, 4480), 4480, "f32", "float32 activations"), ("fp8_token", (2, 3, 2 * 4480), 4480, "bf16", "2 rotation blocks")])
def test_declined_shapes_take_the_two_launches(kind, shape, n, dt, reason, counted):
    plan = dynamic.plan_rotated_k_dynamic(shape, D.DTYPES[dt], n, C.SIZES[n][0], _args(kind)[0])
    assert not plan.fused and plan.key is None and reason in plan.reason, plan.reason
    x = torch.randn(shape, generator=torch.Generator().manual_seed(n), dtype=torch.float32).to(D.DTYPES[dt]).to(DEV)
    fused, comp, calls = _both(x, n, kind, counted)
    assert calls == {"ct_hadamard_k_rows": 1, "ct_dynamic_qdq": 1}, calls
    _assert_same_bits(fused, comp, reason)


def _job(kind, n, rows):
    (had_k, signs), (args, gs) = _factors(n), _args(kind)
    x = torch.randn((1, rows, n), generator=torch.Generator().manual_seed(rows), dtype=torch.float32).to(D.BF16).to(DEV)
    dp = dynamic.plan_rotated_k_dynamic(x.shape, D.BF16, n, C.SIZES[n][0], args, gs).dynamic
    kw = dict(kind=dp.kind, seg_len=dp.seg_len, num_bits=dp.num_bits, symmetric=dp.symmetric, global_scale=gs, scale_shape=dp.scale_shape,
              scale_dtype=dp.scale_dtype, zp_dtype=dp.zp_dtype)
    return x, args, gs, lambda **more: codec.hadamard_k_dynamic_qdq(x, n, had_k, signs, **kw, **more)


CAPTURED = [("fp8_token", 4480, 7), ("nvfp4", 1376, 9), ("int4_group32_asym", 14336, 3)]  # (kind, n, rows) of _job


def test_scales_only_no_host_synchronisation_and_graph_capture():
    """scales only (want_out=False) returns the composition's scale and zero point; the launch never synchronises (sync-debug) and is
    captured once and replayed on changing inputs, every replay against the eager composition (outputs allocated inside the capture)"""
    jobs = [_job(*c) for c in CAPTURED]
    for x, args, gs, call in jobs:  # also the warm-up: the first call loads the library
        (out, scale, zp, rotated), want = call(want_out=False), _eager(x, x.shape[-1], args, gs)
        assert out is None and rotated is None
        assert D.canonical_bytes(scale) == D.canonical_bytes(want[1]) and D.canonical_bytes(zp) == D.canonical_bytes(want[2])
    torch.cuda.set_sync_debug_mode("error")
    try:
        for *_, call in jobs:
            call(want_rotated=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = [call(want_rotated=True) for *_, call in jobs]
    for rep in range(3):
        for (x, *_), got in zip(jobs, outs):
            x.copy_((torch.randn(x.shape, generator=torch.Generator().manual_seed(rep), dtype=torch.float32) * (rep + 1)).to(D.BF16))
            got[0].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for (kind, n, _), (x, args, gs, _), got in zip(CAPTURED, jobs, outs):
            _assert_same_bits(got, _eager(x, n, args, gs), f"replay {rep} of {kind}")


def test_modules_under_fuse_random_input_quantization(counted):
    n = 4480
    weight = C.weight_from_factors(n, *(t.cpu() for t in _factors(n)), torch.float32)
    config = {"config_groups": {"v": dict(C.MODEL_CONFIG["config_groups"]["v"], apply=[{"targets": ["Linear"], "location": "input", "inverse": False, "ignore": []}])}}

    def build(fuse):
        lin = torch.nn.Linear(n, 8, bias=False, dtype=D.BF16)
        with torch.no_grad():
            lin.weight.copy_(C.synth(dict(gen="grid", dtype="bf16", shape=[8, n], salt=63)))
        m = torch.nn.Sequential(lin).to(DEV).requires_grad_(False)
        cta.apply_transform_config(m, config, hadamard_weights=lambda size, dtype, dev, gen: weight.to(device=dev, dtype=dtype))
        m[0].quantization_scheme = QuantizationScheme(targets=["Linear"], input_activations=_args("fp8_token")[0])
        m[0].quantization_status = "frozen"
        m[0].forward = lambda x: torch.nn.functional.linear(dynamic.forward_quantize(m[0], x, "input", m[0].quantization_scheme.input_activations), m[0].weight)
        assert transform.fuse_input_quantization(m) == []  # not a Sylvester rotation: still left alone
        return m, (transform.fuse_random_input_quantization(m) if fuse else [])

    x = torch.randn(2, 5, n, generator=torch.Generator().manual_seed(3), dtype=torch.float32).to(D.BF16).to(DEV)
    (plain, none), (fused, names) = build(False), build(True)
    assert none == [] and names == ["0"]
    counted.clear()
    want = plain(x)
    assert dict(counted) == {"ct_hadamard_k_rows": 1, "ct_dynamic_qdq": 1}, counted
    counted.clear()
    got = fused(x)
    assert dict(counted) == {"ct_hadamard_k_dynamic_qdq": 1}, counted  # one launch per forward
    assert want.dtype == got.dtype and torch.equal(want.view(torch.int16), got.view(torch.int16))
