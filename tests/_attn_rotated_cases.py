"""The cases of the fused head-dim rotation + attention QDQ (csrc/ct_attn_rot.hip): the fixture matrix that
tools/gen_golden_attn_rotated.py runs through the reference (tests/golden/attn_rotated*), and the wider matrix that
tests/test_gpu_attn_rotated.py compares bit for bit against the composition of the two existing launches.

Fixture inputs are integers in [-128, 128] (the integer hash of tests/_hadamard_cases.py) times a per-row power of two
2^((7 * row + salt) % 9 - 4), so every partial sum of the rotation is exact in float32 in any order and the reference's GEMM is a
bit-exact target; the first rows are a zero row, a row with a single non-zero and a constant row.  The reference is compared BY
VALUE (tests/_rotated_cases.py: a GEMM turns a -0.0 into +0.0 where a butterfly does not): zeros count as +0.0."""
import itertools

import torch

import _attn_cases as A
import _hadamard_cases as H
from _rotated_cases import by_value, equal_by_value, sha  # noqa: F401

F32, BF16, F16, F8 = A.F32, A.BF16, A.F16, A.F8
DTYPES = A.DTYPES
KINDS = {k: A.KINDS[k] for k in ("fp8", "int8", "int8_zp", "int4_zp")}
DN_PAIRS = ((8, 8), (16, 16), (64, 64), (128, 128), (256, 256), (512, 512), (256, 128), (384, 128), (128, 4))
LAYOUTS = ("transposed", "contiguous", "fused_k", "decode")
MAX_FIXTURE_BYTES = 512 * 1024


def key_of(r):
    return ".".join([r["mode"], r["kind"], r["strategy"], r["dtypes"].replace("/", "-"), r["layout"], f"{r['B']}x{r['H']}x{r['S']}x{r['D']}", f"n{r['n']}"])


def normalise(r):
    r = dict(r)
    if r["layout"] == "decode":
        r["S"] = 1
    return r


def place(vals, layout):
    """the (B, H, S, D) values in the recipe's storage layout, on vals' device"""
    B, Hh, S, D = vals.shape
    if layout == "contiguous":
        return vals.contiguous()
    if layout in ("transposed", "decode"):  # what a Llama passes: (B, S, H, D).transpose(1, 2); decode: S == 1
        x = torch.empty((B, S, Hh, D), dtype=vals.dtype, device=vals.device).transpose(1, 2)
    elif layout == "fused_k":  # the K slice of one (B, S, (Hq + 2 H) D) projection output, viewed as heads
        width = (A.FUSED_Q_HEADS + 2 * Hh) * D
        base = torch.zeros((B, S, width), dtype=vals.dtype, device=vals.device)
        off = A.FUSED_Q_HEADS * D
        x = base[..., off:off + Hh * D].view(B, S, Hh, D).transpose(1, 2)
    else:
        raise KeyError(layout)
    x.copy_(vals)
    return x


def fixture_values(r):
    B, Hh, S, D = r["B"], r["H"], r["S"], r["D"]
    numel = B * Hh * S * D
    dt = DTYPES[r["dtypes"].split("/")[0]]
    ints = (H._hash(numel, r["salt"]) % 257 - 128).to(torch.float64)
    row = torch.arange(numel, dtype=torch.int64) // D
    x = (ints * torch.pow(2.0, ((row * 7 + r["salt"]) % 9 - 4).to(torch.float64))).to(dt).reshape(-1, D)
    k = torch.arange(D)
    edge = [torch.zeros(D), torch.where(k == D // 3, torch.tensor(64.0), torch.tensor(0.0)), torch.full((D,), 3.0)]
    for i, e in enumerate(edge[: x.shape[0]]):
        x[i] = e.to(dt)
    return x.reshape(B, Hh, S, D)


def make_input(r, device="cpu"):
    return place(fixture_values(r).to(device), r["layout"])


def make_qparams(r):
    return A.make_qparams(r)


def rotation64(x, n):
    """the rotation with the sums accumulated in float64 (exact for the fixtures' inputs), the reference's own quotient — float32
    by float32(sqrt(float64(n))), one IEEE division — and one rounding to x's dtype"""
    v = x.to(torch.float64)
    shape = v.shape
    h = 1
    while h < n:
        v = v.reshape(-1, n // (2 * h), 2, h)
        v = torch.stack((v[:, :, 0] + v[:, :, 1], v[:, :, 0] - v[:, :, 1]), dim=2)
        h *= 2
    v = v.reshape(shape)
    assert torch.equal(v.to(F32).to(torch.float64), v), "a sum is not exact in float32: not a fixture input"
    return (v.to(F32) / torch.tensor(n, dtype=torch.float64).sqrt().to(F32)).to(x.dtype)


def fixture_cases():
    """[(key, recipe)], between 20 and 60: every D / n pair on the transposed view in bf16 FP8 attn_head, every kind in both modes,
    every layout, every dtype pair, both strategies"""
    out, seen = [], set()

    def add(**r):
        base = dict(B=2, H=3, S=5, D=128, n=128, layout="transposed", dtypes="bf16/bf16", kind="fp8", strategy="attn_head", mode="fake")
        base.update(r)
        r = normalise(base)
        r["salt"] = len(out) % 11 + 1
        k = key_of(r)
        if k not in seen:
            seen.add(k)
            out.append((k, r))

    for D, n in DN_PAIRS:
        add(D=D, n=n)
    for kind in KINDS:
        for mode in ("fake", "quantize"):
            add(kind=kind, mode=mode, B=1, H=2, S=40)
    for i, layout in enumerate(LAYOUTS):
        add(layout=layout, D=64, n=64, kind=("int8", "fp8", "int8_zp", "int4_zp")[i])
        add(layout=layout, D=256, n=128, strategy="tensor", mode="quantize" if i % 2 else "fake")
    for i, dtypes in enumerate(("f16/f16", "f32/f32", "bf16/f32", "f16/f32")):
        add(dtypes=dtypes, D=(64, 128, 16, 128)[i], n=(64, 32, 16, 128)[i], kind=("fp8", "int8_zp", "int8", "fp8")[i], layout=LAYOUTS[i],
            mode="quantize" if i == 3 else "fake")
    add(B=2, H=3, S=50, D=16, n=16)  # 300 rows at 2 lanes per row
    add(B=3, H=2, S=1, D=128, n=128, layout="decode", kind="int8")
    add(D=384, n=128, kind="int8_zp", mode="quantize")
    add(D=128, n=2, strategy="tensor0")
    return out


def stored(r) -> bool:
    return r["B"] * r["H"] * r["S"] * r["D"] <= 4096 and r["dtypes"].startswith("bf16")


# ---- the identity matrix of the GPU tests (fused against the composition; no reference needed) -----------------------------------------
SHAPES = {"live_dead": (2, 3, 5), "tail": (1, 2, 40), "decode": (3, 2, 1)}  # (B, H, S): 30 rows, 80 rows, decode
ID_FACTORS = dict(dn=DN_PAIRS, layout=LAYOUTS, dtype=("bf16", "f16", "f32"), kind=tuple(KINDS), strategy=("attn_head", "tensor"), mode=("fake", "quantize"),
                  shape=tuple(SHAPES), scale=(0.05, 1.0, 30.0))


def identity_cases():
    """a greedy pairwise cover of ID_FACTORS, plus every D / n pair on the transposed layout in bf16 FP8 attn_head.  Deterministic."""
    names = list(ID_FACTORS)
    uncovered = {(a, va, b, vb) for a, b in itertools.combinations(names, 2) for va in ID_FACTORS[a] for vb in ID_FACTORS[b]}
    out = []

    def pairs(r):
        return {(a, r[a], b, r[b]) for a, b in itertools.combinations(names, 2)}

    state = 4321
    while uncovered:
        best, gain = None, -1
        for _ in range(48):
            cand = {}
            for nm in names:
                state = (state * 1103515245 + 12345) & 0x7FFFFFFF
                cand[nm] = ID_FACTORS[nm][(state >> 8) % len(ID_FACTORS[nm])]
            g = len(pairs(cand) & uncovered)
            if g > gain:
                best, gain = cand, g
        uncovered -= pairs(best)
        out.append(best)
    for dn in DN_PAIRS:
        out.append(dict(dn=dn, layout="transposed", dtype="bf16", kind="fp8", strategy="attn_head", mode="fake", shape="live_dead", scale=1.0))
    out.append(dict(dn=(16, 16), layout="transposed", dtype="bf16", kind="fp8", strategy="attn_head", mode="fake", shape=(2, 3, 50), scale=1.0))
    return out


def identity_id(c):
    shape = c["shape"] if isinstance(c["shape"], str) else "x".join(map(str, c["shape"]))
    return f"D{c['dn'][0]}n{c['dn'][1]}-{c['layout']}-{c['dtype']}-{c['kind']}-{c['strategy']}-{c['mode']}-{shape}-s{c['scale']}"


def identity_input(c, device, seed):
    B, Hh, S = SHAPES[c["shape"]] if isinstance(c["shape"], str) else c["shape"]
    if c["layout"] == "decode":
        S = 1
    D = c["dn"][0]
    g = torch.Generator().manual_seed(seed)
    vals = (torch.randn((B, Hh, S, D), generator=g, dtype=F32) * c["scale"]).to(DTYPES[c["dtype"]])
    return place(vals.to(device), c["layout"])


def special_values(D, dtype):
    """(1, 2, 4, D): rows of subnormals, +-0, +-inf among ordinary values, a NaN, a constant, and ordinary rows"""
    fi = torch.finfo(dtype)
    k = torch.arange(D)
    base = ((k * 37 % 23) - 11).float() / 4
    rows = [
        torch.full((D,), fi.smallest_normal / 4) * torch.where(k % 2 == 0, 1.0, -1.0),
        torch.where(k % 2 == 0, torch.tensor(0.0), torch.tensor(-0.0)),
        torch.where(k == D // 2, torch.tensor(float("inf")), base),
        torch.where(k == 1, torch.tensor(float("-inf")), base),
        torch.where(k == D - 1, torch.tensor(float("nan")), base),
        torch.full((D,), 3.0),
        base,
        -base * 100,
    ]
    return torch.stack(rows).to(dtype).reshape(1, 2, 4, D)
