"""The case matrix of the attention q / k / v QDQ fixtures (tools/gen_golden_attn.py writes them, tests/test_attn_quant.py and
tests/test_gpu_attn_quant.py read them).  Inputs and scales are synthesised from integer formulas (`_dynamic_cases.synth`), so a
case is fully described by its recipe: the logical (B, H, S, D) values, the storage layout they are placed in, the dtypes, the
quantization kind, the strategy and the mode.  Every case keeps the sha256 of its input and of the reference's output, and the
output's dtype, shape and strides; the small bfloat16 cases also keep the output itself."""
import itertools

import torch

from _dynamic_cases import BF16, DTYPES, F8, F16, F32, canonical_bytes, sha, synth  # noqa: F401

# the smallest shapes at which the kernel can go wrong: 16 = two units, 64 / 128 / 256 = 8 / 16 / 32 lanes per row, 80 = ten units on
# sixteen lanes (not a power of two), 20 = not a whole number of units (element form); one and several batches, heads and rows;
# 33 rows = more than one workgroup pass, odd
D_VALUES = (16, 64, 80, 128, 256, 20)
B_VALUES = (1, 2)
H_VALUES = (1, 2, 8)
S_VALUES = (1, 5, 33)
LAYOUTS = ("contiguous", "transposed", "fused_k", "fused_v", "misaligned", "expanded", "3d")
DTYPE_PAIRS = ("bf16/bf16", "f16/f16", "f32/f32", "bf16/f32", "f16/f32", "f32/bf16")  # x dtype / scale dtype
KINDS = {
    "fp8": dict(num_bits=8, type="float", symmetric=True),
    "int8": dict(num_bits=8, type="int", symmetric=True),
    "int8_zp": dict(num_bits=8, type="int", symmetric=False),
    "int4_zp": dict(num_bits=4, type="int", symmetric=False),
    "int2": dict(num_bits=2, type="int", symmetric=True),
}
STRATEGIES = ("attn_head", "tensor", "tensor0")  # tensor0: a 0-dim scale (it does not promote x)
MODES = ("fake", "quantize", "dequantize")
FACTORS = dict(D=D_VALUES, B=B_VALUES, H=H_VALUES, S=S_VALUES, layout=LAYOUTS, dtypes=DTYPE_PAIRS, kind=tuple(KINDS), strategy=STRATEGIES, mode=MODES)
FUSED_Q_HEADS = 3  # the query heads in front of the K and V slices of a fused projection output


def normalise(r):
    """the constraints between factors: a 3-D tensor has no batch; an expanded one has two"""
    r = dict(r)
    if r["layout"] == "3d":
        r["B"] = 1
    if r["layout"] == "expanded":
        r["B"] = 2
    return r


def key_of(r):
    return ".".join([r["mode"], r["kind"], r["strategy"], r["dtypes"].replace("/", "-"), r["layout"], f"{r['B']}x{r['H']}x{r['S']}x{r['D']}"])


def case_list():
    """[(key, recipe)]: a greedy pairwise cover of FACTORS (every pair of values of every two factors occurs, up to `normalise`),
    plus every layout at every D for the flagship FP8 attn_head fake_quantize in bf16.  Deterministic."""
    names = list(FACTORS)
    uncovered = set()
    for a, b in itertools.combinations(names, 2):
        for va in FACTORS[a]:
            for vb in FACTORS[b]:
                uncovered.add((a, va, b, vb))
    out, seen = [], set()

    def pairs(r):
        return {(a, r[a], b, r[b]) for a, b in itertools.combinations(names, 2)}

    def add(r):
        r = normalise(r)
        r["salt"] = len(out) % 11 + 1
        k = key_of(r)
        if k not in seen:
            seen.add(k)
            out.append((k, r))
        return pairs(r)

    state = 12345
    while uncovered:
        best, best_gain = None, -1
        for _ in range(48):
            cand = {}
            for n in names:
                state = (state * 1103515245 + 12345) & 0x7FFFFFFF
                cand[n] = FACTORS[n][(state >> 8) % len(FACTORS[n])]
            gain = len(pairs(normalise(cand)) & uncovered)
            if gain > best_gain:
                best, best_gain = cand, gain
        if best_gain == 0:
            # what `normalise` makes impossible (3d with B = 2, expanded with B = 1) stays uncovered: drop it
            a, va, b, vb = next(iter(sorted(uncovered)))
            cand = {n: FACTORS[n][0] for n in names}
            cand[a], cand[b] = va, vb
            if not (pairs(normalise(cand)) & uncovered):
                uncovered.discard((a, va, b, vb))
                continue
            best = cand
        uncovered -= add(best)
    for layout in LAYOUTS:
        for D in D_VALUES:
            add(dict(D=D, B=2, H=8, S=5, layout=layout, dtypes="bf16/bf16", kind="fp8", strategy="attn_head", mode="fake"))
    for kind in KINDS:  # every kind in every mode on the view a Llama passes
        for mode in MODES:
            add(dict(D=128, B=2, H=8, S=33, layout="transposed", dtypes="bf16/bf16", kind=kind, strategy="attn_head", mode=mode))
    return out


def logical_shape(r):
    return (r["B"], r["H"], r["S"], r["D"])


def make_input(r, device="cpu"):
    """the (B, H, S, D) values of synth placed in the recipe's storage layout, built ON `device` (a copy to another device would
    compact the storage and lose the layout)"""
    B, H, S, D = logical_shape(r)
    dt = DTYPES[r["dtypes"].split("/")[0]]
    layout = r["layout"]
    if layout == "expanded":
        return synth((1, H, S, D), dt, r["salt"]).to(device).expand(B, H, S, D)
    vals = synth((B, H, S, D), dt, r["salt"]).to(device)
    if layout == "contiguous":
        return vals
    if layout == "3d":
        return vals[0]
    if layout == "transposed":  # what a Llama passes: (B, S, H, D).transpose(1, 2)
        x = torch.empty((B, S, H, D), dtype=dt, device=device).transpose(1, 2)
    elif layout in ("fused_k", "fused_v"):  # the K / V slice of one (B, S, (Hq + 2 H) D) projection output, viewed as heads
        width = (FUSED_Q_HEADS + 2 * H) * D
        base = synth((B, S, width), dt, r["salt"] + 50).to(device)
        off = (FUSED_Q_HEADS + (H if layout == "fused_v" else 0)) * D
        x = base[..., off:off + H * D].view(B, S, H, D).transpose(1, 2)
    elif layout == "misaligned":  # a contiguous tensor one element into its storage: no 16-byte alignment
        x = torch.zeros(B * H * S * D + 1, dtype=dt, device=device)[1:].view(B, H, S, D)
    else:
        raise KeyError(layout)
    x.copy_(vals)
    return x


def make_qparams(r):
    """(scale, zero_point or None): per-head scales all different — head 0 moderate, head 1 tiny (everything saturates), head 2 huge
    (everything rounds to zero) — or one moderate scale; zero points distinct per head"""
    H = r["H"]
    sdt = DTYPES[r["dtypes"].split("/")[1]]
    kind = KINDS[r["kind"]]
    top = 448.0 if kind["type"] == "float" else float(2 ** (kind["num_bits"] - 1) - 1)
    if r["strategy"] == "attn_head":
        vals = [{1: 2.0 ** -20, 2: 2.0 ** 12}.get(h, (3.0 + 0.37 * h) / top) for h in range(H)]
        scale = torch.tensor(vals, dtype=torch.float64).to(sdt).reshape(H, 1, 1)
        zp = torch.tensor([(h * 5) % 7 - 3 for h in range(H)], dtype=torch.int8).reshape(H, 1, 1)
    else:
        scale = torch.tensor(3.3 / top, dtype=torch.float64).to(sdt).reshape(() if r["strategy"] == "tensor0" else (1,))
        zp = torch.tensor(-2, dtype=torch.int8).reshape(scale.shape)
    if kind["type"] == "int" and kind["num_bits"] < 4:
        zp = zp.clamp(-1, 1)
    return scale, (None if kind["symmetric"] else zp)


def eager_fake_quantize(x, scale, zp, kind):
    """the reference's arithmetic restated in eager torch (forward_helpers.py:180-215, quant_args.py:460-496), on the same device"""
    k = KINDS[kind]
    t = x / scale
    if zp is not None:
        t += zp.to(x.dtype)
    if k["type"] == "float":
        q = torch.clamp(t, -448.0, 448.0).to(F8).to(t.dtype)
    else:
        q = torch.round(torch.clamp(t, -(2.0 ** k["num_bits"]) / 2, 2.0 ** k["num_bits"] / 2 - 1))
    d = q.to(scale.dtype)
    if zp is not None:
        d = d - zp.to(scale.dtype)
    return d * scale


# rows wider than the 256 elements of the fixtures, as (B, H, S, D): a row of two waves; a row that is the workgroup, three rows so that
# the second workgroup is partial; the unit loop running twice; the element form with 257 units — the loop's second trip has one lane
# and a 4-element unit
WIDE_SHAPES = ((1, 2, 3, 1024), (1, 1, 3, 2048), (1, 2, 3, 4096), (1, 2, 3, 2052))


def wide_input(shape, dtype, device, seed=0):
    """finite random values laid out as a Llama's states are: (B, S, H, D).transpose(1, 2)"""
    B, H, S, D = shape
    x = torch.randn(B, S, H, D, generator=torch.Generator().manual_seed(seed + D)).to(dtype).to(device).transpose(1, 2)
    assert torch.isfinite(x).all()
    return x


def strategy_of(r):
    return "attn_head" if r["strategy"] == "attn_head" else "tensor"


def quantized_dtype(r):
    return F8 if KINDS[r["kind"]]["type"] == "float" else torch.int8


def stored(r) -> bool:
    B, H, S, D = logical_shape(r)
    return B * H * S * D <= 2048 and r["dtypes"].startswith("bf16")
