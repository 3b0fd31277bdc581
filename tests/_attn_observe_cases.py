"""The case matrix of the attention min-max observer fixtures (tools/gen_golden_attn_observe.py writes them,
tests/test_attn_observe.py and tests/test_gpu_attn_observe.py read them).  Inputs come from `_attn_cases.make_input` (integer
formulas placed in a storage layout), so a case is fully described by its recipe; every case keeps the sha256 of its input and the
reference observer's `min_vals`, `max_vals`, `scale` and `zero_point` themselves (a few bytes each).

synth's first rows are edge rows — zeros, +-0, subnormals, +inf, -inf, NaN, the dtype's maximum — which land in the first heads:
a per-head case sees every one of them in some head and plain values in the others.  `clean` recipes replace the non-finite
values, so that a whole-tensor result is a number."""
import itertools

import torch

import _attn_cases as C
from _attn_cases import BF16, DTYPES, F8, F16, F32, WIDE_SHAPES, canonical_bytes, sha, wide_input  # noqa: F401

D_VALUES = C.D_VALUES  # 16 = two units .. 256 = 32 lanes per row, 80 = ten units on sixteen lanes, 20 = the element form
LAYOUTS = ("contiguous", "transposed", "fused_k", "misaligned", "expanded", "3d")
KINDS = dict(C.KINDS, int4=dict(num_bits=4, type="int", symmetric=True))
FACTORS = dict(B=(1, 2), H=(1, 2, 8), S=(1, 5, 33), dtype=("bf16", "f16", "f32"), kind=("fp8", "int8", "int8_zp", "int4_zp", "int2"),
               strategy=("attn_head", "tensor"), base=("k", "input"))
PAIRWISE_D = 64


def normalise(r):
    """the constraints between factors: an `input` activation is observed per tensor, as a contiguous (B, S, hidden) tensor; a 3-D
    state has no batch, an expanded one has two"""
    r = dict(r)
    if r["base"] == "input":
        r["strategy"], r["layout"] = "tensor", "contiguous"
    if r["layout"] == "3d":
        r["B"] = 1
    if r["layout"] == "expanded":
        r["B"] = 2
    return r


def key_of(r):
    tail = f".{r['special']}" if r.get("special") else ""
    return ".".join([r["base"], r["kind"], r["strategy"], r["dtype"], r["layout"], f"{r['B']}x{r['H']}x{r['S']}x{r['D']}"]) + tail


def case_list():
    """[(key, recipe)]: every layout at every D for the flagship bf16 FP8 attn_head observer, a greedy pairwise cover of FACTORS
    (up to `normalise`) on finite values, and the special cases.  Deterministic."""
    out, seen = [], set()

    def add(r):
        r = normalise(dict(dict(special=None, clean=False), **r))
        r["salt"] = len(out) % 11 + 1
        r["dtypes"] = f"{r['dtype']}/{r['dtype']}"  # what _attn_cases.make_input reads
        k = key_of(r)
        if k not in seen:
            seen.add(k)
            out.append((k, r))
        return r

    for layout in LAYOUTS:
        for D in D_VALUES:
            add(dict(D=D, B=2, H=8, S=5, layout=layout, dtype="bf16", kind="fp8", strategy="attn_head", base="k"))

    names = list(FACTORS)

    def pairs(r):
        return {(a, r[a], b, r[b]) for a, b in itertools.combinations(names, 2)}

    uncovered = set()
    for a, b in itertools.combinations(names, 2):
        for va in FACTORS[a]:
            for vb in FACTORS[b]:
                uncovered.add((a, va, b, vb))
    state = 24680
    while uncovered:
        best, best_gain = None, -1
        for _ in range(48):
            cand = {}
            for n in names:
                state = (state * 1103515245 + 12345) & 0x7FFFFFFF
                cand[n] = FACTORS[n][(state >> 8) % len(FACTORS[n])]
            cand.update(D=PAIRWISE_D, layout="transposed")
            gain = len(pairs(normalise(cand)) & uncovered)
            if gain > best_gain:
                best, best_gain = cand, gain
        if best_gain == 0:
            a, va, b, vb = next(iter(sorted(uncovered)))
            cand = {n: FACTORS[n][0] for n in names}
            cand.update(D=PAIRWISE_D, layout="transposed")
            cand[a], cand[b] = va, vb
            if not (pairs(normalise(cand)) & uncovered):  # what `normalise` makes impossible (input with attn_head)
                uncovered.discard((a, va, b, vb))
                continue
            best = cand
        uncovered -= pairs(add(dict(best, clean=True)))

    flagship = dict(D=64, B=2, H=8, S=5, layout="transposed", dtype="bf16", strategy="attn_head", base="k", clean=True)
    add(dict(flagship, kind="fp8", special="zero_head"))
    add(dict(flagship, kind="int8_zp", special="zero_head"))
    add(dict(flagship, kind="fp8", special="signed_heads"))
    add(dict(flagship, kind="int8_zp", special="signed_heads"))
    add(dict(flagship, kind="fp8", special="nan_inf"))
    add(dict(flagship, kind="int8_zp", special="nan_inf"))
    for strategy in ("tensor", "attn_head"):  # the reference's known answer (test_static_attention_quantization)
        add(dict(D=4, B=1, H=2, S=3, layout="contiguous", dtype="bf16", kind="int4", strategy=strategy, base="k", special="arange"))
    return out


def logical_shape(r):
    return (r["B"], r["H"], r["S"], r["D"])


def make_observed(r, device="cpu"):
    """the tensor the observer is called with, built ON `device`"""
    B, H, S, D = logical_shape(r)
    if r.get("special") == "arange":
        return torch.arange(B * H * S * D, dtype=torch.float32).to(DTYPES[r["dtype"]]).reshape(B, H, S, D).to(device)
    x = C.make_input(r, device)
    if r.get("clean"):
        x.masked_fill_(~torch.isfinite(x), 1.5)
    special = r.get("special")
    if special == "zero_head":  # scale = the dtype's eps
        x[:, 1] = 0
    elif special == "signed_heads":  # an all-negative and an all-positive head: zero joins the range
        x[:, 2] = -x[:, 2].abs() - 1
        x[:, 3] = x[:, 3].abs() + 1
    elif special == "nan_inf":
        x[0, 1, 2, 3] = float("nan")
        x[-1, 4, 0, 1] = float("inf")
    if r["base"] == "input":
        x = x.reshape(B, S, H * D)  # (batch, seq, hidden)
    return x


def reference_view(r, x):
    """what the reference's observer is shown: its flatten is written for 4-D states, so a 3-D state goes in as (1, H, S, D)"""
    return x.unsqueeze(0) if (r["base"] != "input" and x.ndim == 3) else x


def args_of(r):
    return dict(strategy=r["strategy"], **KINDS[r["kind"]])


def expected_shape(r):
    return (r["H"], 1, 1) if r["strategy"] == "attn_head" else (1,)


def zp_dtype(r):
    return F8 if KINDS[r["kind"]]["type"] == "float" else torch.int8


def head_rows(r, x):
    """the values of each scale entry as one row of a 2-D tensor: (entries, everything else)"""
    if r["strategy"] == "tensor":
        return x.reshape(1, -1)
    B, H, S, D = logical_shape(r)
    return x.reshape(B, H, S, D).transpose(0, 1).reshape(H, -1)
