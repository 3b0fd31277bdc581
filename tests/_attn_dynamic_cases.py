"""The case matrix of the dynamic attention q / k / v QDQ fixtures (tools/gen_golden_attn_dynamic.py writes them,
tests/test_attn_dynamic.py and tests/test_gpu_attn_dynamic.py read them).  Recipes as in `_attn_cases`: the logical (B, H, S, D)
values of `_dynamic_cases.synth` placed in a storage layout (`_attn_cases.make_input`), the x dtype and a dynamic preset.  synth's edge
rows (zeros, +-0, subnormals, +-inf, NaN, 448, the dtype's maximum) stay in: rows are independent under group scales, and NaNs are
canonicalised as in the other fixtures.  Every case keeps the sha256 of its input and, of the reference's output, scale and zero
point, the dtype, shape, strides and sha256; the small bfloat16 cases also keep the output itself.

`expected_form` is this file's own rule — written from the kernel's contract, not from the plan — for which form a case must take."""
import itertools

from _attn_cases import canonical_bytes, make_input, sha  # noqa: F401
from _dynamic_cases import BF16, DTYPES, F8, F16, F32, NVFP4_GLOBAL, PRESETS as DYN_PRESETS, global_scale_of  # noqa: F401

# the smallest shapes at which the kernel can go wrong: 16 = one NVFP4 group on two lanes, 64, 80 = five groups of 16 on ten of
# sixteen lanes, 96 = three MX groups on twelve of sixteen lanes, 128, 192 = 24 of 32 lanes, 256; 20 = not whole units (copy form)
D_VALUES = (16, 64, 80, 96, 128, 192, 256, 20)
B_VALUES = (1, 2)
H_VALUES = (1, 2, 8)
S_VALUES = (1, 5, 33)  # 33 rows = more than one workgroup pass, odd
LAYOUTS = ("contiguous", "transposed", "fused_k", "fused_v", "misaligned", "expanded", "3d")
DTYPE_PAIRS = ("bf16/bf16", "f16/f16", "f32/f32")  # _attn_cases.make_input reads the x dtype in front of the slash


def _fp8_group(g):
    return dict(num_bits=8, type="float", strategy="group", group_size=g, symmetric=True, dynamic=True)


# preset -> (arguments; group_size "D": the head dim, one scale per (token, head)), NVFP4 global-scale name
PRESETS = {
    "fp8_group16": (_fp8_group(16), None),
    "fp8_group64": (_fp8_group(64), None),
    "fp8_groupD": (_fp8_group("D"), None),
    "int8_group32": (dict(num_bits=8, type="int", strategy="group", group_size=32, symmetric=True, dynamic=True), None),
    "int4_group32_asym": (DYN_PRESETS["int4_group32_asym"], None),
    "mxfp4": (DYN_PRESETS["mxfp4"], None),
    "mxfp8": (DYN_PRESETS["mxfp8"], None),
    "nvfp4_nogs": (DYN_PRESETS["nvfp4"], "nogs"),
    "nvfp4_gs": (DYN_PRESETS["nvfp4"], "gs"),
    "nvfp4_gsbig": (DYN_PRESETS["nvfp4"], "gsbig"),
    "fp8_token": (DYN_PRESETS["fp8_token"], None),
    "int8_token_asym": (DYN_PRESETS["int8_token_asym"], None),
    "fp8_tensor": (DYN_PRESETS["fp8_tensor"], None),
}
FACTORS = dict(D=D_VALUES, B=B_VALUES, H=H_VALUES, S=S_VALUES, layout=LAYOUTS, dtypes=DTYPE_PAIRS, preset=tuple(PRESETS))


def _pow2(n):
    return n > 0 and n & (n - 1) == 0


def preset_args(r):
    """the arguments of a recipe's preset as a plain dict (group_size "D" resolved)"""
    a = dict(PRESETS[r["preset"]][0])
    if a.get("group_size") == "D":
        a["group_size"] = r["D"]
    return a


def gs_name(r):
    return PRESETS[r["preset"]][1]


def global_scale(r):
    name = gs_name(r)
    return None if name is None else global_scale_of(name)


def normalise(r):
    """the constraints between factors: a 3-D tensor has no batch, an expanded one has two; a group preset whose group does not
    divide D — or, for group == D, is no 8 * 2^k — becomes the FP8 group preset that does (D = 20: only D itself)"""
    r = dict(r)
    if r["layout"] == "3d":
        r["B"] = 1
    if r["layout"] == "expanded":
        r["B"] = 2
    a, D = PRESETS[r["preset"]][0], r["D"]
    if a["strategy"] in ("group", "tensor_group"):
        g = a["group_size"]
        if (g == "D" and not (_pow2(D) or D == 20)) or (g != "D" and D % g):
            r["preset"] = "fp8_groupD" if (_pow2(D) or D == 20) else "fp8_group16"
    return r


def key_of(r):
    return ".".join([r["preset"], r["dtypes"].split("/")[0], r["layout"], f"{r['B']}x{r['H']}x{r['S']}x{r['D']}"])


def case_list():
    """[(key, recipe)]: a greedy pairwise cover of FACTORS (every pair of values of every two factors occurs, up to `normalise`),
    plus every layout at every D for bf16 MXFP4 (D % 32 == 0) and NVFP4 with a global scale, plus every preset on the prefill and
    the decode view a Llama passes.  Deterministic."""
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

    state = 24680
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
            # what `normalise` makes impossible (3d with B = 2, MXFP4 at D = 16, ...) stays uncovered: drop it
            a, va, b, vb = next(iter(sorted(uncovered, key=repr)))
            cand = {n: FACTORS[n][0] for n in names}
            cand[a], cand[b] = va, vb
            if not (pairs(normalise(cand)) & uncovered):
                uncovered.discard((a, va, b, vb))
                continue
            best = cand
        uncovered -= add(best)
    for layout in LAYOUTS:
        for D in D_VALUES:
            if D % 32 == 0:
                add(dict(D=D, B=2, H=8, S=5, layout=layout, dtypes="bf16/bf16", preset="mxfp4"))
            add(dict(D=D, B=2, H=8, S=5, layout=layout, dtypes="bf16/bf16", preset="nvfp4_gs"))
    for preset in PRESETS:
        for S in (33, 1):
            add(dict(D=128, B=2, H=8, S=S, layout="transposed", dtypes="bf16/bf16", preset=preset))
    return out


def possible_pairs():
    """the pairs of factor values `normalise` leaves possible: what the cover must contain"""
    names = list(FACTORS)
    got = set()
    for combo in itertools.product(*FACTORS.values()):
        r = normalise(dict(zip(names, combo)))
        got |= {(a, r[a], b, r[b]) for a, b in itertools.combinations(names, 2)}
    return got


def logical_shape(r):
    return (r["B"], r["H"], r["S"], r["D"])


def x_dtype(r):
    return DTYPES[r["dtypes"].split("/")[0]]


def expected_form(r):
    """"strided" or "copy", from the kernel's contract alone: rows of whole aligned 8-element units, groups of 8 * 2^k <= 512
    elements inside a row; a token scale is a row only at S == 1 and only a power-of-two row is such a group; the tensor strategy
    reduces across rows"""
    a, D, S = preset_args(r), r["D"], r["S"]
    if r["layout"] == "misaligned" or D % 8:
        return "copy"
    if a["strategy"] == "tensor":
        return "copy"
    if a["strategy"] == "token":
        return "strided" if (S == 1 and _pow2(D) and 8 <= D <= 512) else "copy"
    g = a["group_size"]
    assert D % g == 0 and g % 8 == 0 and _pow2(g // 8) and g <= 512, (r, g)  # normalise leaves no other group on whole units
    return "strided"


def stored(r) -> bool:
    B, H, S, D = logical_shape(r)
    return B * H * S * D <= 2048 and r["dtypes"].startswith("bf16")
