"""The case matrix of the NVFP4 -> MXFP4 transcoding, shared by tools/gen_golden_nvfp4_mxfp4.py (which runs the reference over it) and
tests/test_nvfp4_mxfp4.py / tests/test_gpu_nvfp4_mxfp4.py.  Inputs are synthesised from integer formulas, so the fixture
(tests/golden/nvfp4_mxfp4.json) stores outputs only: whole (base64) up to `WHOLE_MAX` bytes, else their sha256."""
import base64
import hashlib
import json
import os

import torch

F32, BF16, F8, U8 = torch.float32, torch.bfloat16, torch.float8_e4m3fn, torch.uint8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "nvfp4_mxfp4.json")
WHOLE_MAX = 8192
GROUPS_PER_BLOCK = 1024  # CT_NVFP4_MX_GROUPS_PER_BLOCK of include/ct_hip.h (tests/test_nvfp4_mxfp4.py holds the two together)
G = GROUPS_PER_BLOCK


def _grid(rows, cols):
    return torch.arange(rows, dtype=torch.int64)[:, None], torch.arange(cols, dtype=torch.int64)[None, :]


def synth_nibbles(rows, cols, salt):
    """the packed NVFP4 codes of a (rows, cols) weight, (rows, cols / 2) uint8, from an integer hash of (row, byte column): every byte value occurs"""
    r, c = _grid(rows, cols // 2)
    return ((r * 7919 + c * 104729 + salt * 13) * 2654435761 >> 13).remainder(256).to(U8)


def synth_scale_bytes(rows, cols, salt):
    """the float8_e4m3fn group scales of a (rows, cols) weight as bytes, (rows, cols / 16) uint8, hashed: zeros, negatives and both NaN bytes occur"""
    r, c = _grid(rows, cols // 16)
    return ((r * 31 + c * 17 + salt) * 2246822519 >> 7).remainder(256).to(U8)


def finite_scales(b):
    """scale bytes with the two NaN bytes (0x7f, 0xff) replaced by the largest finite one of the same sign (0x7e, 0xfe).  The reference's MX scale of
    a group that holds a NaN depends on the host CPU's reduction, so a golden case keeps NaN scales out; they are the business of the fused ==
    composition sweeps"""
    return torch.where((b & 0x7F) == 0x7F, b & 0xFE, b)


# key, rows, cols, global scale.  G = 1024 MX groups per workgroup: 1 x 32 (G - 1) is one lane short of a workgroup, 1 x 32 G exact, 1 x 32 (G + 1) a
# second workgroup with one live lane; 27 x 1216 is 27 * 38 = 1026 groups, so rows end inside the first workgroup and the second one has two live lanes
SHAPES = [
    ("r1x32", 1, 32, 2688.0),
    ("r3x32", 3, 32, 1.0),
    ("r200x320", 200, 320, 2688.0 * 1.25),
    ("r1x8192", 1, 8192, 448.0 * 6.0 / 3.5),
    ("g_minus_1", 1, 32 * (G - 1), 1500.0),
    ("g_exact", 1, 32 * G, 96.0),
    ("g_plus_1", 1, 32 * (G + 1), 3.0 ** 0.5 * 1000.0),
    ("r27x1216", 27, 1216, 777.0),
    ("kv_a_576x7168", 576, 7168, 2688.0 / 0.37),
    ("mixed.down_proj", 384, 512, 1234.5),
    ("mixed.q_proj", 200, 320, 2688.0),
    ("mixed.o_proj", 1, 32, 0.75),
    ("mixed.k_proj", 3, 64, 2.0 ** 12),
    ("mixed.v_proj", 130, 160, 5000.0),
]
CASES = {s[0]: dict(rows=s[1], cols=s[2], gs=s[3], salt=3 + 5 * i) for i, s in enumerate(SHAPES)}
SHAPE_KEYS = [s[0] for s in SHAPES if not s[0].startswith(("mixed.", "kv_a"))]
MIXED_KEYS = [s[0] for s in SHAPES if s[0].startswith("mixed.")]

# the whole scale domain: 256 rows x 64 columns (two MX groups, four NVFP4 groups per row).  Row r holds the scale byte r over one NVFP4 group of
# each MX group and a hashed byte over the other ("first": r is the first of the two, "second": the roles swapped); all 16 codes occur in every
# NVFP4 group.  GOLDEN_SCALES: the finite, non-zero global scales, which the fixture holds with the NaN bytes replaced (`finite_scales`)
SWEEP_ROWS, SWEEP_COLS = 256, 64
SWEEP_SCALES = {"1": 1.0, "2688": 2688.0, "2p-20": 2.0 ** -20, "2p20": 2.0 ** 20, "sqrt3": 3.0 ** 0.5, "2p-140": 2.0 ** -140, "2p100": 2.0 ** 100,
                "0": 0.0, "-1": -1.0, "inf": float("inf")}
GOLDEN_SCALES = ("1", "2688", "2p-20", "2p20", "sqrt3", "2p-140", "2p100")
SWEEP_LAYOUTS = ("first", "second")


def global_scale(value):
    return torch.tensor([value], dtype=F32)


def inputs(key):
    """(weight_packed uint8, weight_scale float8_e4m3fn, weight_global_scale float32 (1,)) of a shape case: NaN scale bytes replaced"""
    c = CASES[key]
    return (synth_nibbles(c["rows"], c["cols"], c["salt"]), finite_scales(synth_scale_bytes(c["rows"], c["cols"], c["salt"])).view(F8),
            global_scale(c["gs"]))


def sweep_inputs(layout, gs_name, finite=False):
    """(weight_packed, weight_scale, weight_global_scale) of a sweep case; `finite`: the NaN scale bytes replaced, as the fixture holds it"""
    r, g = _grid(SWEEP_ROWS, SWEEP_COLS // 16)  # g: the NVFP4 group of the row; its MX group is g // 2
    hashed = ((r * 131 + (g // 2) * 29 + 7) * 2654435761 >> 9).remainder(256)
    own = (g % 2 == 0) if layout == "first" else (g % 2 == 1)
    scale = torch.where(own, r.expand_as(hashed), hashed).to(U8)
    # the 16 codes of every NVFP4 group: k -> (a k + b) mod 16 with a odd, a permutation that depends on (row, group)
    r, c = _grid(SWEEP_ROWS, SWEEP_COLS)
    a, b = 2 * ((r + c // 16) % 8) + 1, (r * 5 + (c // 16) * 3) % 16
    codes = ((a * (c % 16) + b) % 16).to(U8)
    packed = codes[:, 0::2] | (codes[:, 1::2] << 4)  # low nibble first
    return packed.contiguous(), (finite_scales(scale) if finite else scale).view(F8), global_scale(SWEEP_SCALES[gs_name])


def sweep_key(layout, gs_name):
    return f"sweep_{layout}.gs_{gs_name}"


def golden_inputs():
    """{record key: (weight_packed, weight_scale, weight_global_scale)} of everything the fixture holds, in its order"""
    got = {key: inputs(key) for key in CASES}
    for layout in SWEEP_LAYOUTS:
        for name in GOLDEN_SCALES:
            got[sweep_key(layout, name)] = sweep_inputs(layout, name, finite=True)
    return got


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().view(U8).numpy().tobytes()).hexdigest()


def record(t: torch.Tensor) -> dict:
    """the fixture's record of one output"""
    t = t.contiguous()
    rec = dict(shape=list(t.shape), sha256=sha(t), whole=t.numel() <= WHOLE_MAX)
    if rec["whole"]:
        rec["base64"] = base64.b64encode(t.numpy().tobytes()).decode("ascii")
    return rec


_LOADED = []


def load_fixture():
    """tests/golden/nvfp4_mxfp4.json"""
    if not _LOADED:
        with open(FIXTURE) as f:
            _LOADED.append(json.load(f))
    return _LOADED[0]


def assert_golden(record_key: str, packed: torch.Tensor, e8m0: torch.Tensor) -> None:
    """`packed` / `e8m0` against the fixture's record `record_key`: byte for byte where the output is stored, by sha256 where it is not"""
    outputs = load_fixture()["outputs"]
    for name, got in (("packed", packed), ("e8m0", e8m0)):
        rec = outputs[f"{record_key}.{name}"]
        got = got.cpu().contiguous()
        assert got.dtype == U8 and list(got.shape) == rec["shape"], (record_key, name, got.dtype, tuple(got.shape))
        if rec["whole"]:
            want = torch.frombuffer(bytearray(base64.b64decode(rec["base64"])), dtype=U8).view(rec["shape"])
            bad = (got != want).nonzero()
            assert bad.numel() == 0, (record_key, name, f"{bad.shape[0]} bytes differ, first at {bad[0].tolist()}: "
                                      f"got {int(got[tuple(bad[0])]):#x}, want {int(want[tuple(bad[0])]):#x}")
        assert sha(got) == rec["sha256"], (record_key, name)
