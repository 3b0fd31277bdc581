"""The case matrix of the FP8-block -> MXFP4 transcoding and of MXFP4Quantizer, shared by tools/gen_golden_fp8block_mxfp4.py (which runs the
reference over it) and tests/test_fp8block_mxfp4.py / tests/test_gpu_fp8block_mxfp4.py.  Inputs are synthesised from integer formulas — the recipes of
tools/gen_golden_fp8block.py, restated — so the fixture stores outputs only: whole up to `WHOLE_MAX` bytes, else their sha256."""
import hashlib
import json
import os

import torch

F32, BF16, F16, F8 = torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn
DTYPES = {"float32": F32, "bfloat16": BF16, "float16": F16}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WHOLE_MAX = 8192
GROUPS_PER_BLOCK = 512  # CT_FP8BLOCK_MX_GROUPS_PER_BLOCK of include/ct_hip.h (tests/test_fp8block_mxfp4.py holds the two together)


def synth_codes(rows, cols, salt):
    """float8_e4m3fn codes from an integer hash of (row, column): every byte value occurs, NaN codes included"""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    return ((r * 7919 + c * 104729 + salt * 13) * 2654435761 >> 13).remainder(256).to(torch.uint8).view(F8)


def synth_scales(rows, cols, salt, dtype):
    """positive scales in [2^-12, 2^-4) with a hashed mantissa, exactly representable in `dtype`"""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    h = ((r * 31 + c * 17 + salt) * 2246822519 >> 7).remainder(1 << 23)
    e = (h >> 20).remainder(8) + 115  # biased exponent 115..122
    bits = (e << 23) | (h & ((1 << 23) - 1))
    if dtype != F32:
        bits = bits & ~((1 << 13) - 1)  # 10 mantissa bits: exact in float16 (normal here) and, after rounding, in bfloat16
    return bits.to(torch.int32).view(F32).to(dtype)


def finite_codes(w):
    """`w` with its two NaN codes (0x7f, 0xff) replaced by the largest finite code of the same sign (0x7e, 0xfe).  The reference's MX scale of a
    group that holds a NaN depends on the host CPU's reduction, so a case that is about a shape keeps NaN out and is the reference's output in every
    group; NaN codes are the business of the all-codes sweeps and of `NAN_CODE_CASES`"""
    b = w.view(torch.uint8)
    return torch.where((b & 0x7F) == 0x7F, b & 0xFE, b).view(F8)


def sweep_scales():
    """one scale per row of the all-codes case: negative, tiny (subnormal results in every dense dtype), around one, large (float16 overflow to
    inf), and zero of either sign"""
    vals = [1.0, -1.0, 2.0 ** -120, -(2.0 ** -127), 2.0 ** -140, 2.0 ** -14, 2.0 ** -20, -(2.0 ** -24), 0.0, -0.0, 3.0 ** 0.5,
            1.0 / 3.0, 1e-3, 146.0, 147.0, 2.0 ** 8, -(2.0 ** 12), 65504.0 / 448.0, 1.5 * 2.0 ** 7, 2.0 ** 100]
    return torch.tensor(vals, dtype=F32)[:, None]


def synth_dense(rows, cols, salt, dtype):
    """finite dense weights in [-4, 4) on a grid of 1 / 512 (exact in bfloat16 only after its rounding, which is part of the recipe)"""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    h = ((r * 7919 + c * 104729 + salt * 13) * 2654435761 >> 11).remainder(4096)
    return ((h - 2048).to(F32) / 512.0).to(dtype)


# The workgroup of ct_fp8block_mxfp4_batch owns GROUPS_PER_BLOCK = 512 MX groups: 73 x 224 is 73 * 7 = 511 groups (one less than a workgroup), 27 x 608 is
# 27 * 19 = 513 (one more: a second workgroup with one live lane pair).
# key, rows, cols, block, scale dtype, scale layout ("full", "1x1", "1xN", "Nx1", "sweep")
SHAPES = [
    ("r1x32", 1, 32, (128, 128), "float32", "full"),
    ("r3x32", 3, 32, (128, 128), "float32", "full"),
    ("sq128", 128, 128, (128, 128), "float32", "full"),
    ("r200x320", 200, 320, (128, 128), "float32", "full"),
    ("r130x160_b128x64", 130, 160, (128, 64), "float32", "full"),
    ("r96x96_b64x32", 96, 96, (64, 32), "float32", "full"),
    ("sq256_b1x128", 256, 256, (1, 128), "float32", "full"),
    ("r1x8192", 1, 8192, (128, 128), "float32", "full"),
    ("g511_r73x224", 73, 224, (128, 128), "float32", "full"),
    ("g513_r27x608", 27, 608, (128, 128), "float32", "full"),
    ("r200x320_b64_bf16", 200, 320, (64, 64), "bfloat16", "full"),
    ("r200x320_b64_f16", 200, 320, (64, 64), "float16", "full"),
    ("r200x320_b64_bcast11", 200, 320, (64, 64), "float32", "1x1"),
    ("r200x320_b64_bcast_row", 200, 320, (64, 64), "bfloat16", "1xN"),
    ("r200x320_b64_bcast_col", 200, 320, (64, 64), "float16", "Nx1"),
    ("allcodes_b1x256", 20, 256, (1, 256), "float32", "sweep"),
    ("allcodes_b1x32", 20, 256, (1, 32), "float32", "sweep"),
    ("mixed.down_proj", 384, 512, (128, 128), "float32", "full"),
    ("mixed.q_proj", 200, 320, (128, 128), "bfloat16", "full"),
    ("mixed.kv_b_proj", 130, 160, (128, 128), "float16", "full"),
    ("mixed.o_proj", 1, 32, (128, 128), "float32", "full"),
    ("refused_b96x80", 200, 320, (96, 80), "float32", "full"),
    ("kv_a_576x7168", 576, 7168, (128, 128), "float32", "full"),
]
NAN_CODE_CASES = ("mixed.q_proj", "kv_a_576x7168")  # the hashed codes as they come, NaN codes included: one stored case and the large one
CASES = {s[0]: dict(zip(("rows", "cols", "block", "sdt", "layout"), s[1:]), salt=3 + 5 * i) for i, s in enumerate(SHAPES)}
DENSE_DTYPES = ("bfloat16", "float16")
QUANTIZER_SHAPES = {"down_proj": (384, 512), "q_proj": (200, 320), "o_proj": (1, 32)}  # MXFP4Quantizer's dense shard


def inputs(key):
    """(float8_e4m3fn weight, weight_scale_inv) of a case"""
    c = CASES[key]
    rows, cols, (bh, bw), sdt = c["rows"], c["cols"], c["block"], DTYPES[c["sdt"]]
    nrb, ncb = -(-rows // bh), -(-cols // bw)
    if c["layout"] == "sweep":
        w = torch.arange(256, dtype=torch.int64).repeat(rows, cols // 256).to(torch.uint8).view(F8)
        return w, sweep_scales().expand(rows, ncb).contiguous().to(sdt)
    shape = {"full": (nrb, ncb), "1x1": (1, 1), "1xN": (1, ncb), "Nx1": (nrb, 1)}[c["layout"]]
    w = synth_codes(rows, cols, c["salt"])
    if key not in NAN_CODE_CASES:
        w = finite_codes(w)
    return w, synth_scales(*shape, c["salt"], sdt)


def dense_inputs(name, dtype):
    rows, cols = QUANTIZER_SHAPES[name]
    return synth_dense(rows, cols, 101 + len(name), DTYPES[dtype])


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


_LOADED = []


def load_fixture():
    """(tensors, manifest) of tests/golden/fp8block_mxfp4.*"""
    if not _LOADED:
        from safetensors.torch import load_file

        with open(os.path.join(GOLDEN, "fp8block_mxfp4_manifest.json")) as f:
            manifest = json.load(f)
        _LOADED.append((load_file(os.path.join(GOLDEN, "fp8block_mxfp4.safetensors")), manifest))
    return _LOADED[0]


def assert_golden(record_key: str, packed: torch.Tensor, e8m0: torch.Tensor) -> None:
    """`packed` / `e8m0` against the fixture's record `record_key` (`<case>.<dense dtype>`, or `quantizer.<name>.<dtype>`): byte for byte where the
    output is stored, by sha256 where it is not"""
    blob, manifest = load_fixture()
    for name, got in (("packed", packed), ("e8m0", e8m0)):
        rec = manifest["outputs"][f"{record_key}.{name}"]
        got = got.cpu().contiguous()
        assert got.dtype == torch.uint8 and list(got.shape) == rec["shape"], (record_key, name, got.dtype, tuple(got.shape))
        if rec["whole"]:
            want = blob[f"{record_key}.{name}"]
            bad = (got != want).nonzero()
            assert bad.numel() == 0, (record_key, name, f"{bad.shape[0]} bytes differ, first at {bad[0].tolist()}: "
                                      f"got {int(got[tuple(bad[0])]):#x}, want {int(want[tuple(bad[0])]):#x}")
        assert sha(got) == rec["sha256"], (record_key, name)
