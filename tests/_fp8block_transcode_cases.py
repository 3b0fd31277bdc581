"""The case matrix of the FP8-block -> MXFP8 / NVFP4 transcodings, shared by tools/gen_golden_fp8block_transcode.py (which runs the reference over it)
and tests/test_fp8block_transcode.py / tests/test_gpu_fp8block_transcode.py.  The recipes — `synth_codes`, `synth_scales`, `finite_codes`,
`sweep_scales`, `inputs`, `sha` — are those of tests/_fp8block_mxfp4_cases.py, imported; every case of that matrix is a case of both targets here.  The
fixture stores outputs only: whole up to `WHOLE_MAX` bytes, else their sha256."""
import json
import os

import torch

import _fp8block_mxfp4_cases as M
from _fp8block_mxfp4_cases import DENSE_DTYPES, DTYPES, F8, GOLDEN, NAN_CODE_CASES, WHOLE_MAX, finite_codes, sha, sweep_scales, synth_codes, synth_scales  # noqa: F401

TARGETS = ("mxfp8", "nvfp4")
GROUP = {"mxfp8": 32, "nvfp4": 16}
# a workgroup's share of groups: CT_FP8BLOCK_MXFP8_GROUPS_PER_BLOCK / CT_FP8BLOCK_NV_GROUPS_PER_BLOCK of include/ct_hip.h (tests/test_fp8block_transcode.py
# holds each to the header and the binding)
GROUPS_PER_BLOCK = {"mxfp8": 512, "nvfp4": 1024}
# the outputs of a target in the shard's order: (name in the fixture, key suffix in a shard)
OUTPUTS = {"mxfp8": (("codes", "weight"), ("e8m0", "weight_scale")),
           "nvfp4": (("packed", "weight_packed"), ("scale_f8", "weight_scale"), ("global_scale", "weight_global_scale"))}
FLOAT8_OUTPUTS = {("mxfp8", "codes"), ("nvfp4", "scale_f8")}  # stored as bytes; compared with every NaN code as ONE NaN
SWEEP_CASES = ("allcodes_b1x256", "allcodes_b1x32")
HOLDS_NAN_CODES = SWEEP_CASES + tuple(NAN_CODE_CASES)  # every other case is `finite_codes`: the reference's output in every byte


def share_shape(groups: int, group: int):
    """(rows, cols) of a weight of exactly `groups` groups of `group` columns: the most nearly square factorisation"""
    rows = max(r for r in range(1, int(groups ** 0.5) + 1) if groups % r == 0)
    return rows, groups // rows * group


def _own_cases():
    # key, rows, cols, block, scale dtype, scale layout, targets
    own = []
    for t in TARGETS:  # one group fewer and one group more than the kernel's workgroup share
        for tag, n in (("m1", GROUPS_PER_BLOCK[t] - 1), ("p1", GROUPS_PER_BLOCK[t] + 1)):
            own.append((f"share_{tag}.{t}", *share_shape(n, GROUP[t]), (128, 128), "float32", "full", (t,)))
    own += [
        ("nv_r3x48", 3, 48, (128, 128), "float32", "full", ("nvfp4",)),               # columns a multiple of 16 and not of 32
        ("nv_r64x96_b32x48", 64, 96, (32, 48), "bfloat16", "full", ("nvfp4",)),       # a block width that is a multiple of 16 and not of 32
        ("nv_refused_b96x40", 200, 320, (96, 40), "float32", "full", ("nvfp4",)),     # a block width the NVFP4 plan refuses ((96, 80) it admits)
    ]
    return own


OWN = {c[0]: dict(zip(("rows", "cols", "block", "sdt", "layout", "targets"), c[1:]), salt=211 + 7 * i) for i, c in enumerate(_own_cases())}
CASES = {**{k: dict(v, targets=TARGETS) for k, v in M.CASES.items()}, **OWN}
REFUSED = {"mxfp8": "refused_b96x80", "nvfp4": "nv_refused_b96x40"}  # the block each fused plan refuses


def cases_of(target: str):
    return [k for k, c in CASES.items() if target in c["targets"]]


def inputs(key):
    """(float8_e4m3fn weight, weight_scale_inv) of a case"""
    if key in M.CASES:
        return M.inputs(key)
    c = CASES[key]
    rows, cols, (bh, bw) = c["rows"], c["cols"], c["block"]
    return finite_codes(synth_codes(rows, cols, c["salt"])), synth_scales(-(-rows // bh), -(-cols // bw), c["salt"], DTYPES[c["sdt"]])


def canonical(target: str, name: str, t: torch.Tensor) -> torch.Tensor:
    """the bytes of an output that are compared: a float8 output's two NaN codes (0x7f, 0xff) are one NaN; everything else is compared as it is"""
    b = t.cpu().contiguous()
    b = b.view(torch.uint8) if b.dtype != torch.float32 else b.view(torch.int32)
    if (target, name) in FLOAT8_OUTPUTS:
        b = torch.where((b & 0x7F) == 0x7F, torch.full_like(b, 0x7F), b)
    return b


_LOADED = []


def load_fixture():
    """(tensors, manifest) of tests/golden/fp8block_transcode.*"""
    if not _LOADED:
        from safetensors.torch import load_file

        with open(os.path.join(GOLDEN, "fp8block_transcode_manifest.json")) as f:
            manifest = json.load(f)
        _LOADED.append((load_file(os.path.join(GOLDEN, "fp8block_transcode.safetensors")), manifest))
    return _LOADED[0]


_DTYPE_OF = {"codes": F8, "e8m0": torch.uint8, "packed": torch.uint8, "scale_f8": F8, "global_scale": torch.float32}


def assert_golden(target: str, case: str, dtype: str, got) -> None:
    """the outputs `got` (in the target's order) against the fixture's records `<target>.<case>.<dense dtype>.<name>`: dtype, shape, and the compared
    bytes (`canonical`) one by one where the output is stored, by sha256 where it is not"""
    blob, manifest = load_fixture()
    assert len(got) == len(OUTPUTS[target])
    for (name, _), t in zip(OUTPUTS[target], got):
        key = f"{target}.{case}.{dtype}.{name}"
        rec = manifest["outputs"][key]
        assert t.dtype == _DTYPE_OF[name] and list(t.shape) == rec["shape"], (key, t.dtype, tuple(t.shape))
        mine = canonical(target, name, t)
        if rec["whole"]:
            want = blob[key]
            bad = (mine != want).reshape(mine.shape[0], -1).nonzero()
            assert bad.numel() == 0, (key, f"{bad.shape[0]} entries differ, first at {bad[0].tolist()}")
        assert sha(mine) == rec["sha256"], key
