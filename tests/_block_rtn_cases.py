"""The case matrix of the block-wise 8-bit round-to-nearest fixtures (tools/gen_golden_block_rtn.py writes them, tests/test_block_rtn.py and
tests/test_gpu_block_rtn.py read them).  A case is (shape, block, dtype); its input is an integer formula of its recipe, so the manifest keeps only
the sha256 of the input and the fixture the reference's `scale`, `zero_point` and codes `q` for the three kinds."""
import hashlib

import torch

BF16, F16, F32, F8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
DTYPES = {"bf16": BF16, "f16": F16, "f32": F32}
# kind -> the QuantizationArgs of the weights besides strategy and block_structure
KINDS = {"fp8": dict(num_bits=8, type="float", symmetric=True), "int8": dict(num_bits=8, type="int", symmetric=True),
         "int8_zp": dict(num_bits=8, type="int", symmetric=False)}

# what the one-pass kernel's plan takes: one block; 2 x 3 blocks with planted ones; ragged last rows of blocks (100 = one partial block, 200 = a
# whole and a partial one); 64 x 64 blocks (2 units per thread); 32 x 128 (2 units per thread, 16 units per block row); 1 x 128 (16 live threads)
FAST = [((128, 128), (128, 128), None), ((256, 384), (128, 128), "planted"), ((100, 256), (128, 128), None), ((200, 256), (128, 128), None),
        ((192, 192), (64, 64), None), ((96, 256), (32, 128), None), ((8, 256), (1, 128), None)]
# what it refuses: ragged columns (with and without ragged rows), float32 weights
FALLBACK = [((128, 200), (128, 128), "bf16"), ((128, 200), (128, 128), "f16"), ((130, 136), (128, 128), "bf16"), ((130, 136), (128, 128), "f16"),
            ((256, 256), (128, 128), "f32")]


def key_of(shape, block, dtype: str, special=None) -> str:
    return f"{shape[0]}x{shape[1]}.b{block[0]}x{block[1]}.{dtype}" + (f".{special}" if special else "")


def case_list():
    """[(key, recipe)] — recipe = dict(shape, block, dtype, special, fast, salt).  Deterministic."""
    out = []
    for shape, block, special in FAST:
        for dtype in ("bf16", "f16"):
            out.append((key_of(shape, block, dtype, special), dict(shape=list(shape), block=list(block), dtype=dtype, special=special, fast=True)))
    for shape, block, dtype in FALLBACK:
        out.append((key_of(shape, block, dtype), dict(shape=list(shape), block=list(block), dtype=dtype, special=None, fast=False)))
    for i, (_, r) in enumerate(out):
        r["salt"] = i % 7 + 1
    return out


def make_weight(r) -> torch.Tensor:
    """the case's weight on the CPU: a multiplicative hash of the element index mapped to [-7.8, 7.8] in steps of 2^-8, under a per-block magnitude
    of 2^-6 .. 2^3 that differs between neighbouring blocks and signs that make some blocks one-sided"""
    rows, cols = r["shape"]
    bh, bw = r["block"]
    i = torch.arange(rows * cols, dtype=torch.int64).reshape(rows, cols)
    h = ((i + 977 * r["salt"]) * 2654435761) % 4294967296
    v = ((h >> 7) % 4001 - 2000).to(torch.float32) / 256.0
    blk = (torch.arange(rows)[:, None] // bh) * 5 + (torch.arange(cols)[None, :] // bw) * 3 + r["salt"]
    v = v * torch.pow(2.0, (blk % 10 - 6).to(torch.float32))
    v = torch.where(blk % 4 == 1, v.abs() + 0.001, v)    # an all-positive block: zero joins the range
    v = torch.where(blk % 4 == 3, -v.abs() - 0.001, v)   # an all-negative one
    x = v.to(DTYPES[r["dtype"]])
    if r["special"] == "planted":
        x[:bh, bw:2 * bw] = 0                  # an all-zero block: scale = the dtype's eps
        x[bh:2 * bh, :bw] = -2.0 ** -24        # tiny negatives under one large value: their codes round to -0.0 in the cast, behind the zero-point add
        x[bh + 3, 5] = 4.0
        x[bh + 4, 7] = -0.0                    # a -0.0 quotient: + the (all-zero) zero point = +0.0
    return x.contiguous()


def stores_codes(r, kind: str) -> bool:
    """does the fixture hold this case's codes in full (the FP8 kind of a weight of at most 40000 elements), or only their sha256 in the manifest?"""
    return kind == "fp8" and r["shape"][0] * r["shape"][1] <= 40000


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def block_rows(x: torch.Tensor, block):
    """the blocks of `x` as rows, zero-padded to whole blocks, and the block grid's shape"""
    bh, bw = block
    rows, cols = x.shape
    rb, cb = -(-rows // bh), -(-cols // bw)
    p = torch.zeros((rb * bh, cb * bw), dtype=x.dtype)
    p[:rows, :cols] = x
    return p.reshape(rb, bh, cb, bw).transpose(1, 2).reshape(rb * cb, bh * bw).contiguous(), (rb, cb)


def oracle_triple(O, x: torch.Tensor, block, kind: str):
    """(scale, zero_point, q) of the pinned oracle: the blocks as rows under its channel-wise calculate_qparams, then its block quantize — FLOAT with
    the all-zero float8 zero point of a calibrated scheme present"""
    rows_of_blocks, grid = block_rows(x, block)
    if kind == "fp8":
        scale = O.calculate_qparams_float(rows_of_blocks, kind="fp8").reshape(grid)
        zp = torch.zeros(grid, dtype=F8)
        q = O.quantize(x, scale, zp, num_bits=8, strategy="block", block_structure=list(block), dtype=F8, qtype="float")
    else:
        scale, zp = (t.reshape(grid) for t in O.calculate_qparams_minmax(rows_of_blocks, num_bits=8, group_size=None, symmetric=KINDS[kind]["symmetric"]))
        q = O.quantize(x, scale, zp, num_bits=8, strategy="block", block_structure=list(block), dtype=torch.int8)
    return scale.contiguous(), zp.contiguous(), q


def bits(t: torch.Tensor) -> torch.Tensor:
    if t.dtype.itemsize == 1:
        return t.view(torch.uint8)
    return t.view(torch.int16) if t.dtype in (BF16, F16) else t.view(torch.int32) if t.dtype == F32 else t
