"""Generate the FP8 block dequantizer's and the ModelOpt NVFP4 converter's golden vectors by running the UPSTREAM REFERENCE's
FP8BlockDequantizer and ModelOptNvfp4Converter (needs the reference sources; see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_fp8block.py

Writes tests/golden/fp8block.safetensors and tests/golden/fp8block_manifest.json.

- FP8 cases ("cases"): one shard each, converted by the reference's `process` (the manifest keeps the dict order of its input
  and output: a safetensors file keeps none).  The weights and scales of most modules keep only their recipe ("synth"): they
  are synthesised from integer formulas (`synth_codes`, `synth_scales`, restated in tests/test_fp8block_converter.py), and the
  manifest holds the sha256 of the reference's output with every NaN rewritten to one canonical NaN (NaN payload
  and sign are not compared).  The all-codes x scale-sweep modules and the tensors that pass through are stored: inputs under
  `<case>.in.`, the reference's dequantized weights under `<case>.out.`.
- ModelOpt cases ("modelopt"): a ModelOpt-convention shard under `mo.<case>.in.` and the reference's output under
  `mo.<case>.out.`; "modelopt_configs" holds `create_config().model_dump()` of the reference, with and without kv_cache_scheme.

Seeded: two runs write byte-identical files.  TEST INFRASTRUCTURE ONLY.  Nothing in the product imports this.
"""
import hashlib
import json
import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

ref_import.import_reference()

from compressed_tensors.entrypoints.convert import FP8BlockDequantizer, ModelOptNvfp4Converter  # noqa: E402
from compressed_tensors.quantization import QuantizationArgs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def synth_codes(rows, cols, salt):
    """float8_e4m3fn codes from an integer hash of (row, column): every byte value occurs, NaN codes included"""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    return ((r * 7919 + c * 104729 + salt * 13) * 2654435761 >> 13).remainder(256).to(torch.uint8).view(torch.float8_e4m3fn)


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


def canonical_sha(t):
    t = t.clone()
    t[torch.isnan(t)] = float("nan")
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def random_codes(gen, rows, cols):
    return torch.randint(0, 256, (rows, cols), generator=gen, dtype=torch.int64).to(torch.uint8).view(torch.float8_e4m3fn)


def random_scales(gen, shape, dtype):
    return (torch.rand(shape, generator=gen) * 0.02 + 1e-4).to(dtype)


def sweep_scales():
    """one scale per row of the all-codes case: negative, tiny (subnormal results in every output dtype), around one, large
    (float16 overflow to inf), and zero"""
    vals = [1.0, -1.0, 2.0 ** -120, -(2.0 ** -127), 2.0 ** -140, 2.0 ** -14, 2.0 ** -20, -(2.0 ** -24), 0.0, -0.0, 3.0 ** 0.5,
            1.0 / 3.0, 1e-3, 146.0, 147.0, 2.0 ** 8, -(2.0 ** 12), 65504.0 / 448.0, 1.5 * 2.0 ** 7, 2.0 ** 100]
    return torch.tensor(vals, dtype=F32)[:, None]


# name, [(module, rows, cols)], block, scale dtype, output dtype, scale layout ("sweep": the all-codes cases, stored whole)
CASES = [
    ("sq256_b128_f32_bf16", [("model.layers.0.mlp.down_proj", 256, 256)], (128, 128), F32, BF16, "full"),
    ("r200x300_b128_f32_bf16", [("model.layers.0.self_attn.q_proj", 200, 300)], (128, 128), F32, BF16, "full"),
    ("r200x300_b64x128_bf16_f16", [("model.layers.0.self_attn.k_proj", 200, 300)], (64, 128), BF16, F16, "full"),
    ("r200x300_b128x64_f32_f32", [("model.layers.0.self_attn.v_proj", 200, 300)], (128, 64), F32, F32, "full"),
    ("r200x300_b96x80_f32_bf16", [("model.layers.0.self_attn.o_proj", 200, 300)], (96, 80), F32, BF16, "full"),
    ("sq256_b1x128_bf16_bf16", [("model.layers.1.mlp.up_proj", 256, 256)], (1, 128), BF16, BF16, "full"),
    ("sq256_b128_bcast11_f32_f16", [("model.layers.1.mlp.gate_proj", 256, 256)], (128, 128), F32, F16, "1x1"),
    ("r200x300_b64_bcast_row_f32_bf16", [("model.layers.1.self_attn.q_proj", 200, 300)], (64, 64), F32, BF16, "1xN"),
    ("r200x300_b64_bcast_col_bf16_f32", [("model.layers.1.self_attn.k_proj", 200, 300)], (64, 64), BF16, F32, "Nx1"),
    ("mixed_b128_f32_bf16", [("model.layers.2.mlp.down_proj", 384, 512), ("model.layers.2.self_attn.q_proj", 200, 300),
                             ("model.layers.2.self_attn.kv_b_proj", 130, 144)], (128, 128), F32, BF16, "full"),
    ("allcodes_bf16", [("model.layers.3.mlp.down_proj", 20, 256)], (1, 256), F32, BF16, "sweep"),
    ("allcodes_f16", [("model.layers.3.mlp.down_proj", 20, 256)], (1, 256), F32, F16, "sweep"),
    ("allcodes_f32", [("model.layers.3.mlp.down_proj", 20, 256)], (1, 256), F32, F32, "sweep"),
    ("allcodes_general_f16", [("model.layers.3.mlp.up_proj", 20, 256)], (1, 8), F32, F16, "sweep"),
    ("kv_a_576x7168_b128_f32_bf16", [("model.layers.0.self_attn.kv_a_proj_with_mqa", 576, 7168)], (128, 128), F32, BF16, "full"),
    ("o_7168x2048_b128_bf16_bf16", [("model.layers.0.mlp.experts.0.down_proj", 7168, 2048)], (128, 128), BF16, BF16, "full"),
    ("kv_a_576x7168_b128_f32_f16", [("model.layers.0.self_attn.kv_a_proj_with_mqa", 576, 7168)], (128, 128), F32, F16, "full"),
]

TARGETS = ["re:.*proj(_with_mqa)?$"]
IGNORE = ["re:lm_head.*"]

# name, ignore, targets, kv_cache_scheme kwargs (None: no kv_cache_scheme)
MO_CONFIGS = [
    ("plain", ["lm_head"], ["Linear"], None),
    ("kv_fp8", ["lm_head", "re:.*mlp.gate$"], ["re:.*proj$"], {"num_bits": 8, "type": "float", "strategy": "tensor", "dynamic": False,
                                                           "symmetric": True}),
    ("kv_fp8_f32_scale", [], ["re:.*proj$"], {"num_bits": 8, "type": "float", "strategy": "tensor", "dynamic": False, "symmetric": True,
                                              "scale_dtype": "float32"}),
]


def kv_args(kw):
    if kw is None:
        return None
    kw = dict(kw)
    if "scale_dtype" in kw:
        kw["scale_dtype"] = getattr(torch, kw["scale_dtype"])
    return QuantizationArgs(**kw)


def fp8_cases(gen, blob, manifest):
    for ci, (name, modules, block, sdt, odt, layout) in enumerate(CASES):
        tensors, recipes = {}, {}
        for mi, (m, rows, cols) in enumerate(modules):
            nrb, ncb = -(-rows // block[0]), -(-cols // block[1])
            if layout == "sweep":
                tensors[f"{m}.weight"] = torch.arange(256, dtype=torch.int64).repeat(rows, cols // 256).to(torch.uint8).view(torch.float8_e4m3fn)
                tensors[f"{m}.weight_scale_inv"] = sweep_scales().expand(rows, ncb).contiguous().to(sdt)
            else:
                salt = 16 * ci + mi
                scale_shape = {"full": (nrb, ncb), "1x1": (1, 1), "1xN": (1, ncb), "Nx1": (nrb, 1)}[layout]
                tensors[f"{m}.weight"] = synth_codes(rows, cols, salt)
                tensors[f"{m}.weight_scale_inv"] = synth_scales(*scale_shape, salt, sdt)
                recipes[m] = {"name": m, "rows": rows, "cols": cols, "salt": salt, "scale_shape": list(scale_shape),
                              "scale_dtype": str(sdt).split(".")[-1]}
        if name == "sq256_b128_f32_bf16":  # what passes through: an ignored module with its scale, a norm, an embedding
            tensors["lm_head.weight"] = random_codes(gen, 16, 256)
            tensors["lm_head.weight_scale_inv"] = random_scales(gen, (1, 2), F32)
            tensors["model.norm.weight"] = torch.randn(256, generator=gen).to(BF16)
            tensors["model.embed_tokens.weight"] = torch.randn(16, 256, generator=gen).to(BF16)
        conv = FP8BlockDequantizer(ignore=IGNORE, targets=TARGETS, weight_block_size=block, dtype=odt)
        conv.validate(tensors)
        out = conv.process({k: v for k, v in tensors.items()})
        for m, rec in recipes.items():
            rec["sha256"] = canonical_sha(out[f"{m}.weight"])
            rec["nan"] = int(torch.isnan(out[f"{m}.weight"].float()).sum())
        synth = {f"{m}.{p}" for m in recipes for p in ("weight", "weight_scale_inv")}
        for k, v in tensors.items():
            if k not in synth:
                blob[f"{name}.in.{k}"] = v.contiguous()
        for m, _, _ in modules:  # the reference's output of every stored module (the synthesised ones: its sha256)
            if m not in recipes:
                blob[f"{name}.out.{m}.weight"] = out[f"{m}.weight"].contiguous().clone()
        manifest["cases"].append({"name": name, "block": list(block), "dtype": str(odt).split(".")[-1], "targets": TARGETS,
                                  "ignore": IGNORE, "in_order": list(tensors.keys()), "order": list(out.keys()),
                                  "synth": list(recipes.values())})


def modelopt_cases(gen, blob, manifest):
    for name, ignore, targets, kw in MO_CONFIGS:
        tensors = {}
        for proj in ("q_proj", "k_proj", "v_proj", "o_proj"):
            m = f"model.layers.0.self_attn.{proj}"
            tensors[f"{m}.weight"] = torch.randint(0, 256, (64, 32), generator=gen, dtype=torch.int64).to(torch.uint8)
            tensors[f"{m}.weight_scale"] = (torch.rand(64, 4, generator=gen) * 100).to(torch.float8_e4m3fn)
            tensors[f"{m}.weight_scale_2"] = torch.rand((), generator=gen) * 1e-3 + 1e-5
            tensors[f"{m}.input_scale"] = torch.rand((), generator=gen) * 0.1 + 1e-3
            if kw is not None and proj in ("k_proj", "v_proj"):
                tensors[f"{m}.{proj[0]}_scale"] = torch.rand((), generator=gen) + 0.5
        tensors["model.layers.0.mlp.gate.weight"] = torch.randn(8, 64, generator=gen).to(BF16)
        tensors["lm_head.weight"] = torch.randn(16, 64, generator=gen).to(BF16)
        tensors["model.norm.weight"] = torch.randn(64, generator=gen).to(BF16)
        conv = ModelOptNvfp4Converter(ignore=ignore, targets=targets, kv_cache_scheme=kv_args(kw))
        conv.validate(tensors)
        out = conv.process(dict(tensors))
        for k, v in tensors.items():
            blob[f"mo.{name}.in.{k}"] = v.contiguous()
        for k, v in out.items():
            blob[f"mo.{name}.out.{k}"] = v.contiguous().clone()
        manifest["modelopt"].append({"name": name, "ignore": ignore, "targets": targets, "kv_cache_scheme": kw,
                                  "in_order": list(tensors.keys()), "order": list(out.keys())})
        manifest["modelopt_configs"][name] = json.loads(json.dumps(conv.create_config().model_dump(), default=str))


def main():
    gen = torch.Generator().manual_seed(20251016)
    blob, manifest = {}, {"cases": [], "modelopt": [], "modelopt_configs": {}}
    fp8_cases(gen, blob, manifest)
    modelopt_cases(gen, blob, manifest)
    save_file(blob, os.path.join(OUT, "fp8block.safetensors"))
    with open(os.path.join(OUT, "fp8block_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(blob)} tensors, {os.path.getsize(os.path.join(OUT, 'fp8block.safetensors'))} bytes")


if __name__ == "__main__":
    main()
