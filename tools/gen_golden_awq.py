"""Generate the AutoAWQ converter's golden vectors by running the UPSTREAM REFERENCE's AutoAWQConverter (needs the reference sources; see oracle/ref_import.py).

Usage (from the repo root, where the reference sources exist):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_awq.py

Writes tests/golden/awq.safetensors and tests/golden/awq_manifest.json.  Every case is one shard: its AWQ input tensors under
`<case>.in.`, the reference's `process` output under `<case>.out.`; the manifest holds each case's AutoAWQ config and targets,
and the `create_config().model_dump()` dicts of three configs.  Seeded: two runs write byte-identical files.

TEST INFRASTRUCTURE ONLY.  Nothing in the product imports this.
"""
import json
import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

ref_import.import_reference()

from compressed_tensors.entrypoints.convert import AutoAWQConverter  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

# name, AutoAWQ config, targets, scale dtype, [(module, K, N)]
CASES = [
    ("g128_zp_f16", {"group_size": 128, "zero_point": True, "modules_to_not_convert": ["visual"]}, ["Linear"], torch.float16,
     [("model.layers.0.self_attn.q_proj", 512, 256), ("model.layers.0.mlp.down_proj", 256, 128)]),
    ("g64_sym_bf16", {"group_size": 64, "zero_point": False}, ["Linear"], torch.bfloat16,
     [("model.layers.0.self_attn.o_proj", 256, 512), ("model.layers.0.mlp.up_proj", 128, 64)]),
    ("g32_zp_bf16", {"group_size": 32, "zero_point": True}, ["re:.*proj$"], torch.bfloat16,
     [("model.layers.1.mlp.gate_proj", 256, 64), ("model.layers.1.self_attn.k_proj", 96, 264)]),
    ("g1_zp_f16", {"group_size": 384, "zero_point": True}, ["Linear"], torch.float16,
     [("model.layers.2.self_attn.v_proj", 384, 128)]),
    ("k200_g40_zp_f16", {"group_size": 40, "zero_point": True}, ["Linear"], torch.float16,
     [("model.layers.3.mlp.down_proj", 200, 96), ("model.layers.3.mlp.up_proj", 200, 40)]),
    ("k200_g40_sym_bf16", {"group_size": 40, "zero_point": False}, ["Linear"], torch.bfloat16,
     [("model.layers.4.mlp.down_proj", 200, 8), ("model.layers.4.self_attn.q_proj", 16, 200)]),
]

CONFIGS = [
    ("g64_zp_vision", {"bits": 4, "group_size": 64, "zero_point": True, "version": "gemm", "modules_to_not_convert": ["vision_tower"]},
     ["Linear"]),
    ("g128_sym", {"bits": 4, "group_size": 128, "zero_point": False, "version": "gemm"}, ["Linear"]),
    ("g32_zp_targets", {"group_size": 32, "zero_point": True, "modules_to_not_convert": ["visual", "mlp.gate"]}, ["re:.*proj$"]),
]


def words(gen, *shape):
    """random int32 words, sign bit included"""
    return torch.randint(0, 1 << 32, shape, generator=gen, dtype=torch.int64).to(torch.int32)


def main():
    gen = torch.Generator().manual_seed(20251015)
    blob, manifest = {}, {"cases": [], "configs": {}}
    for name, cfg, targets, sdt, modules in CASES:
        gs = cfg["group_size"]
        tensors = {}
        for m, K, N in modules:
            G = -(-K // gs)
            tensors[f"{m}.qweight"] = words(gen, K, N // 8)
            tensors[f"{m}.scales"] = (torch.rand(G, N, generator=gen) * 0.02 + 1e-3).to(sdt)
            # zero_point=False checkpoints carry no qzeros
            if cfg["zero_point"]:
                tensors[f"{m}.qzeros"] = words(gen, G, N // 8)
        if name == "g128_zp_f16":  # what passes through: an ignored module, a modules_to_not_convert module, a norm
            tensors["lm_head.weight"] = torch.randn(64, 256, generator=gen).to(sdt)
            tensors["model.visual.proj.weight"] = torch.randn(32, 64, generator=gen).to(sdt)
            tensors["model.visual.proj.bias"] = torch.randn(32, generator=gen).to(sdt)
            tensors["model.norm.weight"] = torch.randn(256, generator=gen).to(sdt)
        conv = AutoAWQConverter.from_autoawq_config(cfg, targets=targets)
        conv.validate(tensors)
        out = conv.process({k: v.clone() for k, v in tensors.items()})
        for k, v in tensors.items():
            blob[f"{name}.in.{k}"] = v.contiguous()
        for k, v in out.items():
            blob[f"{name}.out.{k}"] = v.contiguous()
        manifest["cases"].append({"name": name, "autoawq_config": cfg, "targets": targets})
    for name, cfg, targets in CONFIGS:
        manifest["configs"][name] = {"autoawq_config": cfg, "targets": targets,
                                     "model_dump": json.loads(json.dumps(AutoAWQConverter.from_autoawq_config(cfg, targets=targets)
                                                                         .create_config().model_dump(), default=str))}
    save_file(blob, os.path.join(OUT, "awq.safetensors"))
    with open(os.path.join(OUT, "awq_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(blob)} tensors, {os.path.getsize(os.path.join(OUT, 'awq.safetensors'))} bytes")


if __name__ == "__main__":
    main()
