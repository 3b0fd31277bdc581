"""developer script: the fused dynamic activation QDQ (csrc/ct_dynamic.hip) against the other ways to compute it.

    python tools/dynamic_bench.py [--iters 20] [--out DIR] [--presets fp8_token,...] [--tokens 16,2048,8192] [--hidden 4096,14336,28672]

Cases: each activation preset (tests/_dynamic_cases.py: FP8_DYNAMIC / W4AFP8 token, INT8_W8A8 token, FP8_BLOCK group 128, NVFP4
tensor_group 16 with a global scale, MXFP4 / MXFP8 group 32) x bfloat16 activations (1, T, H).  Four timings per case:
  * fused:    quantization.dynamic.dynamic_fake_quantize (one launch);
  * compose:  today's kernels, minmax_qparams(_float) followed by fake_quantize_tensor (two launches; the MX compositions have
              no float fake_quantize kernel for E8M0 scales and take FLOAT 8 / 4 with the same scale: same traffic);
  * eager:    the reference's compute_dynamic_scales_and_zp + fake_quantize on the GPU (oracle/ref_import.py), when staged;
  * patched:  the reference's forward_quantize on a module under install(patch_forward=True).
Each is timed with device events over --iters calls, warm (one input, L2 / MALL resident where it fits) and HBM-cold (inputs
rotated over >= 2 x 256 MiB).  Rates are over the algorithmic bytes, 2 * numel * 2 (bf16 in, bf16 out), as a fraction of
8 TB/s.  One JSON line per case; with --out also DIR/dynamic_bench.jsonl.  --kernel-only runs the fused path alone (for a
`rocprofv3 --kernel-trace --stats` run of its own, which confirms the launch counts)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402

import _dynamic_cases as C  # noqa: E402
from compressed_tensors_amd import codec  # noqa: E402
from compressed_tensors_amd.quantization import QuantizationArgs  # noqa: E402
from compressed_tensors_amd.quantization.dynamic import dynamic_fake_quantize  # noqa: E402

HBM_PEAK = 8.0e12
COLD_BYTES = 2 * 256 << 20
PRESETS = ["fp8_token", "int8_token", "fp8_group128", "nvfp4", "mxfp4", "mxfp8"]


def compose(x, preset, gs):
    """minmax_qparams(_float) + fake_quantize_tensor on the (T, H) view"""
    a = C.PRESETS[preset]
    x2 = x.reshape(-1, x.shape[-1])
    if preset == "int8_token":
        s, z = codec.minmax_qparams(x2, num_bits=8, symmetric=True)
        return codec.fake_quantize_tensor(x2, s, z, num_bits=8, strategy="channel")
    if preset == "fp8_token":
        s = codec.minmax_qparams_float(x2, kind="fp8")
        return codec.fake_quantize_tensor(x2, s, None, num_bits=8, strategy="channel", qtype="float")
    if preset == "fp8_group128":
        s = codec.minmax_qparams_float(x2, kind="fp8", group_size=128)
        return codec.fake_quantize_tensor(x2, s, None, num_bits=8, strategy="group", group_size=128, qtype="float")
    if preset == "nvfp4":
        s = codec.minmax_qparams_float(x2, kind="nvfp4", group_size=16, global_scale=gs)
        return codec.fake_quantize_tensor(x2, s, None, num_bits=4, strategy="tensor_group", group_size=16, qtype="float", global_scale=gs)
    s = codec.minmax_qparams_float(x2, kind=preset, group_size=32)
    return codec.fake_quantize_tensor(x2, s, None, num_bits=a["num_bits"], strategy="group", group_size=32, qtype="float")


def timed(fn, inputs, iters):
    """median-free mean ms per call over `iters` calls cycling through `inputs` (device events, one region)"""
    fn(inputs[0])
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(inputs[i % len(inputs)])
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--presets", default=",".join(PRESETS))
    ap.add_argument("--tokens", default="16,2048,8192")
    ap.add_argument("--hidden", default="4096,14336,28672")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gs = torch.tensor([37.5], device=dev)

    up = None
    if not a.kernel_only and not a.no_eager:
        import ref_import

        if ref_import.available():
            ref_import.import_reference()
            import compressed_tensors.quantization.lifecycle.forward as up_forward
            import compressed_tensors.quantization.utils.helpers as up_helpers
            from compressed_tensors.quantization import QuantizationArgs as UpArgs

            import compressed_tensors_amd.install as ct_amd

            up = (up_forward, up_helpers, UpArgs, ct_amd)
    lines = []
    for preset in a.presets.split(","):
        args = QuantizationArgs(**C.PRESETS[preset])
        g = gs if preset == "nvfp4" else None
        for T in (int(t) for t in a.tokens.split(",")):
            for H in (int(h) for h in a.hidden.split(",")):
                nbytes = T * H * 2
                n_cold = max(2, -(-COLD_BYTES // nbytes))
                cold = [torch.randn(1, T, H, device=dev, dtype=torch.bfloat16) for _ in range(n_cold)]
                warm = cold[:1]
                algo = 2 * T * H * 2
                row = {"preset": preset, "T": T, "H": H, "MB": round(nbytes / 1e6, 2)}

                def rec(name, fn):
                    for mode, inputs in (("warm", warm), ("cold", cold)):
                        ms = timed(fn, inputs, a.iters)
                        row[f"{name}_{mode}_us"] = round(ms * 1e3, 2)
                        row[f"{name}_{mode}_GBs"] = round(algo / ms / 1e6, 1)
                        row[f"{name}_{mode}_peak"] = round(algo / ms / 1e-3 / HBM_PEAK, 3)

                rec("fused", lambda x: dynamic_fake_quantize(x, args, g))
                if not a.kernel_only:
                    rec("compose", lambda x: compose(x, preset, g))
                    if up is not None:
                        up_forward, up_helpers, UpArgs, ct_amd = up
                        uargs = UpArgs(**C.PRESETS[preset])
                        orig_cd, orig_fq = up_helpers.compute_dynamic_scales_and_zp, up_forward.fake_quantize

                        def eager(x):
                            s, z = orig_cd(value=x, args=uargs, module=None, global_scale=g)
                            return orig_fq(x=x, scale=s, zero_point=z, args=uargs, global_scale=g)

                        rec("eager", eager)
                        mod = torch.nn.Linear(1, 1, device=dev)
                        mod.quantization_status = up_forward.QuantizationStatus.FROZEN
                        if g is not None:
                            mod.input_global_scale = torch.nn.Parameter(g.clone(), requires_grad=False)
                        ct_amd.install(patch_forward=True)
                        try:
                            fq = up_forward.forward_quantize
                            rec("patched", lambda x: fq(mod, x, "input", uargs))
                        finally:
                            ct_amd.uninstall()
                del cold, warm
                torch.cuda.empty_cache()
                print(json.dumps(row), flush=True)
                lines.append(row)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "dynamic_bench.jsonl"), "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
