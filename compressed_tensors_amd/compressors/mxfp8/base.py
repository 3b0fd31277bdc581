"""mxfp8-quantized codec (reference compressors/mxfp8/base.py:29-118): float8_e4m3fn weights in groups of 32 under
E8M0 (power-of-two) scales stored as uint8 exponents.  The weight path is the FLOAT 8-bit quantize / dequantize
kernels of the naive-quantized codec; only the (1/32-size) scale tensor is converted around them."""
import torch

from ... import codec
from ...config import CompressionFormat
from ...quantization.quant_args import enum_value
from ..base import COMPRESSIBLE_MODULE_TYPES, BaseCompressor, run_rtn_windows
from ..naive_quantized import NaiveQuantizationCompressor

__all__ = ["MXFP8QuantizationCompressor"]

_naive_compress = NaiveQuantizationCompressor.compress.__func__
_naive_decompress = NaiveQuantizationCompressor.decompress.__func__


@BaseCompressor.register(name=CompressionFormat.mxfp8_quantized.value)
class MXFP8QuantizationCompressor(NaiveQuantizationCompressor):
    @classmethod
    def can_compress(cls, module_type: type, scheme) -> bool:
        """mxfp8/base.py:103-118: FLOAT, 8 bits, groups of 32, uint8 (E8M0) scales"""
        w = getattr(scheme, "weights", None)
        if module_type not in COMPRESSIBLE_MODULE_TYPES or w is None:
            return False
        signature = (enum_value(w.type), int(w.num_bits), getattr(w, "group_size", None), getattr(w, "scale_dtype", None))
        return signature == ("float", 8, 32, torch.uint8)

    @classmethod
    def compress(cls, state_dict: dict, scheme) -> dict:
        """mxfp8/base.py:47-72: quantize against the float scale, then keep only the scale's exponent"""
        out = _naive_compress(cls, state_dict, scheme)
        out["weight_scale"] = cls._compress_scale(out["weight_scale"], scheme.weights)
        return out

    @classmethod
    def decompress(cls, state_dict: dict, scheme) -> dict:
        """mxfp8/base.py:74-101: the exponent comes back as a bfloat16 power of two, so the weight is bfloat16 too"""
        widened = dict(state_dict, weight_scale=cls._decompress_scale(state_dict["weight_scale"]))
        return _naive_decompress(cls, widened, scheme)

    @classmethod
    def compress_rtn(cls, weight, scheme) -> dict:
        """Round-to-nearest compression straight from the dense weight: what `compress` returns for calculate_qparams of the weight's group
        min / max — the codes and the E8M0 exponents from ONE pass over the weight (codec.rtn_quantize_group8, mx) where the kernel's plan takes
        it (`group_one_pass`) and the measurement says so; the observer + quantize + compress_mx_scale composition otherwise."""
        from ...quantization.utils import group_one_pass
        from ..naive_quantized.base import RTN_GROUP8_MEASURED_FASTER

        weights = scheme.weights
        base = MXFP8QuantizationCompressor
        if (RTN_GROUP8_MEASURED_FASTER["mxfp8"] and cls.compress.__func__ is base.compress.__func__ and group_one_pass(weight, weights) == "mxfp8"
                and (getattr(weights, "scale_dtype", None) or torch.uint8) is torch.uint8):
            q, _, _, code = codec.rtn_quantize_group8(weight, group_size=32, qtype="float", mx=True)
            return {"weight_scale": code, "weight": q}  # the composition's entry order
        return super().compress_rtn(weight, scheme)

    # the window hook's gate (see NVFP4PackedCompressor): True only where the table was below the per-module loop's minimum on both trees in both runs
    # (profiles/rtn_bench.jsonl, scheme mxfp8): medians 4.66 / 4.72 ms (at most 4.79) against a per-module minimum of 5.06 / 5.07 on the
    # 8B-shaped tree, 1.99 / 2.00 (at most 2.12) against 3.23 / 3.22 on the TinyLlama-shaped one — the per-module loop already on the one-pass kernel
    RTN_TABLE_MEASURED_FASTER = True

    @classmethod
    def compress_rtn_modules(cls, modules) -> None:
        """the window hook (`run_rtn_windows`): the modules with a 16-bit weight on a GPU that the one-pass kernel's plan takes leave in ONE table
        launch per (device, dtype) (codec.launch_rtn_group8_words, kind MXFP8); the others go through `compress_rtn_module`."""
        from ...quantization.utils import group_one_pass

        def item(m, w, table):
            wa = m.quantization_scheme.weights
            if group_one_pass(w, wa) != "mxfp8" or (getattr(wa, "scale_dtype", None) or torch.uint8) is not torch.uint8:
                return None
            got = codec.rtn_group8_table_item(w.data, 32, "float", mx=True, with_scale=False)
            if got is None:
                return None
            return (w.device, w.dtype), got[-1], got

        run_rtn_windows(cls, modules, item, lambda key, flat, jobs: codec.launch_rtn_group8_words(flat, len(jobs), key[1], key[0], 4),
                        lambda w, o: {"weight_scale": o[3], "weight": o[0]})

    # ------------------------------------------------------------------ module loops (round 6)
    # ModelCompressor's per-module loop in the C++ extension (csrc/host/ct_hostpath.cpp mx8_plan_compress / mx8_plan_decompress / mx8_finish): the weights of a
    # window of modules ride ONE launch of the 8-bit tables (float8 codes, groups of 32), their scale tensors ONE launch of ct_mx_scale_batch; whatever the C++
    # loop does not take goes through compress_module / decompress_module as before
    @classmethod
    def _native(cls, modules, direction: str):
        from ... import _lib
        from ...quantization.quant_args import QuantizationStatus
        from ..base import run_planned, zp_drop_mask

        modules = list(modules)
        hp = _lib.hostpath()
        base = MXFP8QuantizationCompressor
        if (hp is None or not hasattr(hp, "mx8_plan_compress") or torch.nn.modules.module._global_parameter_registration_hooks
                or cls.compress.__func__ is not base.compress.__func__ or cls.decompress.__func__ is not base.decompress.__func__):
            return modules

        def info(scheme) -> int:
            if not cls.can_compress(torch.nn.Linear, scheme):
                return 0
            return 1 | (zp_drop_mask(scheme) << 1)

        compress = direction == "compress"
        codes = {1: torch.float16, 2: torch.bfloat16}
        status = QuantizationStatus.COMPRESSED if compress else QuantizationStatus.DECOMPRESSED

        def launch(device, code, words, n, scale_words, scale_n):
            dtype = codes[code & 15]
            if compress:
                codec.launch_q8_words(words, n, "compress", dtype, device, (code >> 4) & 15, 8)
                codec.launch_mx_scale_words(scale_words, scale_n, "compress", device, dtype)
            else:  # the scales first: the weights' table reads their bfloat16 form
                codec.launch_mx_scale_words(scale_words, scale_n, "decompress", device)
                codec.launch_q8_words(words, n, "decompress", dtype, device, (code >> 4) & 15, 8)

        return run_planned(modules, (lambda ms: hp.mx8_plan_compress(ms, info)) if compress else hp.mx8_plan_decompress, launch,
                           lambda jobs: hp.mx8_finish(jobs, status))

    @classmethod
    def compress_modules(cls, modules) -> None:
        super().compress_modules(cls._native(modules, "compress"))

    @classmethod
    def decompress_modules(cls, modules) -> None:
        super().decompress_modules(cls._native(modules, "decompress"))

    @classmethod
    def decompress_many(cls, state_dicts, scheme) -> list:
        """`decompress` for several local-name state dicts (the model-free converter: one safetensors shard): the scale tensors of the usual layout through ONE
        launch of `ct_mx_scale_batch`, the weights through ONE of the 8-bit tables; the rest one by one"""
        base = MXFP8QuantizationCompressor
        if cls.compress.__func__ is not base.compress.__func__ or cls.decompress.__func__ is not base.decompress.__func__:
            return [cls.decompress(sd, scheme) for sd in state_dicts]
        out, words, swords, where = [None] * len(state_dicts), [], [], []
        device = None
        for i, sd in enumerate(state_dicts):
            q, sc = sd.get("weight"), sd.get("weight_scale")
            ok = (q is not None and sc is not None and sd.get("weight_zero_point") is None and sd.get("weight_g_idx") is None and q.is_cuda and q.dim() == 2
                  and q.dtype is torch.float8_e4m3fn and q.is_contiguous() and q.data_ptr() % 16 == 0 and sc.dtype is torch.uint8 and sc.device == q.device
                  and sc.is_contiguous() and sc.dim() == 2 and (device is None or q.device == device))
            if ok:
                rows, cols = int(q.shape[0]), int(q.shape[1])
                ok = rows > 0 and cols % 32 == 0 and tuple(sc.shape) == (rows, cols // 32)
            if not ok:
                out[i] = cls.decompress(sd, scheme)
                continue
            device = q.device
            scale = torch.empty(sc.shape, dtype=torch.bfloat16, device=device)  # decompress_mx_scale: bfloat16, and so is the weight (mxfp8/base.py:74-101)
            weight = torch.empty((rows, cols), dtype=torch.bfloat16, device=device)
            words += codec.item_row(q, scale, None, weight, rows, cols, 32)
            swords += codec.item_row(sc, dst=scale, rows=sc.numel(), cols=1)
            new = dict(sd, weight_scale=scale)
            del new["weight"]
            new["weight"] = weight  # the entries in the order `decompress` leaves them
            out[i] = new
            where.append(i)
        if where:
            codec.launch_mx_scale_words(torch.tensor(swords, dtype=torch.int64), len(where), "decompress", device)  # first: the weights' table reads the bfloat16 scales
            codec.launch_q8_words(torch.tensor(words, dtype=torch.int64), len(where), "decompress", torch.bfloat16, device, 1, 8)
        return out

    # the two hooks keep upstream's names: install() lets upstream's subclass call them
    @classmethod
    def _compress_scale(cls, scale: torch.Tensor, weights) -> torch.Tensor:
        return codec.compress_mx_scale(scale, getattr(weights, "scale_dtype", None) or torch.uint8)

    @classmethod
    def _decompress_scale(cls, scale: torch.Tensor) -> torch.Tensor:
        return codec.decompress_mx_scale(scale)
