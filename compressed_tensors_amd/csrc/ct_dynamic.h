// ct_dynamic.h — the device and host helpers of the dynamic activation QDQ (csrc/ct_dynamic.hip), shared with the fused
// rotation + dynamic QDQ launch of csrc/ct_rotated.hip: the parameter block, the min / max accumulation, calculate_qparams of a
// segment, fake_quantize of a unit, and a unit as its raw words.
#pragma once
#include "ct_quant_core.h"
#include "ct_quant_lean.h"
#include "ct_minmax.h"

namespace ct {

struct DynParams {
    const void* x;
    void* out;        // nullable: scales only (compute_dynamic_scales_and_zp)
    void* scale_out;  // nullable
    void* zp_out;     // nullable
    int64_t segs, seg_len;
    int kind, bits, symmetric, fkind, zdt, vec;
    float qmin, qmax;
    const float* gscale;  // nullable
};

__device__ __forceinline__ MinMax mm_neutral() {
    MinMax m;
    m.mn = __builtin_inff();
    m.mx = -__builtin_inff();
    m.nan = 0;
    return m;
}

__device__ __forceinline__ MinMax mm_acc(MinMax m, const float (&v)[8], int n) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k < n) {
            m.nan |= (v[k] != v[k]);
            m.mn = __builtin_fminf(m.mn, v[k]);
            m.mx = __builtin_fmaxf(m.mx, v[k]);
        }
    }
    return m;
}

template <int XDT>
__device__ __forceinline__ void dyn_load(const DynParams& p, int64_t i0, int n, float (&v)[8]) {
    if (p.vec && n == 8) {
        load8<XDT>(p.x, i0, v);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = k < n ? load_as_f<XDT>(p.x, i0 + k) : 0.0f;
    }
}

template <int XDT>
__device__ __forceinline__ void dyn_store(const DynParams& p, int64_t i0, int n, const float (&v)[8]) {
    if (p.vec && n == 8) {
        store8<XDT>(p.out, i0, v);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < n) store1<XDT>(p.out, i0 + k, v[k]);
    }
}

// calculate_qparams of one segment: the scale (a value of the scale dtype) and the zero point (an integer, 0 for the FLOAT kinds)
template <int XDT>
__device__ __forceinline__ void dyn_qparams(const DynParams& p, MinMax m, float& s, float& z) {
    if (p.kind == QP_INT) {
        compute_qparams<XDT>(m, p.bits, p.symmetric, s, z);
        z = (float)(int)z;  // the int8 round trip of the stored zero point: rint may leave -0.0, zp.to(x.dtype) is +0.0
    } else if (m.nan && (p.kind == QP_MXFP4 || p.kind == QP_MXFP8)) {
        // The reference's NaN amax reaches round_to_power_2 (mxfp_utils.py:62-110) as the all-ones pattern its CPU min / max produce;
        // adding the rounding bit carries out of it, the masked result is +0, log2 gives -inf and the E8M0 code clamps to 0: 2^-127.
        // (compute_qparams_float keeps the weight path's canonical-NaN result, +inf.)
        s = round_to<XDT>(0x1p-127f);
        if (s == 0.0f) s = 1.0f;  // fp16: 2^-127 underflows, eps(uint8) = 1
        z = 0.0f;
    } else {
        s = compute_qparams_float<XDT>(m, p.kind, p.gscale ? p.gscale[0] : 1.0f);  // 1.0f: global * local is then exact
        z = 0.0f;
    }
}

template <int XDT, bool GS>
__device__ __forceinline__ void dyn_write_qparams(const DynParams& p, int64_t idx, float s, float z) {
    if (p.scale_out) {
        if (GS) static_cast<float*>(p.scale_out)[idx] = s;
        else store1<XDT>(p.scale_out, idx, s);
    }
    if (p.zp_out) {
        uint8_t b;
        if (p.zdt == CT_F8E4M3) b = (uint8_t)(f2_to_fp8x2(z, 0.0f) & 0xffu);
        else b = (uint8_t)(int8_t)(int)z;  // int8 (two's complement) or uint8 (always 0: the MX zero points)
        static_cast<uint8_t*>(p.zp_out)[idx] = b;
    }
}

// the reciprocal shortcut quant_units_kernel takes when x, the scale and T share one dtype (0: divide)
template <int XDT>
__device__ __forceinline__ float dyn_rcp(float s) {
    if constexpr (XDT == CT_BF16) return bf16_fast_rcp(s);
    else if constexpr (XDT == CT_F16) return f16_newton_rcp(s);
    else return f32_fast_rcp(s);
}

// fake_quantize of 8 values with the segment's (s, z): se is s / global_scale under GS, rs the reciprocal (unused under GS)
template <int XDT, bool GS>
__device__ __forceinline__ void dyn_qdq8(const DynParams& p, float (&v)[8], int n, float se, float z, float rs) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k < n) {
            if constexpr (GS) {
                const float t = quant_core<CT_F32>(v[k], se, true, z, p.qmin, p.qmax, 0.0f, p.fkind);
                float d = dequant_core<CT_F32>(t, true, z, se);
                // pinned: the fp16 store would otherwise fold the product into v_fma_mixlo_f16 d, s, +0, which loses a -0.0 (mul_round_to)
                if constexpr (XDT == CT_F16) asm("" : "+v"(d));
                v[k] = d;
            } else {
                const float t = quant_core<XDT>(v[k], se, true, z, p.qmin, p.qmax, rs, p.fkind);
                v[k] = dequant_core<XDT>(t, true, z, se);
            }
        }
    }
}

// a unit (8 elements) as its raw words: 4 for the 16-bit dtypes, 8 for float32 — half the registers of 8 floats for bf16 / fp16
template <int XDT>
struct RawUnit {
    static constexpr int W = XDT == CT_F32 ? 8 : 4;
    uint32_t w[W];
};

template <int XDT>
__device__ __forceinline__ void raw_load(const DynParams& p, int64_t i0, int n, RawUnit<XDT>& r) {
    if (p.vec && n == 8) {
        const u32x4* q = reinterpret_cast<const u32x4*>(static_cast<const uint8_t*>(p.x) + i0 * (XDT == CT_F32 ? 4 : 2));
#pragma unroll
        for (int h = 0; h < RawUnit<XDT>::W / 4; ++h) {
            const u32x4 a = q[h];
            r.w[4 * h] = a.x; r.w[4 * h + 1] = a.y; r.w[4 * h + 2] = a.z; r.w[4 * h + 3] = a.w;
        }
    } else if constexpr (XDT == CT_F32) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r.w[k] = k < n ? static_cast<const uint32_t*>(p.x)[i0 + k] : 0u;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t lo = 2 * j < n ? static_cast<const uint16_t*>(p.x)[i0 + 2 * j] : 0u;
            const uint32_t hi = 2 * j + 1 < n ? static_cast<const uint16_t*>(p.x)[i0 + 2 * j + 1] : 0u;
            r.w[j] = lo | (hi << 16);
        }
    }
}

template <int XDT>
__device__ __forceinline__ void raw_unpack(const RawUnit<XDT>& r, float (&v)[8]) {
    if constexpr (XDT == CT_F32) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = bits_f(r.w[k]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) unpack2<XDT>(r.w[j], v[2 * j], v[2 * j + 1]);
    }
}

// one workgroup per segment: the staged form's limits
constexpr int kSegMaxThreads = 512;
constexpr int kSegUnits = 8;  // units (8 elements) a thread holds in registers: 512 x 8 x 8 = 32768 elements

static int fill_dyn(DynParams& p, const void* x, int xdt, int64_t segs, int64_t seg_len, int kind, int bits, int symmetric,
                    const float* gscale, void* out, void* scale_out, void* zp_out, int zdt) {
    CT_REQUIRE(is_float_dt(xdt), "activation dtype code %d is not a float type", xdt);
    CT_REQUIRE(segs >= 0 && seg_len >= 1, "bad segment shape (%lld, %lld)", (long long)segs, (long long)seg_len);
    CT_REQUIRE(kind >= QP_INT && kind <= QP_MXFP8, "dynamic qparams kind must be 0 (int), 1 (fp8), 2 (nvfp4), 3 (mxfp4) or 4 (mxfp8), got %d", kind);
    CT_REQUIRE(kind != QP_INT || (bits >= 1 && bits <= 8), "num_bits must be in [1, 8], got %d", bits);
    CT_REQUIRE(kind == QP_INT || symmetric, "the FLOAT kinds are symmetric");
    CT_REQUIRE(gscale == nullptr || kind == QP_NVFP4, "a global scale is only taken by the nvfp4 kind");
    CT_REQUIRE(zp_out == nullptr || (kind == QP_INT ? zdt == CT_I8 : (zdt == CT_F8E4M3 || zdt == CT_U8 || zdt == CT_I8)),
               "zero-point dtype code %d unsupported for kind %d", zdt, kind);
    p.x = x; p.out = out; p.scale_out = scale_out; p.zp_out = zp_out;
    p.segs = segs; p.seg_len = seg_len;
    p.kind = kind; p.bits = bits; p.symmetric = symmetric; p.zdt = zdt; p.gscale = gscale;
    if (kind == QP_INT) {
        p.fkind = 0;
        p.qmax = (float)((1 << bits) / 2 - 1);
        p.qmin = -(float)((1 << bits) / 2);
    } else if (kind == QP_FP8 || kind == QP_MXFP8) {
        p.fkind = 1; p.qmin = -448.0f; p.qmax = 448.0f;
    } else {
        p.fkind = 2; p.qmin = -6.0f; p.qmax = 6.0f;
    }
    p.vec = aligned16(x) && (out == nullptr || aligned16(out));
    return CT_OK;
}

#define CT_DYN_DISPATCH(xdt, gs, ...)                                                                   \
    do {                                                                                                \
        if (xdt == CT_BF16) { constexpr int X = CT_BF16; if (gs) { constexpr bool G = true; __VA_ARGS__; } else { constexpr bool G = false; __VA_ARGS__; } } \
        else if (xdt == CT_F16) { constexpr int X = CT_F16; if (gs) { constexpr bool G = true; __VA_ARGS__; } else { constexpr bool G = false; __VA_ARGS__; } } \
        else { constexpr int X = CT_F32; if (gs) { constexpr bool G = true; __VA_ARGS__; } else { constexpr bool G = false; __VA_ARGS__; } } \
    } while (0)

}  // namespace ct
