// ct_dynamic.hip — dynamic activation QDQ: compute_dynamic_scales_and_zp followed by fake_quantize
// (quantization/utils/helpers.py:50-195, quantization/lifecycle/forward.py:148-181, forward_helpers.py:180-215) in one pass.
//
// A "segment" is the run of consecutive elements that shares one scale: a token row (token strategy, dims >= 2 of a 3-D+
// activation), a group (group / tensor_group), or the whole tensor (tensor strategy, and token on a 1-D / 2-D input, whose
// reduce-dims tuple is empty upstream).  The observer, calculate_qparams and the element arithmetic are the weight path's
// own device functions (ct_minmax.h: the min / max reduction, compute_qparams, compute_qparams_float; ct_quant_core.h:
// quant_core / dequant_core), so every step rounds exactly as the eager op sequence does:
//   INT / FP8 / MX:      T = S = X (scale in x's dtype), t = q(x / s + zp), out = rnd_X(rnd_X(t - zp) * s)
//   NVFP4 + global:      S = float32 (global_scale * scale promotes), T = float32, s_eff = s / global_scale, out = rnd_X(...)
// The zero point is added even when it is zero (it turns -0 into +0, as upstream's `scaled += zero_point` does).
//
// Kernels
//   dyn_group_kernel    segments of 8..512 elements, a power-of-two number of 8-element units: LPG lanes own a segment, min /
//                       max are finished with DPP inside the wave, the scale stays in registers.  One read, one write.
//   dyn_seg_kernel      one workgroup per segment (64..512 threads).  Rows of up to 512 x 8 units (32768 elements) are held in
//                       registers between the reduction and the QDQ; longer ones are read a second time (two-phase form).
//   dyn_partial_kernel  tensor strategy, launch 1: a min / max partial per workgroup into a CT_DYNAMIC_PARTS-entry workspace
//   dyn_flat_kernel     tensor strategy, launch 2: every workgroup folds the partials, computes the one scale, streams the QDQ
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

// ---- segments of LPG lanes (LPG = seg_len / 8, a power of two <= 64): U units per lane, kBlock apart ------------------------------
template <int XDT, bool GS, int U>
__global__ __launch_bounds__(kBlock) void dyn_group_kernel(DynParams p, int64_t units, int lpg) {
    const int64_t base = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
    float v[U][8];
    MinMax m[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int64_t u = base + (int64_t)i * kBlock;
        m[i] = mm_neutral();
        if (u < units) {
            load8<XDT>(p.x, u << 3, v[i]);
            m[i] = mm_acc(m[i], v[i], 8);
        }
    }
    // units is a multiple of lpg and kBlock of lpg: a segment never straddles a wave, and every lane of a live segment is live
#pragma unroll
    for (int i = 0; i < U; ++i) m[i] = group_reduce(m[i], lpg);
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int64_t u = base + (int64_t)i * kBlock;
        if (u >= units) continue;
        float s, z;
        dyn_qparams<XDT>(p, m[i], s, z);
        if ((threadIdx.x & (lpg - 1)) == 0) dyn_write_qparams<XDT, GS>(p, u / lpg, s, z);
        if (p.out) {
            const float se = GS ? s / p.gscale[0] : s;
            dyn_qdq8<XDT, GS>(p, v[i], 8, se, z, GS ? 0.0f : dyn_rcp<XDT>(s));
            store8<XDT>(p.out, u << 3, v[i]);
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

// ---- one workgroup per segment -----------------------------------------------------------------------------------------------
constexpr int kSegMaxThreads = 512;
constexpr int kSegUnits = 8;  // units (8 elements) a thread holds in registers: 512 x 8 x 8 = 32768 elements

template <int XDT, bool GS>
__global__ __launch_bounds__(kSegMaxThreads) void dyn_seg_kernel(DynParams p) {
    __shared__ MinMax red[kSegMaxThreads / 64];
    const int nt = blockDim.x, tid = threadIdx.x, nw = nt >> 6;
    const int64_t upr = (p.seg_len + 7) >> 3;
    const bool staged = upr <= (int64_t)nt * kSegUnits;
    for (int64_t seg = blockIdx.x; seg < p.segs; seg += gridDim.x) {
        const int64_t base = seg * p.seg_len;
        RawUnit<XDT> raw[kSegUnits];
        MinMax m = mm_neutral();
        if (staged) {
#pragma unroll
            for (int k = 0; k < kSegUnits; ++k) {
                const int64_t u = tid + (int64_t)k * nt;
                if (u < upr) {
                    const int64_t c0 = u << 3;
                    raw_load<XDT>(p, base + c0, (int)(p.seg_len - c0 < 8 ? p.seg_len - c0 : 8), raw[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < kSegUnits; ++k) {
                const int64_t u = tid + (int64_t)k * nt;
                if (u < upr) {
                    const int64_t c0 = u << 3;
                    float v[8];
                    raw_unpack<XDT>(raw[k], v);
                    m = mm_acc(m, v, (int)(p.seg_len - c0 < 8 ? p.seg_len - c0 : 8));
                }
            }
        } else {
            for (int64_t u = tid; u < upr; u += nt) {
                const int64_t c0 = u << 3;
                const int n = (int)(p.seg_len - c0 < 8 ? p.seg_len - c0 : 8);
                float w[8];
                dyn_load<XDT>(p, base + c0, n, w);
                m = mm_acc(m, w, n);
            }
        }
        m = group_reduce(m, 64);
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
        m = red[0];
        for (int w = 1; w < nw; ++w) m = mm_merge(m, red[w]);
        __syncthreads();  // red[] is rewritten by the next segment
        float s, z;
        dyn_qparams<XDT>(p, m, s, z);
        if (tid == 0) dyn_write_qparams<XDT, GS>(p, seg, s, z);
        if (!p.out) continue;
        const float se = GS ? s / p.gscale[0] : s;
        const float rs = GS ? 0.0f : dyn_rcp<XDT>(s);
        if (staged) {
#pragma unroll
            for (int k = 0; k < kSegUnits; ++k) {
                const int64_t u = tid + (int64_t)k * nt;
                if (u < upr) {
                    const int64_t c0 = u << 3;
                    const int n = (int)(p.seg_len - c0 < 8 ? p.seg_len - c0 : 8);
                    float v[8];
                    raw_unpack<XDT>(raw[k], v);
                    dyn_qdq8<XDT, GS>(p, v, n, se, z, rs);
                    dyn_store<XDT>(p, base + c0, n, v);
                }
            }
        } else {
            for (int64_t u = tid; u < upr; u += nt) {
                const int64_t c0 = u << 3;
                const int n = (int)(p.seg_len - c0 < 8 ? p.seg_len - c0 : 8);
                float w[8];
                dyn_load<XDT>(p, base + c0, n, w);
                dyn_qdq8<XDT, GS>(p, w, n, se, z, rs);
                dyn_store<XDT>(p, base + c0, n, w);
            }
        }
    }
}

// ---- tensor strategy: partials, then the QDQ ---------------------------------------------------------------------------------
__device__ __forceinline__ MinMax block_reduce(MinMax m, MinMax* red) {
    m = group_reduce(m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = red[0];
    for (int w = 1; w < kBlock / 64; ++w) m = mm_merge(m, red[w]);
    return m;
}

template <int XDT>
__global__ __launch_bounds__(kBlock) void dyn_partial_kernel(DynParams p, MinMax* __restrict__ parts) {
    __shared__ MinMax red[kBlock / 64];
    const int64_t numel = p.seg_len, units = (numel + 7) >> 3;
    MinMax m = mm_neutral();
    for (int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x; u < units; u += (int64_t)gridDim.x * kBlock) {
        const int64_t c0 = u << 3;
        const int n = (int)(numel - c0 < 8 ? numel - c0 : 8);
        float v[8];
        dyn_load<XDT>(p, c0, n, v);
        m = mm_acc(m, v, n);
    }
    m = block_reduce(m, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = m;
}

template <int XDT, bool GS>
__global__ __launch_bounds__(kBlock) void dyn_flat_kernel(DynParams p, const MinMax* __restrict__ parts, int nparts) {
    __shared__ MinMax red[kBlock / 64];
    MinMax m = mm_neutral();
    for (int i = threadIdx.x; i < nparts; i += kBlock) m = mm_merge(m, parts[i]);
    m = block_reduce(m, red);
    float s, z;
    dyn_qparams<XDT>(p, m, s, z);
    if (blockIdx.x == 0 && threadIdx.x == 0) dyn_write_qparams<XDT, GS>(p, 0, s, z);
    if (!p.out) return;
    const float se = GS ? s / p.gscale[0] : s;
    const float rs = GS ? 0.0f : dyn_rcp<XDT>(s);
    const int64_t numel = p.seg_len, units = (numel + 7) >> 3;
    for (int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x; u < units; u += (int64_t)gridDim.x * kBlock) {
        const int64_t c0 = u << 3;
        const int n = (int)(numel - c0 < 8 ? numel - c0 : 8);
        float v[8];
        dyn_load<XDT>(p, c0, n, v);
        dyn_qdq8<XDT, GS>(p, v, n, se, z, rs);
        dyn_store<XDT>(p, c0, n, v);
    }
}

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

using namespace ct;

extern "C" {

int ct_dynamic_qdq(const void* x, int xdt, int64_t segs, int64_t seg_len, int kind, int bits, int symmetric, const float* global_scale,
                   void* out, void* scale_out, void* zp_out, int zdt, ct_stream_t stream) {
    DynParams p;
    int rc = fill_dyn(p, x, xdt, segs, seg_len, kind, bits, symmetric, global_scale, out, scale_out, zp_out, zdt);
    if (rc) return rc;
    if (segs == 0) return CT_OK;
    const int64_t upr = cdiv64(seg_len, 8);
    const int lpg = (int)upr;
    if (p.vec && seg_len % 8 == 0 && upr <= 64 && log2_exact(upr) >= 0) {
        constexpr int U = 2;  // 4 measured slower (0.43 against 0.47 of the peak at 8192 x 28672)
        const int64_t units = segs * upr;
        const int64_t g = cdiv64(units, (int64_t)kBlock * U);
        CT_REQUIRE(g < ((int64_t)1 << 31), "activation too large for one launch");
        CT_DYN_DISPATCH(xdt, global_scale, hipLaunchKernelGGL((dyn_group_kernel<X, G, U>), dim3((unsigned)g), dim3(kBlock), 0, as_stream(stream), p, units, lpg));
        CT_LAUNCH_CHECK("ct_dynamic_qdq[group]");
    }
    p.vec = p.vec && seg_len % 8 == 0;  // every unit of every segment starts on a 16-byte boundary
    int64_t nt = cdiv64(cdiv64(upr, kSegUnits), 64) * 64;
    if (nt < 64) nt = 64;
    if (nt > kSegMaxThreads) nt = kSegMaxThreads;
    const int64_t g = segs < (1 << 20) ? segs : (1 << 20);
    CT_DYN_DISPATCH(xdt, global_scale, hipLaunchKernelGGL((dyn_seg_kernel<X, G>), dim3((unsigned)g), dim3((unsigned)nt), 0, as_stream(stream), p));
    CT_LAUNCH_CHECK("ct_dynamic_qdq[segment]");
}

int ct_dynamic_qdq_tensor(const void* x, int xdt, int64_t numel, int kind, int bits, int symmetric, const float* global_scale,
                          void* workspace, void* out, void* scale_out, void* zp_out, int zdt, ct_stream_t stream) {
    CT_REQUIRE(numel >= 1, "dynamic tensor qparams of an empty tensor");
    CT_REQUIRE(workspace != nullptr, "ct_dynamic_qdq_tensor needs its workspace (CT_DYNAMIC_WORKSPACE_BYTES)");
    static_assert(sizeof(MinMax) * CT_DYNAMIC_PARTS <= CT_DYNAMIC_WORKSPACE_BYTES, "workspace too small for the partials");
    DynParams p;
    int rc = fill_dyn(p, x, xdt, 1, numel, kind, bits, symmetric, global_scale, out, scale_out, zp_out, zdt);
    if (rc) return rc;
    const int64_t units = cdiv64(numel, 8);
    int64_t parts = cdiv64(units, (int64_t)kBlock * 8);
    if (parts > CT_DYNAMIC_PARTS) parts = CT_DYNAMIC_PARTS;
    MinMax* ws = static_cast<MinMax*>(workspace);
    switch (xdt) {
        case CT_BF16: hipLaunchKernelGGL((dyn_partial_kernel<CT_BF16>), dim3((unsigned)parts), dim3(kBlock), 0, as_stream(stream), p, ws); break;
        case CT_F16: hipLaunchKernelGGL((dyn_partial_kernel<CT_F16>), dim3((unsigned)parts), dim3(kBlock), 0, as_stream(stream), p, ws); break;
        default: hipLaunchKernelGGL((dyn_partial_kernel<CT_F32>), dim3((unsigned)parts), dim3(kBlock), 0, as_stream(stream), p, ws); break;
    }
    rc = hip_check(hipGetLastError(), "ct_dynamic_qdq_tensor[partials]");
    if (rc) return rc;
    int64_t g = cdiv64(units, (int64_t)kBlock * 4);
    if (g > kCUs * 8) g = kCUs * 8;
    if (g < 1) g = 1;
    CT_DYN_DISPATCH(xdt, global_scale, hipLaunchKernelGGL((dyn_flat_kernel<X, G>), dim3((unsigned)g), dim3(kBlock), 0, as_stream(stream), p, ws, (int)parts));
    CT_LAUNCH_CHECK("ct_dynamic_qdq_tensor[qdq]");
}

}  // extern "C"
