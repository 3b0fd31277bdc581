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
#include "ct_dynamic.h"

namespace ct {

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

// ---- one workgroup per segment -----------------------------------------------------------------------------------------------
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
