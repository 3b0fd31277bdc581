// ct_rotated.hip — the online Hadamard rotation (csrc/ct_hadamard.hip) and the dynamic activation QDQ that follows it
// (csrc/ct_dynamic.hip) in ONE launch: r = rnd_X(FWHT_n(x) / sqrt(n)) over runs of n elements, then the min / max observer,
// calculate_qparams and fake_quantize over runs of seg_len elements of r.  The rotated tensor never goes to HBM and back
// (it is written once when the caller asks for it); one read and one write instead of two of each.
//
// The arithmetic is the two parents' own device functions (ct_hadamard.h, ct_dynamic.h) in the parents' order: the butterfly
// stages in float32, ONE quotient by sqrt(n) (had_div8), the rounding to x's dtype that had_store's conversion performs —
// and only those rounded values reach mm_acc / dyn_qparams / dyn_qdq8.  Output, scale and zero point are therefore the bits
// ct_hadamard_rows followed by ct_dynamic_qdq produce (min / max are order-independent up to the sign of a zero, which no
// quantization parameter can tell apart).
//
// Kernels (n the rotation block, L the segment; both runs of the contiguous last dimension)
//   rot_group_kernel  n <= 512, L = 8 * 2^k <= 512: had_group_kernel's stages, then dyn_group_kernel's in-wave reduction and
//                     QDQ on the same registers (both parents use units kBlock apart, U = 2)
//   rot_block_kernel  n = 1024 .. 8192, one workgroup per block (had_block_kernel's stages incl. the LDS exchange: ct_hadamard_block.inc); consecutive
//                     units sit in consecutive lanes, so L <= 512 is reduced inside the wave; L = n (the block is a token row)
//                     is finished across the waves through LDS as dyn_seg_kernel does
//   rot_seg_kernel    n <= 512 < L, n divides L: dyn_seg_kernel's staged form (a token row of up to 32768 elements held as raw
//                     words); the in-wave butterfly runs on each unit after unpacking, the rounded values are repacked
#include "ct_dynamic.h"
#include "ct_hadamard.h"

namespace ct {

// the rotated values of a unit: quotient by sqrt(n), rounded to XDT (what had_store writes and dyn_load reads back)
template <int XDT>
__device__ __forceinline__ void rot_round8(const float (&v)[8], const HadScale<float>& sn, float (&r)[8]) {
    had_div8(v, sn, r);
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = round_to<XDT>(r[k]);
}

// values already rounded to XDT -> a unit's raw words (exact)
template <int XDT>
__device__ __forceinline__ void raw_pack(const float (&v)[8], RawUnit<XDT>& r) {
    if constexpr (XDT == CT_F32) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r.w[k] = f_bits(v[k]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (XDT == CT_BF16) r.w[j] = f_to_bf16_bits(v[2 * j]) | (f_to_bf16_bits(v[2 * j + 1]) << 16);
            else r.w[j] = f_to_f16_bits(v[2 * j]) | (f_to_f16_bits(v[2 * j + 1]) << 16);
        }
    }
}

// ---- n <= 512 and L <= 512: lpb lanes per rotation block, lpg lanes per segment, U units per lane kBlock apart ---------------------
template <int XDT, bool GS>
__global__ __launch_bounds__(kBlock) void rot_group_kernel(DynParams p, void* rotated, int64_t units, int n, int lpg, HadScale<float> sn) {
    constexpr int U = kHadGroupUnits;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
    const int lpb = n >> 3, lane = threadIdx.x & 63;
    float v[U][8];
    // units is a multiple of lpb and of lpg, and kBlock of both: neither a block nor a segment straddles a wave, and every lane
    // of a live one is live.  Dead lanes carry zeros through the exchanges (every lane executes them) and store nothing.
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int64_t u = base + (int64_t)i * kBlock;
        if (u < units) {
            load8<XDT>(p.x, u << 3, v[i]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[i][k] = 0.0f;
        }
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
        unit_stages(v[i], n);
        lane_stages(v[i], lpb, lane);
    }
    MinMax m[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int64_t u = base + (int64_t)i * kBlock;
        m[i] = mm_neutral();
        if (u < units) {
            rot_round8<XDT>(v[i], sn, v[i]);
            if (rotated) store8<XDT>(rotated, u << 3, v[i]);
            m[i] = mm_acc(m[i], v[i], 8);
        }
    }
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

// ---- n = 64 * WAVES * U * 8: one workgroup per rotation block; lpg lanes per segment, or the block is the segment (lpg == 0) ---------
template <int XDT, bool GS, int U, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void rot_block_kernel(DynParams p, void* rotated, int64_t blocks, int lpg, HadScale<float> sn) {
    typedef float A;  // the names ct_hadamard_block.inc expects: float32 accumulation, two 16-byte chunks per unit
    constexpr int T = 64 * WAVES, N = T * U * 8, CH = 4, CPU = 2;
    typedef A chunk_t __attribute__((ext_vector_type(CH)));
    __shared__ chunk_t lds[WAVES > 1 ? N / CH : 1];
    __shared__ MinMax red[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const int64_t u0 = b * (N / 8);  // the block's first unit
        float v[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) load8<XDT>(p.x, (u0 + u * T + tid) << 3, v[u]);
#include "ct_hadamard_block.inc"
        MinMax m[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            rot_round8<XDT>(v[u], sn, v[u]);
            if (rotated) store8<XDT>(rotated, (u0 + u * T + tid) << 3, v[u]);
            m[u] = mm_acc(mm_neutral(), v[u], 8);
        }
        if (lpg) {
#pragma unroll
            for (int u = 0; u < U; ++u) m[u] = group_reduce(m[u], lpg);
        } else {
#pragma unroll
            for (int u = 1; u < U; ++u) m[0] = mm_merge(m[0], m[u]);
            m[0] = group_reduce(m[0], 64);
            if constexpr (WAVES > 1) {
                if (lane == 0) red[wave] = m[0];
                __syncthreads();
                m[0] = red[0];
#pragma unroll
                for (int w = 1; w < WAVES; ++w) m[0] = mm_merge(m[0], red[w]);
                __syncthreads();  // red[] is rewritten by the next block
            }
#pragma unroll
            for (int u = 1; u < U; ++u) m[u] = m[0];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t gu = u0 + u * T + tid;
            float s, z;
            dyn_qparams<XDT>(p, m[u], s, z);
            if (lpg) {
                if ((tid & (lpg - 1)) == 0) dyn_write_qparams<XDT, GS>(p, gu / lpg, s, z);
            } else if (u == 0 && tid == 0) {
                dyn_write_qparams<XDT, GS>(p, b, s, z);
            }
            if (p.out) {
                const float se = GS ? s / p.gscale[0] : s;
                dyn_qdq8<XDT, GS>(p, v[u], 8, se, z, GS ? 0.0f : dyn_rcp<XDT>(s));
                store8<XDT>(p.out, gu << 3, v[u]);
            }
        }
    }
}

// ---- n <= 512 < L: one workgroup per token row of L / n rotation blocks, the row staged in registers as raw words -----------------------
template <int XDT, bool GS>
__global__ __launch_bounds__(kSegMaxThreads) void rot_seg_kernel(DynParams p, void* rotated, int n, HadScale<float> sn) {
    __shared__ MinMax red[kSegMaxThreads / 64];
    const int nt = blockDim.x, tid = threadIdx.x, nw = nt >> 6, lane = tid & 63;
    const int lpb = n >> 3;
    const int64_t upr = p.seg_len >> 3;  // a multiple of lpb, as nt is: unit tid + k * nt keeps a block inside a wave, all live or all dead
    for (int64_t seg = blockIdx.x; seg < p.segs; seg += gridDim.x) {
        const int64_t base = seg * p.seg_len;
        RawUnit<XDT> raw[kSegUnits];
        MinMax m = mm_neutral();
#pragma unroll
        for (int k = 0; k < kSegUnits; ++k) {
            const int64_t u = tid + (int64_t)k * nt;
            if (u < upr) {
                raw_load<XDT>(p, base + (u << 3), 8, raw[k]);
            } else {
#pragma unroll
                for (int j = 0; j < RawUnit<XDT>::W; ++j) raw[k].w[j] = 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < kSegUnits; ++k) {
            const int64_t u = tid + (int64_t)k * nt;
            if (k * nt < upr) {  // workgroup-uniform: dead lanes of a live step carry zeros through the exchanges
                float v[8];
                raw_unpack<XDT>(raw[k], v);
                unit_stages(v, n);
                lane_stages(v, lpb, lane);
                if (u < upr) {
                    rot_round8<XDT>(v, sn, v);
                    if (rotated) store8<XDT>(rotated, base + (u << 3), v);
                    raw_pack<XDT>(v, raw[k]);
                    m = mm_acc(m, v, 8);
                }
            }
        }
        m = group_reduce(m, 64);
        if (lane == 0) red[tid >> 6] = m;
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
#pragma unroll
        for (int k = 0; k < kSegUnits; ++k) {
            const int64_t u = tid + (int64_t)k * nt;
            if (u < upr) {
                float v[8];
                raw_unpack<XDT>(raw[k], v);
                dyn_qdq8<XDT, GS>(p, v, 8, se, z, rs);
                store8<XDT>(p.out, base + (u << 3), v);
            }
        }
    }
}

template <int XDT, bool GS, int U, int WAVES>
static void launch_rot_block(const DynParams& p, void* rotated, int64_t blocks, int lpg, HadScale<float> sn, hipStream_t s) {
    hipLaunchKernelGGL((rot_block_kernel<XDT, GS, U, WAVES>), capped_grid(blocks), dim3(64 * WAVES), 0, s, p, rotated, blocks, lpg, sn);
}

// n = 16384 (<8, 4>: 64 values per thread, 284 VGPRs + 28 AGPRs, one wave per SIMD) was built without scratch and MEASURED slower than the two
// launches (bf16 (1, 4096, 16384): FP8 token 308 against 213 us, FP8 group 128 338 against 189 us): it is left to them
constexpr int64_t kRotMaxBlock = 8192;

}  // namespace ct

using namespace ct;

extern "C" {

int ct_hadamard_dynamic_qdq(const void* x, int xdt, int64_t numel, int64_t n, int64_t seg_len, int kind, int bits, int symmetric,
                            const float* global_scale, void* rotated_out, void* out, void* scale_out, void* zp_out, int zdt, ct_stream_t stream) {
    CT_REQUIRE(n >= 1 && log2_exact(n) >= 0, "Cannot construct deterministic hadamard of size != 2^n");
    CT_REQUIRE(seg_len >= 1 && numel >= 0 && numel % n == 0 && numel % seg_len == 0, "hadamard size %lld and segment length %lld do not both divide %lld elements",
               (long long)n, (long long)seg_len, (long long)numel);
    const int64_t L = seg_len, segs = numel / L;
    DynParams p;
    int rc = fill_dyn(p, x, xdt, segs, L, kind, bits, symmetric, global_scale, out, scale_out, zp_out, zdt);
    if (rc) return rc;
    if (numel == 0) return CT_OK;
    if (!aligned16(x) || (out && !aligned16(out)) || (rotated_out && !aligned16(rotated_out))) CT_UNSUPPORTED("the fused rotation takes 16-byte aligned tensors");
    if (L % 8) CT_UNSUPPORTED("segments of %lld elements are not whole 16-byte units", (long long)L);
    const HadScale<float> sn = make_had_scale<float>(n);
    hipStream_t s = as_stream(stream);
    const int64_t upr = L / 8;
    const bool in_wave = upr <= 64 && log2_exact(upr) >= 0;  // dyn_group_kernel's segments
    if (n <= 512 && in_wave) {
        const int64_t units = numel / 8;
        const int64_t g = cdiv64(units, (int64_t)kBlock * kHadGroupUnits);
        CT_REQUIRE(g < ((int64_t)1 << 31), "activation too large for one launch");
        CT_DYN_DISPATCH(xdt, global_scale, hipLaunchKernelGGL((rot_group_kernel<X, G>), dim3((unsigned)g), dim3(kBlock), 0, s, p, rotated_out, units, (int)n, (int)upr, sn));
        CT_LAUNCH_CHECK("ct_hadamard_dynamic_qdq[group]");
    }
    if (n <= 512) {
        if (segs == 1 && L > 512) CT_UNSUPPORTED("one segment of %lld elements is the tensor form: its reduction is global", (long long)L);
        if (L % n) CT_UNSUPPORTED("hadamard size %lld does not divide the segment length %lld", (long long)n, (long long)L);
        int64_t nt = cdiv64(cdiv64(upr, kSegUnits), 64) * 64;
        if (nt > kSegMaxThreads) nt = kSegMaxThreads;
        if (upr > nt * kSegUnits) CT_UNSUPPORTED("rows of %lld elements exceed the staged form (%d)", (long long)L, kSegMaxThreads * kSegUnits * 8);
        CT_DYN_DISPATCH(xdt, global_scale, hipLaunchKernelGGL((rot_seg_kernel<X, G>), capped_grid(segs), dim3((unsigned)nt), 0, s, p, rotated_out, (int)n, sn));
        CT_LAUNCH_CHECK("ct_hadamard_dynamic_qdq[row]");
    }
    if (n > kRotMaxBlock) CT_UNSUPPORTED("hadamard size %lld exceeds the fused maximum %lld", (long long)n, (long long)kRotMaxBlock);
    if (!(in_wave || L == n)) CT_UNSUPPORTED("a segment of %lld elements over workgroup-sized blocks of %lld is not fused", (long long)L, (long long)n);
    if (L == n && segs == 1) CT_UNSUPPORTED("one segment of %lld elements is the tensor form: its reduction is global", (long long)L);
    const int64_t blocks = numel / n;
    const int lpg = in_wave ? (int)upr : 0;
    switch (n) {
        case 1024: CT_DYN_DISPATCH(xdt, global_scale, (launch_rot_block<X, G, 2, 1>(p, rotated_out, blocks, lpg, sn, s))); break;
        case 2048: CT_DYN_DISPATCH(xdt, global_scale, (launch_rot_block<X, G, 4, 1>(p, rotated_out, blocks, lpg, sn, s))); break;
        case 4096: CT_DYN_DISPATCH(xdt, global_scale, (launch_rot_block<X, G, 4, 2>(p, rotated_out, blocks, lpg, sn, s))); break;
        default: CT_DYN_DISPATCH(xdt, global_scale, (launch_rot_block<X, G, 4, 4>(p, rotated_out, blocks, lpg, sn, s))); break;
    }
    CT_LAUNCH_CHECK("ct_hadamard_dynamic_qdq[block]");
}

}  // extern "C"
