// ct_rotated_k.hip — the random-hadamard rotation of size n = K * M, K > 1 (csrc/ct_hadamard_k.hip, form (b): the mix on the matrix
// cores, the butterfly over M on the accumulators) and the dynamic activation QDQ that follows it (csrc/ct_dynamic.hip) in ONE
// launch.  QuaRot / SpinQuant's R4 in front of down_proj is this rotation (the intermediate sizes 11008, 14336, 18944, 28672 are
// no powers of two); the rotated activation never goes to HBM and back.
//
// rotk_mfma_kernel keeps hadk_mfma_kernel's phases in its order and with its device functions: the A strip of hadK in registers
// for the whole launch, the transposing scatter into image[column][k] with zeroed pad columns, the MFMA mix, lane_stages and the
// tile additions, the barrier, the IEEE division by fl(sqrt n), ONE rounding to the activation dtype, the 2-byte writes into the
// LDS image in the output's order.  From there the rounded block (the group of G = 32 / M blocks when M < 32) sits in LDS as
// 16-byte units, consecutive threads hold consecutive units, and the accumulators are dead.  The QDQ is one more phase on that
// image, with ct_dynamic.h's functions on the rounded values only — output, scale and zero point are the bits ct_hadamard_k_rows
// followed by ct_dynamic_qdq produce:
//   group (lpg > 0)   segments of L = 8 * lpg <= 512 elements, L | n: lpg <= 64 divides 64 and the workgroup is whole waves, so a
//                     segment never straddles a wave.  The store loop's bound is wave-uniform (rounded up, loads and stores
//                     guarded): every lane of a wave runs the lane exchanges of group_reduce, dead lanes carry the neutral element
//   row   (lpg == 0)  L = n with G == 1 (M >= 32: the token row is one rotation block).  Pass one accumulates min / max per thread,
//                     the waves finish through a reduction area BEHIND the image, one barrier, every thread computes the same
//                     qparams, pass two re-reads the image and quantizes.  The closing barrier covers both: the next round of the
//                     grid-stride loop rewrites the image and the area
// The helpers of ct_hadamard_k.hip this file needs (flip8, mfma16, the constants) are repeated, not shared: moving them into a
// header changed the pinned ISA of the parents' objects.
#include "ct_dynamic.h"
#include "ct_hadamard.h"

namespace ct {

constexpr int kRotKMaxK = 256, kRotKMaxSteps = kRotKMaxK / 16, kRotKMaxN = 32768, kRotKMaxLds = 65536;  // kHadKMaxK, kHadKMaxSteps, kHadKMfmaMaxN, kHadKMaxLds
constexpr int kRotKMaxWaves = kRotKMaxK / 32;
constexpr int kRotKRedBytes = 128;  // the row form's reduction area: kRotKMaxWaves MinMax of 12 bytes, rounded up to 16-byte units

typedef float rk_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 rk_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 rk_f16x8 __attribute__((ext_vector_type(8)));

// the sign bits of 8 16-bit words flipped where the sign is -1 (bit 7 of a byte: negative)
__device__ __forceinline__ u32x4 rk_flip8(u32x4 v, const int8_t* __restrict__ signs8) {
    const uint64_t w = *reinterpret_cast<const uint64_t*>(signs8);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t lo = (uint32_t)(w >> (16 * p + 7)) & 1u, hi = (uint32_t)(w >> (16 * p + 15)) & 1u;
        v[p] ^= (lo << 15) | (hi << 31);
    }
    return v;
}

template <int XDT>
__device__ __forceinline__ rk_f32x16 rk_mfma16(u32x4 a, u32x4 b, rk_f32x16 c) {
    if constexpr (XDT == CT_BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(rk_bf16x8, a), __builtin_bit_cast(rk_bf16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(rk_f16x8, a), __builtin_bit_cast(rk_f16x8, b), c, 0, 0, 0);
}

// a 16-byte unit of the LDS image as 8 floats (exact), and its raw words for the rotated tensor
template <int XDT>
__device__ __forceinline__ u32x4 rk_unit(const uint16_t* image, int e, float (&v)[8]) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(image + e);
    RawUnit<XDT> raw;
#pragma unroll
    for (int j = 0; j < 4; ++j) raw.w[j] = w[j];
    raw_unpack<XDT>(raw, v);
    return w;
}

// One workgroup of ceil(K / 32) waves per group of G = max(32 / M, 1) consecutive blocks, C = G * M = 32 * TT columns; the image
// holds C rows of LS = 16 KS + 8 elements while it is the staged (transposed) row, G * n elements in the output's order afterwards
template <int XDT, int TT, bool GS>
__global__ __launch_bounds__(512) void rotk_mfma_kernel(DynParams p, uint16_t* __restrict__ rotated, int64_t blocks, int n, int K, int lm /*log2 M*/,
                                                        const int8_t* __restrict__ had_k, const int8_t* __restrict__ signs, float sn, int lpg) {
    extern __shared__ __attribute__((aligned(16))) uint16_t image[];
    constexpr int C = 32 * TT;
    constexpr uint32_t kOne = XDT == CT_BF16 ? 0x3F80u : 0x3C00u;
    const uint16_t* __restrict__ x = static_cast<const uint16_t*>(p.x);
    const int M = 1 << lm, G = C >> lm;  // G == 1 for M >= 32
    const int KS = (K + 15) >> 4, LS = KS * 16 + 8;
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- 1. the A strip of hadK: rows 32 wave .. 32 wave + 31, KS fragments, in registers for the whole launch
    u32x4 a[kRotKMaxSteps];
    {
        const int kp = 32 * wave + r;
#pragma unroll
        for (int s = 0; s < kRotKMaxSteps; ++s) {
            uint32_t e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {  // branch-free: a clamped read, then the mask
                const int k = 16 * s + 8 * h + j, kc = k < K ? k : K - 1, kpc = kp < K ? kp : K - 1;
                const uint32_t v = kOne | ((had_k[kpc * K + kc] < 0) ? 0x8000u : 0u);
                e[j] = (kp < K && k < K) ? v : 0u;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) a[s][q] = e[2 * q] | (e[2 * q + 1] << 16);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    const int units = (G * n) >> 3;  // 16-byte units of a group
    const int64_t groups = (blocks + G - 1) / G;
    MinMax* red = reinterpret_cast<MinMax*>(image + C * LS);  // behind the image (row form; the launch sized it)
    for (int64_t gi = blockIdx.x; gi < groups; gi += gridDim.x) {
        const int64_t b0 = gi * G;
        // ---- 2. load: signs, transpose into image[c][k]; the pad columns are real zeros (0 * NaN is NaN)
        for (int u = tid; u < units; u += T) {
            const int e = u << 3, g = e / n, rr = e - g * n, k = rr >> lm, t = rr & (M - 1);
            u32x4 w = {0, 0, 0, 0};
            if (b0 + g < blocks) {
                w = *reinterpret_cast<const u32x4*>(x + (b0 * n + e));
                if (signs != nullptr) w = rk_flip8(w, signs + rr);
            }
            uint16_t* col = image + ((g << lm) + t) * LS + k;
#pragma unroll
            for (int j = 0; j < 8; ++j) col[j * LS] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
        }
        const int pad = KS * 16 - K;
        for (int i = tid; i < C * pad; i += T) image[(i / pad) * LS + K + i % pad] = 0;
        __syncthreads();

        // ---- 3. mix
        rk_f32x16 acc[TT];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[tt][q] = 0.0f;
        const uint16_t* brow = image + r * LS + 8 * h;
#pragma unroll
        for (int s = 0; s < kRotKMaxSteps; ++s) {
            if (s < KS) {
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) acc[tt] = rk_mfma16<XDT>(a[s], *reinterpret_cast<const u32x4*>(brow + 32 * tt * LS + 16 * s), acc[tt]);
            }
        }

        // ---- 4. the butterfly over t: lane bits, then tiles
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = acc[tt][8 * half + q];
                lane_stages(v, M < 32 ? M : 32, lane);
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[tt][8 * half + q] = v[q];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int hh = 1; hh < TT; hh <<= 1) {
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) {
                if (!(tt & hh)) {
                    const rk_f32x16 pp = acc[tt], qq = acc[tt | hh];
                    acc[tt] = pp + qq;
                    acc[tt | hh] = pp - qq;
                }
            }
        }
        __syncthreads();  // ---- 5. every wave has read the staged row

        // ---- 6. - 8. quotient, rounding, the image in the output's order (row and column through an empty asm, as the parent:
        // hoisted out of the round loop the 16 * TT addresses cost more registers than the accumulators)
        int row0 = 32 * wave + 4 * h, col0 = r;
        asm volatile("" : "+v"(row0), "+v"(col0));
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
            const int c = 32 * tt + col0, g = c >> lm, t = c & (M - 1);
            uint16_t* o = image + g * n + (row0 << lm) + t;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int dk = (q & 3) + 8 * (q >> 2);
                if (row0 + dk < K) {
                    const float y = acc[tt][q] / sn;
                    o[dk << lm] = (uint16_t)(XDT == CT_BF16 ? f_to_bf16_bits(y) : f_to_f16_bits(y));
                }
            }
        }
        __syncthreads();

        // ---- 9. the QDQ on the rounded image: the accumulators are dead, a unit is 4 + 8 registers
        const int64_t el0 = b0 * n;  // the group's first element
        if (lpg) {
            const int llpg = __builtin_ctz(lpg);  // lpg is a power of two: the segment index is a shift, not a 64-bit division
            for (int ub = 0; ub < units; ub += T) {  // wave-uniform bound: a segment's lanes all run the exchange, or none does
                const int u = ub + tid, e = u << 3;
                const bool live = u < units && (G == 1 || b0 + e / n < blocks);  // whole segments: units, n / 8 and T are multiples of lpg
                float v[8];
                MinMax m = mm_neutral();
                if (live) {
                    const u32x4 w = rk_unit<XDT>(image, e, v);
                    if (rotated) stream_store16(rotated + (el0 + e), w);
                    m = mm_acc(m, v, 8);
                }
                m = group_reduce(m, lpg);
                if (live) {
                    float s, z;
                    dyn_qparams<XDT>(p, m, s, z);
                    if ((tid & (lpg - 1)) == 0) dyn_write_qparams<XDT, GS>(p, ((el0 >> 3) + u) >> llpg, s, z);
                    if (p.out) {
                        const float se = GS ? s / p.gscale[0] : s;
                        dyn_qdq8<XDT, GS>(p, v, 8, se, z, GS ? 0.0f : dyn_rcp<XDT>(s));
                        store8<XDT>(p.out, el0 + e, v);
                    }
                }
            }
        } else {  // G == 1: the block is the token row, every unit is live
            MinMax m = mm_neutral();
            for (int u = tid; u < units; u += T) {
                float v[8];
                const u32x4 w = rk_unit<XDT>(image, u << 3, v);
                if (rotated) stream_store16(rotated + (el0 + (u << 3)), w);
                m = mm_acc(m, v, 8);
            }
            m = group_reduce(m, 64);
            if (lane == 0) red[wave] = m;
            __syncthreads();
            m = red[0];
            for (int w = 1; w < (T >> 6); ++w) m = mm_merge(m, red[w]);
            float s, z;
            dyn_qparams<XDT>(p, m, s, z);
            if (tid == 0) dyn_write_qparams<XDT, GS>(p, gi, s, z);
            if (p.out) {
                const float se = GS ? s / p.gscale[0] : s;
                const float rs = GS ? 0.0f : dyn_rcp<XDT>(s);
                for (int u = tid; u < units; u += T) {
                    float v[8];
                    rk_unit<XDT>(image, u << 3, v);
                    dyn_qdq8<XDT, GS>(p, v, 8, se, z, rs);
                    store8<XDT>(p.out, el0 + (u << 3), v);
                }
            }
        }
        __syncthreads();  // the image and the reduction area are rewritten by the next round
    }
}

static size_t rotk_image_bytes(int64_t k, int64_t m) { return (size_t)(m > 32 ? m : 32) * (size_t)(cdiv64(k, 16) * 16 + 8) * 2; }

template <int XDT, bool GS>
static void launch_rotk(const DynParams& p, void* rotated, int64_t blocks, int64_t n, int64_t k, const int8_t* had_k, const int8_t* signs, int lpg, hipStream_t s) {
    const int64_t m = n / k, per = m >= 32 ? 1 : 32 / m, groups = cdiv64(blocks, per);
    const int64_t g = groups < 2 * kCUs ? groups : 2 * kCUs;  // the A fragments are loaded once per workgroup
    const dim3 grid((unsigned)g), block((unsigned)(64 * cdiv64(k, 32)));
    const size_t lds = rotk_image_bytes(k, m) + (lpg ? 0 : kRotKRedBytes);
    const float sn = (float)__builtin_sqrt((double)n);
    uint16_t* ro = static_cast<uint16_t*>(rotated);
    const int lm = log2_exact(m);
    if (m <= 32) hipLaunchKernelGGL((rotk_mfma_kernel<XDT, 1, GS>), grid, block, lds, s, p, ro, blocks, (int)n, (int)k, lm, had_k, signs, sn, lpg);
    else if (m == 64) hipLaunchKernelGGL((rotk_mfma_kernel<XDT, 2, GS>), grid, block, lds, s, p, ro, blocks, (int)n, (int)k, lm, had_k, signs, sn, lpg);
    else hipLaunchKernelGGL((rotk_mfma_kernel<XDT, 4, GS>), grid, block, lds, s, p, ro, blocks, (int)n, (int)k, lm, had_k, signs, sn, lpg);
}

}  // namespace ct

using namespace ct;

extern "C" {

int ct_hadamard_k_dynamic_qdq(const void* x, int xdt, int64_t numel, int64_t n, int64_t k, const int8_t* had_k, const int8_t* signs, int64_t seg_len, int kind,
                              int bits, int symmetric, const float* global_scale, void* rotated_out, void* out, void* scale_out, void* zp_out, int zdt,
                              ct_stream_t stream) {
    CT_REQUIRE(n >= 1 && k >= 1 && n % k == 0 && log2_exact(n / k) >= 0, "hadamard size %lld is not %lld * 2^m", (long long)n, (long long)k);
    CT_REQUIRE(seg_len >= 1 && numel >= 0 && numel % n == 0 && numel % seg_len == 0, "hadamard size %lld and segment length %lld do not both divide %lld elements",
               (long long)n, (long long)seg_len, (long long)numel);
    CT_REQUIRE((k == 1) == (had_k == nullptr), "had_k is the k x k mix for k > 1 and null for k == 1");
    const int64_t L = seg_len, segs = numel / L, m = n / k;
    DynParams p;
    const int rc = fill_dyn(p, x, xdt, segs, L, kind, bits, symmetric, global_scale, out, scale_out, zp_out, zdt);
    if (rc) return rc;
    if (numel == 0) return CT_OK;
    if (k == 1) CT_UNSUPPORTED("k == 1 (signs and the butterfly) has no fused launch");
    if (xdt == CT_F32) CT_UNSUPPORTED("the fused mix takes 16-bit activations");
    if (k > kRotKMaxK) CT_UNSUPPORTED("the mix takes k <= %d, got %lld", kRotKMaxK, (long long)k);
    if (m < 8 || m > 128 || n > kRotKMaxN) CT_UNSUPPORTED("the fused mix takes runs of 8 .. 128 elements and n <= %d, got %lld x %lld", kRotKMaxN, (long long)k, (long long)m);
    if (!aligned16(x) || (out && !aligned16(out)) || (rotated_out && !aligned16(rotated_out))) CT_UNSUPPORTED("the fused rotation takes 16-byte aligned tensors");
    if (!aligned_to<8>(signs)) CT_UNSUPPORTED("the hadamard kernels take 8-byte aligned signs");
    const int64_t upr = L / 8;
    int lpg;
    if (L % 8 == 0 && upr <= 64 && log2_exact(upr) >= 0 && n % L == 0) {
        lpg = (int)upr;  // in-wave segments inside a block
    } else if (L == n) {
        if (m < 32) CT_UNSUPPORTED("a token row of %lld elements shares its workgroup with %lld more blocks", (long long)n, (long long)(32 / m - 1));
        if (segs == 1) CT_UNSUPPORTED("one segment of %lld elements is the tensor form: its reduction is global", (long long)L);
        lpg = 0;
    } else {
        CT_UNSUPPORTED("a segment of %lld elements over rotation blocks of %lld is not fused", (long long)L, (long long)n);
    }
    if (rotk_image_bytes(k, m) + (lpg ? 0 : kRotKRedBytes) > (size_t)kRotKMaxLds) CT_UNSUPPORTED("the staged row of %lld x %lld exceeds the LDS", (long long)k, (long long)m);
    hipStream_t s = as_stream(stream);
    if (xdt == CT_BF16) {
        if (global_scale) launch_rotk<CT_BF16, true>(p, rotated_out, numel / n, n, k, had_k, signs, lpg, s);
        else launch_rotk<CT_BF16, false>(p, rotated_out, numel / n, n, k, had_k, signs, lpg, s);
    } else {
        if (global_scale) launch_rotk<CT_F16, true>(p, rotated_out, numel / n, n, k, had_k, signs, lpg, s);
        else launch_rotk<CT_F16, false>(p, rotated_out, numel / n, n, k, had_k, signs, lpg, s);
    }
    CT_LAUNCH_CHECK("ct_hadamard_k_dynamic_qdq");
}

}  // extern "C"
