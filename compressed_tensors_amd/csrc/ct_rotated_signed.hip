// ct_rotated_signed.hip — the random-hadamard rotation whose size is a power of two (K = 1: a vector of +-1 signs, then the
// Walsh-Hadamard butterfly; csrc/ct_hadamard_k.hip, form (a)) and the dynamic activation QDQ that follows it (csrc/ct_dynamic.hip)
// in ONE launch: r = rnd_X(FWHT_n(s . x) / sqrt(n)) over runs of n elements, then the min / max observer, calculate_qparams and
// fake_quantize over runs of seg_len elements of r.  QuIP-style input rotations on hidden sizes 2048 / 4096 / 8192, R4 in front of
// down_proj where the intermediate size is a power of two, every head-dim rotation: one read and one write instead of two of each.
//
// The signs.  A thread meets the SAME positions of a rotation block in every unit it ever loads: the units of a thread are a
// multiple of the block's lanes apart (n <= 512) or sit at (u * T + tid) * 8 of a workgroup-sized block.  So a thread reads its 8
// sign bytes per position ONCE, before the first row — one 8-byte load per position and workgroup, none in front of the exchanges —
// and keeps them as ONE register per position: bit k of the byte spread so that a shift by j and one mask give the sign bits of
// the two 16-bit elements of word j (sg_pack / sg_flip).  +-1 is then a XOR on the raw 16-byte unit between the load and the
// conversion to float32: exact, -0.0, inf and NaN included, and the bits hadk_load's flip of the converted float gives.  The
// workgroups stride over the rows (a capped grid), which is what spreads the one sign load over many rows.
//
// Everything behind the flip is the parents' device functions in the parents' order (ct_hadamard.h, ct_hadamard_block.inc,
// ct_dynamic.h): the butterfly stages in float32, ONE quotient by sqrt(n) (had_div8), ONE rounding to x's dtype, and only the rounded
// values reach mm_acc / dyn_qparams / dyn_qdq8 — output, scale and zero point are the bits ct_hadamard_k_rows (k = 1) followed by
// ct_dynamic_qdq produce.
//
// Kernels (n the rotation block, L the segment; 16-bit activations only)
//   sg_group_kernel  n <= 512, L = 8 * 2^k <= 512: tiles of kBlock * 2 units, butterfly, reduction and QDQ inside a wave
//   sg_seg_kernel    n <= 512 < L, n divides L: one workgroup per token row of up to 32768 elements, the row held as raw words —
//                    flipped in place at the load, overwritten by the rounded rotated values, quantized after the row's reduction
//   sg_block_kernel  n = 1024 .. 8192, one workgroup per block (ct_hadamard_block.inc); L <= 512 is reduced inside the wave,
//                    L = n (the block is the token row) across the waves through LDS
#include "ct_dynamic.h"
#include "ct_hadamard.h"

namespace ct {

// ---- the signs ----------------------------------------------------------------------------------------------------------------------------
// 8 sign bytes (bit 7 of a byte: negative) as one word: the bit of element 2 j at 15 - j, of element 2 j + 1 at 31 - j
__device__ __forceinline__ uint32_t sg_pack(const int8_t* __restrict__ signs8) {
    const uint64_t w = *reinterpret_cast<const uint64_t*>(signs8);
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s |= ((uint32_t)(w >> (8 * k + 7)) & 1u) << (((k & 1) ? 31 : 15) - (k >> 1));
    return s;
}

// a raw unit of 8 16-bit elements with the sign bit flipped where the sign is -1: the shift puts pair j's two bits at 15 and 31,
// the bits of the pairs below j land in 16 .. 18 or leave the word, those above stay below 15 and 31 — the mask drops them
__device__ __forceinline__ u32x4 sg_flip(u32x4 w, uint32_t s) {
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] ^= (s << j) & 0x80008000u;
    return w;
}

__device__ __forceinline__ u32x4 sg_load(const uint16_t* __restrict__ x, int64_t i0, uint32_t s) {
    return sg_flip(*reinterpret_cast<const u32x4*>(x + i0), s);
}

template <int XDT>
__device__ __forceinline__ void sg_unpack(u32x4 w, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) unpack2<XDT>(w[j], v[2 * j], v[2 * j + 1]);
}

// the rotated values of a unit: quotient by sqrt(n), rounded to XDT (what hadk_store writes and dyn_load reads back)
template <int XDT>
__device__ __forceinline__ void sg_round8(float (&v)[8], const HadScale<float>& sn) {
    float q[8];
    had_div8(v, sn, q);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = round_to<XDT>(q[k]);
}

// values already rounded to XDT -> the unit's raw words (exact)
template <int XDT>
__device__ __forceinline__ u32x4 sg_words(const float (&v)[8]) {
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (XDT == CT_BF16) w[j] = f_to_bf16_bits(v[2 * j]) | (f_to_bf16_bits(v[2 * j + 1]) << 16);
        else w[j] = f_to_f16_bits(v[2 * j]) | (f_to_f16_bits(v[2 * j + 1]) << 16);
    }
    return w;
}

// ---- n <= 512 and L <= 512: lpb lanes per rotation block, lpg lanes per segment; a workgroup strides over tiles of kBlock * U units ------
template <int XDT, bool GS>
__global__ __launch_bounds__(kBlock) void sg_group_kernel(DynParams p, void* rotated, const int8_t* __restrict__ signs, int64_t units, int64_t tiles, int n, int lpg,
                                                          HadScale<float> sn) {
    constexpr int U = kHadGroupUnits;
    const uint16_t* __restrict__ x = static_cast<const uint16_t*>(p.x);
    const int lpb = n >> 3, lane = threadIdx.x & 63;
    // a tile, and kBlock, are whole blocks: every unit of this thread is unit (tid mod lpb) of its block
    const uint32_t sb = sg_pack(signs + ((threadIdx.x & (lpb - 1)) << 3));
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t base = t * (kBlock * U) + threadIdx.x;
        float v[U][8];
        // units is a multiple of lpb and of lpg, and kBlock of both: neither a block nor a segment straddles a wave, and every lane
        // of a live one is live.  Dead lanes carry zeros through the exchanges (every lane executes them) and store nothing.
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int64_t u = base + (int64_t)i * kBlock;
            if (u < units) {
                sg_unpack<XDT>(sg_load(x, u << 3, sb), v[i]);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) v[i][k] = 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            unit_stages(v[i], 8);
            lane_stages(v[i], lpb, lane);
        }
        MinMax m[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int64_t u = base + (int64_t)i * kBlock;
            m[i] = mm_neutral();
            if (u < units) {
                sg_round8<XDT>(v[i], sn);
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
}

// ---- n <= 512 < L: one workgroup per token row of L / n rotation blocks, the row staged in registers as raw words -----------------------
template <int XDT, bool GS>
__global__ __launch_bounds__(kSegMaxThreads) void sg_seg_kernel(DynParams p, uint16_t* __restrict__ rotated, const int8_t* __restrict__ signs, int n,
                                                                HadScale<float> sn) {
    __shared__ MinMax red[kSegMaxThreads / 64];
    const uint16_t* __restrict__ x = static_cast<const uint16_t*>(p.x);
    const int nt = blockDim.x, tid = threadIdx.x, nw = nt >> 6, lane = tid & 63;
    const int lpb = n >> 3;
    const int64_t upr = p.seg_len >> 3;  // a multiple of lpb, as nt is: unit tid + k * nt keeps a block inside a wave, all live or all dead,
    const uint32_t sb = sg_pack(signs + ((tid & (lpb - 1)) << 3));  // and is unit (tid mod lpb) of its block for every k and every row
    for (int64_t seg = blockIdx.x; seg < p.segs; seg += gridDim.x) {
        const int64_t base = seg * p.seg_len;
        u32x4 raw[kSegUnits];
        MinMax m = mm_neutral();
#pragma unroll
        for (int k = 0; k < kSegUnits; ++k) {
            const int64_t u = tid + (int64_t)k * nt;
            raw[k] = u < upr ? sg_load(x, base + (u << 3), sb) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int k = 0; k < kSegUnits; ++k) {
            const int64_t u = tid + (int64_t)k * nt;
            if (k * nt < upr) {  // workgroup-uniform: dead lanes of a live step carry zeros through the exchanges
                float v[8];
                sg_unpack<XDT>(raw[k], v);
                unit_stages(v, 8);
                lane_stages(v, lpb, lane);
                if (u < upr) {
                    sg_round8<XDT>(v, sn);
                    raw[k] = sg_words<XDT>(v);
                    if (rotated) stream_store16(rotated + (base + (u << 3)), raw[k]);
                    m = mm_acc(m, v, 8);
                }
            }
        }
        m = group_reduce(m, 64);
        if (lane == 0) red[tid >> 6] = m;
        __syncthreads();
        m = red[0];
        for (int w = 1; w < nw; ++w) m = mm_merge(m, red[w]);
        __syncthreads();  // red[] is rewritten by the next row
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
                sg_unpack<XDT>(raw[k], v);
                dyn_qdq8<XDT, GS>(p, v, 8, se, z, rs);
                store8<XDT>(p.out, base + (u << 3), v);
            }
        }
    }
}

// ---- n = 64 * WAVES * U * 8: one workgroup per rotation block; lpg lanes per segment, or the block is the segment (lpg == 0) ---------
template <int XDT, bool GS, int U, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void sg_block_kernel(DynParams p, void* rotated, const int8_t* __restrict__ signs, int64_t blocks, int lpg,
                                                              HadScale<float> sn) {
    typedef float A;  // the names ct_hadamard_block.inc expects: float32 accumulation, two 16-byte chunks per unit
    constexpr int T = 64 * WAVES, N = T * U * 8, CH = 4, CPU = 2;
    typedef A chunk_t __attribute__((ext_vector_type(CH)));
    __shared__ chunk_t lds[WAVES > 1 ? N / CH : 1];
    __shared__ MinMax red[WAVES];
    const uint16_t* __restrict__ x = static_cast<const uint16_t*>(p.x);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t sb[U];  // the block's n signs, one bit each, for every block this workgroup rotates
#pragma unroll
    for (int u = 0; u < U; ++u) sb[u] = sg_pack(signs + ((u * T + tid) << 3));
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const int64_t u0 = b * (N / 8);  // the block's first unit
        float v[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) sg_unpack<XDT>(sg_load(x, (u0 + u * T + tid) << 3, sb[u]), v[u]);
#include "ct_hadamard_block.inc"
        MinMax m[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            sg_round8<XDT>(v[u], sn);
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

// ---- host ----------------------------------------------------------------------------------------------------------------------------
constexpr int64_t kSignedMaxBlock = 8192;  // kRotMaxBlock of csrc/ct_rotated.hip
constexpr int64_t kSignedWavesPerCU = 16;  // what the capped grids keep resident: the rest of the rows are later rounds of the same signs

inline dim3 signed_grid(int64_t work, int64_t waves) {
    const int64_t cap = kCUs * kSignedWavesPerCU / waves;
    return dim3((unsigned)(work < cap ? work : cap));
}

template <int XDT, bool GS, int U, int WAVES>
static void launch_sg_block(const DynParams& p, void* rotated, const int8_t* signs, int64_t blocks, int lpg, HadScale<float> sn, hipStream_t s) {
    hipLaunchKernelGGL((sg_block_kernel<XDT, GS, U, WAVES>), signed_grid(blocks, WAVES), dim3(64 * WAVES), 0, s, p, rotated, signs, blocks, lpg, sn);
}

// __VA_ARGS__ with X the 16-bit activation dtype and G "a global scale is applied" as compile-time constants
#define CT_SIGNED_DISPATCH(xdt, gs, ...)                                        \
    for_dt16(xdt, [&](auto XD) {                                                \
        for_bool((gs) != nullptr, [&](auto GB) {                                \
            constexpr int X = decltype(XD)::value;                              \
            constexpr bool G = decltype(GB)::value;                             \
            __VA_ARGS__;                                                        \
        });                                                                     \
    })

}  // namespace ct

using namespace ct;

extern "C" {

int ct_hadamard_signed_dynamic_qdq(const void* x, int xdt, int64_t numel, int64_t n, const int8_t* signs, int64_t seg_len, int kind, int bits, int symmetric,
                                   const float* global_scale, void* rotated_out, void* out, void* scale_out, void* zp_out, int zdt, ct_stream_t stream) {
    CT_REQUIRE(n >= 1 && log2_exact(n) >= 0, "hadamard size %lld is not a power of two: the signed butterfly is the k == 1 rotation", (long long)n);
    CT_REQUIRE(seg_len >= 1 && numel >= 0 && numel % n == 0 && numel % seg_len == 0, "hadamard size %lld and segment length %lld do not both divide %lld elements",
               (long long)n, (long long)seg_len, (long long)numel);
    CT_REQUIRE(signs != nullptr, "signs is the int8 vector of n values +-1 (ct_hadamard_dynamic_qdq is the rotation without)");
    const int64_t L = seg_len, segs = numel / L;
    DynParams p;
    const int rc = fill_dyn(p, x, xdt, segs, L, kind, bits, symmetric, global_scale, out, scale_out, zp_out, zdt);
    if (rc) return rc;
    if (numel == 0) return CT_OK;
    if (xdt == CT_F32) CT_UNSUPPORTED("float32 activations take the two launches: the fused sign is a flip of a 16-bit word");
    if (!aligned16(x) || (out && !aligned16(out)) || (rotated_out && !aligned16(rotated_out))) CT_UNSUPPORTED("the fused rotation takes 16-byte aligned tensors");
    if (!aligned_to<8>(signs)) CT_UNSUPPORTED("the hadamard kernels take 8-byte aligned signs");
    if (n > kSignedMaxBlock) CT_UNSUPPORTED("hadamard size %lld exceeds the fused maximum %lld", (long long)n, (long long)kSignedMaxBlock);
    if (n < 8 || L % 8) CT_UNSUPPORTED("blocks of %lld and segments of %lld elements are not whole 16-byte units", (long long)n, (long long)L);
    const HadScale<float> sn = make_had_scale<float>(n);
    hipStream_t s = as_stream(stream);
    const int64_t upr = L / 8;
    const bool in_wave = upr <= 64 && log2_exact(upr) >= 0;  // dyn_group_kernel's segments
    if (n <= 512 && in_wave) {
        const int64_t units = numel / 8, tiles = cdiv64(units, (int64_t)kBlock * kHadGroupUnits);
        CT_SIGNED_DISPATCH(xdt, global_scale, hipLaunchKernelGGL((sg_group_kernel<X, G>), signed_grid(tiles, kBlock / 64), dim3(kBlock), 0, s, p, rotated_out, signs,
                                                                 units, tiles, (int)n, (int)upr, sn));
        CT_LAUNCH_CHECK("ct_hadamard_signed_dynamic_qdq[group]");
    }
    if (n <= 512) {
        if (segs == 1 && L > 512) CT_UNSUPPORTED("one segment of %lld elements is the tensor form: its reduction is global", (long long)L);
        if (L % n) CT_UNSUPPORTED("hadamard size %lld does not divide the segment length %lld", (long long)n, (long long)L);
        int64_t nt = cdiv64(cdiv64(upr, kSegUnits), 64) * 64;
        if (nt > kSegMaxThreads) nt = kSegMaxThreads;
        if (upr > nt * kSegUnits) CT_UNSUPPORTED("rows of %lld elements exceed the staged form (%d)", (long long)L, kSegMaxThreads * kSegUnits * 8);
        CT_SIGNED_DISPATCH(xdt, global_scale, hipLaunchKernelGGL((sg_seg_kernel<X, G>), signed_grid(segs, nt / 64), dim3((unsigned)nt), 0, s, p,
                                                                 static_cast<uint16_t*>(rotated_out), signs, (int)n, sn));
        CT_LAUNCH_CHECK("ct_hadamard_signed_dynamic_qdq[row]");
    }
    if (!(in_wave || L == n)) CT_UNSUPPORTED("a segment of %lld elements over workgroup-sized blocks of %lld is not fused", (long long)L, (long long)n);
    if (L == n && segs == 1) CT_UNSUPPORTED("one segment of %lld elements is the tensor form: its reduction is global", (long long)L);
    const int64_t blocks = numel / n;
    const int lpg = in_wave ? (int)upr : 0;
    switch (n) {
        case 1024: CT_SIGNED_DISPATCH(xdt, global_scale, (launch_sg_block<X, G, 2, 1>(p, rotated_out, signs, blocks, lpg, sn, s))); break;
        case 2048: CT_SIGNED_DISPATCH(xdt, global_scale, (launch_sg_block<X, G, 4, 1>(p, rotated_out, signs, blocks, lpg, sn, s))); break;
        case 4096: CT_SIGNED_DISPATCH(xdt, global_scale, (launch_sg_block<X, G, 4, 2>(p, rotated_out, signs, blocks, lpg, sn, s))); break;
        default: CT_SIGNED_DISPATCH(xdt, global_scale, (launch_sg_block<X, G, 4, 4>(p, rotated_out, signs, blocks, lpg, sn, s))); break;
    }
    CT_LAUNCH_CHECK("ct_hadamard_signed_dynamic_qdq[block]");
}

}  // extern "C"
