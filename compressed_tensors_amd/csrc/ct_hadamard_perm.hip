// ct_hadamard_perm.hip — the permuted Hadamard rotation of `TransformScheme.randomize=True` (transform/factory/hadamard.py:94-95:
// W' = W[p][:, p]) in one launch.  For every location, module type and `inverse`
//     T_W'(x) = G_p( T_W( G_q(x) ) )     with G_i(v)[j] = v[i[j]] and q = argsort(p):
// gather the block by q, run the rotation of ct_hadamard.hip (with the signs of form (a) of ct_hadamard_k.hip, when given),
// gather the result by p.  No n x n object; one read and one write of the tensor.
//
// Both gathers go through LDS; global access stays contiguous (16-byte loads and stores):
//   load    the raw 2- or 4-byte words of a block are written to LDS in the tensor's order; element k of a unit is then
//           the word at q[k] & (n - 1) of its block: one aligned 16-byte read of the table per unit, 8 scattered LDS reads
//   core    unit stages, lane stages, the U stages, the wave exchange with its fma signs (ct_hadamard_block.inc), one division, one
//           rounding — the stage order of had_group_kernel / had_block_kernel exactly, so the launch computes the bits of the composition
//           index_select(q) -> ct_hadamard_rows -> index_select(p)
//   store   the ROUNDED words go to LDS in natural order; output element j is the word at p[j] & (n - 1)
// The mask keeps every index inside the block whatever the table holds: the host validates the permutation once, the mask is what
// stands between a corrupted table and an access outside the block.
//
// Kernels
//   hadp_group_kernel  n <= 512: a block never straddles a wave, so a wave stages its own 512 elements and nothing but a wave
//                      barrier orders the exchange.  n < 8: the index of element e is (e & ~(n - 1)) + q[e & (n - 1)]
//   hadp_block_kernel  n = 1024 .. 16384: one workgroup per block.  The staging image (n words of the tensor's dtype) lies IN the
//                      exchange buffer of the parent (n accumulators), separated from it by workgroup barriers
// In-place is legal: every global load of a block (group form: of a wave's blocks) is in LDS before any of its stores is issued.
#include "ct_hadamard.h"

namespace ct {

template <int XDT>
struct HadpWord {
    typedef uint16_t type;
};
template <>
struct HadpWord<CT_F32> {
    typedef uint32_t type;
};

template <int XDT>
__device__ __forceinline__ float hadp_word_f(uint32_t w) {
    if constexpr (XDT == CT_F32) return bits_f(w);
    else if constexpr (XDT == CT_F16) return f16_bits_to_f(w);
    else return bf16_bits_to_f(w);
}

template <int XDT>
__device__ __forceinline__ uint32_t hadp_f_word(float v) {
    if constexpr (XDT == CT_F32) return f_bits(v);
    else if constexpr (XDT == CT_F16) return f_to_f16_bits(v);
    else return f_to_bf16_bits(v);
}

// sign8 of csrc/ct_hadamard_k.hip: v[k] = signs[(e0 + k) & nmask] * v[k] as a flip of the sign bit
__device__ __forceinline__ void hadp_sign8(float (&v)[8], const int8_t* __restrict__ signs, int64_t e0, int nmask) {
    uint64_t w = 0;
    if (nmask >= 7) {
        w = *reinterpret_cast<const uint64_t*>(signs + (e0 & nmask));
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) w |= (uint64_t)(uint8_t)signs[(e0 + k) & nmask] << (8 * k);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = bits_f(f_bits(v[k]) ^ (((uint32_t)(w >> (8 * k + 7)) & 1u) << 31));
}

// the 8 words of the unit at word offset e0 (a multiple of 8) of an LDS image whose blocks of n = nmask + 1 words start at
// multiples of n, taken through the table: word k is image[block + (table[(e0 + k) & nmask] & nmask)]
template <typename E>
__device__ __forceinline__ void hadp_gather8(const E* image, int e0, int nmask, const uint16_t* __restrict__ table, uint32_t (&w)[8]) {
    if (nmask >= 7) {
        const u32x4 t = *reinterpret_cast<const u32x4*>(table + (e0 & nmask));
        const E* block = image + (e0 & ~nmask);
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = block[(t[k >> 1] >> (16 * (k & 1))) & (uint32_t)nmask];
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = e0 + k;
            w[k] = image[(e & ~nmask) + (table[e & nmask] & nmask)];
        }
    }
}

// 8 words -> 8 consecutive LDS words at a 16-byte aligned position
template <typename E>
__device__ __forceinline__ void hadp_put8(E* dst, const uint32_t (&w)[8]) {
    if constexpr (sizeof(E) == 4) {
        reinterpret_cast<u32x4*>(dst)[0] = u32x4{w[0], w[1], w[2], w[3]};
        reinterpret_cast<u32x4*>(dst)[1] = u32x4{w[4], w[5], w[6], w[7]};
    } else {
        reinterpret_cast<u32x4*>(dst)[0] = u32x4{w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16)};
    }
}

// global -> LDS, the raw words of the unit at element i0: 16-byte loads inside the tensor, zeros past its end
template <typename E>
__device__ __forceinline__ void hadp_stage8(const void* x, int64_t i0, int64_t numel, E* dst) {
    const E* src = static_cast<const E*>(x) + i0;
    if (i0 + 8 <= numel) {
#pragma unroll
        for (int j = 0; j < (int)sizeof(E) / 2; ++j) reinterpret_cast<u32x4*>(dst)[j] = reinterpret_cast<const u32x4*>(src)[j];
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = i0 + k < numel ? src[k] : (E)0;
    }
}

// 8 words -> global at element i0: 16-byte non-temporal stores (store8 of ct_common.h), single words in the last, partial unit
template <typename E>
__device__ __forceinline__ void hadp_store8(void* out, int64_t i0, int64_t numel, const uint32_t (&w)[8]) {
    E* dst = static_cast<E*>(out) + i0;
    if (i0 + 8 <= numel) {
        if constexpr (sizeof(E) == 4) {
            stream_store16(dst, u32x4{w[0], w[1], w[2], w[3]});
            stream_store16(dst + 4, u32x4{w[4], w[5], w[6], w[7]});
        } else {
            stream_store16(dst, u32x4{w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16)});
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (i0 + k < numel) dst[k] = (E)w[k];
    }
}

// words of the gathered unit -> accumulators, with the plain form's signs at natural positions
template <int XDT, typename A>
__device__ __forceinline__ void hadp_unpack(const uint32_t (&w)[8], A (&v)[8], const int8_t* __restrict__ signs, int64_t e0, int nmask) {
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = hadp_word_f<XDT>(w[k]);
    if (signs != nullptr) hadp_sign8(f, signs, e0, nmask);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (A)f[k];
}

// accumulators -> the rounded words of had_store (one division, the transposed form's signs, one rounding through float)
template <int XDT, typename A>
__device__ __forceinline__ void hadp_pack(const A (&v)[8], const HadScale<A>& sn, const int8_t* __restrict__ signs, int64_t e0, int nmask, uint32_t (&w)[8]) {
    float f[8];
    had_div8(v, sn, f);
    if (signs != nullptr) hadp_sign8(f, signs, e0, nmask);
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = hadp_f_word<XDT>(f[k]);
}

// the LDS writes of a wave are visible to its own later reads: no workgroup barrier
__device__ __forceinline__ void hadp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- n <= 512: had_group_kernel between two wave-private gathers ------------------------------------------------------------------------
template <int XDT, typename A>
__global__ __launch_bounds__(kBlock) void hadp_group_kernel(const void* x, void* out, int64_t numel, int n, const uint16_t* __restrict__ gather_in,
                                                            const uint16_t* __restrict__ gather_out, const int8_t* __restrict__ signs, int transposed,
                                                            HadScale<A> sn) {
    typedef typename HadpWord<XDT>::type E;
    constexpr int U = kHadGroupUnits;
    // image[i][wave]: the 512 words the wave holds in unit slot i, in the tensor's order
    __shared__ __attribute__((aligned(16))) E image[U][kBlock / 64][512];
    const int64_t base = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
    const int lpb = n >> 3, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nmask = n - 1;
    // numel is a multiple of n and kBlock of lpb: a block never straddles a wave.  Lanes past the end stage zeros, take part in
    // every exchange and store nothing.
#pragma unroll
    for (int i = 0; i < U; ++i) hadp_stage8<E>(x, (base + (int64_t)i * kBlock) << 3, numel, &image[i][wave][lane * 8]);
    hadp_wave_sync();
    A v[U][8];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        uint32_t w[8];
        hadp_gather8<E>(image[i][wave], lane * 8, nmask, gather_in, w);
        hadp_unpack<XDT, A>(w, v[i], transposed ? nullptr : signs, (base + (int64_t)i * kBlock) << 3, nmask);
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
        unit_stages(v[i], n);
        lane_stages(v[i], lpb, lane);
    }
    hadp_wave_sync();  // every lane has read the staged input
#pragma unroll
    for (int i = 0; i < U; ++i) {
        uint32_t w[8];
        hadp_pack<XDT, A>(v[i], sn, transposed ? signs : nullptr, (base + (int64_t)i * kBlock) << 3, nmask, w);
        hadp_put8<E>(&image[i][wave][lane * 8], w);
    }
    hadp_wave_sync();
#pragma unroll
    for (int i = 0; i < U; ++i) {
        uint32_t w[8];
        hadp_gather8<E>(image[i][wave], lane * 8, nmask, gather_out, w);
        hadp_store8<E>(out, (base + (int64_t)i * kBlock) << 3, numel, w);
    }
}

// ---- n = 64 * WAVES * U * 8: had_block_kernel between two gathers through the exchange buffer ---------------------------------------------
template <int XDT, typename A, int U, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void hadp_block_kernel(const void* x, void* out, int64_t blocks, const uint16_t* __restrict__ gather_in,
                                                                const uint16_t* __restrict__ gather_out, const int8_t* __restrict__ signs,
                                                                int transposed, HadScale<A> sn) {
    typedef typename HadpWord<XDT>::type E;
    constexpr int T = 64 * WAVES, N = T * U * 8;
    constexpr int CH = 16 / (int)sizeof(A), CPU = 8 / CH;
    typedef A chunk_t __attribute__((ext_vector_type(CH)));
    // the exchange buffer of had_block_kernel (N accumulators; none for one wave) and, in its place, the image of N words
    __shared__ __attribute__((aligned(16))) unsigned char raw[WAVES > 1 ? N * sizeof(A) : N * sizeof(E)];
    chunk_t* lds = reinterpret_cast<chunk_t*>(raw);
    E* image = reinterpret_cast<E*>(raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const int64_t e0 = b * N;
#pragma unroll
        for (int u = 0; u < U; ++u) hadp_stage8<E>(x, e0 + ((int64_t)u * T + tid) * 8, e0 + N, image + (u * T + tid) * 8);
        __syncthreads();
        A v[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            uint32_t w[8];
            hadp_gather8<E>(image, (u * T + tid) * 8, N - 1, gather_in, w);
            hadp_unpack<XDT, A>(w, v[u], transposed ? nullptr : signs, (int64_t)(u * T + tid) * 8, N - 1);
            if constexpr (U >= 8) __builtin_amdgcn_sched_barrier(0);  // one unit's gather at a time, as the stages below
        }
        __syncthreads();  // the image is read: the exchange and the output image overwrite it
#include "ct_hadamard_block.inc"  // WAVES > 1: its last barrier stands between the reads of the exchange and the output image laid over it
#pragma unroll
        for (int u = 0; u < U; ++u) {
            uint32_t w[8];
            hadp_pack<XDT, A>(v[u], sn, transposed ? signs : nullptr, (int64_t)(u * T + tid) * 8, N - 1, w);
            hadp_put8<E>(image + (u * T + tid) * 8, w);
            if constexpr (U >= 8) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            uint32_t w[8];
            hadp_gather8<E>(image, (u * T + tid) * 8, N - 1, gather_out, w);
            hadp_store8<E>(out, e0 + ((int64_t)u * T + tid) * 8, e0 + N, w);
            if constexpr (U >= 8) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // the image is rewritten by the next block
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
constexpr int64_t kHadPMaxF32 = 16384, kHadPMaxF64 = 8192;  // float64 at 16384 spills here (it does not in the parent): the composition takes it

// the launch path of ct_hadamard.h around this file's two kernels
template <int XDT, typename A>
static int launch_prows(const void* x, void* out, int64_t numel, int64_t n, const uint16_t* q, const uint16_t* p, const int8_t* signs, int transposed,
                        hipStream_t s) {
    return launch_had_rows<A>(
        numel, n,
        [&](dim3 grid, HadScale<A> sn) { hipLaunchKernelGGL((hadp_group_kernel<XDT, A>), grid, dim3(kBlock), 0, s, x, out, numel, (int)n, q, p, signs, transposed, sn); },
        [&](auto U, auto W, dim3 grid, int64_t blocks, HadScale<A> sn) {
            // n = 16384: 64 float64 accumulators per thread beside the gathers spill (the compiler's resource report): declined in check_hadp
            if constexpr (U() < 8 || sizeof(A) == 4)
                hipLaunchKernelGGL((hadp_block_kernel<XDT, A, U(), W()>), grid, dim3(64 * W()), 0, s, x, out, blocks, q, p, signs, transposed, sn);
        });
}

static int check_hadp(const void* x, const void* out, int dt, int64_t numel, int64_t n, int acc64, const void* gather_in, const void* gather_out,
                      const int8_t* signs, int transposed) {
    const int rc = check_had_common(
        x, out, dt, numel, n, acc64, transposed,
        [&]() -> int {
            CT_REQUIRE(n >= 1 && log2_exact(n) >= 0, "Cannot construct deterministic hadamard of size != 2^n");
            return CT_OK;
        },
        [&]() -> int {
            CT_REQUIRE(gather_in != nullptr && gather_out != nullptr, "the permuted rotation needs both gather tables");
            if (n > (acc64 ? kHadPMaxF64 : kHadPMaxF32))
                CT_UNSUPPORTED("hadamard size %lld exceeds the supported maximum %lld of the permuted rotation with the %s accumulator", (long long)n,
                               (long long)(acc64 ? kHadPMaxF64 : kHadPMaxF32), acc64 ? "float64" : "float32");
            return CT_OK;
        });
    if (rc) return rc;
    if (!aligned16(gather_in) || !aligned16(gather_out)) CT_UNSUPPORTED("the hadamard kernels take 16-byte aligned gather tables");
    if (!aligned_to<8>(signs)) CT_UNSUPPORTED("the hadamard kernels take 8-byte aligned signs");
    return CT_OK;
}

static int dispatch_prows(const void* x, void* out, int dt, int64_t numel, int64_t n, int acc64, const void* gather_in, const void* gather_out,
                          const int8_t* signs, int transposed, hipStream_t s) {
    if (numel == 0) return CT_OK;
    const uint16_t* q = static_cast<const uint16_t*>(gather_in);
    const uint16_t* p = static_cast<const uint16_t*>(gather_out);
    return for_had_types(dt, acc64, [&](auto X, auto a) { return launch_prows<X(), decltype(a)>(x, out, numel, n, q, p, signs, transposed, s); });
}

}  // namespace ct

using namespace ct;

extern "C" {

int ct_hadamard_perm_rows(const void* x, void* out, int dt, int64_t numel, int64_t n, int acc64, const void* gather_in, const void* gather_out,
                          const int8_t* signs, int transposed, ct_stream_t stream) {
    int rc = check_hadp(x, out, dt, numel, n, acc64, gather_in, gather_out, signs, transposed);
    if (rc) return rc;
    rc = dispatch_prows(x, out, dt, numel, n, acc64, gather_in, gather_out, signs, transposed, as_stream(stream));
    if (rc) return rc;
    CT_LAUNCH_CHECK("ct_hadamard_perm_rows");
}

int ct_hadamard_perm_cols(const void* x, void* out, void* workspace, int dt, int64_t rows, int64_t cols, int64_t n, int acc64, const void* gather_in,
                          const void* gather_out, const int8_t* signs, int transposed, ct_stream_t stream) {
    hipStream_t s = as_stream(stream);
    // had_cols_form of ct_hadamard.h: launch_transpose_words, the row form in place (a block is in LDS before it is written), launch_transpose_words
    return had_cols_form(
        "ct_hadamard_perm_cols", "of rows * cols elements", x, out, workspace, dt, rows, cols, s,
        [&] { return check_hadp(x, out, dt, rows, n, acc64, gather_in, gather_out, signs, transposed); },  // n divides the ROWS
        [&](void* w, int64_t numel) { return dispatch_prows(w, w, dt, numel, n, acc64, gather_in, gather_out, signs, transposed, s); });
}

}  // extern "C"
