// ct_hadamard_perm.hip — the permuted Hadamard rotation of `TransformScheme.randomize=True` (transform/factory/hadamard.py:94-95:
// W' = W[p][:, p]) in one launch.  For every location, module type and `inverse`
//     T_W'(x) = G_p( T_W( G_q(x) ) )     with G_i(v)[j] = v[i[j]] and q = argsort(p):
// gather the block by q, run the rotation of ct_hadamard.hip (with the signs of form (a) of ct_hadamard_k.hip, when given),
// gather the result by p.  No n x n object; one read and one write of the tensor.
//
// Both gathers go through LDS; global access stays contiguous (16-byte loads and stores):
//   load    the raw 2- or 4-byte words of a block are written to LDS in the tensor's order; element k of a unit is then
//           the word at q[k] & (n - 1) of its block: one aligned 16-byte read of the table per unit, 8 scattered LDS reads
//   core    unit stages, lane stages, the U stages, the wave exchange with its fma signs, one division, one rounding — the stage
//           order of had_group_kernel / had_block_kernel exactly, so the launch computes the bits of the composition
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
constexpr int kHadPGroupUnits = 2;  // kHadGroupUnits

template <int XDT, typename A>
__global__ __launch_bounds__(kBlock) void hadp_group_kernel(const void* x, void* out, int64_t numel, int n, const uint16_t* __restrict__ gather_in,
                                                            const uint16_t* __restrict__ gather_out, const int8_t* __restrict__ signs, int transposed,
                                                            HadScale<A> sn) {
    typedef typename HadpWord<XDT>::type E;
    constexpr int U = kHadPGroupUnits;
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
#pragma unroll
        for (int u = 0; u < U; ++u) {
            unit_stages(v[u], 8);
            lane_stages(v[u], 64, lane);
            if constexpr (U >= 8) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int h = 1; h < U; h <<= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!(u & h)) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const A a = v[u][k], c = v[u | h][k];
                        v[u][k] = a + c;
                        v[u | h][k] = a - c;
                    }
                }
            }
        }
        if constexpr (WAVES > 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int c = 0; c < CPU; ++c) {
                    chunk_t w;
#pragma unroll
                    for (int e = 0; e < CH; ++e) w[e] = v[u][c * CH + e];
                    lds[(u * CPU + c) * T + tid] = w;
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int c = 0; c < CPU; ++c) {
                    chunk_t r = lds[(u * CPU + c) * T + lane];  // wave 0: sign + for every reader
#pragma unroll
                    for (int w = 1; w < WAVES; ++w) {
                        const chunk_t p = lds[(u * CPU + c) * T + w * 64 + lane];
                        const A sign = (__builtin_popcount(w & wave) & 1) ? (A)-1 : (A)1;  // wave-uniform
#pragma unroll
                        for (int e = 0; e < CH; ++e) r[e] = fma_t(p[e], sign, r[e]);
                    }
#pragma unroll
                    for (int e = 0; e < CH; ++e) v[u][c * CH + e] = r[e];
                    if constexpr (U >= 8) __builtin_amdgcn_sched_barrier(0);
                }
            }
            __syncthreads();  // the exchange is read: the output image overwrites it
        }
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

template <int XDT, typename A, int U, int WAVES>
static void launch_pblock(const void* x, void* out, int64_t blocks, const uint16_t* q, const uint16_t* p, const int8_t* signs, int transposed, HadScale<A> sn,
                          hipStream_t s) {
    const int64_t g = blocks < kMaxGridX ? blocks : kMaxGridX;
    hipLaunchKernelGGL((hadp_block_kernel<XDT, A, U, WAVES>), dim3((unsigned)g), dim3(64 * WAVES), 0, s, x, out, blocks, q, p, signs, transposed, sn);
}

template <int XDT, typename A>
static int launch_prows(const void* x, void* out, int64_t numel, int64_t n, const uint16_t* q, const uint16_t* p, const int8_t* signs, int transposed,
                        hipStream_t s) {
    HadScale<A> sn;
    sn.sn = (A)__builtin_sqrt((double)n);
    sn.rn = (A)1 / sn.sn;
    sn.mode = log2_exact(n) % 2 == 0 ? HAD_MUL : (sizeof(A) == 4 ? HAD_FAST : HAD_IEEE);
    if (n <= 512) {
        const int64_t g = cdiv64(cdiv64(numel, 8), (int64_t)kBlock * kHadPGroupUnits);
        CT_REQUIRE(g < ((int64_t)1 << 31), "tensor too large for one launch");
        hipLaunchKernelGGL((hadp_group_kernel<XDT, A>), dim3((unsigned)g), dim3(kBlock), 0, s, x, out, numel, (int)n, q, p, signs, transposed, sn);
        return CT_OK;
    }
    const int64_t blocks = numel / n;
    switch (n) {
        case 1024: launch_pblock<XDT, A, 2, 1>(x, out, blocks, q, p, signs, transposed, sn, s); break;
        case 2048: launch_pblock<XDT, A, 4, 1>(x, out, blocks, q, p, signs, transposed, sn, s); break;
        case 4096: launch_pblock<XDT, A, 4, 2>(x, out, blocks, q, p, signs, transposed, sn, s); break;
        case 8192: launch_pblock<XDT, A, 4, 4>(x, out, blocks, q, p, signs, transposed, sn, s); break;
        case 16384:
            // 64 float64 accumulators per thread beside the gathers spill (the compiler's resource report): declined in check_hadp
            if constexpr (sizeof(A) == 4) launch_pblock<XDT, A, 8, 4>(x, out, blocks, q, p, signs, transposed, sn, s);
            break;
        default: break;  // unreachable: check_hadp
    }
    return CT_OK;
}

static int check_hadp(const void* x, const void* out, int dt, int64_t numel, int64_t n, int acc64, const void* gather_in, const void* gather_out,
                      const int8_t* signs, int transposed) {
    CT_REQUIRE(is_float_dt(dt), "dtype code %d is not a float type", dt);
    CT_REQUIRE(n >= 1 && log2_exact(n) >= 0, "Cannot construct deterministic hadamard of size != 2^n");
    CT_REQUIRE(numel >= 0 && numel % n == 0, "hadamard size %lld does not divide %lld elements", (long long)n, (long long)numel);
    CT_REQUIRE(acc64 == 0 || acc64 == 1, "accumulator selector must be 0 (float32) or 1 (float64), got %d", acc64);
    CT_REQUIRE(transposed == 0 || transposed == 1, "transposed must be 0 or 1, got %d", transposed);
    CT_REQUIRE(gather_in != nullptr && gather_out != nullptr, "the permuted rotation needs both gather tables");
    if (n > (acc64 ? kHadPMaxF64 : kHadPMaxF32)) CT_UNSUPPORTED("hadamard size %lld exceeds the supported maximum %lld of the permuted rotation with the %s accumulator",
                                                               (long long)n, (long long)(acc64 ? kHadPMaxF64 : kHadPMaxF32), acc64 ? "float64" : "float32");
    if (!aligned16(x) || !aligned16(out)) CT_UNSUPPORTED("the hadamard kernels take 16-byte aligned tensors");
    if (!aligned16(gather_in) || !aligned16(gather_out)) CT_UNSUPPORTED("the hadamard kernels take 16-byte aligned gather tables");
    if (!aligned_to<8>(signs)) CT_UNSUPPORTED("the hadamard kernels take 8-byte aligned signs");
    return CT_OK;
}

static int dispatch_prows(const void* x, void* out, int dt, int64_t numel, int64_t n, int acc64, const void* gather_in, const void* gather_out,
                          const int8_t* signs, int transposed, hipStream_t s) {
    if (numel == 0) return CT_OK;
    const uint16_t* q = static_cast<const uint16_t*>(gather_in);
    const uint16_t* p = static_cast<const uint16_t*>(gather_out);
#define CT_HADP_ROWS(X) \
    (acc64 ? launch_prows<X, double>(x, out, numel, n, q, p, signs, transposed, s) : launch_prows<X, float>(x, out, numel, n, q, p, signs, transposed, s))
    const int rc = dt == CT_BF16 ? CT_HADP_ROWS(CT_BF16) : dt == CT_F16 ? CT_HADP_ROWS(CT_F16) : CT_HADP_ROWS(CT_F32);
#undef CT_HADP_ROWS
    return rc;
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
    CT_REQUIRE(rows >= 0 && cols >= 0, "bad matrix shape (%lld, %lld)", (long long)rows, (long long)cols);
    int rc = check_hadp(x, out, dt, rows, n, acc64, gather_in, gather_out, signs, transposed);  // n divides the ROWS
    if (rc) return rc;
    CT_REQUIRE(workspace != nullptr && aligned16(workspace), "ct_hadamard_perm_cols needs a 16-byte aligned workspace of rows * cols elements");
    if (rows == 0 || cols == 0) return CT_OK;
    CT_REQUIRE(cdiv64(rows, 64) * cdiv64(cols, 64) < ((int64_t)1 << 31), "matrix too large for one launch");
    hipStream_t s = as_stream(stream);
    launch_transpose_words(x, workspace, dt_size(dt), rows, cols, s);
    rc = hip_check(hipGetLastError(), "ct_hadamard_perm_cols[transpose]");
    if (rc) return rc;
    rc = dispatch_prows(workspace, workspace, dt, rows * cols, n, acc64, gather_in, gather_out, signs, transposed, s);  // in place: a block is in LDS before it is written
    if (rc) return rc;
    rc = hip_check(hipGetLastError(), "ct_hadamard_perm_cols[rows]");
    if (rc) return rc;
    launch_transpose_words(workspace, out, dt_size(dt), cols, rows, s);
    CT_LAUNCH_CHECK("ct_hadamard_perm_cols[transpose back]");
}

}  // extern "C"
