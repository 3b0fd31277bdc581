// ct_hadamard_k.hip — the random-hadamard rotation (transform/factory/random_hadamard.py with transform/utils/hadamard.py:53-151)
// of size n = K * M, M a power of two: the matrix is W = diag(s) * (hadK (x) H_M)^T with s the drawn +-1 vector, hadK a K x K
// +-1 matrix and H_M the Sylvester matrix in natural order.  A block of n elements is a K x M matrix (M contiguous):
//   plain       value @ W:    y = (hadK   (x) H_M)(s . x) / sqrt(n) — signs first
//   transposed  value @ W.T:  y = s . ((hadK^T (x) H_M) x) / sqrt(n) — signs last
// The Kronecker factors commute: the mix over k (hadK) and the butterfly over t (H_M) run in either order.
//
// Forms
//   (a) k == 1           the butterfly of ct_hadamard.hip with the signs at the load (plain) or before the store (transposed):
//                        hadk_group_kernel (n <= 512) and hadk_block_kernel (1024 .. 16384), float32 or float64 accumulators
//   (b) k > 1, 16-bit x, float32 accumulation, M = 8 .. 128: hadk_mfma_kernel, ONE launch, every element read and written once.
//                        The mix runs FIRST, on the matrix cores: hadK (+-1) and the raw 16-bit input (its sign bit flipped for
//                        the plain form) are exact operands of v_mfma_f32_32x32x16_{bf16,f16}.  The butterfly then runs in
//                        float32 on the accumulators (the column of an accumulator tile is the lane: lane_stages), then one IEEE
//                        division and one rounding; the transposed form flips the sign bit of the rounded word.
//   (c) k > 1 otherwise  (float32 x, float64 accumulation, M < 8 or M > 128): hadk_mix_kernel (one thread per output element,
//                        K terms, into the caller's workspace in the accumulator type) then hadk_runs_kernel (the butterfly over
//                        runs of M through LDS, signs, division, rounding).  Correctness first: the fused weight locations run
//                        once per checkpoint.
// sqrt(n) is none of the divisors HadScale's fast quotient was proven for when k > 1: those forms take the IEEE division.
#include "ct_hadamard.h"

namespace ct {

// ---- signs ---------------------------------------------------------------------------------------------------------------------------
// v[k] = signs[(e0 + k) & nmask] * v[k] as a flip of the sign bit: e0 is a multiple of 8, so for n >= 8 the 8 signs are one
// aligned 8-byte load (bit 7 of a byte: negative)
__device__ __forceinline__ void sign8(float (&v)[8], const int8_t* __restrict__ signs, int64_t e0, int nmask) {
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

// had_load / had_store of ct_hadamard.h with the signs on the float values: at the load for the plain form, on the rounded-to-float
// quotient for the transposed one (a sign commutes with the division and with every rounding)
template <int XDT, typename A>
__device__ __forceinline__ void hadk_load(const void* x, int64_t i0, int64_t numel, A (&v)[8], const int8_t* __restrict__ signs, int64_t e0, int nmask) {
    float f[8];
    if (i0 + 8 <= numel) {
        load8<XDT>(x, i0, f);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = i0 + k < numel ? load_as_f<XDT>(x, i0 + k) : 0.0f;
    }
    if (signs != nullptr) sign8(f, signs, e0, nmask);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (A)f[k];
}

template <int XDT, typename A>
__device__ __forceinline__ void hadk_store(void* out, int64_t i0, int64_t numel, const A (&v)[8], const HadScale<A>& sn, const int8_t* __restrict__ signs,
                                           int64_t e0, int nmask) {
    float f[8];
    had_div8(v, sn, f);
    if (signs != nullptr) sign8(f, signs, e0, nmask);
    if (i0 + 8 <= numel) {
        store8<XDT>(out, i0, f);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (i0 + k < numel) store1<XDT>(out, i0 + k, f[k]);
    }
}

// the sign bits of 8 16-bit words flipped where the sign is -1
__device__ __forceinline__ u32x4 flip8(u32x4 v, const int8_t* __restrict__ signs8) {
    const uint64_t w = *reinterpret_cast<const uint64_t*>(signs8);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t lo = (uint32_t)(w >> (16 * p + 7)) & 1u, hi = (uint32_t)(w >> (16 * p + 15)) & 1u;  // bit 7 of a byte: negative
        v[p] ^= (lo << 15) | (hi << 31);
    }
    return v;
}

// ---- (a) n <= 512: had_group_kernel with signs ------------------------------------------------------------------------------------------
template <int XDT, typename A>
__global__ __launch_bounds__(kBlock) void hadk_group_kernel(const void* x, void* out, int64_t numel, int n, const int8_t* __restrict__ signs,
                                                            int transposed, HadScale<A> sn) {
    constexpr int U = kHadGroupUnits;
    const int64_t units = (numel + 7) >> 3;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
    const int lpb = n >> 3, lane = threadIdx.x & 63;
    A v[U][8];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int64_t u = base + (int64_t)i * kBlock;
        if (u < units) {
            hadk_load<XDT, A>(x, u << 3, numel, v[i], transposed ? nullptr : signs, u << 3, n - 1);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[i][k] = (A)0;
        }
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
        unit_stages(v[i], n);
        lane_stages(v[i], lpb, lane);
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int64_t u = base + (int64_t)i * kBlock;
        if (u < units) {
            hadk_store<XDT, A>(out, u << 3, numel, v[i], sn, transposed ? signs : nullptr, u << 3, n - 1);
        }
    }
}

// ---- (a) n = 64 * WAVES * U * 8: had_block_kernel with signs (the same ct_hadamard_block.inc between the loads and the stores) ------------
template <int XDT, typename A, int U, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void hadk_block_kernel(const void* x, void* out, int64_t blocks, const int8_t* __restrict__ signs,
                                                                int transposed, HadScale<A> sn) {
    constexpr int T = 64 * WAVES, N = T * U * 8;
    constexpr int CH = 16 / (int)sizeof(A), CPU = 8 / CH;
    typedef A chunk_t __attribute__((ext_vector_type(CH)));
    __shared__ chunk_t lds[WAVES > 1 ? N / CH : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const int64_t e0 = b * N;
        A v[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            hadk_load<XDT, A>(x, e0 + ((int64_t)u * T + tid) * 8, e0 + N, v[u], transposed ? nullptr : signs, (int64_t)(u * T + tid) * 8, N - 1);
        }
#include "ct_hadamard_block.inc"
#pragma unroll
        for (int u = 0; u < U; ++u) {
            hadk_store<XDT, A>(out, e0 + ((int64_t)u * T + tid) * 8, e0 + N, v[u], sn, transposed ? signs : nullptr, (int64_t)(u * T + tid) * 8, N - 1);
            if constexpr (U >= 8) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ---- (b) the MFMA mix + butterfly ----------------------------------------------------------------------------------------------------
// One workgroup of ceil(K / 32) waves per group of G = max(32 / M, 1) consecutive blocks: C = G * M = 32 * TT columns c = (g, t).
//   load    16 bytes per thread; the row is staged TRANSPOSED, image[c][k] (k contiguous, the row stride KS * 16 + 8 elements: an
//           odd number of 16-byte chunks), so that a B fragment B[k = 16 s + 8 h + j][col] is ONE 16-byte LDS read.  Columns
//           K .. 16 KS - 1 are written as zeros every round: 0 * NaN is NaN, the pad must be real zeros.
//   mix     wave w holds rows 32 w .. 32 w + 31 of hadK (of hadK^T for the transposed form) as KS A fragments in registers for
//           the whole launch and runs KS MFMAs per tile of 32 columns
//   H_M     accumulator register r of lane l is (row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31): the butterfly over t is
//           lane_stages over the lane bits below min(M, 32), then additions between the TT tiles
//   store   quotient, one rounding, 2-byte LDS writes into an image in the OUTPUT's order (over the staged row, which every wave
//           has finished reading), then 16-byte non-temporal stores
constexpr int kHadKMaxK = 256, kHadKMaxSteps = kHadKMaxK / 16, kHadKMfmaMaxN = 32768, kHadKMaxLds = 65536;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int XDT>
__device__ __forceinline__ f32x16 mfma16(u32x4 a, u32x4 b, f32x16 c) {
    if constexpr (XDT == CT_BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

template <int XDT, int TT>
__global__ __launch_bounds__(512) void hadk_mfma_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ out, int64_t blocks, int n, int K,
                                                        int lm /*log2 M*/, const int8_t* __restrict__ had_k, const int8_t* __restrict__ signs,
                                                        int transposed, float sn) {
    extern __shared__ __attribute__((aligned(16))) uint16_t image[];
    constexpr int C = 32 * TT;
    constexpr uint32_t kOne = XDT == CT_BF16 ? 0x3F80u : 0x3C00u;
    const int M = 1 << lm, G = C >> lm;  // G == 1 for M >= 32
    const int KS = (K + 15) >> 4, LS = KS * 16 + 8;
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    u32x4 a[kHadKMaxSteps];
    {
        const int kp = 32 * wave + r;  // this lane's row of the mix
#pragma unroll
        for (int s = 0; s < kHadKMaxSteps; ++s) {
            uint32_t e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {  // branch-free: a clamped read, then the mask
                const int k = 16 * s + 8 * h + j, kc = k < K ? k : K - 1, kpc = kp < K ? kp : K - 1;
                const uint32_t v = kOne | ((had_k[transposed ? kc * K + kpc : kpc * K + kc] < 0) ? 0x8000u : 0u);
                e[j] = (kp < K && k < K) ? v : 0u;
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) a[s][p] = e[2 * p] | (e[2 * p + 1] << 16);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    const int units = (G * n) >> 3;  // 16-byte units of a group
    const int64_t groups = (blocks + G - 1) / G;
    for (int64_t gi = blockIdx.x; gi < groups; gi += gridDim.x) {
        const int64_t b0 = gi * G;
        // ---- load: signs (plain), transpose into image[c][k]
        for (int u = tid; u < units; u += T) {
            const int e = u << 3, g = e / n, rr = e - g * n, k = rr >> lm, t = rr & (M - 1);
            u32x4 w = {0, 0, 0, 0};
            if (b0 + g < blocks) {
                w = *reinterpret_cast<const u32x4*>(x + (b0 * n + e));
                if (signs != nullptr && !transposed) w = flip8(w, signs + rr);
            }
            uint16_t* col = image + ((g << lm) + t) * LS + k;
#pragma unroll
            for (int j = 0; j < 8; ++j) col[j * LS] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
        }
        const int pad = KS * 16 - K;
        for (int i = tid; i < C * pad; i += T) image[(i / pad) * LS + K + i % pad] = 0;
        __syncthreads();

        // ---- mix
        f32x16 acc[TT];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[tt][q] = 0.0f;
        const uint16_t* brow = image + r * LS + 8 * h;
#pragma unroll
        for (int s = 0; s < kHadKMaxSteps; ++s) {
            if (s < KS) {
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) acc[tt] = mfma16<XDT>(a[s], *reinterpret_cast<const u32x4*>(brow + 32 * tt * LS + 16 * s), acc[tt]);
            }
        }

        // ---- the butterfly over t: lane bits, then tiles
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
                    const f32x16 p = acc[tt], q = acc[tt | hh];
                    acc[tt] = p + q;
                    acc[tt | hh] = p - q;
                }
            }
        }
        __syncthreads();  // every wave has read the staged row

        // ---- quotient, rounding, the image in the output's order
        // (the lane's row and column pass through an empty asm: left visible, the 16 * TT addresses and row tests are loop
        // invariants, and hoisted out of the round loop they cost more registers than the accumulators)
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
        for (int u = tid; u < units; u += T) {
            const int e = u << 3, g = e / n;
            if (b0 + g < blocks) {
                u32x4 w = *reinterpret_cast<const u32x4*>(image + e);
                if (signs != nullptr && transposed) w = flip8(w, signs + (e - g * n));
                stream_store16(out + (b0 * n + e), w);
            }
        }
        __syncthreads();  // the image is rewritten by the next round
    }
}

// ---- (c) the mix on the vector ALU: ws[b][k'][t] = sum_k hadK[k'][k] * s[k][t] * x[b][k][t] in A ------------------------------------------
template <int XDT, typename A>
__global__ __launch_bounds__(kBlock) void hadk_mix_kernel(const void* __restrict__ x, A* __restrict__ ws, int64_t numel, int n, int K, int lm,
                                                          const int8_t* __restrict__ had_k, const int8_t* __restrict__ signs, int transposed) {
    const int M = 1 << lm;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < numel; i += (int64_t)gridDim.x * kBlock) {
        const int64_t b = i / n;
        const int rr = (int)(i - b * n), kp = rr >> lm, t = rr & (M - 1);
        A acc = (A)0;
        for (int k = 0; k < K; ++k) {
            const int j = (k << lm) + t;
            A v = (A)load_as_f<XDT>(x, b * n + j);
            A sg = (A)had_k[transposed ? k * K + kp : kp * K + k];
            if (signs != nullptr && !transposed) sg *= (A)signs[j];
            acc += sg * v;  // the product is exact: one rounding per term, as a sum
        }
        ws[i] = acc;
    }
}

// the butterfly over runs of M elements of ws through LDS (a workgroup takes max(M, 1024) elements), then the transposed form's signs,
// the IEEE division in A and the rounding through float, as torch's cast does
constexpr int kHadKRunsMaxM = 4096;

template <int XDT, typename A>
__global__ __launch_bounds__(kBlock) void hadk_runs_kernel(const A* __restrict__ ws, void* __restrict__ out, int64_t numel, int n, int lm,
                                                           const int8_t* __restrict__ signs, int transposed, A sn) {
    __shared__ A l[kHadKRunsMaxM];
    const int M = 1 << lm, CHUNK = M > 1024 ? M : 1024;
    const int64_t c0 = (int64_t)blockIdx.x * CHUNK;
    for (int i = threadIdx.x; i < CHUNK; i += kBlock) l[i] = c0 + i < numel ? ws[c0 + i] : (A)0;
    __syncthreads();
    for (int lh = 0; lh < lm; ++lh) {
        const int hh = 1 << lh;
        for (int p = threadIdx.x; p < CHUNK / 2; p += kBlock) {
            const int lo = ((p >> lh) << (lh + 1)) | (p & (hh - 1));
            const A u = l[lo], w = l[lo + hh];
            l[lo] = u + w;
            l[lo + hh] = u - w;
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < CHUNK; i += kBlock) {
        const int64_t e = c0 + i;
        if (e < numel) {
            A v = l[i];
            if (signs != nullptr && transposed) v *= (A)signs[e % n];
            store1<XDT>(out, e, (float)(v / sn));
        }
    }
}

// ---- (a), float64 accumulation: the signs as a pass of their own around ct_hadamard_rows (fused locations run once) ----------------------
template <typename E>
__global__ __launch_bounds__(kBlock) void hadk_flip_kernel(const E* in, E* out, int64_t numel, int nmask, const int8_t* __restrict__ signs) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < numel; i += (int64_t)gridDim.x * kBlock)
        out[i] = signs[i & nmask] < 0 ? (E)(in[i] ^ ((E)1 << (8 * sizeof(E) - 1))) : in[i];
}

static void launch_flip(const void* in, void* out, int dt, int64_t numel, int64_t n, const int8_t* signs, hipStream_t s) {
    const int64_t g = cdiv64(numel, kBlock);
    const dim3 grid((unsigned)(g < kMaxGridX ? g : kMaxGridX));
    if (dt == CT_F32) hipLaunchKernelGGL((hadk_flip_kernel<uint32_t>), grid, dim3(kBlock), 0, s, static_cast<const uint32_t*>(in), static_cast<uint32_t*>(out), numel, (int)(n - 1), signs);
    else hipLaunchKernelGGL((hadk_flip_kernel<uint16_t>), grid, dim3(kBlock), 0, s, static_cast<const uint16_t*>(in), static_cast<uint16_t*>(out), numel, (int)(n - 1), signs);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
enum { HADK_BUTTERFLY = 0, HADK_MFMA = 1, HADK_VALU = 2 };

static size_t mfma_lds_bytes(int64_t k, int64_t m) { return (size_t)(m > 32 ? m : 32) * (size_t)(cdiv64(k, 16) * 16 + 8) * 2; }

static int form_of(int dt, int64_t n, int64_t k, int acc64) {
    if (k == 1) return HADK_BUTTERFLY;
    const int64_t m = n / k;
    if (dt != CT_F32 && !acc64 && m >= 8 && m <= 128 && n <= kHadKMfmaMaxN && mfma_lds_bytes(k, m) <= (size_t)kHadKMaxLds) return HADK_MFMA;
    return HADK_VALU;
}

static int check_hadk(const void* x, const void* out, int dt, int64_t numel, int64_t n, int64_t k, const int8_t* had_k, const int8_t* signs, int transposed,
                      int acc64) {
    const int rc = check_had_common(
        x, out, dt, numel, n, acc64, transposed,
        [&]() -> int {
            CT_REQUIRE(n >= 1 && k >= 1 && n % k == 0 && log2_exact(n / k) >= 0, "hadamard size %lld is not %lld * 2^m", (long long)n, (long long)k);
            return CT_OK;
        },
        [&]() -> int {
            CT_REQUIRE((k == 1) == (had_k == nullptr), "had_k is the k x k mix for k > 1 and null for k == 1");
            if (k == 1 && n > kHadMaxF32) CT_UNSUPPORTED("hadamard size %lld exceeds the supported maximum %lld of the butterfly", (long long)n, (long long)kHadMaxF32);
            if (k > kHadKMaxK) CT_UNSUPPORTED("the mix takes k <= %d, got %lld", kHadKMaxK, (long long)k);
            if (k > 1 && n > kHadKMfmaMaxN) CT_UNSUPPORTED("hadamard size %lld exceeds the supported maximum %d of the mixed forms", (long long)n, kHadKMfmaMaxN);
            if (k > 1 && form_of(dt, n, k, acc64) == HADK_VALU && n / k > kHadKRunsMaxM)
                CT_UNSUPPORTED("the vector form takes runs of up to %d elements, got %lld", kHadKRunsMaxM, (long long)(n / k));
            return CT_OK;
        });
    if (rc) return rc;
    if (!aligned_to<8>(signs)) CT_UNSUPPORTED("the hadamard kernels take 8-byte aligned signs");
    return CT_OK;
}

// form (a) with float32 accumulation: the launch path of ct_hadamard.h around hadk_group_kernel / hadk_block_kernel
template <int XDT, typename A>
static int launch_butterfly(const void* x, void* out, int64_t numel, int64_t n, const int8_t* signs, int transposed, hipStream_t s) {
    return launch_had_rows<A>(
        numel, n,
        [&](dim3 grid, HadScale<A> sn) { hipLaunchKernelGGL((hadk_group_kernel<XDT, A>), grid, dim3(kBlock), 0, s, x, out, numel, (int)n, signs, transposed, sn); },
        [&](auto U, auto W, dim3 grid, int64_t blocks, HadScale<A> sn) {
            hipLaunchKernelGGL((hadk_block_kernel<XDT, A, U(), W()>), grid, dim3(64 * W()), 0, s, x, out, blocks, signs, transposed, sn);
        });
}

template <int XDT>
static int launch_mfma(const void* x, void* out, int64_t numel, int64_t n, int64_t k, const int8_t* had_k, const int8_t* signs, int transposed, hipStream_t s) {
    const int64_t m = n / k, blocks = numel / n, per = m >= 32 ? 1 : 32 / m, groups = cdiv64(blocks, per);
    const int64_t g = groups < 2 * kCUs ? groups : 2 * kCUs;  // the A fragments are loaded once per workgroup
    const dim3 grid((unsigned)g), block((unsigned)(64 * cdiv64(k, 32)));
    const size_t lds = mfma_lds_bytes(k, m);
    const float sn = (float)__builtin_sqrt((double)n);
    const uint16_t* xi = static_cast<const uint16_t*>(x);
    uint16_t* oi = static_cast<uint16_t*>(out);
    const int lm = log2_exact(m);
    if (m <= 32) hipLaunchKernelGGL((hadk_mfma_kernel<XDT, 1>), grid, block, lds, s, xi, oi, blocks, (int)n, (int)k, lm, had_k, signs, transposed, sn);
    else if (m == 64) hipLaunchKernelGGL((hadk_mfma_kernel<XDT, 2>), grid, block, lds, s, xi, oi, blocks, (int)n, (int)k, lm, had_k, signs, transposed, sn);
    else hipLaunchKernelGGL((hadk_mfma_kernel<XDT, 4>), grid, block, lds, s, xi, oi, blocks, (int)n, (int)k, lm, had_k, signs, transposed, sn);
    return CT_OK;
}

template <int XDT, typename A>
static int launch_valu(const void* x, void* out, int64_t numel, int64_t n, int64_t k, const int8_t* had_k, const int8_t* signs, int transposed, void* workspace,
                       hipStream_t s) {
    const int lm = log2_exact(n / k);
    A* ws = static_cast<A*>(workspace);
    const int64_t g1 = cdiv64(numel, kBlock), chunk = (n / k) > 1024 ? n / k : 1024, g2 = cdiv64(numel, chunk);
    CT_REQUIRE(g2 < ((int64_t)1 << 31), "tensor too large for one launch");
    hipLaunchKernelGGL((hadk_mix_kernel<XDT, A>), dim3((unsigned)(g1 < kMaxGridX ? g1 : kMaxGridX)), dim3(kBlock), 0, s, x, ws, numel, (int)n, (int)k, lm, had_k,
                       signs, transposed);
    const int rc = hip_check(hipGetLastError(), "ct_hadamard_k[mix]");
    if (rc) return rc;
    hipLaunchKernelGGL((hadk_runs_kernel<XDT, A>), dim3((unsigned)g2), dim3(kBlock), 0, s, ws, out, numel, (int)n, lm, signs, transposed,
                       (A)__builtin_sqrt((double)n));
    return CT_OK;
}

template <int XDT>
static int dispatch_dt(const void* x, void* out, int64_t numel, int64_t n, int64_t k, const int8_t* had_k, const int8_t* signs, int transposed, int acc64,
                       void* workspace, hipStream_t s) {
    const int form = form_of(XDT, n, k, acc64);
    if (form == HADK_BUTTERFLY) {
        if (!acc64) return launch_butterfly<XDT, float>(x, out, numel, n, signs, transposed, s);
        // float64: a flip of the sign bit is exact in any dtype and commutes with the division and the rounding
        if (!transposed) launch_flip(x, out, XDT, numel, n, signs, s);
        int rc = hip_check(hipGetLastError(), "ct_hadamard_k[signs]");
        if (rc) return rc;
        rc = ct_hadamard_rows(transposed ? x : out, out, XDT, numel, n, 1, reinterpret_cast<ct_stream_t>(s));  // in place: one thread reads and writes an element
        if (rc) return rc;
        if (transposed) launch_flip(out, out, XDT, numel, n, signs, s);
        return CT_OK;
    }
    if constexpr (XDT != CT_F32)
        if (form == HADK_MFMA) return launch_mfma<XDT>(x, out, numel, n, k, had_k, signs, transposed, s);
    CT_REQUIRE(workspace != nullptr && aligned16(workspace), "this form needs a 16-byte aligned workspace of numel accumulators");
    return acc64 ? launch_valu<XDT, double>(x, out, numel, n, k, had_k, signs, transposed, workspace, s)
                 : launch_valu<XDT, float>(x, out, numel, n, k, had_k, signs, transposed, workspace, s);
}

static int dispatch_k_rows(const void* x, void* out, int dt, int64_t numel, int64_t n, int64_t k, const int8_t* had_k, const int8_t* signs, int transposed,
                           int acc64, void* workspace, hipStream_t s) {
    if (numel == 0) return CT_OK;
    if (k == 1 && signs == nullptr) return ct_hadamard_rows(x, out, dt, numel, n, acc64, reinterpret_cast<ct_stream_t>(s));  // the Sylvester rotation itself
    int rc = CT_OK;
    for_dt(dt, [&](auto X) { rc = dispatch_dt<X()>(x, out, numel, n, k, had_k, signs, transposed, acc64, workspace, s); });
    return rc;
}

}  // namespace ct

using namespace ct;

extern "C" {

int ct_hadamard_k_rows(const void* x, void* out, int dt, int64_t numel, int64_t n, int64_t k, const int8_t* had_k, const int8_t* signs, int transposed, int acc64,
                       void* workspace, ct_stream_t stream) {
    int rc = check_hadk(x, out, dt, numel, n, k, had_k, signs, transposed, acc64);
    if (rc) return rc;
    rc = dispatch_k_rows(x, out, dt, numel, n, k, had_k, signs, transposed, acc64, workspace, as_stream(stream));
    if (rc) return rc;
    CT_LAUNCH_CHECK("ct_hadamard_k_rows");
}

int ct_hadamard_k_cols(const void* x, void* out, int dt, int64_t rows, int64_t cols, int64_t n, int64_t k, const int8_t* had_k, const int8_t* signs,
                       int transposed, int acc64, void* workspace, ct_stream_t stream) {
    hipStream_t s = as_stream(stream);
    return had_cols_form(
        "ct_hadamard_k_cols", "(ct_hadamard_k_workspace_bytes)", x, out, workspace, dt, rows, cols, s,
        [&] { return check_hadk(x, out, dt, rows, n, k, had_k, signs, transposed, acc64); },  // n divides the ROWS
        [&](void* w, int64_t numel) {  // in place: a block is read whole before it is written; behind the transposed tensor, the accumulators of the vector form
            void* rest = static_cast<char*>(w) + ((numel * dt_size(dt) + 15) & ~(int64_t)15);
            return dispatch_k_rows(w, w, dt, numel, n, k, had_k, signs, transposed, acc64, rest, s);
        });
}

int64_t ct_hadamard_k_workspace_bytes(int dt, int64_t numel, int64_t n, int64_t k, int acc64, int cols_form) {
    if (!is_float_dt(dt) || numel < 0 || n < 1 || k < 1 || n % k) return -1;
    const int64_t t = cols_form ? (numel * dt_size(dt) + 15) & ~(int64_t)15 : 0;
    return t + (form_of(dt, n, k, acc64) == HADK_VALU ? numel * (acc64 ? 8 : 4) : 0);
}

}  // extern "C"
