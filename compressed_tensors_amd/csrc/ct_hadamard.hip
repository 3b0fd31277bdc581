// ct_hadamard.hip — the Sylvester Hadamard rotation y = FWHT_n(x) / sqrt(n) (transform/factory/hadamard.py:91-108 with
// transform/utils/hadamard.py:21-50 and the block-diagonal `_multihead_matmul`, transform/utils/matrix.py:124-158) as a fast
// Walsh-Hadamard butterfly: log2 n additions per element instead of the reference's n, and no n x n matrix.
//
// x is a run of independent blocks of n consecutive elements (n a power of two).  Every stage of the butterfly pairs the two
// elements whose index differs in one bit, (a, b) -> (a + b, a - b); the stages commute, so each bit is handled where it lives:
//   bits 0..2    the 8 consecutive elements a lane loads with one 16-byte load (two for float32): registers
//   bits 3..8    the lane index inside the wave: DPP quad_perm (xor 1, 2), ds_swizzle (xor 4, 16), DPP row_ror:8 (xor 8) and
//                one bpermute (xor 32) — no LDS memory
//   next         the wave index inside the workgroup (WAVES = 1, 2, 4): ONE exchange through LDS, every thread reads the
//                other waves' value at its own position and adds it with the sign (-1)^popcount(w & w')
//   top bits     the U units a thread holds, n / U apart: registers
// The accumulator A is float (online rotations in float32) or double (fused, offline rotations: float64 upstream).  The sum is
// divided by sqrt(n) with ONE IEEE division in A (a multiplication by the reciprocal differs from the reference when n is not
// a power of 4) and rounded to the output dtype the way torch's cast does (double -> float -> bf16 / fp16).
//
// Kernels
//   had_group_kernel  n <= 512: n / 8 lanes own a block (n < 8: one lane owns 8 / n blocks), several blocks per wave
//   had_block_kernel  n = 1024 .. 16384: one workgroup of WAVES waves per block, U units per thread
//   transpose_kernel  the column form (transformed dimension is dim 0 of a rows x cols matrix): transpose into the workspace,
//                     row form in place, transpose back — 3 x the traffic of the row form, the same arithmetic
#include "ct_hadamard.h"

namespace ct {

// ---- n <= 512: lpb = max(n / 8, 1) lanes per block, U units per lane kBlock apart ------------------------------------------------
constexpr int kHadGroupUnits = 2;

template <int XDT, typename A>
__global__ __launch_bounds__(kBlock) void had_group_kernel(const void* x, void* out, int64_t numel, int n, HadScale<A> sn) {
    constexpr int U = kHadGroupUnits;
    const int64_t units = (numel + 7) >> 3;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
    const int lpb = n >> 3, lane = threadIdx.x & 63;
    A v[U][8];
    // numel is a multiple of n and kBlock of lpb: a block never straddles a wave, and every lane of a live block is live.
    // Dead lanes carry zeros through the exchanges (every lane executes them) and store nothing.
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int64_t u = base + (int64_t)i * kBlock;
        if (u < units) {
            had_load<XDT, A>(x, u << 3, numel, v[i]);
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
        if (u < units) had_store<XDT, A>(out, u << 3, numel, v[i], sn);
    }
}

// ---- n = 64 * WAVES * U * 8: one workgroup per block --------------------------------------------------------------------------------
template <int XDT, typename A, int U, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void had_block_kernel(const void* x, void* out, int64_t blocks, HadScale<A> sn) {
    constexpr int T = 64 * WAVES, N = T * U * 8;
    constexpr int CH = 16 / (int)sizeof(A), CPU = 8 / CH;  // elements of a 16-byte chunk, chunks per unit
    typedef A chunk_t __attribute__((ext_vector_type(CH)));
    // chunk c of unit u of thread t at ((u * CPU + c) * T + t): consecutive lanes 16 bytes apart, for the writes and for the reads
    __shared__ chunk_t lds[WAVES > 1 ? N / CH : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const int64_t e0 = b * N;
        A v[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) had_load<XDT, A>(x, e0 + ((int64_t)u * T + tid) * 8, e0 + N, v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            unit_stages(v[u], 8);
            lane_stages(v[u], 64, lane);
            if constexpr (U >= 8) __builtin_amdgcn_sched_barrier(0);  // one unit's exchanges at a time: 64 values per thread leave no room for more
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
            __syncthreads();  // lds is rewritten by the next block
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            had_store<XDT, A>(out, e0 + ((int64_t)u * T + tid) * 8, e0 + N, v[u], sn);
            if constexpr (U >= 8) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ---- out[c][r] = in[r][c] for elements of 2 or 4 bytes: 64 x 64 tiles through LDS ---------------------------------------------------
template <typename E>
__global__ __launch_bounds__(kBlock) void transpose_kernel(const E* __restrict__ in, E* __restrict__ out, int64_t rows, int64_t cols, int64_t tiles_c) {
    __shared__ E tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t r0 = ((int64_t)blockIdx.x / tiles_c) * 64, c0 = ((int64_t)blockIdx.x % tiles_c) * 64;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int64_t r = r0 + ty + 4 * j, c = c0 + tx;
        if (r < rows && c < cols) tile[ty + 4 * j][tx] = in[r * cols + c];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int64_t c = c0 + ty + 4 * j, r = r0 + tx;
        if (r < rows && c < cols) out[c * rows + r] = tile[tx][ty + 4 * j];
    }
}

template <int XDT, typename A, int U, int WAVES>
static void launch_block(const void* x, void* out, int64_t blocks, HadScale<A> sn, hipStream_t s) {
    const int64_t g = blocks < kMaxGridX ? blocks : kMaxGridX;
    hipLaunchKernelGGL((had_block_kernel<XDT, A, U, WAVES>), dim3((unsigned)g), dim3(64 * WAVES), 0, s, x, out, blocks, sn);
}

constexpr int64_t kHadMaxF32 = 16384, kHadMaxF64 = 16384;  // 64 values per thread at 4 waves; the forms tried for 32768 (8 x 8 waves, 16 x 4) spill

template <int XDT, typename A>
static int launch_rows(const void* x, void* out, int64_t numel, int64_t n, hipStream_t s) {
    HadScale<A> sn;
    sn.sn = (A)__builtin_sqrt((double)n);  // float32(sqrt(float64(n))), as the reference's `/ self._scale` in float32
    sn.rn = (A)1 / sn.sn;
    sn.mode = log2_exact(n) % 2 == 0 ? HAD_MUL : (sizeof(A) == 4 ? HAD_FAST : HAD_IEEE);
    if (n <= 512) {
        const int64_t g = cdiv64(cdiv64(numel, 8), (int64_t)kBlock * kHadGroupUnits);
        CT_REQUIRE(g < ((int64_t)1 << 31), "tensor too large for one launch");
        hipLaunchKernelGGL((had_group_kernel<XDT, A>), dim3((unsigned)g), dim3(kBlock), 0, s, x, out, numel, (int)n, sn);
        return CT_OK;
    }
    const int64_t blocks = numel / n;
    switch (n) {
        case 1024: launch_block<XDT, A, 2, 1>(x, out, blocks, sn, s); break;
        case 2048: launch_block<XDT, A, 4, 1>(x, out, blocks, sn, s); break;
        case 4096: launch_block<XDT, A, 4, 2>(x, out, blocks, sn, s); break;
        case 8192: launch_block<XDT, A, 4, 4>(x, out, blocks, sn, s); break;
        case 16384: launch_block<XDT, A, 8, 4>(x, out, blocks, sn, s); break;
        default: break;  // unreachable: check_had
    }
    return CT_OK;
}

static int check_had(const void* x, const void* out, int dt, int64_t numel, int64_t n, int acc64) {
    CT_REQUIRE(is_float_dt(dt), "dtype code %d is not a float type", dt);
    CT_REQUIRE(n >= 1 && log2_exact(n) >= 0, "Cannot construct deterministic hadamard of size != 2^n");
    CT_REQUIRE(numel >= 0 && numel % n == 0, "hadamard size %lld does not divide %lld elements", (long long)n, (long long)numel);
    CT_REQUIRE(acc64 == 0 || acc64 == 1, "accumulator selector must be 0 (float32) or 1 (float64), got %d", acc64);
    if (n > (acc64 ? kHadMaxF64 : kHadMaxF32)) CT_UNSUPPORTED("hadamard size %lld exceeds the supported maximum %lld of the %s accumulator", (long long)n,
                                                             (long long)(acc64 ? kHadMaxF64 : kHadMaxF32), acc64 ? "float64" : "float32");
    if (!aligned16(x) || !aligned16(out)) CT_UNSUPPORTED("the hadamard kernels take 16-byte aligned tensors");
    return CT_OK;
}

static int dispatch_rows(const void* x, void* out, int dt, int64_t numel, int64_t n, int acc64, hipStream_t s) {
    if (numel == 0) return CT_OK;
#define CT_HAD_ROWS(X) (acc64 ? launch_rows<X, double>(x, out, numel, n, s) : launch_rows<X, float>(x, out, numel, n, s))
    const int rc = dt == CT_BF16 ? CT_HAD_ROWS(CT_BF16) : dt == CT_F16 ? CT_HAD_ROWS(CT_F16) : CT_HAD_ROWS(CT_F32);
#undef CT_HAD_ROWS
    return rc;
}

template <typename E>
static void launch_transpose(const void* in, void* out, int64_t rows, int64_t cols, hipStream_t s) {
    const int64_t tc = cdiv64(cols, 64), g = cdiv64(rows, 64) * tc;
    hipLaunchKernelGGL((transpose_kernel<E>), dim3((unsigned)g), dim3(kBlock), 0, s, static_cast<const E*>(in), static_cast<E*>(out), rows, cols, tc);
}

void launch_transpose_words(const void* in, void* out, int elem_size, int64_t rows, int64_t cols, hipStream_t s) {
    if (elem_size == 4) launch_transpose<uint32_t>(in, out, rows, cols, s);
    else launch_transpose<uint16_t>(in, out, rows, cols, s);
}

}  // namespace ct

using namespace ct;

extern "C" {

int ct_hadamard_rows(const void* x, void* out, int dt, int64_t numel, int64_t n, int acc64, ct_stream_t stream) {
    int rc = check_had(x, out, dt, numel, n, acc64);
    if (rc) return rc;
    rc = dispatch_rows(x, out, dt, numel, n, acc64, as_stream(stream));
    if (rc) return rc;
    CT_LAUNCH_CHECK("ct_hadamard_rows");
}

int ct_hadamard_cols(const void* x, void* out, void* workspace, int dt, int64_t rows, int64_t cols, int64_t n, int acc64, ct_stream_t stream) {
    CT_REQUIRE(rows >= 0 && cols >= 0, "bad matrix shape (%lld, %lld)", (long long)rows, (long long)cols);
    int rc = check_had(x, out, dt, rows, n, acc64);  // n divides the ROWS
    if (rc) return rc;
    CT_REQUIRE(workspace != nullptr && aligned16(workspace), "ct_hadamard_cols needs a 16-byte aligned workspace of rows * cols elements");
    if (rows == 0 || cols == 0) return CT_OK;
    CT_REQUIRE(cdiv64(rows, 64) * cdiv64(cols, 64) < ((int64_t)1 << 31), "matrix too large for one launch");
    hipStream_t s = as_stream(stream);
    if (dt == CT_F32) launch_transpose<uint32_t>(x, workspace, rows, cols, s);
    else launch_transpose<uint16_t>(x, workspace, rows, cols, s);
    rc = hip_check(hipGetLastError(), "ct_hadamard_cols[transpose]");
    if (rc) return rc;
    rc = dispatch_rows(workspace, workspace, dt, rows * cols, n, acc64, s);  // in place: every element is read and written by one thread
    if (rc) return rc;
    rc = hip_check(hipGetLastError(), "ct_hadamard_cols[rows]");
    if (rc) return rc;
    if (dt == CT_F32) launch_transpose<uint32_t>(workspace, out, cols, rows, s);
    else launch_transpose<uint16_t>(workspace, out, cols, rows, s);
    CT_LAUNCH_CHECK("ct_hadamard_cols[transpose back]");
}

}  // extern "C"
