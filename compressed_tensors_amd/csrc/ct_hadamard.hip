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
//   had_block_kernel  n = 1024 .. 16384: one workgroup of WAVES waves per block, U units per thread; the stages between its loads and its
//                     stores are ct_hadamard_block.inc, shared with the block kernels of ct_hadamard_k.hip, ct_hadamard_perm.hip and ct_rotated.hip
//   transpose_kernel  the column form (transformed dimension is dim 0 of a rows x cols matrix): transpose into the workspace,
//                     row form in place, transpose back — 3 x the traffic of the row form, the same arithmetic
#include "ct_hadamard.h"

namespace ct {

// ---- n <= 512: lpb = max(n / 8, 1) lanes per block, U units per lane kBlock apart ------------------------------------------------
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
    __shared__ chunk_t lds[WAVES > 1 ? N / CH : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const int64_t e0 = b * N;
        A v[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) had_load<XDT, A>(x, e0 + ((int64_t)u * T + tid) * 8, e0 + N, v[u]);
#include "ct_hadamard_block.inc"
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

// ---- host: the launch path of ct_hadamard.h around this file's two kernels -----------------------------------------------------------------
template <int XDT, typename A>
static int launch_rows(const void* x, void* out, int64_t numel, int64_t n, hipStream_t s) {
    return launch_had_rows<A>(
        numel, n, [&](dim3 grid, HadScale<A> sn) { hipLaunchKernelGGL((had_group_kernel<XDT, A>), grid, dim3(kBlock), 0, s, x, out, numel, (int)n, sn); },
        [&](auto U, auto W, dim3 grid, int64_t blocks, HadScale<A> sn) {
            hipLaunchKernelGGL((had_block_kernel<XDT, A, U(), W()>), grid, dim3(64 * W()), 0, s, x, out, blocks, sn);
        });
}

static int check_had(const void* x, const void* out, int dt, int64_t numel, int64_t n, int acc64) {
    return check_had_common(
        x, out, dt, numel, n, acc64, 0,
        [&]() -> int {
            CT_REQUIRE(n >= 1 && log2_exact(n) >= 0, "Cannot construct deterministic hadamard of size != 2^n");
            return CT_OK;
        },
        [&]() -> int {
            if (n > (acc64 ? kHadMaxF64 : kHadMaxF32)) CT_UNSUPPORTED("hadamard size %lld exceeds the supported maximum %lld of the %s accumulator", (long long)n,
                                                                     (long long)(acc64 ? kHadMaxF64 : kHadMaxF32), acc64 ? "float64" : "float32");
            return CT_OK;
        });
}

static int dispatch_rows(const void* x, void* out, int dt, int64_t numel, int64_t n, int acc64, hipStream_t s) {
    if (numel == 0) return CT_OK;
    return for_had_types(dt, acc64, [&](auto X, auto a) { return launch_rows<X(), decltype(a)>(x, out, numel, n, s); });
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
    hipStream_t s = as_stream(stream);
    return had_cols_form(
        "ct_hadamard_cols", "of rows * cols elements", x, out, workspace, dt, rows, cols, s, [&] { return check_had(x, out, dt, rows, n, acc64); },  // n divides the ROWS
        [&](void* w, int64_t numel) { return dispatch_rows(w, w, dt, numel, n, acc64, s); });  // in place: every element is read and written by one thread
}

}  // extern "C"
