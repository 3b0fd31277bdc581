// ct_hadamard.h — what the rotation files share (csrc/ct_hadamard.hip, ct_hadamard_k.hip, ct_hadamard_perm.hip, ct_rotated.hip, ct_attn_rot.hip).
// Device: the lane exchanges, the butterfly stages, the 1 / sqrt(n) quotient; the block butterfly itself is csrc/ct_hadamard_block.inc.
// Host: the scale, the n -> (U, WAVES) table, the grids, the shared argument checks and the column-form driver.
#pragma once
#include "ct_common.h"

namespace ct {

template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}

// the 32-bit value of lane (id ^ M)
template <int M>
__device__ __forceinline__ int lane_xor_i(int v) {
    if constexpr (M == 1) return dpp_i<0xB1>(v);                                // quad_perm [1,0,3,2]
    else if constexpr (M == 2) return dpp_i<0x4E>(v);                           // quad_perm [2,3,0,1]
    else if constexpr (M == 4) return __builtin_amdgcn_ds_swizzle(v, 0x101F);   // bit mode: and 0x1f, or 0, xor 4
    else if constexpr (M == 8) return dpp_i<0x128>(v);                          // row_ror:8 == xor 8 inside a row of 16
    else if constexpr (M == 16) return __builtin_amdgcn_ds_swizzle(v, 0x401F);  // xor 16
    else return __shfl_xor(v, 32, 64);
}

template <int M>
__device__ __forceinline__ float lane_xor(float v) {
    return __builtin_bit_cast(float, lane_xor_i<M>(__builtin_bit_cast(int, v)));
}

template <int M>
__device__ __forceinline__ double lane_xor(double v) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)lane_xor_i<M>((int)(uint32_t)b), hi = (uint32_t)lane_xor_i<M>((int)(uint32_t)(b >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// one butterfly stage across the lanes whose index differs in bit M: the lower lane keeps a + b, the upper one a - b.  Both are
// partner + sign * own with sign = +-1 — one fma, exact in the product, rounded once like the addition it replaces
template <int M, typename A>
__device__ __forceinline__ void lane_stage(A (&v)[8], bool upper) {
    const A sign = upper ? (A)-1 : (A)1;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = fma_t(v[k], sign, lane_xor<M>(v[k]));
}

// the stages of the lane bits below `lpb` (lanes per block, a power of two <= 64; uniform over the launch)
template <typename A>
__device__ __forceinline__ void lane_stages(A (&v)[8], int lpb, int lane) {
    if (lpb > 1) lane_stage<1>(v, lane & 1);
    if (lpb > 2) lane_stage<2>(v, lane & 2);
    if (lpb > 4) lane_stage<4>(v, lane & 4);
    if (lpb > 8) lane_stage<8>(v, lane & 8);
    if (lpb > 16) lane_stage<16>(v, lane & 16);
    if (lpb > 32) lane_stage<32>(v, lane & 32);
}

// the stages inside a unit: element bits below n (n >= 8: all three)
template <typename A>
__device__ __forceinline__ void unit_stages(A (&v)[8], int n) {
#pragma unroll
    for (int h = 1; h < 8; h <<= 1) {
        if (h < n) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!(k & h)) {
                    const A a = v[k], b = v[k | h];
                    v[k] = a + b;
                    v[k | h] = a - b;
                }
            }
        }
    }
}

template <int XDT, typename A>
__device__ __forceinline__ void had_load(const void* x, int64_t i0, int64_t numel, A (&v)[8]) {
    float f[8];
    if (i0 + 8 <= numel) {
        load8<XDT>(x, i0, f);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = i0 + k < numel ? load_as_f<XDT>(x, i0 + k) : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (A)f[k];
}

// v / sqrt(n), correctly rounded, for the divisor every thread shares.  sqrt(n) is 2^k (n a power of 4) or fl(2^k * sqrt 2):
//   HAD_MUL   2^k: v * 2^-k is the same correctly rounded quotient, one multiplication
//   HAD_FAST  float, fl(2^k * sqrt 2): q = fl(v * r), e = v - q * sn (exact, one fma), q' = fl(q + e * r) with r = fl(1 / sn) —
//             Markstein's correction step; checked over all 2^23 significands of v (two binades) against the IEEE quotient on the
//             CPU and by tests/test_gpu_hadamard.py on the GPU.  Scaling by 2^k commutes with every step while nothing under- or
//             overflows: a unit (8 values) that holds a zero, |v| < 2^-90, |v| > 2^100, inf or NaN takes the IEEE division (3 instructions against ~11)
//   HAD_IEEE  the division itself (double, fl(2^k * sqrt 2))
enum { HAD_MUL = 0, HAD_FAST = 1, HAD_IEEE = 2 };

template <typename A>
struct HadScale {
    A sn, rn;  // fl(sqrt n) and fl(1 / sn)
    int mode;
};

// the 8 quotients of a unit; the mode is uniform over the launch, the range test of HAD_FAST is per lane (one branch per unit)
__device__ __forceinline__ void had_div8(const float (&v)[8], const HadScale<float>& s, float (&f)[8]) {
    if (s.mode == HAD_MUL) {
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = v[k] * s.rn;
        return;
    }
    float lo = __builtin_inff(), hi = 0.0f;  // a NaN fails `lo >=`: fminf / fmaxf would drop it, so it is counted separately
    bool nan = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float a = __builtin_fabsf(v[k]);
        lo = __builtin_fminf(lo, a);
        hi = __builtin_fmaxf(hi, a);
        nan |= v[k] != v[k];
    }
    if (!nan && lo >= 0x1p-90f && hi <= 0x1p100f) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float q = v[k] * s.rn;
            f[k] = __builtin_fmaf(__builtin_fmaf(-q, s.sn, v[k]), s.rn, q);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = v[k] / s.sn;
    }
}

__device__ __forceinline__ void had_div8(const double (&v)[8], const HadScale<double>& s, float (&f)[8]) {
    if (s.mode == HAD_MUL) {
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = (float)(v[k] * s.rn);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = (float)(v[k] / s.sn);
    }
}

// divide by sqrt(n) in A, round as torch's cast does (through float) and store
template <int XDT, typename A>
__device__ __forceinline__ void had_store(void* out, int64_t i0, int64_t numel, const A (&v)[8], const HadScale<A>& sn) {
    float f[8];
    had_div8(v, sn, f);
    if (i0 + 8 <= numel) {
        store8<XDT>(out, i0, f);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (i0 + k < numel) store1<XDT>(out, i0 + k, f[k]);
    }
}

// ---- host: the launch path the rotation entries share (ct_hadamard.hip, ct_hadamard_k.hip, ct_hadamard_perm.hip; the scale and the grids also
// ct_rotated.hip and ct_attn_rot.hip) ------------------------------------------------------------------------------------------------------
constexpr int kHadGroupUnits = 2;  // units per lane, kBlock apart, of every group kernel (n <= 512); also the U of ct_dynamic_qdq's group launch
constexpr int64_t kHadMaxF32 = 16384, kHadMaxF64 = 16384;  // 64 values per thread at 4 waves; the forms tried for 32768 (8 x 8 waves, 16 x 4) spill

template <typename A>
inline HadScale<A> make_had_scale(int64_t n) {
    HadScale<A> sn;
    sn.sn = (A)__builtin_sqrt((double)n);  // float32(sqrt(float64(n))), as the reference's `/ self._scale` in float32
    sn.rn = (A)1 / sn.sn;
    sn.mode = log2_exact(n) % 2 == 0 ? HAD_MUL : (sizeof(A) == 4 ? HAD_FAST : HAD_IEEE);  // n is a power of two: the divisors HadScale was proven for
    return sn;
}

// n = 1024 .. 16384 -> f(U, WAVES) with the block kernels' units per thread and waves as compile-time constants (n = 64 * WAVES * U * 8)
template <typename F>
inline void for_had_block(int64_t n, F&& f) {
    using std::integral_constant;
    switch (n) {
        case 1024: f(integral_constant<int, 2>{}, integral_constant<int, 1>{}); break;
        case 2048: f(integral_constant<int, 4>{}, integral_constant<int, 1>{}); break;
        case 4096: f(integral_constant<int, 4>{}, integral_constant<int, 2>{}); break;
        case 8192: f(integral_constant<int, 4>{}, integral_constant<int, 4>{}); break;
        case 16384: f(integral_constant<int, 8>{}, integral_constant<int, 4>{}); break;
        default: break;  // unreachable: the entries' checks
    }
}

// the grid of a group kernel over numel elements: kHadGroupUnits units of 8 elements per thread
inline int had_group_grid(int64_t numel, dim3& grid) {
    const int64_t g = cdiv64(cdiv64(numel, 8), (int64_t)kBlock * kHadGroupUnits);
    CT_REQUIRE(g < ((int64_t)1 << 31), "tensor too large for one launch");
    grid = dim3((unsigned)g);
    return CT_OK;
}

// the grid of a kernel whose workgroups stride over `blocks` pieces of work
inline dim3 capped_grid(int64_t blocks) { return dim3((unsigned)(blocks < kMaxGridX ? blocks : kMaxGridX)); }

// the row form of a rotation over runs of n elements: `group(grid, sn)` launches the entry's group kernel (n <= 512),
// `block(U, WAVES, grid, blocks, sn)` its block kernel
template <typename A, typename G, typename B>
inline int launch_had_rows(int64_t numel, int64_t n, G&& group, B&& block) {
    const HadScale<A> sn = make_had_scale<A>(n);
    if (n <= 512) {
        dim3 grid;
        const int rc = had_group_grid(numel, grid);
        if (rc) return rc;
        group(grid, sn);
        return CT_OK;
    }
    const int64_t blocks = numel / n;
    for_had_block(n, [&](auto U, auto W) { block(U, W, capped_grid(blocks), blocks, sn); });
    return CT_OK;
}

// rows(X, A) for the tensor's dtype as a compile-time constant and an accumulator of the selected type
template <typename F>
inline int for_had_types(int dt, int acc64, F&& rows) {
    int rc = CT_OK;
    for_dt(dt, [&](auto X) { rc = acc64 ? rows(X, double()) : rows(X, float()); });
    return rc;
}

// the checks the rotation entries share, in the entries' order: `size()` is the entry's own rule for n (and k) behind the dtype, `own()` its
// pointers and caps behind the selectors; both return a status.  An entry without a `transposed` argument passes 0.
template <typename S, typename O>
inline int check_had_common(const void* x, const void* out, int dt, int64_t numel, int64_t n, int acc64, int transposed, S&& size, O&& own) {
    CT_REQUIRE(is_float_dt(dt), "dtype code %d is not a float type", dt);
    int rc = size();
    if (rc) return rc;
    CT_REQUIRE(numel >= 0 && numel % n == 0, "hadamard size %lld does not divide %lld elements", (long long)n, (long long)numel);
    CT_REQUIRE(acc64 == 0 || acc64 == 1, "accumulator selector must be 0 (float32) or 1 (float64), got %d", acc64);
    CT_REQUIRE(transposed == 0 || transposed == 1, "transposed must be 0 or 1, got %d", transposed);
    rc = own();
    if (rc) return rc;
    if (!aligned16(x) || !aligned16(out)) CT_UNSUPPORTED("the hadamard kernels take 16-byte aligned tensors");
    return CT_OK;
}

// out[c][r] = in[r][c] for elements of 2 or 4 bytes on stream s (transpose_kernel of csrc/ct_hadamard.hip)
void launch_transpose_words(const void* in, void* out, int elem_size, int64_t rows, int64_t cols, hipStream_t s);

// the column form of an entry (the transformed dimension is dim 0 of a row-major rows x cols matrix, which n divides): transpose into the
// workspace, `rows_form(workspace, rows * cols)` — the entry's row dispatcher, in place — and transpose back: 3 x the traffic of the row
// form, the same arithmetic.  `check()` is the entry's own argument check; `need` ends "<entry> needs a 16-byte aligned workspace ...".
template <typename C, typename R>
inline int had_cols_form(const char* entry, const char* need, const void* x, void* out, void* workspace, int dt, int64_t rows, int64_t cols, hipStream_t s,
                         C&& check, R&& rows_form) {
    CT_REQUIRE(rows >= 0 && cols >= 0, "bad matrix shape (%lld, %lld)", (long long)rows, (long long)cols);
    int rc = check();
    if (rc) return rc;
    CT_REQUIRE(workspace != nullptr && aligned16(workspace), "%s needs a 16-byte aligned workspace %s", entry, need);
    if (rows == 0 || cols == 0) return CT_OK;
    CT_REQUIRE(cdiv64(rows, 64) * cdiv64(cols, 64) < ((int64_t)1 << 31), "matrix too large for one launch");
    const auto launched = [&](const char* step) {  // "<entry>[<step>]" names a failed launch
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return (int)CT_OK;
        char tag[96];
        snprintf(tag, sizeof(tag), "%s[%s]", entry, step);
        return hip_check(e, tag);
    };
    launch_transpose_words(x, workspace, dt_size(dt), rows, cols, s);
    rc = launched("transpose");
    if (rc) return rc;
    rc = rows_form(workspace, rows * cols);
    if (rc) return rc;
    rc = launched("rows");
    if (rc) return rc;
    launch_transpose_words(workspace, out, dt_size(dt), cols, rows, s);
    return launched("transpose back");
}

}  // namespace ct
