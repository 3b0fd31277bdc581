// ct_fp8block.h — the element of an FP8 block-quantized weight, shared by the dequantize (ct_fp8block.hip) and the transcodings to MXFP4, NVFP4
// (ct_fp4.hip) and MXFP8 (ct_quant.hip): a global-address-space view of a table's pointers, one scale widened exactly, the pinned float32 product,
// the rounding to the dense dtype, and what the transcoding kernels and their plans have in common (the coordinates of a lane's steps, the scale of a
// unit, the item of a workgroup, the checks of an item's source half).
#pragma once

#include "ct_common.h"

namespace ct {

// the table's pointers are generic ones: as flat accesses their loads would count against both wait counters and be waited for one
// by one, so the fast path reads through global-address-space views of them
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* fp8b_global(const void* p) {
    return (const __attribute__((address_space(1))) T*)p;
}

// one scale of sdt CT_F32 / CT_BF16 / CT_F16, widened exactly
template <int SDT>
__device__ __forceinline__ float fp8b_scale(const void* p, int64_t i) {
    if constexpr (SDT == CT_F32) return fp8b_global<float>(p)[i];
    else if constexpr (SDT == CT_BF16) return bf16_bits_to_f(fp8b_global<uint16_t>(p)[i]);
    else return f16_bits_to_f(fp8b_global<uint16_t>(p)[i]);
}

__device__ __forceinline__ float fp8b_scale(const void* p, int sdt, int64_t i) {
    if (sdt == CT_F32) return static_cast<const float*>(p)[i];
    const uint32_t h = static_cast<const uint16_t*>(p)[i];
    return sdt == CT_BF16 ? bf16_bits_to_f(h) : f16_bits_to_f(h);
}

// the product, pinned in a register before any cast to half: see mul_round_to
__device__ __forceinline__ float fp8b_mul(float q, float s) {
    float p = q * s;
    asm("" : "+v"(p));
    return p;
}

// two products -> one word of two XDT values, rounded as store8 rounds them
template <int XDT>
__device__ __forceinline__ uint32_t fp8b_mx_pair(float a, float b) {
    if constexpr (XDT == CT_BF16) {
        typedef float f2 __attribute__((ext_vector_type(2)));
        typedef bf16_t b2 __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{a, b}, b2));
    } else {
        return f_to_f16_bits(a) | (f_to_f16_bits(b) << 16);
    }
}

// 16 codes under the scale s -> the 16 dense values of dtype XDT, as the dequantize would have stored them (eight words of two)
template <int XDT>
__device__ __forceinline__ void fp8b_dense16(const u32x4 q, float s, uint32_t (&d)[8]) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    const uint32_t words[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)words[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)words[i], true);
        d[2 * i] = fp8b_mx_pair<XDT>(fp8b_mul(lo.x, s), fp8b_mul(lo.y, s));
        d[2 * i + 1] = fp8b_mx_pair<XDT>(fp8b_mul(hi.x, s), fp8b_mul(hi.y, s));
    }
}

// (row, unit column) of the units u0 + k * stride, k = 0 .. STEPS - 1, of a tensor of upr units per row, as 32-bit numbers (the plans keep rows and
// columns below 2^31)
template <int STEPS>
__device__ __forceinline__ void fp8b_step_coords(int64_t u0, int64_t upr, int stride, uint32_t (&rs)[STEPS], uint32_t (&cs)[STEPS]) {
    int64_t r = u0 / upr, c = u0 - r * upr;
    const int64_t dq = stride / upr, dr = stride - dq * upr;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        rs[k] = (uint32_t)r;
        cs[k] = (uint32_t)c;
        r += dq;
        c += dr;
        if (c >= upr) {
            c -= upr;
            ++r;
        }
    }
}

// the scale of the unit at (row r, first column c0) of an item whose units lie under one scale block each
template <int SDT, typename Item>
__device__ __forceinline__ float fp8b_unit_scale(const Item& it, uint32_t r, uint32_t c0) {
    return fp8b_scale<SDT>(it.scale, (int64_t)(r / (uint32_t)it.block_h) * it.scale_stride[0] + (int64_t)(c0 / (uint32_t)it.block_w) * it.scale_stride[1]);
}

// the item of a table whose rows carry `first_block`: the last one that starts at or before this workgroup
template <typename Item>
__device__ __forceinline__ const Item& fp8b_find(const Item* __restrict__ items, int n, int64_t block) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].first_block <= block) lo = mid; else hi = mid - 1;
    }
    return items[lo];
}

// The checks every transcoding plan makes of an item's source half (pointers, shape, block, scale dtype and shape, whole groups of `group` codes
// under one scale block each, the aligned weight), under the plan's `name`; fills the scale strides.  false: ct_last_error names the item.
template <typename Item>
inline bool fp8b_plan_source(Item& it, int i, const char* name, int group, const char* group_text, bool pointers) {
    constexpr int64_t kDimMax = int64_t(1) << 31;  // as ct_fp8block_dequant_plan: the kernels divide rows and columns as 32-bit numbers
    if (!pointers) {
        set_error("%s: item %d has a NULL pointer", name, i);
        return false;
    }
    if (!(it.rows > 0 && it.cols > 0 && it.rows < kDimMax && it.cols < kDimMax)) {
        set_error("%s: item %d has shape (%lld, %lld) (need positive sizes below 2^31)", name, i, (long long)it.rows, (long long)it.cols);
        return false;
    }
    if (!(it.block_h > 0 && it.block_w > 0 && it.block_h < kDimMax && it.block_w < kDimMax)) {
        set_error("%s: item %d has block size (%lld, %lld) (need positive sizes below 2^31)", name, i, (long long)it.block_h, (long long)it.block_w);
        return false;
    }
    if (it.sdt != CT_F32 && it.sdt != CT_BF16 && it.sdt != CT_F16) {
        set_error("%s: item %d: weight_scale_inv must be float32, bfloat16 or float16 (dtype code %d)", name, i, it.sdt);
        return false;
    }
    if (it.cols % group != 0) {
        set_error("%s: item %d: columns (%lld) must be a multiple of the %s group size %d", name, i, (long long)it.cols, group_text, group);
        return false;
    }
    if (it.block_w % group != 0) {
        set_error("%s: item %d: block width %lld is not a multiple of %d (a group would straddle two scale blocks)", name, i, (long long)it.block_w, group);
        return false;
    }
    const int64_t nrb = cdiv64(it.rows, it.block_h), ncb = cdiv64(it.cols, it.block_w);
    const int64_t s0 = it.scale_shape[0], s1 = it.scale_shape[1];
    if (!((s0 == nrb || s0 == 1) && (s1 == ncb || s1 == 1))) {
        set_error("%s: item %d: weight_scale_inv of shape (%lld, %lld) for a (%lld, %lld) weight in (%lld, %lld) blocks, expected (%lld, %lld) or a "
                  "broadcast of it", name, i, (long long)s0, (long long)s1, (long long)it.rows, (long long)it.cols, (long long)it.block_h,
                  (long long)it.block_w, (long long)nrb, (long long)ncb);
        return false;
    }
    if (!aligned16(it.w)) {
        set_error("%s: item %d: weight is not 16-byte aligned", name, i);
        return false;
    }
    it.scale_stride[0] = s0 == 1 ? 0 : s1;
    it.scale_stride[1] = s1 == 1 ? 0 : 1;
    it.units_per_row = it.cols / group;
    it.units = it.rows * it.units_per_row;
    return true;
}

}  // namespace ct
