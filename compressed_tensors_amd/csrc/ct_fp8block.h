// ct_fp8block.h — the element of an FP8 block-quantized weight, shared by the dequantize (ct_fp8block.hip) and the transcoding to MXFP4
// (ct_fp4.hip): a global-address-space view of a table's pointers, one scale widened exactly, and the pinned float32 product.
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

}  // namespace ct
