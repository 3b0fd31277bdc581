// ct_fp8block.hip — FP8 block-quantized checkpoints -> dense weights (reference entrypoints/convert/converters/fp8block_dequantizer.py,
// FP8BlockDequantizer._create_dequantized_weight) for a whole table of modules in ONE launch.
//
// The reference pads the weight to whole blocks, reshapes it to (row blocks, block_h, column blocks, block_w), transposes, widens
// codes and scales to float32, multiplies, casts, transposes back and truncates.  Element by element that is
//   out[r, c] = rnd_odt( f32(w[r, c]) * f32(scale[r / block_h, c / block_w]) )
// with the scale broadcast the way torch broadcasts it (a size-1 scale dimension has stride 0 here).  The padding is never
// materialised: a ragged last block row or column only changes which scale an index maps to.
//
// Work unit: 16 consecutive codes of one row; a 256-lane workgroup owns 1024 consecutive units of one item.  The plan picks one
// of two paths per item:
//   fast     cols % 16 == 0, block_w % 16 == 0, 16-byte aligned tensors: the unit is element 16u of the flat tensor and never
//            straddles a scale block.  Two neighbouring lanes share a unit, eight codes each (an 8-byte load, ONE scale, a
//            16-byte non-temporal store), so that every wave-wide load and store covers one contiguous range (fp8b_fast);
//   general  everything else (ragged columns, narrow or odd block widths): lane t takes the units t, t + 256, t + 512,
//            t + 768 with byte loads, one scale per element and scalar stores, elements past the end of the row skipped.
// Arithmetic: v_cvt_pk_f32_fp8 widens exactly (gfx950's OCP E4M3), one f32 multiply, then the RNE cast of the output dtype
// (v_cvt_pk_bf16_f32 / v_cvt_f16_f32).  The product is pinned in a register before a cast to half, as in mul_round_to: this
// keeps clang from selecting v_fma_mixlo_f16 a, b, +0, which loses the sign of a zero product.
#include "ct_common.h"
#include "ct_fp8block.h"

namespace ct {

namespace {

constexpr int kFp8bUnit = 16;                                    // codes per unit
constexpr int kFp8bUnitsPerLane = 4;
constexpr int64_t kFp8bUnitsPerBlock = int64_t(kBlock) * kFp8bUnitsPerLane;
constexpr int64_t kFp8bMaxBlocks = (int64_t(1) << 24) - 1;     // one launch: workgroups x 256 lanes < 2^32
constexpr int64_t kFp8bDimMax = int64_t(1) << 31;

// eight codes at element e of the flat tensor: one 8-byte load's worth, one scale, one 16-byte store (two for float32)
template <int ODT>
__device__ __forceinline__ void fp8b_fast_half(const ct_fp8block_item& it, int64_t e, float s, const u32x2 q) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    const uint32_t words[2] = {q.x, q.y};
    float v[8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)words[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)words[i], true);
        v[4 * i] = fp8b_mul(lo.x, s);
        v[4 * i + 1] = fp8b_mul(lo.y, s);
        v[4 * i + 2] = fp8b_mul(hi.x, s);
        v[4 * i + 3] = fp8b_mul(hi.y, s);
    }
    store8<ODT>(it.out, e, v);
}

// The fast path's lanes work on HALF units: lane t takes half t % 2 of the units wg_u0 + t / 2 + 128 k, k = 0..7, so that every
// load and store instruction of a wave covers one contiguous range (8-byte loads, 16-byte stores of the 16-bit outputs).  One
// 16-byte piece per lane and unit would split each store instruction into 16-byte pieces 32 bytes apart: measured at 0.38-0.40
// of the HBM peak on the bench tables, against 0.72 for this layout's cousin in the 8-bit tables.
template <int ODT, int SDT>
__device__ __forceinline__ void fp8b_fast(const ct_fp8block_item& it, int64_t wg_u0, int64_t units) {
    constexpr int kSteps = 2 * kFp8bUnitsPerLane, kStride = kBlock / 2;  // units between a lane's steps
    const int half = threadIdx.x & 1;
    const int64_t u0 = wg_u0 + (threadIdx.x >> 1);
    if (u0 >= units) return;  // no barriers below
    const int64_t upr = it.units_per_row;
    int64_t r = u0 / upr, c = u0 - r * upr;
    const int64_t dq = kStride / upr, dr = kStride - dq * upr;
    uint32_t rs[kSteps], cs[kSteps];
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
        rs[k] = (uint32_t)r;
        cs[k] = (uint32_t)c;
        r += dq;
        c += dr;
        if (c >= upr) {
            c -= upr;
            ++r;
        }
    }
    const auto src = fp8b_global<u32x2>(it.w);
    const auto scale_of = [&](int k) {
        return fp8b_scale<SDT>(it.scale, (int64_t)(rs[k] / (uint32_t)it.block_h) * it.scale_stride[0] +
                                             (int64_t)((kFp8bUnit * cs[k]) / (uint32_t)it.block_w) * it.scale_stride[1]);
    };
    const auto piece = [&](int k) { return 2 * (u0 + (int64_t)kStride * k) + half; };  // in 8-code pieces
    if (u0 + (int64_t)kStride * (kSteps - 1) < units) {
        // every step exists: all loads first (eight 8-byte code loads and eight scale loads in flight), with no condition the
        // compiler could sink them into, then the arithmetic and the stores
        u32x2 q[kSteps];
        float s[kSteps];
#pragma unroll
        for (int k = 0; k < kSteps; ++k) {
            q[k] = src[piece(k)];
            s[k] = scale_of(k);
        }
#pragma unroll
        for (int k = 0; k < kSteps; ++k) fp8b_fast_half<ODT>(it, 8 * piece(k), s[k], q[k]);
    } else {
        // the item's last workgroup
        for (int k = 0; k < kSteps && u0 + (int64_t)kStride * k < units; ++k) fp8b_fast_half<ODT>(it, 8 * piece(k), scale_of(k), src[piece(k)]);
    }
}

template <int ODT>
__device__ __forceinline__ void fp8b_general_unit(const ct_fp8block_item& it, int64_t r, int64_t c) {
    const int64_t c0 = kFp8bUnit * c, base = r * it.cols + c0;
    const int64_t srow = (r / it.block_h) * it.scale_stride[0];
    const uint8_t* __restrict__ w = it.w;
#pragma unroll 1
    for (int j = 0; j < kFp8bUnit; ++j) {
        if (c0 + j < it.cols) {
            const float s = fp8b_scale(it.scale, it.sdt, srow + ((c0 + j) / it.block_w) * it.scale_stride[1]);
            store1<ODT>(it.out, base + j, fp8b_mul(fp8_to_f(w[base + j]), s));
        }
    }
}

template <int ODT>
__global__ __launch_bounds__(kBlock) void fp8block_dequant_kernel(const ct_fp8block_item* __restrict__ items, int n) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].first_block <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const ct_fp8block_item it = items[lo];
    const int64_t upr = it.units_per_row, units = it.rows * upr;
    const int64_t wg_u0 = ((int64_t)blockIdx.x - it.first_block) * kFp8bUnitsPerBlock;
    if (it.fast) {
        // one straight-line body per scale dtype: a branch on the dtype between the loads would make each wait for the last
        switch (it.sdt) {
            case CT_F32: fp8b_fast<ODT, CT_F32>(it, wg_u0, units); break;
            case CT_BF16: fp8b_fast<ODT, CT_BF16>(it, wg_u0, units); break;
            default: fp8b_fast<ODT, CT_F16>(it, wg_u0, units); break;
        }
        return;
    }
    const int64_t u0 = wg_u0 + threadIdx.x;
    if (u0 >= units) return;  // no barriers below
    // (row, unit column) of the lane's first unit; the next ones are kBlock units further on
    int64_t r = u0 / upr, c = u0 - r * upr;
    const int64_t dq = kBlock / upr, dr = kBlock - dq * upr;
#pragma unroll 1
    for (int k = 0; k < kFp8bUnitsPerLane && u0 + k * kBlock < units; ++k) {
        fp8b_general_unit<ODT>(it, r, c);
        r += dq;
        c += dr;
        if (c >= upr) {
            c -= upr;
            ++r;
        }
    }
}

}  // namespace

}  // namespace ct

using namespace ct;

extern "C" {

int64_t ct_fp8block_dequant_plan(ct_fp8block_item* items, int n) {
    if (n < 0 || (n > 0 && items == nullptr)) {
        set_error("ct_fp8block_dequant_plan: bad arguments");
        return -1;
    }
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        ct_fp8block_item& it = items[i];
        if (!(it.w && it.scale && it.out)) {
            set_error("ct_fp8block_dequant_plan: item %d has a NULL pointer", i);
            return -1;
        }
        if (!(it.rows > 0 && it.cols > 0 && it.rows < kFp8bDimMax && it.cols < kFp8bDimMax)) {
            set_error("ct_fp8block_dequant_plan: item %d has shape (%lld, %lld) (need positive sizes below 2^31)", i, (long long)it.rows,
                      (long long)it.cols);
            return -1;
        }
        if (!(it.block_h > 0 && it.block_w > 0 && it.block_h < kFp8bDimMax && it.block_w < kFp8bDimMax)) {
            set_error("ct_fp8block_dequant_plan: item %d has block size (%lld, %lld) (need positive sizes below 2^31)", i,
                      (long long)it.block_h, (long long)it.block_w);
            return -1;
        }
        if (it.sdt != CT_F32 && it.sdt != CT_BF16 && it.sdt != CT_F16) {
            set_error("ct_fp8block_dequant_plan: item %d: weight_scale_inv must be float32, bfloat16 or float16 (dtype code %d)", i, it.sdt);
            return -1;
        }
        const int64_t nrb = cdiv64(it.rows, it.block_h), ncb = cdiv64(it.cols, it.block_w);
        const int64_t s0 = it.scale_shape[0], s1 = it.scale_shape[1];
        if (!((s0 == nrb || s0 == 1) && (s1 == ncb || s1 == 1))) {
            set_error("ct_fp8block_dequant_plan: item %d: weight_scale_inv of shape (%lld, %lld) for a (%lld, %lld) weight in (%lld, %lld) "
                      "blocks, expected (%lld, %lld) or a broadcast of it", i, (long long)s0, (long long)s1, (long long)it.rows,
                      (long long)it.cols, (long long)it.block_h, (long long)it.block_w, (long long)nrb, (long long)ncb);
            return -1;
        }
        it.scale_stride[0] = s0 == 1 ? 0 : s1;
        it.scale_stride[1] = s1 == 1 ? 0 : 1;
        it.fast = it.cols % kFp8bUnit == 0 && it.block_w % kFp8bUnit == 0 && aligned16(it.w) && aligned16(it.out) ? 1 : 0;
        it.units_per_row = cdiv64(it.cols, kFp8bUnit);
        it.first_block = blocks;
        blocks += cdiv64(it.rows * it.units_per_row, kFp8bUnitsPerBlock);
        if (blocks > kFp8bMaxBlocks) {
            set_error("ct_fp8block_dequant_plan: more than %lld workgroups for one launch; split the batch", (long long)kFp8bMaxBlocks);
            return -1;
        }
    }
    return blocks;
}

int ct_fp8block_dequant_batch(const ct_fp8block_item* items_dev, int n, int64_t total_blocks, int odt, ct_stream_t stream) {
    CT_REQUIRE(odt == CT_BF16 || odt == CT_F16 || odt == CT_F32, "ct_fp8block_dequant_batch: output dtype must be bfloat16, float16 or float32 (dtype code %d)", odt);
    CT_REQUIRE(n >= 0 && total_blocks >= 0 && total_blocks <= kFp8bMaxBlocks, "ct_fp8block_dequant_batch: bad batch size");
    if (n == 0 || total_blocks == 0) return CT_OK;
    CT_REQUIRE(items_dev != nullptr, "ct_fp8block_dequant_batch: table is NULL");
    const dim3 grid((unsigned)total_blocks), block(kBlock);
    switch (odt) {
        case CT_BF16: hipLaunchKernelGGL(fp8block_dequant_kernel<CT_BF16>, grid, block, 0, as_stream(stream), items_dev, n); break;
        case CT_F16: hipLaunchKernelGGL(fp8block_dequant_kernel<CT_F16>, grid, block, 0, as_stream(stream), items_dev, n); break;
        default: hipLaunchKernelGGL(fp8block_dequant_kernel<CT_F32>, grid, block, 0, as_stream(stream), items_dev, n); break;
    }
    CT_LAUNCH_CHECK("ct_fp8block_dequant_batch");
}

}  // extern "C"
