// ct_attn.hip — static quantize / dequantize / fake_quantize of the query, key and value states of an attention module
// (ct_attn_qdq of include/ct_hip.h): 4-D tensors (B, H, S, D) read and written in place through their strides — the
// `(B, S, H, D).transpose(1, 2)` views a Llama hands its attention function and its KV cache, slices of a fused projection,
// expanded batches — with one scale per tensor or per head, K and V in one launch.
//
// The arithmetic is ct_quant.hip's (quant_core / fake_dequant_rt / dequant_core of ct_quant_core.h, the same reciprocal
// shortcuts as quant_units_kernel), so the bits are those of ct_fake_quantize / ct_quantize / ct_dequantize on the same values.
//
// Shape of the work: a row of D elements is one scale and one contiguous run.  The rows are enumerated in the OUTPUT's memory
// order — the host sorts the b / h / s dimensions by output stride, so that a transposed view's neighbouring rows (b, s, h), not its
// logical neighbours (b, h, s), share a workgroup: whole-page runs instead of one 256-byte row per 8 KB.  A row is served by the
// next power of two >= D / 8 lanes (at most a workgroup), one 8-element unit per lane — 16 bytes of bf16 / fp16 in, 16 bytes out — so a workgroup takes
// 256 / lanes rows per pass and two passes; both rows' loads are issued before the first is used.  The (b, h, s) decomposition and
// the scale fetch happen once per row and lane (every lane of a row reads the same scale word: a broadcast), never per element.
// Streaming work, no reuse: no LDS.
#include "ct_attn.h"

namespace ct {

// MODE ATTN_FQ / ATTN_Q: XDT = x dtype, TDT = the dtype of x / scale.  MODE ATTN_DQ: TDT = the scale dtype (XDT unused: the
// codes' dtype is p.xdt).
template <int XDT, int TDT, int MODE>
__global__ __launch_bounds__(kBlock) void attn_qdq_kernel(AttnParams p) {
    const AttnT& t = p.t[(p.n == 2 && blockIdx.x >= p.t[1].first_block) ? 1 : 0];
    const uint32_t lpr = 1u << t.lpr_shift, rpb = (uint32_t)kBlock >> t.lpr_shift;
    const uint32_t lane = threadIdx.x & (lpr - 1u), rl = threadIdx.x >> t.lpr_shift;
    const uint32_t upr = (t.D + 7u) >> 3;
    const uint32_t row0 = (blockIdx.x - t.first_block) * (rpb * kAttnRows) + rl;
    const bool has_zp = t.zp != nullptr;
    const bool vec = t.vec != 0u;
    AttnRow r[kAttnRows];
#pragma unroll
    for (int i = 0; i < kAttnRows; ++i) r[i] = attn_row(t, row0 + (uint32_t)i * rpb);

    for (uint32_t c = lane; c < upr; c += lpr) {
        const uint32_t c0 = c << 3;
        const int n = (int)((t.D - c0) < 8u ? (t.D - c0) : 8u);
        float v[kAttnRows][8];
#pragma unroll
        for (int i = 0; i < kAttnRows; ++i) {
            if (!r[i].valid) continue;
            const int64_t i0 = r[i].xoff + c0;
            if constexpr (MODE == ATTN_DQ) {
                if (vec && p.xdt == CT_I8) {
                    const u32x2 w = *reinterpret_cast<const u32x2*>(static_cast<const int8_t*>(t.x) + i0);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v[i][k] = (float)(int8_t)(w.x >> (8 * k));
                        v[i][4 + k] = (float)(int8_t)(w.y >> (8 * k));
                    }
                } else if (vec && p.xdt == CT_F8E4M3) {
                    const u32x2 w = *reinterpret_cast<const u32x2*>(static_cast<const uint8_t*>(t.x) + i0);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {  // float8 -> S is exact for every S
                        v[i][k] = fp8_to_f((w.x >> (8 * k)) & 0xffu);
                        v[i][4 + k] = fp8_to_f((w.y >> (8 * k)) & 0xffu);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[i][k] = k < n ? round_to<TDT>(load_rt(t.x, p.xdt, i0 + k)) : 0.0f;  // x_q.to(S)
                }
            } else {
                if (vec) {
                    load8<XDT>(t.x, i0, v[i]);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[i][k] = k < n ? load_as_f<XDT>(t.x, i0 + k) : 0.0f;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kAttnRows; ++i) {
            if (!r[i].valid) continue;
            const float s = load_rt(t.scale, p.sdt, r[i].si);
            const float zraw = has_zp ? load_rt(t.zp, p.zdt, r[i].si) : 0.0f;
            if constexpr (MODE == ATTN_DQ) {
                const float z = round_to<TDT>(zraw);  // zp.to(scale.dtype)
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < n) v[i][k] = dequant_core<TDT>(v[i][k], has_zp, z, s);
            } else {
                const float z = round_to<XDT>(zraw);           // zp.to(x.dtype)
                const float zs = round_to_rt(p.sdt, zraw);     // zp.to(scale.dtype)
                // one reciprocal per row instead of a divide per element where quant_units_kernel takes it too
                const bool can_rcp = (XDT == CT_BF16 && TDT == CT_BF16 && p.sdt == CT_BF16) || (XDT == CT_F16 && TDT == CT_F16 && p.sdt == CT_F16) ||
                                     TDT == CT_F32;
                const float rs = can_rcp ? (TDT == CT_BF16 ? bf16_fast_rcp(s) : (TDT == CT_F16 ? f16_newton_rcp(s) : f32_fast_rcp(s))) : 0.0f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (k < n) {
                        float q = quant_core<TDT>(v[i][k], s, has_zp, z, p.qmin, p.qmax, rs, p.fkind);
                        if constexpr (MODE == ATTN_FQ) q = fake_dequant_rt(p.sdt, q, has_zp, zs, s);
                        v[i][k] = q;
                    }
                }
            }
            store_unit(t.out, p.odt, r[i].ooff + c0, v[i], n, vec);
        }
    }
}

}  // namespace ct

using namespace ct;

extern "C" int ct_attn_qdq(const ct_attn_tensor* tensors, int n, int mode, int kind, int bits, int xdt, int sdt, int zdt, int tdt, int odt,
                           ct_stream_t stream) {
    CT_REQUIRE(tensors != nullptr && (n == 1 || n == 2), "ct_attn_qdq takes one or two tensors, got %d", n);
    CT_REQUIRE(mode >= ATTN_FQ && mode <= ATTN_DQ, "mode must be 0 (fake), 1 (quantize) or 2 (dequantize), got %d", mode);
    CT_REQUIRE(kind == 0 || kind == 1, "kind must be 0 (INT) or 1 (FLOAT 8-bit), got %d", kind);
    CT_REQUIRE(is_float_dt(sdt), "scale dtype code %d is not a float type", sdt);
    if (mode == ATTN_DQ) {
        CT_REQUIRE(xdt == CT_I8 || xdt == CT_I32 || xdt == CT_F8E4M3 || is_float_dt(xdt), "unsupported x_q dtype %d", xdt);
        CT_REQUIRE(is_float_dt(odt), "unsupported output dtype %d", odt);
    } else {
        CT_REQUIRE(kind == 1 || (bits >= 1 && bits <= 8), "num_bits must be in [1, 8], got %d", bits);
        CT_REQUIRE(xt_ok(xdt, tdt), "unsupported (x dtype, result dtype) = (%d, %d)", xdt, tdt);
        if (mode == ATTN_FQ) CT_REQUIRE(is_float_dt(odt), "unsupported output dtype %d", odt);
        else if (kind) CT_REQUIRE(odt == CT_F8E4M3 || is_float_dt(odt), "unsupported output dtype %d", odt);
        else CT_REQUIRE(odt == CT_I8 || odt == CT_I32 || is_float_dt(odt), "unsupported output dtype %d", odt);
    }
    AttnParams p;
    int64_t blocks = 0;
    const int rc = attn_fill(p, tensors, n, kind, bits, xdt, sdt, zdt, odt, mode != ATTN_DQ || xdt == CT_I8 || xdt == CT_F8E4M3, blocks, "ct_attn_qdq");
    if (rc) return rc;
    if (blocks == 0) return CT_OK;
    const dim3 grid((unsigned)blocks);
    if (mode == ATTN_DQ) {
        switch (sdt) {
            case CT_BF16: hipLaunchKernelGGL((attn_qdq_kernel<CT_BF16, CT_BF16, ATTN_DQ>), grid, dim3(kBlock), 0, as_stream(stream), p); break;
            case CT_F16: hipLaunchKernelGGL((attn_qdq_kernel<CT_F16, CT_F16, ATTN_DQ>), grid, dim3(kBlock), 0, as_stream(stream), p); break;
            default: hipLaunchKernelGGL((attn_qdq_kernel<CT_F32, CT_F32, ATTN_DQ>), grid, dim3(kBlock), 0, as_stream(stream), p); break;
        }
    } else if (mode == ATTN_Q) {
        CT_DISPATCH_XT(xdt, tdt, hipLaunchKernelGGL((attn_qdq_kernel<X, T, ATTN_Q>), grid, dim3(kBlock), 0, as_stream(stream), p));
    } else {
        CT_DISPATCH_XT(xdt, tdt, hipLaunchKernelGGL((attn_qdq_kernel<X, T, ATTN_FQ>), grid, dim3(kBlock), 0, as_stream(stream), p));
    }
    CT_LAUNCH_CHECK("ct_attn_qdq");
}
