// ct_attn.hip — static quantize / dequantize / fake_quantize of the query, key and value states of an attention module
// (ct_attn_qdq of include/ct_hip.h): 4-D tensors (B, H, S, D) read and written in place through their strides — the
// `(B, S, H, D).transpose(1, 2)` views a Llama hands its attention function and its KV cache, slices of a fused projection,
// expanded batches — with one scale per tensor or per head, K and V in one launch.
//
// The arithmetic is ct_quant.hip's (quant_core / fake_dequant_rt / dequant_core of ct_quant_core.h, the same reciprocal
// shortcuts as quant_units_kernel: attn_row_qparams / attn_quant_unit of ct_attn.h, shared with ct_attn_rot.hip), so the bits are those of ct_fake_quantize / ct_quantize / ct_dequantize on the same values.
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
    const AttnT& t = p.t[attn_tensor_of(p)];
    const AttnLanes g = attn_lanes(t);
    const uint32_t row0 = (blockIdx.x - t.first_block) * (g.rpb * kAttnRows) + g.rl;
    const bool vec = t.vec != 0u;
    AttnRow r[kAttnRows];
#pragma unroll
    for (int i = 0; i < kAttnRows; ++i) r[i] = attn_row(t, row0 + (uint32_t)i * g.rpb);

    for (uint32_t c = g.lane; c < g.upr; c += g.lpr) {
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
            if constexpr (MODE == ATTN_DQ) {
                const bool has_zp = t.zp != nullptr;
                const float s = load_rt(t.scale, p.sdt, r[i].si);
                const float z = round_to<TDT>(has_zp ? load_rt(t.zp, p.zdt, r[i].si) : 0.0f);  // zp.to(scale.dtype)
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < n) v[i][k] = dequant_core<TDT>(v[i][k], has_zp, z, s);
            } else {
                attn_quant_unit<TDT, MODE>(p, attn_row_qparams<XDT, TDT>(p, t, r[i].si), v[i], n);
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
    int rc = attn_qdq_check(mode, kind, bits, xdt, sdt, tdt, odt);
    if (rc) return rc;
    AttnParams p;
    int64_t blocks = 0;
    rc = attn_qdq_fill(p, tensors, n, kind, bits, xdt, sdt, zdt, odt, mode != ATTN_DQ || xdt == CT_I8 || xdt == CT_F8E4M3, false, blocks, "ct_attn_qdq");
    if (rc) return rc;
    if (blocks == 0) return CT_OK;
    const dim3 grid((unsigned)blocks);
    if (mode == ATTN_DQ) {
        switch (sdt) {
            case CT_BF16: hipLaunchKernelGGL((attn_qdq_kernel<CT_BF16, CT_BF16, ATTN_DQ>), grid, dim3(kBlock), 0, as_stream(stream), p); break;
            case CT_F16: hipLaunchKernelGGL((attn_qdq_kernel<CT_F16, CT_F16, ATTN_DQ>), grid, dim3(kBlock), 0, as_stream(stream), p); break;
            default: hipLaunchKernelGGL((attn_qdq_kernel<CT_F32, CT_F32, ATTN_DQ>), grid, dim3(kBlock), 0, as_stream(stream), p); break;
        }
    } else {
        CT_ATTN_DISPATCH_FQ_Q(mode, xdt, tdt, hipLaunchKernelGGL((attn_qdq_kernel<X, T, M>), grid, dim3(kBlock), 0, as_stream(stream), p));
    }
    CT_LAUNCH_CHECK("ct_attn_qdq");
}
