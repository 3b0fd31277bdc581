// ct_attn_dyn.hip — dynamic group QDQ of the query, key and value states of an attention module (ct_attn_dyn_qdq of
// include/ct_hip.h): compute_dynamic_scales_and_zp followed by fake_quantize (quantization/utils/helpers.py:140-195,
// lifecycle/forward.py:292-329) over groups that lie INSIDE a row of D elements — MXFP4 / MXFP8 (32), NVFP4 (16, with its global
// scale), FP8 or INT groups up to the whole head dim — on 4-D tensors (B, H, S, D) read and written in place through their
// strides, K and V in one launch.  The `.contiguous()` copy in front of ct_dynamic_qdq and the copy back are gone.
//
// Two halves joined.  The walk is ct_attn.hip's (attn_tensor_of / attn_lanes / attn_row_at of ct_attn.h): rows enumerated in
// the OUTPUT's memory order, the next power of two >= D / 8 lanes per row, one 8-element unit per lane, kAttnRows rows per thread,
// both rows' loads issued before the first is used.  The arithmetic per unit is dyn_group_kernel's (mm_acc, group_reduce over the
// lpg = group / 8 lanes of a group, dyn_qparams, dyn_qdq8, dyn_write_qparams of ct_dynamic.h), so the bits are those of
// ct_dynamic_qdq on the same values.  lpg is a power of two <= 64 that divides the lanes of a row: a group straddles neither a
// row nor a wave, and because the group divides D its lanes are all live or all idle.  Idle lanes (D / 8 no power of two) and rows
// past the end carry the neutral min / max through the exchanges — every lane of the wave executes them — and store nothing.
// The scale tensor is contiguous in LOGICAL (b, h, s) order whatever the enumeration order: the host hands over its three row
// strides permuted like xs / os.  No cross-row reduction, no LDS, no scratch.
#include "ct_attn.h"
#include "ct_dynamic.h"

namespace ct {

struct AttnDynParams {
    AttnParams a;      // the walk's geometry (its scale / zp / range fields are unused)
    DynParams d[2];    // per tensor: what ct_dynamic.h's helpers read (x / out / segs / seg_len / vec unused: the walk addresses)
    int64_t ls[2][3];  // row strides of the scale, in rows of D / group entries, in enumeration order
};

template <int XDT, bool GS>
__global__ __launch_bounds__(kBlock) void attn_dyn_kernel(AttnDynParams p, int lpg) {
    const int ti = attn_tensor_of(p.a);
    const AttnT& t = p.a.t[ti];
    const DynParams& d = p.d[ti];
    const AttnLanes g = attn_lanes(t);
    const uint32_t row0 = (blockIdx.x - t.first_block) * (g.rpb * kAttnRows) + g.rl;
    const uint32_t c0 = g.lane << 3;
    const uint32_t gpr = t.D / ((uint32_t)lpg << 3);  // groups per row
    AttnRow r[kAttnRows];
    int64_t lrow[kAttnRows];
    bool live[kAttnRows];
    float v[kAttnRows][8];
    MinMax m[kAttnRows];
#pragma unroll
    for (int i = 0; i < kAttnRows; ++i) {
        const uint32_t row = row0 + (uint32_t)i * g.rpb;
        const uint32_t q = row / t.n2, i2 = row - q * t.n2;  // attn_row's decomposition: the indices also place the scale
        const uint32_t i0 = q / t.n1, i1 = q - i0 * t.n1;
        r[i] = attn_row_at(t, row, i0, i1, i2);
        lrow[i] = (int64_t)i0 * p.ls[ti][0] + (int64_t)i1 * p.ls[ti][1] + (int64_t)i2 * p.ls[ti][2];
        live[i] = r[i].valid && c0 < t.D;
        m[i] = mm_neutral();
        if (live[i]) {
            load8<XDT>(t.x, r[i].xoff + c0, v[i]);
            m[i] = mm_acc(m[i], v[i], 8);
        }
    }
#pragma unroll
    for (int i = 0; i < kAttnRows; ++i) m[i] = group_reduce(m[i], lpg);
#pragma unroll
    for (int i = 0; i < kAttnRows; ++i) {
        if (!live[i]) continue;
        float s, z;
        dyn_qparams<XDT>(d, m[i], s, z);
        if ((g.lane & ((uint32_t)lpg - 1u)) == 0u) dyn_write_qparams<XDT, GS>(d, lrow[i] * gpr + g.lane / (uint32_t)lpg, s, z);
        if (t.out) {
            const float se = GS ? s / d.gscale[0] : s;
            dyn_qdq8<XDT, GS>(d, v[i], 8, se, z, GS ? 0.0f : dyn_rcp<XDT>(s));
            store8<XDT>(t.out, r[i].ooff + c0, v[i]);
        }
    }
}

}  // namespace ct

using namespace ct;

extern "C" int ct_attn_dyn_qdq(const ct_attn_dyn_tensor* tensors, int n, int group, int kind, int bits, int symmetric, int xdt, int zdt,
                               ct_stream_t stream) {
    CT_REQUIRE(tensors != nullptr && (n == 1 || n == 2), "ct_attn_dyn_qdq takes one or two tensors, got %d", n);
    CT_REQUIRE(group >= 1, "group size must be positive, got %d", group);
    CT_REQUIRE(n == 1 || (tensors[0].global_scale == nullptr) == (tensors[1].global_scale == nullptr),
               "the two tensors of one launch both take a global scale or neither does");
    if (group % 8 || group > 512 || log2_exact(group / 8) < 0) CT_UNSUPPORTED("ct_attn_dyn_qdq takes groups of 8 * 2^k <= 512 elements, got %d", group);
    AttnDynParams p;
    attn_params(p.a, n, 0, 8, xdt, xdt, zdt, xdt);  // dtypes of the walk: input and output are x's; the range is DynParams'
    int64_t blocks = 0;
    for (int i = 0; i < 2; ++i) {
        const ct_attn_dyn_tensor& a = tensors[i < n ? i : 0];
        CT_REQUIRE(a.B >= 0 && a.H >= 0 && a.S >= 0 && a.D >= 0, "negative shape (%lld, %lld, %lld, %lld)", (long long)a.B, (long long)a.H, (long long)a.S, (long long)a.D);
        p.a.t[i].scale = nullptr; p.a.t[i].zp = nullptr;
        int ord[3];
        // rows in the output's memory order; a launch that only writes scales walks the input's
        int rc = attn_fill(p.a, i, a.x, a.B, a.H, a.S, a.D, a.x_stride, a.out, a.out ? a.out_stride : nullptr, 0, true, a.out == nullptr, blocks,
                           "ct_attn_dyn_qdq", ord);
        if (rc) return rc;
        const AttnT& t = p.a.t[i];
        rc = fill_dyn(p.d[i], a.x, xdt, (int64_t)t.rows * (a.D / group), group, kind, bits, symmetric, a.global_scale, a.out, a.scale_out, a.zp_out, zdt);
        if (rc) return rc;
        const int64_t logical[3] = {a.H * a.S, a.S, 1};
        for (int k = 0; k < 3; ++k) p.ls[i][k] = logical[ord[k]];
        if (t.rows == 0u) continue;
        if (t.D % 8u || t.D / 8u > (uint32_t)kBlock) CT_UNSUPPORTED("tensor %d: rows of %u elements are not 1 .. %d whole 8-element units", i, t.D, kBlock);
        if (t.D % (uint32_t)group) CT_UNSUPPORTED("tensor %d: groups of %d elements do not divide rows of %u", i, group, t.D);
        if (!t.vec) CT_UNSUPPORTED("tensor %d: the strided dynamic QDQ takes rows of aligned 8-element units on both sides", i);
    }
    if (blocks == 0) return CT_OK;
    CT_REQUIRE(blocks < ((int64_t)1 << 31), "too many rows for one launch");
    const int lpg = group / 8;
    CT_DYN_DISPATCH(xdt, tensors[0].global_scale != nullptr,
                    hipLaunchKernelGGL((attn_dyn_kernel<X, G>), dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), p, lpg));
    CT_LAUNCH_CHECK("ct_attn_dyn_qdq");
}
