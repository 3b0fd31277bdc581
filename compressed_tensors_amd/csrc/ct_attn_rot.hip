// ct_attn_rot.hip — the head-dim Hadamard rotation of the query / key states (csrc/ct_hadamard.hip, had_group_kernel) and the
// static q / k / v QDQ that follows it (csrc/ct_attn.hip) in ONE launch (ct_attn_rot_qdq of include/ct_hip.h): the
// `(B, S, H, D).transpose(1, 2)` view is read in place through its strides, rotated in registers over runs of n elements of its
// last dimension, and quantized; the copy to a contiguous tensor, the rotated tensor and their two round trips through HBM are gone.
//
// The arithmetic is the two parents' own device functions in the parents' order: load8, the butterfly stages in float32
// (unit_stages, lane_stages), ONE quotient by sqrt(n) (had_div8 with the HadScale ct_hadamard_rows builds), the rounding to x's
// dtype that had_store's conversion performs — and only those rounded values reach the row step attn_qdq_kernel takes too
// (attn_row_qparams / attn_quant_unit of ct_attn.h).  The output is therefore the bits ct_hadamard_rows followed by ct_attn_qdq
// produce.  The unrotated tensor of a pair (V next to a rotated K) takes that row step alone.
//
// Shape of the work: ct_attn.hip's.  A row of D elements is served by the next power of two >= D / 8 lanes, one 8-element unit
// per lane, two rows per thread, rows enumerated in the INPUT's memory order (the output of a rotated tensor is a new contiguous
// (B, H, S, D) while the input is the transposed view: sequential reads, 256-byte-row writes); both rows' loads are issued before
// the first butterfly.  n / 8 lanes own a rotation block; n / 8 divides the lanes of a row, so a block straddles neither a row nor a wave.
// No LDS, no scratch.
#include "ct_attn.h"
#include "ct_hadamard.h"

namespace ct {

template <int XDT, int TDT, int MODE>
__global__ __launch_bounds__(kBlock) void attn_rot_kernel(AttnParams p, int n, int rot_mask, HadScale<float> sn) {
    const int ti = attn_tensor_of(p);
    const AttnT& t = p.t[ti];
    const bool rot = (rot_mask >> ti) & 1;  // uniform over the workgroup
    const AttnLanes g = attn_lanes(t);
    const uint32_t row0 = (blockIdx.x - t.first_block) * (g.rpb * kAttnRows) + g.rl;
    const uint32_t c0 = g.lane << 3;
    AttnRow r[kAttnRows];
    bool live[kAttnRows];
    float v[kAttnRows][8];
    // n divides D and n / 8 the lanes of a row: every lane of a live rotation block is live.  Rows past the end and the idle lanes
    // of a row whose units are no power of two carry zeros through the exchanges (every lane of the wave executes them) and store nothing.
#pragma unroll
    for (int i = 0; i < kAttnRows; ++i) {
        r[i] = attn_row(t, row0 + (uint32_t)i * g.rpb);
        live[i] = r[i].valid && c0 < t.D;
        if (live[i]) {
            load8<XDT>(t.x, r[i].xoff + c0, v[i]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[i][k] = 0.0f;
        }
    }
    if (rot) {
        const int lpb = n >= 8 ? n >> 3 : 1, wlane = threadIdx.x & 63;
#pragma unroll
        for (int i = 0; i < kAttnRows; ++i) {
            unit_stages(v[i], n);
            lane_stages(v[i], lpb, wlane);
        }
    }
#pragma unroll
    for (int i = 0; i < kAttnRows; ++i) {
        if (!live[i]) continue;
        if (rot) {  // the rotated values: quotient by sqrt(n), rounded to XDT (what had_store writes and load8 reads back)
            had_div8(v[i], sn, v[i]);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[i][k] = round_to<XDT>(v[i][k]);
        }
        attn_quant_unit<TDT, MODE>(p, attn_row_qparams<XDT, TDT>(p, t, r[i].si), v[i], 8);
        store_unit(t.out, p.odt, r[i].ooff + c0, v[i], 8, true);
    }
}

}  // namespace ct

using namespace ct;

extern "C" int ct_attn_rot_qdq(const ct_attn_tensor* tensors, int n, int rot_size, int rot_mask, int mode, int kind, int bits, int xdt, int sdt, int zdt,
                               int tdt, int odt, ct_stream_t stream) {
    CT_REQUIRE(tensors != nullptr && (n == 1 || n == 2), "ct_attn_rot_qdq takes one or two tensors, got %d", n);
    CT_REQUIRE(mode == ATTN_FQ || mode == ATTN_Q, "mode must be 0 (fake) or 1 (quantize), got %d", mode);
    int rc = attn_qdq_check(mode, kind, bits, xdt, sdt, tdt, odt);
    if (rc) return rc;
    CT_REQUIRE(rot_size >= 1 && log2_exact(rot_size) >= 0, "Cannot construct deterministic hadamard of size != 2^n");
    CT_REQUIRE(rot_mask >= 0 && rot_mask < (1 << n), "rot_mask %d names a tensor beyond the %d given", rot_mask, n);
    if (rot_size < 2 || rot_size > 512) CT_UNSUPPORTED("the fused attention rotation takes blocks of 2 .. 512 elements, got %d", rot_size);
    AttnParams p;
    int64_t blocks = 0;
    // rows in the INPUT's memory order: the transposed view is read sequentially, the contiguous output takes the strided side
    // (measured against the output's order at q (1, 32, 8192, 128): 54.9 against 56.2-56.4 us; the k+v rows alike: DESIGN 5.15)
    rc = attn_qdq_fill(p, tensors, n, kind, bits, xdt, sdt, zdt, odt, true, /*input_order=*/true, blocks, "ct_attn_rot_qdq");
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        const AttnT& t = p.t[i];
        if (t.rows == 0u) continue;
        if (t.D % 8u || t.D / 8u > (uint32_t)kBlock) CT_UNSUPPORTED("tensor %d: rows of %u elements are not 1 .. %d whole 8-element units", i, t.D, kBlock);
        if (!t.vec) CT_UNSUPPORTED("tensor %d: the fused attention rotation takes rows of aligned 8-element units on both sides", i);
        if (((rot_mask >> i) & 1) && t.D % (uint32_t)rot_size) CT_UNSUPPORTED("tensor %d: hadamard size %d does not divide rows of %u elements", i, rot_size, t.D);
    }
    if (blocks == 0) return CT_OK;
    const HadScale<float> sn = make_had_scale<float>(rot_size);  // ct_hadamard_rows'
    const dim3 grid((unsigned)blocks);
    CT_ATTN_DISPATCH_FQ_Q(mode, xdt, tdt, hipLaunchKernelGGL((attn_rot_kernel<X, T, M>), grid, dim3(kBlock), 0, as_stream(stream), p, rot_size, rot_mask, sn));
    CT_LAUNCH_CHECK("ct_attn_rot_qdq");
}
