// ct_attn.h — the strided row walker of the attention q / k / v launches: the descriptors a kernel gets, the row decomposition,
// the alignment rule of the vector form and the host's descriptor fill.  Shared by csrc/ct_attn.hip (ct_attn_qdq) and
// csrc/ct_attn_rot.hip (ct_attn_rot_qdq: the same walk behind a head-dim Hadamard rotation).
#pragma once
#include "ct_quant_core.h"

namespace ct {

enum { ATTN_FQ = 0, ATTN_Q = 1, ATTN_DQ = 2 };
constexpr int kAttnRows = 2;  // rows per thread

struct AttnT {
    const void* x;
    void* out;
    const void* scale;
    const void* zp;
    int64_t xs[3], os[3];  // element strides of the three row dimensions, outermost first in enumeration order
    uint32_t n1, n2, D, rows;  // sizes of the middle and the innermost enumerated dimension
    uint32_t head_pos;     // 0: one scale entry; 1 + the position of the head dimension in the enumeration order
    uint32_t vec;          // whole 8-element units, aligned on both sides
    uint32_t lpr_shift;    // log2(lanes per row)
    uint32_t first_block;
};

struct AttnParams {
    AttnT t[2];
    int n;
    int xdt, sdt, zdt, odt;
    float qmin, qmax;
    int fkind;
};

struct AttnRow {
    int64_t xoff, ooff;
    uint32_t si;
    bool valid;
};

__device__ __forceinline__ AttnRow attn_row(const AttnT& t, uint32_t row) {
    AttnRow r;
    r.valid = row < t.rows;
    const uint32_t q = row / t.n2, i2 = row - q * t.n2;
    const uint32_t i0 = q / t.n1, i1 = q - i0 * t.n1;
    r.xoff = (int64_t)i0 * t.xs[0] + (int64_t)i1 * t.xs[1] + (int64_t)i2 * t.xs[2];
    r.ooff = (int64_t)i0 * t.os[0] + (int64_t)i1 * t.os[1] + (int64_t)i2 * t.os[2];
    r.si = t.head_pos == 0u ? 0u : (t.head_pos == 1u ? i0 : (t.head_pos == 2u ? i1 : i2));
    return r;
}

// bytes a lane moves per 8-element unit on one side, capped at the 16-byte vector; the alignment every unit needs
static inline int64_t unit_align(int dt) {
    const int64_t b = 8 * (int64_t)dt_size(dt);
    return b < 16 ? b : 16;
}

static inline bool side_aligned(const void* base, const int64_t* stride, const int64_t* size, int dt) {
    const int64_t a = unit_align(dt), isz = dt_size(dt);
    if (reinterpret_cast<uintptr_t>(base) % (uintptr_t)a) return false;
    for (int k = 0; k < 3; ++k)
        if (size[k] > 1 && (stride[k] * isz) % a) return false;
    return true;
}

// host: the quantization range and the descriptors of `n` tensors (t[1] of a single tensor is an empty copy of t[0]); `blocks`
// receives the grid.  codes_vec: the input side has a vector form (always, except dequantize from a wide code dtype)
static inline int attn_fill(AttnParams& p, const ct_attn_tensor* tensors, int n, int kind, int bits, int xdt, int sdt, int zdt, int odt, bool codes_vec,
                            int64_t& blocks, const char* entry, bool input_order = false) {
    p.n = n;
    p.xdt = xdt; p.sdt = sdt; p.zdt = zdt; p.odt = odt;
    p.fkind = kind;
    if (kind) { p.qmin = -448.0f; p.qmax = 448.0f; }  // torch.finfo(float8_e4m3fn)
    else { p.qmax = (float)((1 << bits) / 2 - 1); p.qmin = -(float)((1 << bits) / 2); }
    blocks = 0;
    for (int i = 0; i < 2; ++i) {
        const ct_attn_tensor& a = tensors[i < n ? i : 0];
        AttnT& t = p.t[i];
        CT_REQUIRE(a.B >= 0 && a.H >= 0 && a.S >= 0 && a.D >= 0, "negative shape (%lld, %lld, %lld, %lld)", (long long)a.B, (long long)a.H, (long long)a.S,
                   (long long)a.D);
        for (int k = 0; k < 3; ++k)
            CT_REQUIRE(a.x_stride[k] >= 0 && a.out_stride[k] >= 0, "negative stride in tensor %d", i);
        CT_REQUIRE(a.zp == nullptr || zdt_ok(zdt), "zero-point dtype code %d unsupported", zdt);
        const int64_t rows = a.B * a.H * a.S;
        CT_REQUIRE(a.B < ((int64_t)1 << 31) && a.H < ((int64_t)1 << 31) && a.S < ((int64_t)1 << 31) && a.D < ((int64_t)1 << 31) && rows < ((int64_t)1 << 31),
                   "tensor %d has %lld rows: %s indexes rows in 32 bits", i, (long long)rows, entry);
        t.x = a.x; t.out = a.out; t.scale = a.scale; t.zp = a.zp;
        const int64_t size[3] = {a.B, a.H, a.S};
        // enumeration order: by output stride (input_order: by input stride), largest first (insertion sort, ties and size-1
        // dimensions keep the logical order)
        const int64_t* key = input_order ? a.x_stride : a.out_stride;
        int ord[3] = {0, 1, 2};
        for (int k = 1; k < 3; ++k)
            for (int j = k; j > 0 && size[ord[j]] > 1 && (size[ord[j - 1]] <= 1 || key[ord[j]] > key[ord[j - 1]]); --j) {
                const int tmp = ord[j]; ord[j] = ord[j - 1]; ord[j - 1] = tmp;
            }
        for (int k = 0; k < 3; ++k) { t.xs[k] = a.x_stride[ord[k]]; t.os[k] = a.out_stride[ord[k]]; }
        t.n1 = (uint32_t)(size[ord[1]] > 0 ? size[ord[1]] : 1); t.n2 = (uint32_t)(size[ord[2]] > 0 ? size[ord[2]] : 1); t.D = (uint32_t)a.D;
        t.rows = (i < n && a.D > 0) ? (uint32_t)rows : 0u;
        t.head_pos = 0u;
        if (a.per_head)
            for (int k = 0; k < 3; ++k)
                if (ord[k] == 1) t.head_pos = (uint32_t)k + 1u;
        t.vec = (a.D % 8 == 0 && codes_vec && side_aligned(a.x, a.x_stride, size, xdt) && side_aligned(a.out, a.out_stride, size, odt)) ? 1u : 0u;
        const int64_t upr = cdiv64(a.D, 8);
        uint32_t shift = 0;
        while (shift < 8 && ((int64_t)1 << shift) < upr) ++shift;
        t.lpr_shift = shift;
        t.first_block = (uint32_t)blocks;
        blocks += cdiv64((int64_t)t.rows, (int64_t)(kBlock >> shift) * kAttnRows);
    }
    return CT_OK;
}

}  // namespace ct
