// ct_attn.h — the strided row walker of the attention q / k / v launches: the descriptors a kernel gets, the prologue every
// kernel opens with, the row decomposition, the per-row quantize step, the alignment rule of the vector form and the
// host's checks, descriptor fill and dispatch.  Shared by csrc/ct_attn.hip (ct_attn_qdq), csrc/ct_attn_rot.hip (ct_attn_rot_qdq: the
// same walk behind a head-dim Hadamard rotation), csrc/ct_attn_observe.hip (ct_attn_observe: the same walk, reading only) and
// csrc/ct_attn_dyn.hip (ct_attn_dyn_qdq: the same walk with ct_dynamic.h's group arithmetic on each row).
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

// the prologue: the tensor a workgroup serves ...
__device__ __forceinline__ int attn_tensor_of(const AttnParams& p) { return (p.n == 2 && blockIdx.x >= p.t[1].first_block) ? 1 : 0; }

// ... and how its threads lie over the rows: `lpr` lanes per row (a power of two, at most the workgroup), `rpb` rows per pass, this
// thread's `lane` within its row `rl` of the pass, `upr` 8-element units per row
struct AttnLanes {
    uint32_t lpr, rpb, lane, rl, upr;
};

__device__ __forceinline__ AttnLanes attn_lanes(const AttnT& t) {
    AttnLanes g;
    g.lpr = 1u << t.lpr_shift;
    g.rpb = (uint32_t)kBlock >> t.lpr_shift;
    g.lane = threadIdx.x & (g.lpr - 1u);
    g.rl = threadIdx.x >> t.lpr_shift;
    g.upr = (t.D + 7u) >> 3;
    return g;
}

struct AttnRow {
    int64_t xoff, ooff;
    uint32_t si;
    bool valid;
};

// the offsets and the scale index of the row (i0, i1, i2) in enumeration order: the tail of every row decomposition
__device__ __forceinline__ AttnRow attn_row_at(const AttnT& t, uint32_t row, uint32_t i0, uint32_t i1, uint32_t i2) {
    AttnRow r;
    r.valid = row < t.rows;
    r.xoff = (int64_t)i0 * t.xs[0] + (int64_t)i1 * t.xs[1] + (int64_t)i2 * t.xs[2];
    r.ooff = (int64_t)i0 * t.os[0] + (int64_t)i1 * t.os[1] + (int64_t)i2 * t.os[2];
    r.si = t.head_pos == 0u ? 0u : (t.head_pos == 1u ? i0 : (t.head_pos == 2u ? i1 : i2));
    return r;
}

__device__ __forceinline__ AttnRow attn_row(const AttnT& t, uint32_t row) {
    const uint32_t q = row / t.n2, i2 = row - q * t.n2;
    const uint32_t i0 = q / t.n1, i1 = q - i0 * t.n1;
    return attn_row_at(t, row, i0, i1, i2);
}

// what quantize / fake_quantize need of a row's scale entry: the scale, the zero point rounded to x's dtype (z) and to the scale's
// (zs), and one reciprocal per row instead of a divide per element where quant_units_kernel takes it too (rs; 0: divide)
struct AttnQ {
    float s, z, zs, rs;
    bool has_zp;
};

template <int XDT, int TDT>
__device__ __forceinline__ AttnQ attn_row_qparams(const AttnParams& p, const AttnT& t, uint32_t si) {
    AttnQ q;
    q.has_zp = t.zp != nullptr;
    q.s = load_rt(t.scale, p.sdt, si);
    const float zraw = q.has_zp ? load_rt(t.zp, p.zdt, si) : 0.0f;
    q.z = round_to<XDT>(zraw);         // zp.to(x.dtype)
    q.zs = round_to_rt(p.sdt, zraw);   // zp.to(scale.dtype)
    const bool can_rcp = (XDT == CT_BF16 && TDT == CT_BF16 && p.sdt == CT_BF16) || (XDT == CT_F16 && TDT == CT_F16 && p.sdt == CT_F16) || TDT == CT_F32;
    q.rs = can_rcp ? (TDT == CT_BF16 ? bf16_fast_rcp(q.s) : (TDT == CT_F16 ? f16_newton_rcp(q.s) : f32_fast_rcp(q.s))) : 0.0f;
    return q;
}

// quantize (MODE ATTN_Q) or fake_quantize (ATTN_FQ) the first n elements of a unit in place
template <int TDT, int MODE>
__device__ __forceinline__ void attn_quant_unit(const AttnParams& p, const AttnQ& q, float (&v)[8], int n) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k < n) {
            float c = quant_core<TDT>(v[k], q.s, q.has_zp, q.z, p.qmin, p.qmax, q.rs, p.fkind);
            if constexpr (MODE == ATTN_FQ) c = fake_dequant_rt(p.sdt, c, q.has_zp, q.zs, q.s);
            v[k] = c;
        }
    }
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

// host: the dtypes and the quantization range of a launch over `n` tensors
static inline void attn_params(AttnParams& p, int n, int kind, int bits, int xdt, int sdt, int zdt, int odt) {
    p.n = n;
    p.xdt = xdt; p.sdt = sdt; p.zdt = zdt; p.odt = odt;
    p.fkind = kind;
    if (kind) { p.qmin = -448.0f; p.qmax = 448.0f; }  // torch.finfo(float8_e4m3fn)
    else { p.qmax = (float)((1 << bits) / 2 - 1); p.qmin = -(float)((1 << bits) / 2); }
}

// host: the geometry of descriptor i — (B, H, S, D) read at `x` through the b / h / s strides `xs` and, where the launch writes,
// written at `out` through `os` (both NULL: a launch that only reads) — and its share of the grid, added to `blocks`.
// i >= p.n: an empty copy (no rows).  codes_vec: the input side has a vector form (always, except dequantize from a wide code
// dtype).  The rows are enumerated by output stride (input_order: by input stride); ord_out receives that order (the logical dimension
// at each enumeration position) for a caller that places more than x and out by it.
static inline int attn_fill(AttnParams& p, int i, const void* x, int64_t B, int64_t H, int64_t S, int64_t D, const int64_t* xs, void* out, const int64_t* os,
                            int per_head, bool codes_vec, bool input_order, int64_t& blocks, const char* entry, int* ord_out = nullptr) {
    static const int64_t none[3] = {0, 0, 0};
    if (os == nullptr) os = none;
    AttnT& t = p.t[i];
    CT_REQUIRE(B >= 0 && H >= 0 && S >= 0 && D >= 0, "negative shape (%lld, %lld, %lld, %lld)", (long long)B, (long long)H, (long long)S, (long long)D);
    for (int k = 0; k < 3; ++k)
        CT_REQUIRE(xs[k] >= 0 && os[k] >= 0, "negative stride in tensor %d", i);
    const int64_t rows = B * H * S;
    CT_REQUIRE(B < ((int64_t)1 << 31) && H < ((int64_t)1 << 31) && S < ((int64_t)1 << 31) && D < ((int64_t)1 << 31) && rows < ((int64_t)1 << 31),
               "tensor %d has %lld rows: %s indexes rows in 32 bits", i, (long long)rows, entry);
    t.x = x; t.out = out;
    const int64_t size[3] = {B, H, S};
    // enumeration order: largest stride first (insertion sort, ties and size-1 dimensions keep the logical order)
    const int64_t* key = input_order ? xs : os;
    int ord[3] = {0, 1, 2};
    for (int k = 1; k < 3; ++k)
        for (int j = k; j > 0 && size[ord[j]] > 1 && (size[ord[j - 1]] <= 1 || key[ord[j]] > key[ord[j - 1]]); --j) {
            const int tmp = ord[j]; ord[j] = ord[j - 1]; ord[j - 1] = tmp;
        }
    for (int k = 0; k < 3; ++k) { t.xs[k] = xs[ord[k]]; t.os[k] = os[ord[k]]; }
    if (ord_out)
        for (int k = 0; k < 3; ++k) ord_out[k] = ord[k];
    t.n1 = (uint32_t)(size[ord[1]] > 0 ? size[ord[1]] : 1); t.n2 = (uint32_t)(size[ord[2]] > 0 ? size[ord[2]] : 1); t.D = (uint32_t)D;
    t.rows = (i < p.n && D > 0) ? (uint32_t)rows : 0u;
    t.head_pos = 0u;
    if (per_head)
        for (int k = 0; k < 3; ++k)
            if (ord[k] == 1) t.head_pos = (uint32_t)k + 1u;
    t.vec = (D % 8 == 0 && codes_vec && side_aligned(x, xs, size, p.xdt) && side_aligned(out, os, size, p.odt)) ? 1u : 0u;
    const int64_t upr = cdiv64(D, 8);
    uint32_t shift = 0;
    while (shift < 8 && ((int64_t)1 << shift) < upr) ++shift;
    t.lpr_shift = shift;
    t.first_block = (uint32_t)blocks;
    blocks += cdiv64((int64_t)t.rows, (int64_t)(kBlock >> shift) * kAttnRows);
    return CT_OK;
}

// host: what ct_attn_qdq and ct_attn_rot_qdq check of the arguments they share, after their own check of `mode`
static inline int attn_qdq_check(int mode, int kind, int bits, int xdt, int sdt, int tdt, int odt) {
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
    return CT_OK;
}

// host: the parameters of such a launch from the public descriptors (t[1] of a single tensor is an empty copy of t[0]); `blocks`
// receives the grid
static inline int attn_qdq_fill(AttnParams& p, const ct_attn_tensor* tensors, int n, int kind, int bits, int xdt, int sdt, int zdt, int odt, bool codes_vec,
                                bool input_order, int64_t& blocks, const char* entry) {
    attn_params(p, n, kind, bits, xdt, sdt, zdt, odt);
    blocks = 0;
    for (int i = 0; i < 2; ++i) {
        const ct_attn_tensor& a = tensors[i < n ? i : 0];
        CT_REQUIRE(a.zp == nullptr || zdt_ok(zdt), "zero-point dtype code %d unsupported", zdt);
        p.t[i].scale = a.scale; p.t[i].zp = a.zp;
        const int rc = attn_fill(p, i, a.x, a.B, a.H, a.S, a.D, a.x_stride, a.out, a.out_stride, (int)a.per_head, codes_vec, input_order, blocks, entry);
        if (rc) return rc;
    }
    return CT_OK;
}

// host: the statement with X, T (CT_DISPATCH_XT's, for xdt and tdt) and M (the mode: ATTN_Q, else ATTN_FQ) as compile-time constants
#define CT_ATTN_DISPATCH_FQ_Q(mode, xdt, tdt, ...)                                              \
    do {                                                                                        \
        if (mode == ATTN_Q) { constexpr int M = ATTN_Q; CT_DISPATCH_XT(xdt, tdt, __VA_ARGS__); } \
        else { constexpr int M = ATTN_FQ; CT_DISPATCH_XT(xdt, tdt, __VA_ARGS__); }              \
    } while (0)

}  // namespace ct
