// ct_attn_observe.hip — the min-max calibration observer of the attention q / k / v states and of static activations
// (ct_attn_observe of include/ct_hip.h): the running minimum and maximum per head (attn_head) or per tensor of one or two 4-D
// tensors (B, H, S, D) read in place through their strides, and the scale / zero point calculate_qparams gives for them — what
// ct_attn_qdq consumes.
//
// Two launches.  FOLD walks the rows in the INPUT's memory order (attn_fill's input_order: a transposed view is read as whole
// pages), one 8-element unit per lane (16-bit units as packed 16-bit order keys, widened once per row), reduces a row over its lanes with DPP
// on 32-bit order keys (ct_minmax.h: integer min / max, exact and order-free, a NaN surfaces as an extreme), accumulates per scale entry in LDS over every row the workgroup owns and
// then folds its table into the caller's state with at most two global integer atomics per entry it touched.  The grid is capped
// (kObsCap workgroups) and loops over the rows: the atomics on an entry are bounded by the cap, not by the row count.
// FINALIZE: one thread per entry decodes the keys, runs the weight path's compute_qparams / compute_qparams_float — or, kind 2,
// generate_gparam's arithmetic (gparam_from_amax) on the same amax — and stores scale, zero point and (optionally) the extremes; unless `keep` it re-arms the state.  Stream order between the two launches is
// the only synchronisation.
#include "ct_attn.h"
#include "ct_minmax.h"

namespace ct {

constexpr int kObsMaxEntries = 1024;  // the LDS table: 2 x 4 KB of keys per workgroup
constexpr int kObsRows = 4;           // rows per thread and step: their loads are issued before the first is used
constexpr int kObsMinSteps = 2;       // a workgroup owns at least this many steps where the tensor has them (halves the atomics)
constexpr int kObsCap = 4 * kCUs;     // workgroups of one launch, whatever the row count

struct ObsT {
    int32_t* state;  // entries min keys, then entries max keys
    void* scale;
    void* zp;
    void* min_vals;
    void* max_vals;
    uint32_t entries, steps, blocks, first_entry;
    uint32_t magic1, shift1, magic2, shift2;  // row / n2 and (row / n2) / n1 as a multiplication (obs_magic)
};

// floor(n / d) for every n < 2^31 as (n * M) >> sh with M = ceil(2^(31 + s) / d) < 2^32, s = ceil(log2 d) (Granlund & Montgomery):
// attn_row's two 32-bit divisions per row and lane were a third of this kernel's instructions
static inline void obs_magic(uint32_t d, uint32_t& M, uint32_t& sh) {
    int s = 0;
    while (((uint64_t)1 << s) < d) ++s;
    M = (uint32_t)((((uint64_t)1 << (31 + s)) + d - 1) / d);
    sh = 31u + (uint32_t)s;
}

__device__ __forceinline__ AttnRow obs_row(const AttnT& t, const ObsT& o, uint32_t row) {
    const uint32_t q = (uint32_t)(((uint64_t)row * o.magic2) >> o.shift2), i2 = row - q * t.n2;
    const uint32_t i0 = (uint32_t)(((uint64_t)q * o.magic1) >> o.shift1), i1 = q - i0 * t.n1;
    return attn_row_at(t, row, i0, i1, i2);  // (the output side of a reader is zeros)
}

// the extremes of packed 16-bit keys (ct_minmax.h: 2.5 operations per element against 6 on widened values) as 32-bit keys
template <int XDT>
__device__ __forceinline__ MinMaxKey32 obs_widen(MinMaxKey a) {
    const int mn_lo = (int)(int16_t)(a.mn & 0xffffu), mn_hi = (int)(int16_t)(a.mn >> 16);
    const int mx_lo = (int)(int16_t)(a.mx & 0xffffu), mx_hi = (int)(int16_t)(a.mx >> 16);
    const int kmn = mn_lo < mn_hi ? mn_lo : mn_hi, kmx = mx_lo > mx_hi ? mx_lo : mx_hi;
    const uint32_t bmn = ((uint32_t)kmn ^ ((uint32_t)(kmn >> 15) & 0x7fffu)) & 0xffffu, bmx = ((uint32_t)kmx ^ ((uint32_t)(kmx >> 15) & 0x7fffu)) & 0xffffu;
    if constexpr (XDT == CT_BF16) return MinMaxKey32{mm_key32(bmn << 16), mm_key32(bmx << 16)};
    else return MinMaxKey32{mm_key32(f_bits(f16_bits_to_f(bmn))), mm_key32(f_bits(f16_bits_to_f(bmx)))};
}

struct ObsParams {
    AttnParams a;  // t[i].x / xs / rows / head_pos / vec / lpr_shift / first_block are read; the output side is unused
    ObsT o[2];
    int bits, symmetric, keep;
};

template <int XDT>
__global__ __launch_bounds__(kBlock) void attn_observe_fold_kernel(ObsParams p) {
    __shared__ int32_t smn[kObsMaxEntries], smx[kObsMaxEntries];
    const int ti = attn_tensor_of(p.a);
    const AttnT& t = p.a.t[ti];
    const ObsT& o = p.o[ti];
    for (uint32_t e = threadIdx.x; e < o.entries; e += kBlock) { smn[e] = kKey32EmptyMin; smx[e] = kKey32EmptyMax; }
    __syncthreads();

    const AttnLanes g = attn_lanes(t);
    const uint32_t lpr = g.lpr, rpb = g.rpb, lane = g.lane, upr = g.upr;
    const int lpg = (int)(lpr < 64u ? lpr : 64u);  // a row wider than a wave: each of its waves reduces and posts
    const bool poster = (threadIdx.x & (uint32_t)(lpg - 1)) == 0u;
    const bool vec = t.vec != 0u;
    const bool per_head = t.head_pos != 0u;
    MinMaxKey32 whole = mmk32_init();  // the tensor strategy: one entry, kept in registers over the whole loop

    for (uint32_t step = blockIdx.x - t.first_block; step < o.steps; step += o.blocks) {  // uniform per workgroup
        const uint32_t row0 = step * (rpb * kObsRows) + g.rl;
        AttnRow r[kObsRows];
#pragma unroll
        for (int i = 0; i < kObsRows; ++i) r[i] = obs_row(t, o, row0 + (uint32_t)i * rpb);
        MinMaxKey32 m[kObsRows];
#pragma unroll
        for (int i = 0; i < kObsRows; ++i) m[i] = mmk32_init();
        if (XDT != CT_F32 && vec) {  // 16-bit units: min / max on the raw pairs, widened once per row and lane
            MinMaxKey k[kObsRows];
#pragma unroll
            for (int i = 0; i < kObsRows; ++i) k[i] = mmk_init();
            for (uint32_t c = lane; c < upr; c += lpr) {
                u32x4 w[kObsRows];
#pragma unroll
                for (int i = 0; i < kObsRows; ++i)
                    if (r[i].valid) w[i] = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(t.x) + r[i].xoff + (c << 3));
#pragma unroll
                for (int i = 0; i < kObsRows; ++i)
                    if (r[i].valid) k[i] = mmk_acc(mmk_acc(mmk_acc(mmk_acc(k[i], w[i].x), w[i].y), w[i].z), w[i].w);
            }
            if constexpr (XDT != CT_F32) {  // (obs_widen has no float32 form)
#pragma unroll
                for (int i = 0; i < kObsRows; ++i)
                    if (r[i].valid && lane < upr) m[i] = obs_widen<XDT>(k[i]);  // a lane without a unit keeps the empty keys
            }
        } else {
            for (uint32_t c = lane; c < upr; c += lpr) {
                const uint32_t c0 = c << 3;
                const int n = (int)((t.D - c0) < 8u ? (t.D - c0) : 8u);
                float v[kObsRows][8];
#pragma unroll
                for (int i = 0; i < kObsRows; ++i) {
                    if (!r[i].valid) continue;
                    const int64_t i0 = r[i].xoff + c0;
                    if (vec) {  // float32
                        load8<XDT>(t.x, i0, v[i]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k) v[i][k] = k < n ? load_as_f<XDT>(t.x, i0 + k) : 0.0f;
                    }
                }
#pragma unroll
                for (int i = 0; i < kObsRows; ++i) {
                    if (!r[i].valid) continue;
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < n) m[i] = mmk32_acc(m[i], v[i][k]);
                }
            }
        }
        if (per_head) {
#pragma unroll
            for (int i = 0; i < kObsRows; ++i) {
                const MinMaxKey32 g = mmk32_group_reduce(m[i], lpg);  // every lane: rows past the end carry the empty keys
                if (poster && r[i].valid) {
                    atomicMin(&smn[r[i].si], g.mn);
                    atomicMax(&smx[r[i].si], g.mx);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < kObsRows; ++i) whole = mmk32_merge(whole, m[i].mn, m[i].mx);
        }
    }
    if (!per_head) {
        const MinMaxKey32 g = mmk32_group_reduce(whole, 64);
        if ((threadIdx.x & 63u) == 0u) {
            atomicMin(&smn[0], g.mn);
            atomicMax(&smx[0], g.mx);
        }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < o.entries; e += kBlock) {
        const int32_t kmn = smn[e], kmx = smx[e];
        if (kmn != kKey32EmptyMin) atomicMin(o.state + e, kmn);
        if (kmx != kKey32EmptyMax) atomicMax(o.state + o.entries + e, kmx);
    }
}

template <int XDT>
__global__ __launch_bounds__(kBlock) void attn_observe_finalize_kernel(ObsParams p) {
    const uint32_t g = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const int ti = (p.a.n == 2 && g >= p.o[1].first_entry) ? 1 : 0;
    const ObsT& o = p.o[ti];
    const uint32_t e = g - o.first_entry;
    if (e >= o.entries) return;
    int32_t* kmn = o.state + e;
    int32_t* kmx = o.state + o.entries + e;
    const MinMax m = mmk32_finish(MinMaxKey32{*kmn, *kmx});
    float s, z = 0.0f;
    if (p.a.fkind == 2) s = gparam_from_amax<XDT>(compute_qparams_float<XDT>(m, QP_AMAX, 0.0f));  // generate_gparam(min, max): the NVFP4 global scale
    else if (p.a.fkind) s = compute_qparams_float<XDT>(m, QP_FP8, 0.0f);
    else compute_qparams<XDT>(m, p.bits, p.symmetric, s, z);
    store_rt(o.scale, p.a.sdt, e, s);
    if (o.zp) store_rt(o.zp, p.a.zdt, e, z);
    const float nanv = __builtin_nanf("");
    if (o.min_vals) store1<XDT>(o.min_vals, e, m.nan ? nanv : m.mn);  // torch.amin / amax: a NaN anywhere is the result of both
    if (o.max_vals) store1<XDT>(o.max_vals, e, m.nan ? nanv : m.mx);
    if (!p.keep) { *kmn = kKey32EmptyMin; *kmx = kKey32EmptyMax; }
}

}  // namespace ct

using namespace ct;

extern "C" int ct_attn_observe(const ct_attn_observe_tensor* tensors, int n, int kind, int bits, int symmetric, int xdt, int sdt, int zdt, int keep,
                               ct_stream_t stream) {
    CT_REQUIRE(tensors != nullptr && (n == 1 || n == 2), "ct_attn_observe takes one or two tensors, got %d", n);
    CT_REQUIRE(kind >= 0 && kind <= 2, "kind must be 0 (INT), 1 (FLOAT 8-bit) or 2 (the NVFP4 global scale), got %d", kind);
    CT_REQUIRE(kind != 0 || (bits >= 1 && bits <= 8), "num_bits must be in [1, 8], got %d", bits);
    CT_REQUIRE(kind != 2 || sdt == CT_F32, "a global scale is float32, got scale dtype code %d", sdt);
    CT_REQUIRE(is_float_dt(xdt), "observed dtype code %d is not a float type", xdt);
    CT_REQUIRE(is_float_dt(sdt), "scale dtype code %d is not a float type", sdt);
    CT_REQUIRE(keep == 0 || keep == 1, "keep must be 0 or 1, got %d", keep);
    for (int i = 0; i < n; ++i) {  // (a negative size passes here and is attn_fill's to refuse)
        const ct_attn_observe_tensor& a = tensors[i];
        CT_REQUIRE(a.x != nullptr && a.state != nullptr && a.scale != nullptr, "tensor %d: x, state and scale must not be NULL", i);
        CT_REQUIRE(kind != 2 || a.zp == nullptr, "tensor %d: a global scale has no zero point", i);
        CT_REQUIRE(a.zp == nullptr || zdt == CT_I8 || zdt == CT_I32 || zdt == CT_F8E4M3 || is_float_dt(zdt), "zero-point dtype code %d unsupported", zdt);
        CT_REQUIRE(a.B != 0 && a.H != 0 && a.S != 0 && a.D != 0, "tensor %d is empty: the minimum of no elements is undefined", i);
        if (a.per_head && a.H > kObsMaxEntries) CT_UNSUPPORTED("%lld heads: the observer's table holds %d entries", (long long)a.H, kObsMaxEntries);
    }
    ObsParams p;
    attn_params(p.a, n, kind, kind ? 8 : bits, xdt, sdt, zdt, xdt);
    p.bits = bits; p.symmetric = symmetric; p.keep = keep;
    int64_t unused = 0;
    uint32_t blocks = 0, entries = 0;
    for (int i = 0; i < 2; ++i) {
        const ct_attn_observe_tensor& a = tensors[i < n ? i : 0];
        const int rc = attn_fill(p.a, i, a.x, a.B, a.H, a.S, a.D, a.x_stride, nullptr, nullptr, (int)a.per_head, true, true, unused, "ct_attn_observe");
        if (rc) return rc;
        AttnT& t = p.a.t[i];
        t.scale = nullptr; t.zp = nullptr;
        ObsT& o = p.o[i];
        obs_magic(t.n1, o.magic1, o.shift1);
        obs_magic(t.n2, o.magic2, o.shift2);
        o.state = a.state; o.scale = a.scale; o.zp = a.zp; o.min_vals = a.min_vals; o.max_vals = a.max_vals;
        o.entries = i < n ? (uint32_t)(a.per_head ? a.H : 1) : 0u;
        const int64_t rows_per_step = (int64_t)(kBlock >> t.lpr_shift) * kObsRows;
        o.steps = (uint32_t)cdiv64((int64_t)t.rows, rows_per_step);
        const int64_t want = cdiv64((int64_t)o.steps, kObsMinSteps), cap = kObsCap / n;
        o.blocks = (uint32_t)(want < cap ? want : cap);
        t.first_block = blocks;
        o.first_entry = entries;
        blocks += o.blocks;
        entries += o.entries;
    }
    CT_DISPATCH_XT(xdt, xdt, hipLaunchKernelGGL((attn_observe_fold_kernel<X>), dim3(blocks), dim3(kBlock), 0, as_stream(stream), p));
    const int rc_fold = hip_check(hipGetLastError(), "ct_attn_observe (fold)");
    if (rc_fold) return rc_fold;
    const dim3 fgrid((unsigned)cdiv64((int64_t)entries, kBlock));
    CT_DISPATCH_XT(xdt, xdt, hipLaunchKernelGGL((attn_observe_finalize_kernel<X>), fgrid, dim3(kBlock), 0, as_stream(stream), p));
    CT_LAUNCH_CHECK("ct_attn_observe (finalize)");
}
