// ct_awq.hip — AutoAWQ GEMM checkpoints -> pack-quantized (reference entrypoints/convert/converters/autoawq.py,
// AutoAWQConverter.process) for a whole table of modules in ONE launch.
//
// The reference widens every nibble of qweight to int8, gathers the nibbles back into natural order, transposes and re-packs
// (the -8 of its unpack and the +8 of pack_to_int32 cancel).  Bit for bit that is a 4-bit transpose:
//   weight_packed[n, w] nibble i  =  qweight[8w + i, n / 8] nibble P[n % 8],   P = [0,4,1,5,2,6,3,7]
// i.e. every 8 x 8 block of nibbles (eight qweight words of one column, consecutive rows) becomes eight weight_packed words of
// one column (consecutive rows), with the AWQ interleave undone on the way.  The zero points are a word transpose with the same
// nibble permutation, the scales a 16-bit transpose; they are a few percent of the bytes and run in tail workgroups of each item.
//
// Weight tile: 256 qweight rows x 32 words (32 KiB in, 32 KiB out) per 256-lane workgroup.  Lane (cg = t % 8, rg = t / 8) loads
// rows 8rg..8rg+7 of words 4cg..4cg+3 — eight 16-byte loads, eight lanes on each 128-byte row segment — which are four whole
// nibble blocks: it transposes them in registers and scatters the 32 result words, one per weight_packed row, into an LDS image
// of the output tile (256 rows x 32 words).  After one barrier every lane reads 16-byte pieces of output rows back and streams
// them out, eight lanes per 128-byte row segment.  The image is XOR-swizzled in 16-byte slots: the scatter (ds_write_b32) and
// the read-back (ds_read_b128) are both free of bank conflicts.
#include "ct_common.h"

namespace ct {

namespace {

constexpr int kAwqTileK = 256;                  // qweight rows per weight tile = 32 weight_packed words per output row
constexpr int kAwqTileJ = 32;                   // qweight words per tile row = 256 weight_packed rows
constexpr int kAwqTileWords = kAwqTileK * kAwqTileJ;
constexpr int kAwqT = 64;                       // side of the zero-point / scale transpose tiles
constexpr int64_t kAwqMaxBlocks = (int64_t(1) << 24) - 1;  // one launch: workgroups x 256 lanes < 2^32

__device__ __forceinline__ int64_t awq_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// a word of eight AWQ nibbles in natural order: nibble c of the result is nibble P[c] of x
__device__ __forceinline__ uint32_t awq_natural(uint32_t x) {
    uint32_t y = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) y |= ((x >> (4 * ((c >> 1) + 4 * (c & 1)))) & 0xFu) << (4 * c);
    return y;
}

// x[i]: qweight words of rows 8w + i of one column j -> y[c]: weight_packed words of rows 8j + c, column w
__device__ __forceinline__ void awq_block_transpose(const uint32_t (&x)[8], uint32_t (&y)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int s = 4 * ((c >> 1) + 4 * (c & 1));
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) v |= ((x[i] >> s) & 0xFu) << (4 * i);
        y[c] = v;
    }
}

// LDS word of output-tile row r, column w: 16-byte slot (w / 4) XOR (r / 32)
__device__ __forceinline__ int awq_lds_index(int r, int w) { return r * kAwqTileJ + ((((w >> 2) ^ (r >> 5)) & 7) << 2) + (w & 3); }

__device__ void awq_weight_tile(const ct_awq_item& it, int64_t b, uint32_t* lds) {
    const int64_t W = it.N >> 3, KW = (it.K + 7) >> 3;
    const int64_t tiles_j = awq_cdiv(W, kAwqTileJ);
    const int64_t tk = b / tiles_j, tj = b - tk * tiles_j;
    const int64_t k0 = tk * kAwqTileK, j0 = tj * kAwqTileJ;
    const int t = threadIdx.x, cg = t & 7, rg = t >> 3;
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(it.qweight);

    // eight rows x four words.  Rows past K read as zero (the tail word of weight_packed holds zero nibbles there); every address
    // is clamped into the tensor so the eight loads issue back to back, unconditionally
    const int64_t j = j0 + 4 * cg;
    uint32_t x[4][8];
    if (it.wide & 1) {  // W % 4 == 0, 16-byte aligned rows
        const bool jok = j < W;
        const int64_t jc = jok ? j : W - 4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t k = k0 + 8 * rg + i;
            const bool ok = jok && k < it.K;
            const u32x4 v = *reinterpret_cast<const u32x4*>(src + (k < it.K ? k : it.K - 1) * W + jc);
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q][i] = ok ? v[q] : 0u;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t k = k0 + 8 * rg + i;
            const int64_t row = (k < it.K ? k : it.K - 1) * W;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool ok = j + q < W && k < it.K;
                const uint32_t v = src[row + (j + q < W ? j + q : W - 1)];
                x[q][i] = ok ? v : 0u;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t y[8];
        awq_block_transpose(x[q], y);
#pragma unroll
        for (int c = 0; c < 8; ++c) lds[awq_lds_index(32 * cg + 8 * q + c, rg)] = y[c];
    }
    __syncthreads();

    const int64_t n0 = 8 * j0, w0 = k0 >> 3;
    const int ch = t & 7;
    int32_t* __restrict__ dst = it.weight_packed;
#pragma unroll
    for (int p = 0; p < kAwqTileWords / 4 / kBlock; ++p) {
        const int r = (t >> 3) + 32 * p;
        const u32x4 v = *reinterpret_cast<const u32x4*>(lds + awq_lds_index(r, 4 * ch));
        const int64_t nn = n0 + r, w = w0 + 4 * ch;
        if (nn >= it.N) continue;
        int32_t* out = dst + nn * KW + w;
        if (it.wide & 2) {  // KW % 4 == 0, 16-byte aligned rows
            if (w < KW) stream_store16(out, v);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (w + q < KW) out[q] = (int32_t)v[q];
        }
    }
}

// src (R, C) -> dst (C, R), one 64 x 64 tile; NATURAL: the elements are AWQ zero-point words, put into natural nibble order
template <typename T, bool NATURAL>
__device__ void awq_transpose_tile(const T* __restrict__ src, T* __restrict__ dst, int64_t R, int64_t C, int64_t b, uint32_t* lds) {
    const int64_t tiles_c = awq_cdiv(C, kAwqT);
    const int64_t tr = b / tiles_c, tc = b - tr * tiles_c;
    const int64_t r0 = tr * kAwqT, c0 = tc * kAwqT;
    const int tx = threadIdx.x & (kAwqT - 1), ty = threadIdx.x / kAwqT;
    constexpr int kPitch = kAwqT + 1;
#pragma unroll
    for (int i = 0; i < kAwqT; i += kBlock / kAwqT) {
        const int64_t r = r0 + ty + i, c = c0 + tx;
        if (r < R && c < C) lds[(ty + i) * kPitch + tx] = (uint32_t)src[r * C + c];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kAwqT; i += kBlock / kAwqT) {
        const int64_t c = c0 + ty + i, r = r0 + tx;
        if (r < R && c < C) {
            const uint32_t v = lds[tx * kPitch + ty + i];
            dst[c * R + r] = (T)(NATURAL ? awq_natural(v) : v);
        }
    }
}

__global__ __launch_bounds__(kBlock) void awq_repack_batch_kernel(const ct_awq_item* __restrict__ items, int n) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kAwqTileWords];
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].first_block <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const ct_awq_item it = items[lo];
    int64_t b = (int64_t)blockIdx.x - it.first_block;
    if (b < it.weight_blocks) {
        awq_weight_tile(it, b, lds);
        return;
    }
    b -= it.weight_blocks;
    if (b < it.zp_blocks) {
        awq_transpose_tile<uint32_t, true>(reinterpret_cast<const uint32_t*>(it.qzeros), reinterpret_cast<uint32_t*>(it.zp_packed), it.G,
                                           it.N >> 3, b, lds);
        return;
    }
    b -= it.zp_blocks;
    awq_transpose_tile<uint16_t, false>(static_cast<const uint16_t*>(it.scales), static_cast<uint16_t*>(it.scale_t), it.G, it.N, b, lds);
}

}  // namespace

}  // namespace ct

using namespace ct;

extern "C" {

int64_t ct_awq_repack_plan(ct_awq_item* items, int n) {
    if (n < 0 || (n > 0 && items == nullptr)) {
        set_error("ct_awq_repack_plan: bad arguments");
        return -1;
    }
    constexpr int64_t kDimMax = int64_t(1) << 31;
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        ct_awq_item& it = items[i];
        if (!(it.qweight && it.scales && it.weight_packed && it.scale_t) || (it.qzeros == nullptr) != (it.zp_packed == nullptr)) {
            set_error("ct_awq_repack_plan: item %d has a NULL pointer (qzeros and zp_packed go together)", i);
            return -1;
        }
        if (!(it.K > 0 && it.N > 0 && it.G > 0 && it.K < kDimMax && it.N < kDimMax && it.G < kDimMax) || it.N % 8) {
            set_error("ct_awq_repack_plan: item %d has shape K %lld, N %lld, G %lld (need positive sizes below 2^31, N a multiple of 8)", i,
                      (long long)it.K, (long long)it.N, (long long)it.G);
            return -1;
        }
        if (it.scale_dt != CT_F16 && it.scale_dt != CT_BF16) {
            set_error("ct_awq_repack_plan: item %d: scales must be float16 or bfloat16 (dtype code %d)", i, it.scale_dt);
            return -1;
        }
        if (it.scale_shape[0] != it.G || it.scale_shape[1] != it.N) {
            set_error("ct_awq_repack_plan: item %d: scales of shape (%lld, %lld), expected (G, N) = (%lld, %lld)", i, (long long)it.scale_shape[0],
                      (long long)it.scale_shape[1], (long long)it.G, (long long)it.N);
            return -1;
        }
        if (it.qzeros && (it.zp_shape[0] != it.G || it.zp_shape[1] != it.N / 8)) {
            set_error("ct_awq_repack_plan: item %d: qzeros of shape (%lld, %lld), expected (G, N / 8) = (%lld, %lld)", i, (long long)it.zp_shape[0],
                      (long long)it.zp_shape[1], (long long)it.G, (long long)(it.N / 8));
            return -1;
        }
        const int64_t W = it.N / 8, KW = cdiv64(it.K, 8);
        it.wide = (W % 4 == 0 && aligned16(it.qweight) ? 1 : 0) | (KW % 4 == 0 && aligned16(it.weight_packed) ? 2 : 0);
        it.weight_blocks = cdiv64(it.K, kAwqTileK) * cdiv64(W, kAwqTileJ);
        it.zp_blocks = it.qzeros ? cdiv64(it.G, kAwqT) * cdiv64(W, kAwqT) : 0;
        it.first_block = blocks;
        blocks += it.weight_blocks + it.zp_blocks + cdiv64(it.G, kAwqT) * cdiv64(it.N, kAwqT);
        if (blocks > kAwqMaxBlocks) {
            set_error("ct_awq_repack_plan: more than %lld workgroups for one launch; split the batch", (long long)kAwqMaxBlocks);
            return -1;
        }
    }
    return blocks;
}

int ct_awq_repack_batch(const ct_awq_item* items_dev, int n, int64_t total_blocks, ct_stream_t stream) {
    CT_REQUIRE(n >= 0 && total_blocks >= 0 && total_blocks <= kAwqMaxBlocks, "ct_awq_repack_batch: bad batch size");
    if (n == 0 || total_blocks == 0) return CT_OK;
    CT_REQUIRE(items_dev != nullptr, "ct_awq_repack_batch: table is NULL");
    hipLaunchKernelGGL(awq_repack_batch_kernel, dim3((unsigned)total_blocks), dim3(kBlock), 0, as_stream(stream), items_dev, n);
    CT_LAUNCH_CHECK("ct_awq_repack_batch");
}

}  // extern "C"
