/*
 * ct_hip.h — C ABI of libct_hip.so: the MI355X (gfx950) implementation of the
 * compressed-tensors compress/decompress hot path.
 *
 * Every entry point takes plain device pointers + sizes + a HIP stream (as void*), launches
 * asynchronously on that stream, performs no host synchronisation and no allocation, and
 * returns a ct_status.  ct_last_error() returns a thread-local message for the last
 * non-OK status.  The functions are re-entrant (no global scratch).
 *
 * Each declaration names the reference interface it replaces; paths are relative to
 * /root/reference/src/compressed_tensors/.  The Python host in compressed_tensors_amd/
 * binds these with ctypes (compressed_tensors_amd/_lib.py); INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Tensors are row-major and contiguous unless a stride parameter says otherwise.
 */
#ifndef CT_HIP_H
#define CT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ct_stream_t; /* hipStream_t */

/* element type codes (shared with the oracle) */
enum ct_dtype {
    CT_F32 = 0,
    CT_F16 = 1,
    CT_BF16 = 2,
    CT_I8 = 3,
    CT_I32 = 4,
    CT_U8 = 5,
    CT_I16 = 6,
    CT_I64 = 7,
    CT_F8E4M3 = 8 /* float8_e4m3fn (OCP: max 448, 0x7f / 0xff = NaN, no inf) */
};

enum ct_status {
    CT_OK = 0,
    CT_ERR_INVALID_ARG = 1, /* maps to ValueError on the Python side */
    CT_ERR_UNSUPPORTED = 2, /* maps to NotImplementedError                */
    CT_ERR_HIP = 3          /* maps to RuntimeError (message has the HIP error string) */
};

const char* ct_last_error(void);
int ct_abi_version(void);

/* ------------------------------------------------------------------------------------
 * Host mailbox — the only entries that wait.  Two points of the reference's interface hand a
 * DEVICE result to the HOST before the call may return: the number of kept values of the
 * sparse-bitmask codec (`tensor[mask]` sizes its result on the host; restated S1 over
 * utils/helpers.py:306-343) and the 2:4 structure verdict of the marlin-24 codec
 * (`tensor_follows_mask_structure(...)` raises from the call, utils/helpers.py:87-109).
 * With torch that is a D2H copy + a synchronisation per call (`.item()`, `.cpu()`: 20-30 us).
 * Here the kernels write the word straight into pinned, device-mapped host memory (one
 * system-scope store) and the host spins on it.
 *   ct_mailbox_alloc     `bytes` of zeroed pinned host memory; *dev_ptr is what the kernels get
 *   ct_mailbox_wait_i64  returns in *value the 64-bit word at host_word as soon as it differs
 *                        from `pending` (the host writes `pending` before the launch); if the
 *                        stream drains first, whatever the word holds then
 *   ct_stream_wait       returns when every launch queued on `stream` has completed (spins on
 *                        hipStreamQuery: ~1 us after completion, no interrupt, no copy) */
int ct_mailbox_alloc(int64_t bytes, void** host_ptr, void** dev_ptr);
int ct_mailbox_free(void* host_ptr);
int ct_mailbox_wait_i64(const int64_t* host_word, int64_t pending, ct_stream_t stream, int64_t* value);
int ct_stream_wait(ct_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Scale / zero-point addressing used by every quantization entry point:
 *     idx(r, c) = (r / rdiv) * scale_cols + (col_group ? col_group[c] : c / cdiv)
 * tensor:  rdiv = rows, cdiv = cols, scale_cols = 1
 * channel: rdiv = 1,    cdiv = cols, scale_cols = 1           (token: same)
 * group:   rdiv = 1 (or rows if the scale has a single row), cdiv = group_size,
 *          scale_cols = cols / group_size
 * block:   rdiv = block_h, cdiv = block_w, scale_cols = ceil(cols / block_w)
 * col_group (nullable, int32[cols], device) carries activation ordering:
 *          argsort(argsort(g_idx)) / group_size  (quantization/lifecycle/forward_helpers.py:147-175)
 * tdt is the torch result dtype of `x / scale` — every intermediate of the reference's
 * eager op sequence is rounded to it (forward_helpers.py:523-546, quant_args.py:460-496).
 * zp may be NULL (no zero point); zdt in {CT_I8, CT_I32, CT_F32, CT_F16, CT_BF16}.
 * ------------------------------------------------------------------------------------ */

/* pack_to_int32(value, num_bits, packed_dim=1)   compressors/pack_quantized/helpers.py:20-101
 * q: int8 (rows, cols); out: int32 (rows, out_row_stride >= ceil(cols*bits/32)) */
int ct_pack_int32(const int8_t* q, int64_t rows, int64_t cols, int bits, int32_t* out,
                  int64_t out_row_stride, ct_stream_t stream);

/* unpack_from_int32(value, num_bits, shape, packed_dim=1)   helpers.py:104-180
 * p: int32 (rows, words) with row stride p_row_stride; out: int8 (rows, cols) */
int ct_unpack_int32(const int32_t* p, int64_t rows, int64_t words, int64_t p_row_stride,
                    int64_t cols, int bits, int8_t* out, ct_stream_t stream);

/* pack_to_int32(zp, num_bits, packed_dim=0).contiguous()   compressors/pack_quantized/base.py:107-110
 * q: int8 (rows, cols) packed along ROWS; out: int32 (ceil(rows*bits/32), cols) contiguous */
int ct_pack_int32_dim0(const int8_t* q, int64_t rows, int64_t cols, int bits, int32_t* out,
                       ct_stream_t stream);

/* unpack_from_int32(zp, num_bits, shape, packed_dim=0)   base.py:147-153
 * p: int32 (words, cols) contiguous; out: int8 (rows, cols) */
int ct_unpack_int32_dim0(const int32_t* p, int64_t words, int64_t cols, int64_t rows, int bits,
                         int8_t* out, ct_stream_t stream);

/* quantize(x, scale, zero_point, args, dtype)   quantization/lifecycle/forward.py:36-73
 * odt in {CT_I8, CT_I32, CT_F32, CT_F16, CT_BF16} */
int ct_quantize(const void* x, int xdt, const void* scale, int sdt, const void* zp, int zdt,
                int64_t rows, int64_t cols, int64_t rdiv, int64_t cdiv, int64_t scale_cols,
                const int32_t* col_group, int bits, int tdt, void* out, int odt, ct_stream_t stream);

/* dequantize(x_q, scale, zero_point, ...)   forward.py:76-145; forward_helpers.py:549-572
 * xq: qdt in {CT_I8, CT_I32, CT_F8E4M3, float types}; arithmetic in sdt; odt in {CT_F32, CT_F16, CT_BF16} */
int ct_dequantize(const void* xq, int qdt, const void* scale, int sdt, const void* zp, int zdt,
                  int64_t rows, int64_t cols, int64_t rdiv, int64_t cdiv, int64_t scale_cols,
                  const int32_t* col_group, void* out, int odt, ct_stream_t stream);

/* fake_quantize(x, scale, zero_point, args)   forward.py:148-181; forward_helpers.py:180-215 */
int ct_fake_quantize(const void* x, int xdt, const void* scale, int sdt, const void* zp, int zdt,
                     int64_t rows, int64_t cols, int64_t rdiv, int64_t cdiv, int64_t scale_cols,
                     const int32_t* col_group, int bits, int tdt, void* out, int odt,
                     ct_stream_t stream);

/* The same three for FLOAT 8-bit args (QuantizationType.FLOAT, num_bits 8; quant_args.py:463-486,
 * utils/helpers.py:212-214): clamp to +-448 and round to float8_e4m3fn instead of rint.  odt of
 * ct_quantize_fp8 in {CT_F8E4M3, CT_F32, CT_F16, CT_BF16}; zero points may be CT_F8E4M3 too.  Dequantize is
 * ct_dequantize with qdt = CT_F8E4M3.  These are the weight paths of float-quantized / naive-quantized(float)
 * (compressors/naive_quantized/base.py:48-126) and mxfp8-quantized (compressors/mxfp8/base.py:47-101). */
int ct_quantize_fp8(const void* x, int xdt, const void* scale, int sdt, const void* zp, int zdt,
                    int64_t rows, int64_t cols, int64_t rdiv, int64_t cdiv, int64_t scale_cols,
                    const int32_t* col_group, int tdt, void* out, int odt, ct_stream_t stream);
int ct_fake_quantize_fp8(const void* x, int xdt, const void* scale, int sdt, const void* zp, int zdt,
                         int64_t rows, int64_t cols, int64_t rdiv, int64_t cdiv, int64_t scale_cols,
                         const int32_t* col_group, int tdt, void* out, int odt, ct_stream_t stream);

/* FLOAT 4-bit args (E2M1; quant_args.py:463-486 -> cast_to_fp4, range +-6 utils/helpers.py:215-217), optionally
 * under a global scale (tensor_group strategy: effective scale = fl32(scale / global_scale[0]), the quotient and the
 * dequantize arithmetic are float32 then, forward_helpers.py:535-538,560-563; tdt must be CT_F32).  Values come back
 * in a float dtype (upstream has no 4-bit storage dtype; the packed weight path is ct_fp4_quant_pack).
 * global_scale: device float32[1] or NULL. */
int ct_quantize_fp4(const void* x, int xdt, const void* scale, int sdt, const void* zp, int zdt,
                    int64_t rows, int64_t cols, int64_t rdiv, int64_t cdiv, int64_t scale_cols,
                    const int32_t* col_group, const float* global_scale, int tdt, void* out, int odt,
                    ct_stream_t stream);
int ct_fake_quantize_fp4(const void* x, int xdt, const void* scale, int sdt, const void* zp, int zdt,
                         int64_t rows, int64_t cols, int64_t rdiv, int64_t cdiv, int64_t scale_cols,
                         const int32_t* col_group, const float* global_scale, int tdt, void* out, int odt,
                         ct_stream_t stream);
/* dequantize(x_q, scale, zero_point, global_scale=...): arithmetic in float32 */
int ct_dequantize_gs(const void* xq, int qdt, const void* scale, int sdt, const void* zp, int zdt,
                     int64_t rows, int64_t cols, int64_t rdiv, int64_t cdiv, int64_t scale_cols,
                     const int32_t* col_group, const float* global_scale, void* out, int odt,
                     ct_stream_t stream);

/* Fused PackedQuantizationCompressor.compress weight path: quantize(dtype=int8) followed by
 * pack_to_int32, without the int8 intermediate.   compressors/pack_quantized/base.py:96-104
 * packed: int32 (rows, ceil(cols*bits/32)) contiguous */
int ct_quant_pack(const void* x, int xdt, const void* scale, int sdt, const void* zp, int zdt,
                  int64_t rows, int64_t cols, int64_t rdiv, int64_t cdiv, int64_t scale_cols,
                  const int32_t* col_group, int bits, int tdt, int32_t* packed, ct_stream_t stream);

/* Round-to-nearest W4 compress in one pass: the min-max observer + calculate_qparams
 * (quantization/utils/helpers.py:50-137) and PackedQuantizationCompressor's weight path
 * (compressors/pack_quantized/base.py:96-104) fused: x is read once, packed int32 (rows, cols/8), scale
 * (rows, cols/group) in x's dtype and zero point int8 (rows, cols/group) come out.  Bit-identical to
 * ct_minmax_qparams followed by ct_quant_pack.  group = 32 * 2^k <= 2048, cols % group == 0, int4. */
int ct_rtn_quant_pack_w4(const void* x, int xdt, int64_t rows, int64_t cols, int64_t group, int symmetric,
                         int32_t* packed, void* scale_out, int8_t* zp_out, ct_stream_t stream);

/* Channel-wise 8-bit round-to-nearest in one pass (W8A8 int8 / FP8 weights): per-row min-max observer +
 * calculate_qparams (helpers.py:50-137) + quantize(dtype = int8 resp. float8_e4m3fn) (forward.py:36-73).  out: one
 * byte per element; scale_out (rows, 1) in x's dtype; zp_out int8 (rows, 1), required when !symmetric (int8 only).
 * cols % 8 == 0, cols <= CT_RTN_CHANNEL8_MAX_COLS.  Bit-identical to ct_minmax_qparams(_float) followed by ct_quantize(_fp8).
 * Three forms by row length, the same bits in each (min and max do not depend on the order): a WAVE per row (rows of at most 2048 columns, and
 * asymmetric rows of at most 8192: the row in the wave's registers, no LDS), a WORKGROUP per row (up to 16384 columns: the row in the registers of
 * 256 threads, one barrier) and the LONG form beyond (the first 16384 columns in registers, the rest of the row read twice by the same workgroup:
 * the second read comes from the L2). */
#define CT_RTN_CHANNEL8_MAX_COLS 65536
int ct_rtn_quant_channel8(const void* x, int xdt, int64_t rows, int64_t cols, int fp8, int symmetric, void* out,
                          void* scale_out, int8_t* zp_out, ct_stream_t stream);

/* Fused PackedQuantizationCompressor.decompress weight path: unpack_from_int32 followed by
 * dequantize.   base.py:155-161.  zp is the UNPACKED zero point (int8) or NULL. */
int ct_unpack_dequant(const int32_t* packed, int64_t rows, int64_t words, int64_t cols, int bits,
                      const void* scale, int sdt, const void* zp, int zdt, int64_t rdiv,
                      int64_t cdiv, int64_t scale_cols, const int32_t* col_group, void* out, int odt,
                      ct_stream_t stream);

/* Activation ordering (quantization/lifecycle/forward_helpers.py:147-175): the `col_group` table the entries above take, from a module's `weight_g_idx` —
 * col_group[c] = (position of column c in the stable sort of g_idx) / group_size, or c / group_size while g_idx still holds a -1 (not initialised; the
 * reference tests `-1 in g_idx` on the host, here the choice is made on the device: no synchronisation).  `mode_word`: one int32 that receives what was
 * found (0: a -1 left, 1: balanced — every group exactly group_size columns, the usual case: no sort at all —, 2: the general stable rank).  One small launch. */
int ct_gidx_col_group(const int32_t* g_idx, int64_t cols, int64_t group_size, int32_t* col_group, int32_t* mode_word, ct_stream_t stream);

/* Batched W4A16 (int4, 16-bit weights and scales of one dtype, group or channel scales, int8 zero
 * points): one launch for a whole table of tensors — the per-module loop of
 * ModelCompressor.compress_model / decompress_model (compressors/model_compressors/
 * model_compressor.py:167-169,196-198) without a launch per module.
 * The caller fills src / scale / zp / dst / rows / cols / group of every item, calls
 * ct_w4_batch_plan on the HOST copy (fills the derived fields, returns the workgroup count or -1),
 * copies the table to the device and launches.  direction: 0 = compress (src = weights,
 * dst = packed int32), 1 = decompress (src = packed, dst = weights). */
typedef struct ct_w4_item {
    const void* src;
    const void* scale;
    const void* zp; /* int8, shape of scale, or NULL (with zp_packed on the decompress side: an OUTPUT, see there) */
    void* dst;
    int64_t rows, cols, group; /* group <= 0 or >= cols: one scale per row */
    int64_t first_block;       /* derived */
    int64_t units;             /* derived */
    int32_t upg_shift, upg;    /* derived */
    /* W4 batches only (ct_zp4_* / ct_q8_* ignore it; NULL = none).  The zero points of an asymmetric scheme in their STORED form,
     * int32 (ceil(rows * 4 / 32), cols / group) = pack_to_int32(zp, 4, packed_dim=0) (compressors/pack_quantized/base.py:107-110),
     * handled by the SAME launch as the weights (round 6):
     *   compress   (direction 0): OUTPUT.  `zp` (required) is quantized against as always, and tail workgroups of the item's block range
     *              also write its packed form here.  Any item the batch takes may carry it.
     *   decompress (direction 1): INPUT.  The kernel takes every zero point straight from the packed words — no unpacked copy has to
     *              exist first — and, when `zp` is non-NULL, tail workgroups also WRITE the unpacked int8 (rows, cols / group) zero
     *              points there (what decompress stores back into the state dict, base.py:147-153).  Needs group == 128,
     *              cols % 512 == 0, a 16-byte aligned zp_packed and an 8-byte aligned scale (ct_w4_batch_plan refuses the item
     *              otherwise: unpack with ct_zp4_pack_dim0_batch first and pass `zp`). */
    void* zp_packed;
    int64_t main_blocks;       /* derived: the item's blocks in front of its zero-point tail */
    uint32_t g_magic;          /* derived: n / (cols / group) == (n * g_magic) >> g_shift for n < 2^31 */
    int32_t g_shift;           /* derived */
} ct_w4_item;                  /* 13 64-bit words */
int64_t ct_w4_batch_plan(ct_w4_item* items_host, int n, int direction);
int ct_quant_pack_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int dt, ct_stream_t stream);
int ct_unpack_dequant_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int dt, ct_stream_t stream);

/* One asymmetric W4A16 tensor, zero points in their stored (packed) form, ONE launch per direction — the single-module
 * PackedQuantizationCompressor.compress / .decompress of an asymmetric scheme (base.py:96-110 resp. 147-161) without the separate
 * pack_to_int32(zp, 4, packed_dim=0) / unpack_from_int32(..., packed_dim=0) launch.  The kernels are the batch kernels on a table of
 * one item handed over by value (no table in device memory, no plan call): same bits as the batch and as ct_quant_pack +
 * ct_pack_int32_dim0 resp. ct_unpack_int32_dim0 + ct_unpack_dequant.
 *   ct_quant_pack_w4_zp      x (rows, cols) bf16 / fp16, scale (rows, cols / group) of x's dtype, zp int8 (rows, cols / group) ->
 *                            packed int32 (rows, cols / 8) and zp_packed int32 (ceil(rows / 8), cols / group).
 *                            cols % 32 == 0, group % 32 == 0, cols % group == 0 (group <= 0 or >= cols: channel-wise).
 *   ct_unpack_dequant_w4_zp  packed + scale + zp_packed -> out (rows, cols) of the scale's dtype sdt and, if zp_out != NULL, the
 *                            unpacked int8 zero points.  group == 128 and cols % 512 == 0 (CT_ERR_UNSUPPORTED otherwise: unpack the
 *                            zero points with ct_unpack_int32_dim0 and call ct_unpack_dequant). */
int ct_quant_pack_w4_zp(const void* x, int xdt, const void* scale, const int8_t* zp, int64_t rows, int64_t cols, int64_t group,
                        int32_t* packed, int32_t* zp_packed, ct_stream_t stream);
int ct_unpack_dequant_w4_zp(const int32_t* packed, const void* scale, int sdt, const int32_t* zp_packed, int64_t rows, int64_t cols,
                            int64_t group, void* out, int8_t* zp_out, ct_stream_t stream);

/* Batched 4-bit zero-point packing along rows: pack_to_int32(zp, 4, packed_dim=0) / unpack_from_int32(..., packed_dim=0) of
 * PackedQuantizationCompressor (compressors/pack_quantized/base.py:107-110,147-153) for the zero points of many asymmetric
 * modules in one launch.  Items: src / dst + rows, cols of the UNPACKED int8 matrix (the other fields are ignored);
 * direction 0: int8 (rows, cols) -> int32 (ceil(rows * 4 / 32), cols); 1: the inverse.  Plan on the host copy first. */
int64_t ct_zp4_batch_plan(ct_w4_item* items_host, int n);
int ct_zp4_pack_dim0_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int direction, ct_stream_t stream);

/* Batched round-to-nearest W4 compress in one pass: ct_rtn_quant_pack_w4 — the min-max observer + calculate_qparams
 * (quantization/utils/helpers.py:50-137) and PackedQuantizationCompressor's weight path (compressors/pack_quantized/base.py:96-110) fused —
 * for a whole table of tensors in one launch: the data-free counterpart of ct_quant_pack_batch.  The table is `struct ct_w4_item` read this way:
 * src = the weights, dst = packed int32 (rows, cols / 8), scale = OUTPUT (rows, cols / group) in the weights' dtype, zp = OUTPUT int8 of the same
 * shape (NULL only in a table launched with symmetric != 0: the store is then skipped), group <= 0 or >= cols = one group per row, zp_packed =
 * NULL.  ct_rtn_w4_batch_plan (host only) admits what ct_rtn_quant_pack_w4 admits, per item — 16-byte aligned src / dst, cols % group == 0,
 * group = 32 * 2^k <= 2048, the scale output — fills the derived fields and returns the workgroup count, or -1 with the error text set (also
 * for 2^31 workgroups or more).  The stored zero points of an asymmetric scheme (pack_to_int32(zp, 4, packed_dim=0), base.py:107-110) depend on
 * zero points that other workgroups of the launch compute: issue ct_zp4_pack_dim0_batch over the asymmetric items behind it on the same stream.
 * Bit-identical to ct_rtn_quant_pack_w4 per item. */
int64_t ct_rtn_w4_batch_plan(ct_w4_item* items_host, int n);
int ct_rtn_quant_pack_w4_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int dt, int symmetric, ct_stream_t stream);

/* The same one pass for the integer widths next to 4 and 8 (the reference's W2A16 ... W7A16 presets): bits in {2, 3, 5, 6, 7}.  x is read once;
 * packed int32 (rows, cols * bits / 32) = pack_to_int32(quantize(x), bits) (compressors/pack_quantized/helpers.py:74-93), scale (rows, cols / group)
 * in x's dtype and zero point int8 (rows, cols / group) come out.  Bit-identical to ct_minmax_qparams followed by ct_quant_pack.  Needs bf16 / fp16
 * weights, group = 32 * 2^k <= 2048, cols % group == 0, a 16-byte aligned x, 4-byte aligned packed words.  bits of 4 or 8 and anything outside 2..7
 * return CT_ERR_UNSUPPORTED with the entry that serves that width named in ct_last_error (ct_rtn_quant_pack_w4, ct_rtn_quant_group8 with words != 0,
 * ct_minmax_qparams + ct_quant_pack): there is no fallback inside the library.
 * The table form reads `struct ct_w4_item` exactly as ct_rtn_quant_pack_w4_batch does — src = the weights, dst = packed int32 (rows, cols * bits / 32),
 * scale / zp = OUTPUTS (zp NULL only in a table launched with symmetric != 0), group <= 0 or >= cols = one group per row, zp_packed = NULL — with ONE
 * width per launch.  ct_rtn_wb_batch_plan (host only) admits per item what ct_rtn_quant_pack_wb admits, fills the derived fields and returns the
 * workgroup count, or -1 with the reason in ct_last_error.  The stored zero points of an asymmetric scheme (pack_to_int32(zp, bits, packed_dim=0))
 * come from ct_pack_int32_dim0 behind the launch.  Bit-identical to ct_rtn_quant_pack_wb per item. */
int ct_rtn_quant_pack_wb(const void* x, int xdt, int64_t rows, int64_t cols, int64_t group, int bits, int symmetric, int32_t* packed,
                         void* scale_out, int8_t* zp_out, ct_stream_t stream);
int64_t ct_rtn_wb_batch_plan(ct_w4_item* items_host, int n, int bits);
int ct_rtn_quant_pack_wb_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int dt, int bits, int symmetric, ct_stream_t stream);

/* Block-wise 8-bit round-to-nearest in one pass (FP8_BLOCK weights; INT8 blocks, symmetric or not): the block min-max observer over
 * block_h x block_w blocks (maybe_pad_tensor_for_block_quant, helpers.py:400-428: the zero padding of a ragged last row of blocks never exists
 * here, calculate_qparams clamps min <= 0 <= max anyway) + calculate_qparams (helpers.py:50-137) + quantize(strategy = block)
 * (forward_helpers.py:62-115).  out: one byte per element, or NULL = the qparams only (the block observer); scale_out (ceil(rows / block_h),
 * cols / block_w) in x's dtype; zp_out int8 of the same shape, required when !symmetric (int8 only).  FLOAT codes are quantized as with the
 * all-zero zero point of a calibrated scheme present (a -0.0 code becomes +0.0), like ct_rtn_quant_channel8.  Needs bf16 / fp16 weights, block
 * sides powers of two, block_w >= 16, block_h * block_w <= 16384, cols % block_w == 0, 16-byte aligned x and out.  One workgroup per block.
 * The table form takes `struct ct_w4_item` rows read this way: src = the weights, dst = the codes or NULL, scale / zp = OUTPUTS (zp NULL in a FLOAT
 * or symmetric table), group = -((block_h << 24) | block_w) as the 8-bit tables encode blocks; ct_rtn_block8_batch_plan (host only) admits per item what
 * ct_rtn_quant_block8 admits, fills the derived fields and returns the workgroup count — ceil(rows / block_h) * (cols / block_w) per item —, or -1 with
 * the reason named in ct_last_error.  Bit-identical to ct_rtn_quant_block8 per item. */
int ct_rtn_quant_block8(const void* x, int xdt, int64_t rows, int64_t cols, int64_t block_h, int64_t block_w, int fp8, int symmetric, void* out,
                        void* scale_out, int8_t* zp_out, ct_stream_t stream);
int64_t ct_rtn_block8_batch_plan(ct_w4_item* items_host, int n);
int ct_rtn_quant_block8_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int xdt, int fp8, int symmetric, ct_stream_t stream);

/* The table form of ct_rtn_quant_channel8 (FP8_DYNAMIC / W8A8 weights of a whole shard in one launch).  `struct ct_w4_item` rows read this way:
 * src = the weights, dst = the codes, scale = the scale OUTPUT (rows, 1) in the weights' dtype, zp = the int8 zero-point OUTPUT (rows, 1) or NULL
 * (NULL in a FLOAT or symmetric table: the store is skipped; an item WITH a zero-point output is planned as asymmetric), group and zp_packed are
 * ignored.  ct_rtn_channel8_batch_plan (host only) admits per item what ct_rtn_quant_channel8 admits — rows, cols > 0, cols % 8 == 0, cols <=
 * CT_RTN_CHANNEL8_MAX_COLS, src / dst / scale present, src and dst 16-byte aligned, fewer than 2^31 workgroups — and writes into the derived fields:
 *   upg_shift   = the item's form: 0 a wave per row, 1 a workgroup per row, 2 the long form (the rule of ct_rtn_quant_channel8)
 *   upg         = 16-byte units per row (cols / 8)
 *   units       = rows * upg
 *   main_blocks = the item's workgroups: ceil(rows / 4) in the wave form (four rows per workgroup), rows in the other two
 *   first_block = the workgroups in front of the item; g_magic = g_shift = 0
 * It returns the table's workgroup count, or -1 with the reason named in ct_last_error.  One table may hold items of all three forms; a launch is
 * one dtype, FLOAT or INT, symmetric or not.  Bit-identical to ct_rtn_quant_channel8 per item: the kernels share the per-row bodies. */
int64_t ct_rtn_channel8_batch_plan(ct_w4_item* items_host, int n);
int ct_rtn_quant_channel8_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int xdt, int fp8, int symmetric, ct_stream_t stream);

/* Group-wise 8-bit round-to-nearest in one pass (MXFP8; W8A16; any FLOAT / INT 8-bit group scheme): the min-max observer over groups of `group`
 * consecutive columns + calculate_qparams (helpers.py:50-137, mxfp_utils.py:37-143) + quantize(strategy = group) (forward_helpers.py:62-115)
 * (+ compress_mx_scale).  kind is the observer's numbering (ct_minmax_qparams_float): 0 INT (symmetric or not; int8 codes, or with words != 0
 * the (code + 128) bytes of the 8-bit pack-quantized words), 1 FP8 (symmetric; float8_e4m3fn codes), 4 MXFP8 (symmetric, group == 32; float8_e4m3fn
 * codes and one E8M0 exponent byte per group in e8m0_out; code_table = the table of ct_mx_scale_compress, 65536 bytes of the scale's dtype,
 * read only for a scale that is inf or NaN, NULL for the other kinds).  out: one byte per element; scale_out (rows, cols / group) in x's dtype (optional
 * for MXFP8, required otherwise); zp_out int8 of that shape: required when !symmetric, optional for symmetric INT, NULL for FLOAT.  FLOAT codes
 * are quantized as with the all-zero zero point of a calibrated scheme present, like ct_rtn_quant_channel8.  Needs bf16 / fp16 weights,
 * group = 32 * 2^k <= 1024 (one wave reduces a group), cols % group == 0, 16-byte aligned x and out.  Bit-identical to ct_minmax_qparams /
 * ct_minmax_qparams_float with cdiv = group followed by ct_quantize / ct_quantize_fp8 / ct_quant_pack at 8 bits (and ct_mx_scale_compress).
 * The table form takes `struct ct_w4_item` rows read this way: src = the weights, dst = the codes, scale = the float-scale OUTPUT (may be NULL in
 * an MXFP8 table), zp = the int8 zero-point OUTPUT or NULL, zp_packed = the E8M0 OUTPUT of an MXFP8 table, group = the group size;
 * ct_rtn_group8_batch_plan (host only) admits per item what ct_rtn_quant_group8 admits, fills the derived fields and returns the workgroup count
 * — ceil(rows * cols / 4096) per item —, or -1 with the reason named in ct_last_error.  Bit-identical to ct_rtn_quant_group8 per item. */
int ct_rtn_quant_group8(const void* x, int xdt, int64_t rows, int64_t cols, int64_t group, int kind, int symmetric, int words, void* out,
                        void* scale_out, int8_t* zp_out, uint8_t* e8m0_out, const uint8_t* code_table, ct_stream_t stream);
int64_t ct_rtn_group8_batch_plan(ct_w4_item* items_host, int n);
int ct_rtn_quant_group8_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int xdt, int kind, int symmetric, int words, const uint8_t* code_table,
                              ct_stream_t stream);

/* Batched 8-bit codecs (Naive / Int / FloatQuantizationCompressor.compress / decompress, compressors/naive_quantized/
 * base.py:48-126, looped per module by model_compressor.py:167-169,196-198): quantize to int8 (num_bits <= 8, clamped to the
 * num_bits range) or float8_e4m3fn, and the inverse, for a whole table of 16-bit tensors in one launch.  Same table type and
 * protocol as the W4 batch; `group` counts the consecutive elements that share one scale: 0 or cols (one per row), a
 * divisor of cols, or >= rows * cols (one per tensor); a NEGATIVE group is the block strategy (forward.py:198-216, the FP8-block
 * checkpoints): -group = (rows per block << 24) | columns per block, both powers of two, the width >= 16 and a divisor of cols,
 * scale / zero point of shape (ceil(rows / block rows), cols / block columns).  Needs cols % 16 == 0 and group % 16 == 0; zero points int8 or NULL —
 * `fp8` = 2 (round 6): float8 codes whose zero points are float8_e4m3fn bytes (what a calibrated FLOAT scheme carries; 1: int8 or none);
 * `fp8` = 3 (round 6): int8 codes stored + 128, four to an int32 word — the 8-bit words of pack_to_int32 (pack_quantized/helpers.py:39-75;
 * PackedQuantizationCompressor with num_bits = 8, e.g. the W8A16 preset): dst / src = int32 (rows, cols / 4), cols % 32 == 0.
 * direction: 0 = quantize (src = weights, dst = codes), 1 = dequantize (src = codes, dst = weights). */
int64_t ct_q8_batch_plan(ct_w4_item* items_host, int n, int direction);
int ct_q8_quant_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int dt, int fp8, int bits,
                      ct_stream_t stream);
int ct_q8_dequant_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int dt, int fp8, ct_stream_t stream);

/* Min/max observer + calculate_qparams for weight groups (rows x ceil(cols/cdiv) groups of
 * cdiv consecutive columns).   quantization/utils/helpers.py:50-137
 * scale_out has x's dtype; zp_out is int8 (may be NULL for symmetric). */
int ct_minmax_qparams(const void* x, int xdt, int64_t rows, int64_t cols, int64_t cdiv, int bits,
                      int symmetric, void* scale_out, int8_t* zp_out, ct_stream_t stream);

/* The same reduction for the symmetric FLOAT schemes (helpers.py:50-137, mxfp_utils.py:37-143); amax = max(|min(mn, 0)|,
 * |max(mx, 0)|) of each group:
 *   kind 1 FP8    scale = rnd_X(amax / 448), zero -> eps(X)                                     scale_out: x's dtype
 *   kind 2 NVFP4  scale = float8_e4m3fn(clamp(global_scale * rnd_X(amax / 6), +-448)), 0 -> 1/8  scale_out: float32
 *   kind 3 MXFP4 / 4 MXFP8 (group 32): amax's significand rounded at a quarter and masked off, E8M0 exponent
 *          127 + log2 - 2 (resp. - 8) through uint8, scale = 2^(e - 127) in x's dtype, zero -> 1 scale_out: x's dtype
 *   kind 5 the raw amax of each group in x's dtype (the input of generate_gparam, helpers.py:308-337)
 * Zero points of these schemes are all-zero tensors of the scheme's zp_dtype (made by the host). */
int ct_minmax_qparams_float(const void* x, int xdt, int64_t rows, int64_t cols, int64_t cdiv, int kind,
                            const float* global_scale, void* scale_out, ct_stream_t stream);

/* Dynamic activation QDQ in one pass: compute_dynamic_scales_and_zp (quantization/utils/helpers.py:140-195, with
 * calculate_qparams, helpers.py:50-137) followed by fake_quantize (quantization/lifecycle/forward.py:148-181,
 * forward_helpers.py:180-215) — the dynamic branch of forward_quantize (forward.py:304-335).  x is `segs` contiguous
 * segments of `seg_len` elements, one scale each: a token row, or a group.  kind: 0 INT (bits, symmetric; zero point int8),
 * 1 FP8, 2 NVFP4 (global_scale: device float32[1] or NULL), 3 MXFP4, 4 MXFP8, with the scales of ct_minmax_qparams_float.
 * out (nullable: scales only) has x's dtype.  scale_out (nullable, segs entries) has x's dtype, float32 for NVFP4 under a
 * global scale.  zp_out (nullable, segs bytes) has zdt: CT_I8 for INT; CT_F8E4M3, CT_U8 or CT_I8 zeros for the FLOAT kinds.
 * One launch; segments of 8 * 2^k <= 512 elements are reduced inside a wave, longer ones by one workgroup each. */
int ct_dynamic_qdq(const void* x, int xdt, int64_t segs, int64_t seg_len, int kind, int bits, int symmetric,
                   const float* global_scale, void* out, void* scale_out, void* zp_out, int zdt, ct_stream_t stream);

/* The same with ONE segment of `numel` elements (tensor strategy; token strategy on a 1-D / 2-D input, whose reduce dims
 * are empty upstream, helpers.py:187-188) in two launches: min / max partials into `workspace` (device memory of
 * CT_DYNAMIC_WORKSPACE_BYTES, no initialisation needed), then the QDQ.  scale_out / zp_out: one entry. */
#define CT_DYNAMIC_PARTS 1024
#define CT_DYNAMIC_WORKSPACE_BYTES 16384
int ct_dynamic_qdq_tensor(const void* x, int xdt, int64_t numel, int kind, int bits, int symmetric,
                          const float* global_scale, void* workspace, void* out, void* scale_out, void* zp_out, int zdt,
                          ct_stream_t stream);

/* The Sylvester Hadamard rotation of HadamardTransform.forward (transform/factory/hadamard.py:91-108; the matrix of
 * transform/utils/hadamard.py:21-50, block-diagonal as in transform/utils/matrix.py:124-158) as a fast Walsh-Hadamard
 * butterfly: out = FWHT_n(x) / sqrt(n) over every run of n consecutive elements (n a power of two that divides numel), no
 * n x n matrix and no GEMM.  dt: CT_BF16, CT_F16 or CT_F32 for x and out alike.  acc64: 0 accumulates in float32 (online
 * rotations), 1 in float64 (fused rotations: hadamard.py:44); the sum is divided once by sqrt(n) in that type and rounded to
 * dt as torch's cast does.  One launch.  n up to 16384, beyond that CT_ERR_UNSUPPORTED; x and
 * out are 16-byte aligned and distinct. */
int ct_hadamard_rows(const void* x, void* out, int dt, int64_t numel, int64_t n, int acc64, ct_stream_t stream);

/* The same along dim 0 of a row-major rows x cols matrix (n divides rows): Linear `weight_output`, Embedding `weight_input`
 * (matrix.py:107-114).  Three launches: transpose into `workspace` (device memory of rows * cols elements of dt), the row
 * form in place, transpose back into out. */
int ct_hadamard_cols(const void* x, void* out, void* workspace, int dt, int64_t rows, int64_t cols, int64_t n, int acc64,
                     ct_stream_t stream);

/* The random-hadamard rotation (transform/factory/random_hadamard.py; the matrix of transform/utils/hadamard.py:53-151) of size
 * n = k * 2^m over every run of n consecutive elements.  The matrix is W = diag(signs) * (had_k (x) H_M)^T, M = n / k, H_M the
 * Sylvester matrix; a run is a k x M matrix with M contiguous.  transposed == 0: out = x @ W / sqrt(n) (signs, then the mix and
 * the butterfly); transposed == 1: out = x @ W^T / sqrt(n) (had_k^T, the signs last).
 *   had_k   int8, k x k, row-major, entries +-1; NULL exactly when k == 1
 *   signs   int8, n entries of +-1, 8-byte aligned; NULL for none
 *   acc64   0: float32 accumulation (online), 1: float64 (fused locations); one division by fl(sqrt n) in that type
 * Forms: k == 1 the butterfly of ct_hadamard_rows with signs (n <= 16384); k > 1 with 16-bit x, acc64 == 0 and 8 <= M <= 128:
 * ONE launch, the mix on the matrix cores (exact: +-1 times a 16-bit float, float32 accumulation); every other k > 1 case two
 * launches on the vector ALU through `workspace` (ct_hadamard_k_workspace_bytes; may be NULL when that returns 0).
 * CT_ERR_UNSUPPORTED: k > 256, n > 32768 with k > 1, n > 16384 with k == 1, M > 4096 in the vector form, misaligned tensors. */
int ct_hadamard_k_rows(const void* x, void* out, int dt, int64_t numel, int64_t n, int64_t k, const int8_t* had_k,
                       const int8_t* signs, int transposed, int acc64, void* workspace, ct_stream_t stream);

/* The same along dim 0 of a row-major rows x cols matrix (n divides rows), on the transposes of ct_hadamard_cols: transpose
 * into `workspace`, the row form in place, transpose back.  workspace: ct_hadamard_k_workspace_bytes(..., cols_form = 1). */
int ct_hadamard_k_cols(const void* x, void* out, int dt, int64_t rows, int64_t cols, int64_t n, int64_t k, const int8_t* had_k,
                       const int8_t* signs, int transposed, int acc64, void* workspace, ct_stream_t stream);

/* bytes of device workspace the two entries above need for `numel` elements (host arithmetic only); -1 for bad arguments */
int64_t ct_hadamard_k_workspace_bytes(int dt, int64_t numel, int64_t n, int64_t k, int acc64, int cols_form);

/* The permuted rotation of `TransformScheme.randomize=True` (transform/factory/hadamard.py:94-95: the weight W[p][:, p]) in one
 * launch: over every run of n consecutive elements, out[j] = z[p[j]] with z = T(g), g[k] = x[q[k]], q = argsort(p) and T the
 * rotation of ct_hadamard_rows (signs == NULL) or of ct_hadamard_k_rows with k == 1 (signs, transposed as there; the signs sit
 * at the natural positions of g / z).  The bits are those of gather by q -> that entry -> gather by p.
 *   gather_in   q: n entries of 16 bits, 16-byte aligned device memory
 *   gather_out  p: likewise
 * Every entry is masked with n - 1 before it is used: no table content addresses outside its run (the caller validates that
 * the tables are permutations).  n a power of two up to 16384 (acc64 == 0) or 8192 (acc64 == 1), beyond that
 * CT_ERR_UNSUPPORTED; x and out are 16-byte aligned and may be the same tensor. */
int ct_hadamard_perm_rows(const void* x, void* out, int dt, int64_t numel, int64_t n, int acc64, const void* gather_in,
                          const void* gather_out, const int8_t* signs, int transposed, ct_stream_t stream);

/* The same along dim 0 of a row-major rows x cols matrix (n divides rows), as ct_hadamard_cols: transpose into `workspace`
 * (rows * cols elements of dt), the permuted row form in place, transpose back.  Three launches. */
int ct_hadamard_perm_cols(const void* x, void* out, void* workspace, int dt, int64_t rows, int64_t cols, int64_t n, int acc64,
                          const void* gather_in, const void* gather_out, const int8_t* signs, int transposed, ct_stream_t stream);

/* HadamardTransform.forward (online, float32 accumulation) followed by the dynamic branch of forward_quantize, one launch:
 * r = round_to_xdt(FWHT_n(x) / sqrt(n)) over runs of n elements, then ct_dynamic_qdq's observer / calculate_qparams /
 * fake_quantize over runs of seg_len elements of r.  rotated_out (nullable) receives r.  out / scale_out / zp_out / zdt /
 * kind / bits / symmetric / global_scale as in ct_dynamic_qdq.  Output, scale and zero point are the bits ct_hadamard_rows
 * followed by ct_dynamic_qdq produce.  Fused: n <= 512 with seg_len = 8 * 2^k <= 512 (in-wave); n = 1024 .. 8192 with such a
 * seg_len or seg_len == n (one workgroup per block); n <= 512 dividing a longer seg_len of up to 32768 elements (a token row of
 * head-dim blocks).  CT_ERR_UNSUPPORTED for a combination it does not fuse: one segment (the tensor form), 1024 <= n < seg_len,
 * longer rows, n > 8192 (16384 measured slower than the two launches), tensors that are not 16-byte aligned. */
int ct_hadamard_dynamic_qdq(const void* x, int xdt, int64_t numel, int64_t n, int64_t seg_len, int kind, int bits, int symmetric,
                            const float* global_scale, void* rotated_out, void* out, void* scale_out, void* zp_out, int zdt,
                            ct_stream_t stream);

/* Static quantize / dequantize / fake_quantize of the query, key and value states of an attention module
 * (modeling/attention.py, modeling/kvcache.py -> forward_quantize -> forward_helpers.py:180-215, 525-572): one or two 4-D
 * tensors (B, H, S, D) read and written IN PLACE through their strides.  The last dimension has stride 1; the b / h / s
 * strides of input and output are non-negative element counts (0: an expanded dimension).  scale / zp hold one entry
 * (`per_head` 0, the tensor strategy) or H entries (`per_head` 1, the attn_head strategy: entry h).  A row of D elements is one
 * scale and one contiguous run; rows of whole 8-element units whose bases and strides keep the units aligned (16 bytes of a
 * 16-bit dtype) move as vectors, everything else element by element.  B * H * S < 2^31 per tensor. */
typedef struct ct_attn_tensor {
    const void* x;
    void* out;
    const void* scale;
    const void* zp;                /* NULL: symmetric */
    int64_t B, H, S, D;
    int64_t x_stride[3];           /* b, h, s: elements */
    int64_t out_stride[3];
    int64_t per_head;
} ct_attn_tensor;                  /* 15 64-bit words */

/* mode 0 fake_quantize, 1 quantize, 2 dequantize; kind 0 INT (bits 1..8), 1 FLOAT 8-bit (float8_e4m3fn; bits ignored).
 * xdt: a float dtype (modes 0, 1), or CT_I8 / CT_I32 / CT_F8E4M3 / a float dtype (mode 2).  tdt: the torch result dtype of
 * x / scale (modes 0, 1).  odt: a float dtype (modes 0, 2); CT_I8 / CT_I32 / CT_F8E4M3 / a float dtype (mode 1).  n = 2: both
 * tensors (K and V) share every dtype, the kind, bits and mode, and are served by ONE launch.  The descriptors travel as
 * kernel arguments: `tensors` is host memory, nothing is uploaded and the library keeps no device state.  The results are the
 * bits ct_fake_quantize{,_fp8} / ct_quantize{,_fp8} / ct_dequantize give on the same values. */
int ct_attn_qdq(const ct_attn_tensor* tensors, int n, int mode, int kind, int bits, int xdt, int sdt, int zdt, int tdt, int odt,
                ct_stream_t stream);

/* ct_hadamard_rows over runs of `rot_size` elements of the last dimension (float32 accumulation) followed by ct_attn_qdq, in ONE
 * launch: the strided input is read once, rotated in registers and quantized; the output holds the bits of the two launches.
 * `tensors` / `n` / kind / bits / the dtype codes are ct_attn_qdq's; mode is 0 (fake_quantize) or 1 (quantize) — dequantize is
 * CT_ERR_INVALID_ARG.  rot_mask: bit i set = tensor i is rotated (K and V of one cache update: 1 — K rotated, V quantized only).
 * rot_size: a power of two (anything else: CT_ERR_INVALID_ARG, the reference's ValueError).  CT_ERR_UNSUPPORTED outside
 * 2 <= rot_size <= 512, for a rotated tensor whose D is not a multiple of rot_size, for D % 8 != 0 or D / 8 > 256 (a row is one
 * pass of one 8-element unit per lane) and for tensors outside ct_attn_qdq's vector form (bases and strides that keep the units
 * aligned on both sides).  Allocates nothing, never synchronises, keeps no device state. */
int ct_attn_rot_qdq(const ct_attn_tensor* tensors, int n, int rot_size, int rot_mask, int mode, int kind, int bits, int xdt, int sdt,
                    int zdt, int tdt, int odt, ct_stream_t stream);

/* The min-max calibration observer of the states ct_attn_qdq serves (an observer's forward: torch.amin / amax per head or per
 * tensor, then quantization/utils/helpers.py:50-137 calculate_qparams): one or two 4-D tensors (B, H, S, D) read IN PLACE through
 * their strides (as ct_attn_tensor: unit last stride, non-negative b / h / s element strides, 0 = an expanded dimension); rows of
 * whole aligned 8-element units move as vectors, everything else element by element.  `per_head` 0: one entry (the tensor
 * strategy); 1: H entries (attn_head), at most 1024 (more: CT_ERR_UNSUPPORTED).
 * `state`: caller-owned device memory, 2 * entries 32-bit order keys — all minimum keys, then all maximum keys.  A key is the
 * float32 bit pattern b of an element mapped by b ^ ((b >> 31, arithmetic) & 0x7fffffff): signed integer order == float order, a
 * positive NaN above +inf, a negative NaN below -inf.  Armed (empty) state: 0x7fffffff in the minimum half, 0x80000000 in the
 * maximum half.  The call folds the tensor into the state with integer min / max (exact, order-free: bit-deterministic), then
 * writes `scale` (dtype sdt) and `zp` (dtype zdt; NULL: not written) of the running extremes and, where given, `min_vals` /
 * `max_vals` (dtype xdt; both NaN where a NaN was seen).  keep 0: the state is re-armed behind the call (a memoryless observer);
 * 1: it stays, and the next call folds into it. */
typedef struct ct_attn_observe_tensor {
    const void* x;
    int32_t* state;
    void* scale;
    void* zp;                      /* NULL: not written */
    void* min_vals;                /* NULL: not written */
    void* max_vals;
    int64_t B, H, S, D;
    int64_t x_stride[3];           /* b, h, s: elements */
    int64_t per_head;
} ct_attn_observe_tensor;          /* 14 64-bit words */

/* kind 0 INT (bits 1..8, symmetric or not), 1 FLOAT 8-bit (float8_e4m3fn, symmetric; bits ignored), 2 the NVFP4 global scale: same fold, same
 * state, and `scale` (sdt must be float32, zp NULL) receives generate_gparam(min, max) of the running extremes (helpers.py:308-337, the
 * arithmetic of ct_generate_gparam below, evaluated in xdt) — what an observer's get_global_scale returns.  xdt: a float dtype; the
 * arithmetic of calculate_qparams runs in it, as ct_minmax_qparams{,_float} run it.  n = 2: both tensors (K and V) share every
 * argument and every launch.  Two launches (fold, finalize), whatever the size; the descriptors travel as kernel arguments.
 * Allocates nothing, never synchronises, keeps no device state.  CT_ERR_INVALID_ARG for a negative shape or stride, an empty
 * tensor (the minimum of no elements is undefined: torch.amin raises) and B * H * S >= 2^31. */
int ct_attn_observe(const ct_attn_observe_tensor* tensors, int n, int kind, int bits, int symmetric, int xdt, int sdt, int zdt, int keep,
                    ct_stream_t stream);

/* Dynamic group QDQ of the states ct_attn_qdq serves: compute_dynamic_scales_and_zp + fake_quantize (helpers.py:140-195,
 * lifecycle/forward.py:292-329) of one or two 4-D tensors (B, H, S, D) read and written IN PLACE through their strides (as
 * ct_attn_tensor), over groups of `group` elements that lie inside a row of D — the group / tensor_group strategies, and a
 * per-row scale as group == D.  `out` NULL: scales only.  `scale_out` (x's dtype; float32 under a global scale) / `zp_out` (zdt)
 * receive B * H * S * (D / group) entries, contiguous in logical (b, h, s, group) order whatever the strides of x; NULL: the
 * values stay in registers.  `global_scale`: device float32[1], NVFP4 only, or NULL. */
typedef struct ct_attn_dyn_tensor {
    const void* x;
    void* out;                     /* NULL: qparams only */
    void* scale_out;               /* NULL: not written */
    void* zp_out;                  /* NULL: not written */
    const float* global_scale;     /* NULL: none */
    int64_t B, H, S, D;
    int64_t x_stride[3];           /* b, h, s: elements */
    int64_t out_stride[3];
} ct_attn_dyn_tensor;              /* 15 64-bit words */

/* kind / bits / symmetric / zdt as ct_dynamic_qdq (kind 0 INT .. 4 MXFP8); xdt: a float dtype, of x and out alike.  n = 2: both
 * tensors (K and V) share dtypes, kind, bits and group — shapes, strides, outputs and global-scale pointers are their own, but both
 * take a global scale or neither does (CT_ERR_INVALID_ARG otherwise) — and are served by ONE launch.  The results are the bits
 * ct_dynamic_qdq gives on the contiguous copy.  The descriptors travel as kernel arguments; the entry allocates nothing, never
 * synchronises and keeps no device state.  CT_ERR_UNSUPPORTED (nothing launched) unless D % 8 == 0, D / 8 <= 256 (a row is one
 * pass of one 8-element unit per lane), group = 8 * 2^k <= 512, D % group == 0, and bases and strides keep the units aligned on
 * both sides (ct_attn_qdq's vector form).  B * H * S < 2^31 per tensor. */
int ct_attn_dyn_qdq(const ct_attn_dyn_tensor* tensors, int n, int group, int kind, int bits, int symmetric, int xdt, int zdt,
                    ct_stream_t stream);

/* generate_gparam of a whole weight (quantization/utils/helpers.py:308-337, the NVFP4 global scale): amax = max |x| (NaN if any
 * element is), clamped from below to finfo(x dtype).tiny; global_scale = rnd_X(rnd_X(1 / amax) * 2688) as float32 — `float / tensor`
 * is evaluated by torch as reciprocal times float, two roundings to x's dtype; a non-finite result becomes 1.  Two launches: the
 * row maxima (kind 5 above) into `row_amax` (scratch: rows elements of x's dtype), then one workgroup.  global_scale_out: device float32[1]. */
int ct_generate_gparam(const void* x, int xdt, int64_t rows, int64_t cols, void* row_amax, float* global_scale_out,
                       ct_stream_t stream);

/* ---------------------------------------------------------------------------- FP4 (E2M1) codecs
 * nvfp4-pack-quantized / mxfp4-pack-quantized weight paths (compressors/nvfp4/base.py:68-139,
 * mxfp4/base.py:27-65): quantize(x, scale, global_scale) -> cast_to_fp4 -> pack_fp4_to_uint8 fused, and the
 * inverse.  group: 16 (nvfp4) or 32 (mxfp4); cols % group == 0.  global_scale: device float32[1] or NULL.
 * packed: uint8 (rows, cols/2), element 2i in the low nibble of byte i.
 * compress: scale is the float scale tensor (rows, cols/group) the reference passes to quantize(); x: bf16 / fp16 weights (the lean kernels) or
 * float32 ones (round 6: a plain one-unit-per-lane kernel, IEEE float32 quotient).
 * decompress: scale_kind 0 = float tensor of dtype sdt, 1 = the stored fp8-e4m3fn bytes (nvfp4), 2 = the stored
 * E8M0 exponent bytes (mxfp4); odt in {CT_BF16, CT_F16} (the reference always produces bf16). */
int ct_fp4_quant_pack(const void* x, int xdt, const void* scale, int sdt, const float* global_scale,
                      int64_t rows, int64_t cols, int64_t group, uint8_t* packed, ct_stream_t stream);
int ct_fp4_unpack_dequant(const uint8_t* packed, int64_t rows, int64_t cols, const void* scale, int scale_kind,
                          int sdt, const float* global_scale, int64_t group, void* out, int odt,
                          ct_stream_t stream);
/* The same two launches with the scale tensors of the compressors' state dicts written by the kernel (round 6: the class calls composed them from 1-4
 * tensor ops per module — 5-20 us of launches beside a 10-30 us kernel):
 *   ct_fp4_quant_pack_stored: also writes the STORED scale — NVFP4: `scale.to(float8_e4m3fn)` bytes (rows, cols/16) (nvfp4/base.py:96-100; torch's
 *     conversion: RNE, a magnitude rounding beyond 448 or a NaN -> 0x7f | sign); MXFP4: `compress_mx_scale(scale, uint8)` codes (rows, cols/32)
 *     (mx_utils.py:18-31), read from `mx_code_table`, a device uint8[65536] the caller fills ONCE per scale dtype with that expression evaluated over
 *     every 16-bit pattern (so the codes are the reference's for every input, log2's rounding in the scale dtype included); NULL for NVFP4.
 *     CT_ERR_UNSUPPORTED (nothing launched) unless rows * cols % 32 == 0, the scale is 8-byte aligned and, for MXFP4, 16-bit with a table.
 *   ct_fp4_unpack_dequant_scale: also writes the decompressed scale as bfloat16 (rows, cols/group) — `scale.to(bfloat16)` of the float8 bytes
 *     (nvfp4/base.py:133-137) resp. `decompress_mx_scale` = 2 ** (code - 127) (mx_utils.py:34-44). */
int ct_fp4_quant_pack_stored(const void* x, int xdt, const void* scale, int sdt, const float* global_scale,
                             int64_t rows, int64_t cols, int64_t group, uint8_t* packed, uint8_t* scale_stored,
                             const uint8_t* mx_code_table, ct_stream_t stream);
int ct_fp4_unpack_dequant_scale(const uint8_t* packed, int64_t rows, int64_t cols, const void* scale, int scale_kind,
                                int sdt, const float* global_scale, int64_t group, void* out, int odt,
                                void* scale_bf16_out, ct_stream_t stream);
/* Tables of FP4 tensors: ONE launch per direction for the modules of an NVFP4 / MXFP4 checkpoint (the per-module loop of ModelCompressor.compress_model /
 * decompress_model, model_compressor.py:167-169,196-198, over NVFP4PackedCompressor / MXFP4PackedCompressor, nvfp4/base.py:68-139, mxfp4/base.py:27-65) —
 * ct_fp4_quant_pack_stored / ct_fp4_unpack_dequant_scale for every item.  The table is `struct ct_w4_item` read this way: src / dst = weights and packed
 * bytes in the direction's order, scale = the float scale (compress) resp. the stored float8 / E8M0 bytes (decompress), zp = the item's global scale (one
 * float32 on the device; group 16) or NULL (group 32), group = 16 or 32 (one value per table), zp_packed = the stored-scale output (compress: float8 bytes
 * resp. E8M0 codes, (rows, cols / group)) resp. the bfloat16 scale output (decompress).  ct_fp4_batch_plan fills the derived fields on the HOST copy and
 * returns the workgroup count, or -1 (error set) for an item outside the layout: rows * cols % 32 == 0, cols % group == 0, 16-byte aligned weights / packed
 * bytes (decompress: 4-byte aligned packed bytes), 8-byte aligned float scale.  xdt / sdt: the weights' and the float scales' dtype (one per table; MXFP4:
 * 16-bit scales and `mx_code_table` as in ct_fp4_quant_pack_stored).  odt: bfloat16 (what the reference returns) or float16. */
int64_t ct_fp4_batch_plan(ct_w4_item* items_host, int n, int direction);
int ct_fp4_quant_pack_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int xdt, int sdt, int group,
                            const uint8_t* mx_code_table, ct_stream_t stream);
int ct_fp4_unpack_dequant_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int group, int odt, ct_stream_t stream);
/* compress_mx_scale / decompress_mx_scale (compressors/mx_utils.py:18-44) on their own — the MXFP8 codec's scale conversions and upstream's helpers:
 * codes_out[i] = code_table[bits of scale[i]] (16-bit scales; the table as above) resp. scale_bf16_out[i] = 2 ** (codes[i] - 127) as bfloat16
 * (code 0: the bfloat16 subnormal 2^-127, code 255: inf). */
int ct_mx_scale_compress(const void* scale, int sdt, int64_t n, const uint8_t* code_table, uint8_t* codes_out, ct_stream_t stream);
/* ... for a table of scale tensors in one launch (the MXFP8 modules of a checkpoint: ModelCompressor's loop over MXFP8QuantizationCompressor.compress /
 * .decompress, compressors/mxfp8/base.py:47-101; the weights ride ct_q8_quant_batch / ct_q8_dequant_batch with groups of 32).  Items: src, dst and `rows` = the
 * element count (the other fields are ignored); direction 0: 16-bit scales (dtype `sdt`, one per table) -> uint8 codes through `code_table`; 1: codes ->
 * bfloat16.  Plan on the host copy first. */
int64_t ct_mx_scale_batch_plan(ct_w4_item* items_host, int n);
int ct_mx_scale_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int direction, int sdt, const uint8_t* code_table, ct_stream_t stream);
int ct_mx_scale_decompress(const uint8_t* codes, int64_t n, void* scale_bf16_out, ct_stream_t stream);

/* Round-to-nearest MXFP4 in one pass: per 32-element group the min-max observer, calculate_qparams' MX branch
 * (helpers.py:50-137, mxfp_utils.py:118-143), quantize -> cast_to_fp4 -> pack (nvfp4/base.py:88-95) and
 * compress_mx_scale (mx_utils.py:18-31).  packed: uint8 (rows, cols/2); scale_e8m0: uint8 (rows, cols/32), the
 * stored form of the scale; scale_out (nullable): the float scale (x's dtype) calculate_qparams would return.
 * Bit-identical to ct_minmax_qparams_float(kind 3) + ct_fp4_quant_pack + the E8M0 encoding. */
int ct_rtn_mxfp4_quant_pack(const void* x, int xdt, int64_t rows, int64_t cols, uint8_t* packed,
                            uint8_t* scale_e8m0, void* scale_out, ct_stream_t stream);
/* The same for a whole table of tensors in one launch (the per-module loop over MXFP4PackedCompressor, compressors/mxfp4/base.py, without a
 * launch per module).  The table is `struct ct_w4_item` read this way: src = the weights, dst = the packed bytes (rows, cols / 2), zp_packed =
 * the E8M0 code OUTPUT uint8 (rows, cols / 32) (the role the field plays in ct_fp4_quant_pack_batch), scale = the optional float-scale output
 * (the weights' dtype) or NULL, group = 32.  ct_rtn_mxfp4_batch_plan (host only) admits what ct_rtn_mxfp4_quant_pack admits, per item, fills the
 * derived fields and returns the workgroup count, or -1 with the error text set.  Bit-identical to ct_rtn_mxfp4_quant_pack per item. */
int64_t ct_rtn_mxfp4_batch_plan(ct_w4_item* items_host, int n);
int ct_rtn_mxfp4_quant_pack_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int xdt, ct_stream_t stream);
/* The NVFP4 counterpart (groups of 16 under `global_scale`, device float32[1], e.g. generate_gparam of the weight):
 * scale_f8: float8_e4m3fn bytes (rows, cols/16), the stored form; scale_out (nullable): the float32 scales. cols % 32 == 0. */
int ct_rtn_nvfp4_quant_pack(const void* x, int xdt, int64_t rows, int64_t cols, const float* global_scale,
                            uint8_t* packed, uint8_t* scale_f8, float* scale_out, ct_stream_t stream);
/* ... with generate_gparam of each weight, for a whole table of tensors in TWO launches (the per-module loop over NVFP4PackedCompressor: the two
 * launches of ct_generate_gparam and ct_rtn_nvfp4_quant_pack per module).  The table is `struct ct_w4_item` read this way: src = the weights, dst =
 * the packed bytes (rows, cols / 2), zp_packed = the float8 scale OUTPUT (rows, cols / 16), zp = the item's amax KEY — one 32-bit word of device
 * memory, its own per item, ZERO before the fold (one fill of a per-table buffer) —, scale = the item's weight_global_scale OUTPUT (float32[1]),
 * group = 16.  ct_rtn_nvfp4_batch_plan (host only) admits what ct_rtn_nvfp4_quant_pack admits, per item (n <= 0: an error), fills the derived
 * fields and returns the workgroup count, or -1 with the error text set.
 *   ct_rtn_nvfp4_amax_batch: folds max |x| of every item into its key as the 16-bit magnitude pattern (unsigned integer order == float order, a
 *     NaN above inf, 0 the identity) with vector atomic maxima: exact, independent of scheduling.
 *   ct_rtn_nvfp4_quant_pack_batch, behind it on the same stream: every lane derives the item's global scale from the key (the arithmetic of
 *     ct_generate_gparam), one lane per item stores it, and the weights are quantized under it.  Bit-identical to ct_generate_gparam +
 *     ct_rtn_nvfp4_quant_pack per item.  The library allocates nothing and never synchronises. */
int64_t ct_rtn_nvfp4_batch_plan(ct_w4_item* items_host, int n);
int ct_rtn_nvfp4_amax_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int xdt, ct_stream_t stream);
int ct_rtn_nvfp4_quant_pack_batch(const ct_w4_item* items_dev, int n, int64_t total_blocks, int xdt, ct_stream_t stream);

/* The stand-alone primitives the reference exposes as ImplBackend entry points (utils/impl_backend.py:50-79):
 * cast_to_fp4 (quantization/utils/fp4_utils.py:77-98): n float elements -> the nearest E2M1 value in the same
 *   dtype; ties as upstream's thresholds, -0.0 -> +0.0, negative-rounds-to-zero -> -0.0, NaN -> NaN.
 * pack_fp4_to_uint8 (compressors/nvfp4/helpers.py:108-150): n (even) E2M1-valued elements -> n / 2 bytes,
 *   bit 3 of a nibble = the IEEE sign bit.  Values off the E2M1 grid are rounded to it (upstream leaves them
 *   undefined).
 * unpack_fp4_from_uint8 (helpers.py:153-193): n / 2 bytes -> n elements of dtype odt; code 8 -> -0.0. */
int ct_fp4_cast(const void* x, int xdt, void* out, int64_t n, ct_stream_t stream);
int ct_fp4_pack(const void* x, int xdt, uint8_t* packed, int64_t n, ct_stream_t stream);
int ct_fp4_unpack(const uint8_t* packed, int64_t n, void* out, int odt, ct_stream_t stream);

/* Proof obligation of ct_fp4_quant_pack's reciprocal quotient (ct_fp4.hip): counts the (x, s) pairs, s = 1.m for
 * every 23-bit mantissa m in [m_lo, m_hi) and x = every mantissa of dtype xdt (CT_BF16 / CT_F16) in [1, 2), for which
 * it differs from the IEEE fp32 quotient.  *mismatches (device uint64) must come back 0. */
int ct_selftest_fp4_div(int xdt, uint32_t m_lo, uint32_t m_hi, unsigned long long* mismatches, ct_stream_t stream);

/* ---------------------------------------------------------------------------- sparse codecs
 * The compressor classes for these formats were removed from the reference snapshot
 * (compressors/base.py:43-44); the formats and primitives remain: config/base.py:17-18,23,
 * utils/helpers.py:306-343 (pack_bitmasks / unpack_bitmasks, numpy little-endian packbits),
 * utils/semi_structured_conversions.py:33-298, utils/permutations_24.py:20-53.
 * `dt` describes the element for the `!= 0` test and its size; values are copied bit-for-bit.
 */

/* pack_bitmasks(mask)   utils/helpers.py:306-318.  mask: uint8/bool (rows, cols) */
int ct_pack_bitmasks(const uint8_t* mask, int64_t rows, int64_t cols, uint8_t* out, ct_stream_t stream);
/* unpack_bitmasks(packed, shape)   utils/helpers.py:321-343 */
int ct_unpack_bitmasks(const uint8_t* packed, int64_t rows, int64_t cols, uint8_t* mask, ct_stream_t stream);

/* sparse-bitmask compress, pass 1: bitmask = pack_bitmasks(x != 0), row_counts[r] = nnz of row r */
int ct_bitmask_count(const void* x, int dt, int64_t rows, int64_t cols, uint8_t* bitmask,
                     int64_t* row_counts, ct_stream_t stream);
/* exclusive scan of int64 counts -> row_offsets (n) and the grand total (total[0]) */
int ct_exclusive_scan_i64(const int64_t* counts, int64_t n, int64_t* offsets, int64_t* total,
                          ct_stream_t stream);
/* sparse-bitmask compress, pass 2: values[row_offsets[r] + rank] = x[r, c] for non-zero x */
int ct_bitmask_scatter(const void* x, int dt, int64_t rows, int64_t cols, const int64_t* row_offsets,
                       void* values, ct_stream_t stream);
/* sparse-bitmask compress, fused form: bitmask, row_offsets, values and total[0] = nnz with no host
 * round trip.  16- and 32-bit payloads with cols % 8 == 0 (a 32-bit element travels as its two
 * 16-bit halves; the bitmask, the row offsets and the total are per ELEMENT): ONE pass over x — every workgroup keeps its share
 * of the tensor in registers, compacts it while the loads land, publishes its count as one 64-bit
 * word and stores once it has the counts of the workgroups before it; a count that does not arrive
 * within 2 ms is recomputed by the waiting workgroup, so the call cannot fail or deadlock.
 * CT_BITMASK_RESIDENT=0 selects count + scatter (x read twice, no inter-workgroup waiting).
 * 8-bit payloads / other column counts: count, scan, scatter.  `values` must hold `values_capacity` elements
 * (numel is always enough; the one-pass paths never write beyond the capacity and still report the
 * needed size in total).  `workspace` = ct_bitmask_compress_workspace_bytes(rows, cols) bytes, 8-byte
 * aligned, need not be initialised.  (HIP graphs: every compute entry of this header can be captured; this one and its batch form bake a
 * per-launch generation tag into the launch, so a graph that contains them clears `workspace` inside the graph before the launch.) */
int64_t ct_bitmask_compress_workspace_bytes(int64_t rows, int64_t cols);
int ct_bitmask_compress(const void* x, int dt, int64_t rows, int64_t cols, void* values,
                        int64_t values_capacity, uint8_t* bitmask, int64_t* row_offsets, int64_t* total,
                        void* workspace, int64_t workspace_bytes, ct_stream_t stream);
/* The same compress for a TABLE of tensors in ONE launch (round 6): a checkpoint's sparse weights, e.g. what the restated
 * BitmaskCompressor.compress_state_dict loops over.  One ct_bitmask_compress launch of a checkpoint-sized tensor is a latency chain
 * (9 us for 1 MB, 10 us for 8 MB, 17 us for 23 MB of bf16: 2-27 % of the HBM rate); in one grid the tensors' chains run side by
 * side.  16- or 32-bit payloads (ONE element size per table), cols % 8 == 0, x and values 16-byte aligned, at most 1 GiB of payload
 * per tensor.  Protocol as the W4 batch: fill x / dt / rows / cols / values / values_capacity / bitmask / row_offsets / total of every
 * item, call ct_bitmask_batch_plan on the HOST copy (derived fields; returns the workgroup count or -1 and, in *workspace_bytes, the
 * size of the one workspace the launch needs: 8-byte aligned device memory, need not be initialised), copy the table to the device,
 * launch.  total[0] of every item receives its nnz (a word of a ct_mailbox_alloc block, for a host that waits; or device memory).
 * Outputs are bit-identical to ct_bitmask_compress item by item. */
typedef struct ct_bitmask_item {
    const void* x;
    void* values;
    uint8_t* bitmask;
    int64_t* row_offsets;
    int64_t* total;
    int64_t rows, cols, values_capacity; /* capacity in elements; numel is always enough */
    int32_t dt;                          /* element type code */
    int32_t is_float;                    /* derived */
    int64_t first_block, units, upr, slots_offset; /* derived */
    int32_t nwg, tpw, mask_dwords;                 /* derived */
    uint32_t gen;                                  /* derived */
} ct_bitmask_item;                       /* 15 64-bit words */
int64_t ct_bitmask_batch_plan(ct_bitmask_item* items_host, int n, int64_t* workspace_bytes);
int ct_bitmask_compress_batch(const ct_bitmask_item* items_dev, int n, int64_t total_blocks, int element_size, void* workspace,
                              int64_t workspace_bytes, ct_stream_t stream);

/* The decompress side of the same loop — loading a sparse checkpoint (the restated BitmaskCompressor.decompress_state_dict) — for a TABLE of
 * tensors in one launch: out = zeros; out[mask] = values per item, bit-identical to ct_bitmask_decompress item by item.  16- or 32-bit payloads
 * (ONE element size per table), cols x element size % 64 == 0, row_offsets given, values / out 16-byte and bitmask 4-byte aligned.
 * ct_bitmask_decompress_batch_plan fills the derived fields on the host copy and returns the workgroup count or -1. */
typedef struct ct_bitmask_ditem {
    const void* values;
    const uint8_t* bitmask;
    const int64_t* row_offsets;
    void* out;
    int64_t rows, cols, values_len; /* values_len in elements */
    int32_t dt;                     /* element type code */
    int32_t single;                 /* derived */
    int64_t first_block;            /* derived */
} ct_bitmask_ditem;                 /* 9 64-bit words */
int64_t ct_bitmask_decompress_batch_plan(ct_bitmask_ditem* items_host, int n);
int ct_bitmask_decompress_batch(const ct_bitmask_ditem* items_dev, int n, int64_t total_blocks, int element_size, ct_stream_t stream);

/* n byte ranges copied by one launch (the exact-size `values` of a batch leave the worst-case arena the kernels wrote into:
 * tensor[mask] owns nnz elements, restated S1 over utils/helpers.py:306-343).  ct_copy_batch_plan fills first_block on the host
 * copy and returns the workgroup count (16 KiB per workgroup) or -1. */
typedef struct ct_copy_item {
    const void* src;
    void* dst;
    int64_t bytes;
    int64_t first_block; /* derived */
} ct_copy_item;
int64_t ct_copy_batch_plan(ct_copy_item* items_host, int n);
int ct_copy_batch(const ct_copy_item* items_dev, int n, int64_t total_blocks, ct_stream_t stream);

/* AutoAWQ GEMM -> pack-quantized (entrypoints/convert/converters/autoawq.py, AutoAWQConverter.process) for a TABLE of modules in ONE
 * launch.  Per item, with K = in_features, N = out_features, G = number of groups:
 *   qweight int32 (K, N / 8)          -> weight_packed int32 (N, ceil(K / 8)): nibble i of word (n, w) is the AWQ nibble of element
 *                                        (k = 8w + i, n); the AWQ nibble of column c of a word sits at position [0,4,1,5,2,6,3,7][c];
 *                                        nibbles past K are zero
 *   qzeros  int32 (G, N / 8) or NULL  -> zp_packed int32 (N / 8, G): word (j, g) is qzeros[g, j] with its nibbles in natural order
 *   scales  16-bit (G, N)             -> scale_t (N, G), the same bits (scale_dt: CT_F16 or CT_BF16)
 * scale_shape / zp_shape are the shapes the caller found (checked against N and G).  Protocol as the other batches: fill the
 * non-derived fields, call ct_awq_repack_plan on the HOST copy (derived fields; returns the workgroup count, or -1 with ct_last_error
 * set for a malformed item or a batch too large for one launch — split it), copy the table to the device, launch. */
typedef struct ct_awq_item {
    const int32_t* qweight;
    const int32_t* qzeros;
    const void* scales;
    int32_t* weight_packed;
    int32_t* zp_packed;        /* NULL exactly when qzeros is */
    void* scale_t;
    int64_t K, N, G;
    int64_t scale_shape[2];
    int64_t zp_shape[2];       /* ignored without qzeros */
    int32_t scale_dt;
    int32_t wide;              /* derived: bit 0 = 16-byte qweight loads, bit 1 = 16-byte weight_packed stores */
    int64_t first_block;       /* derived */
    int64_t weight_blocks;     /* derived: the 4-bit transpose; the zero-point and scale tails follow */
    int64_t zp_blocks;         /* derived */
} ct_awq_item;                 /* 17 64-bit words */
int64_t ct_awq_repack_plan(ct_awq_item* items_host, int n);
int ct_awq_repack_batch(const ct_awq_item* items_dev, int n, int64_t total_blocks, ct_stream_t stream);

/* FP8 block dequantize (entrypoints/convert/converters/fp8block_dequantizer.py, FP8BlockDequantizer._create_dequantized_weight) for a
 * TABLE of modules in ONE launch.  Per item and element:
 *   out[r, c] = rnd_odt( f32(w[r, c]) * f32(scale[r / block_h, c / block_w]) )
 * w is float8_e4m3fn (rows, cols) row-major, out (rows, cols) of odt (CT_BF16, CT_F16 or CT_F32: one per launch), the scale
 * (weight_scale_inv) of sdt CT_F32 / CT_BF16 / CT_F16 with scale_shape (ceil(rows / block_h), ceil(cols / block_w)) or a shape torch
 * broadcasts the same way (a dimension of 1).  Block sizes are any positive sizes; a ragged last block row or column is handled
 * without padding.  Protocol as the other batches: fill the non-derived fields, call ct_fp8block_dequant_plan on the HOST copy
 * (derived fields; returns the workgroup count, or -1 with ct_last_error set for a malformed item or a batch too large for one
 * launch — split it), copy the table to the device, launch. */
typedef struct ct_fp8block_item {
    const uint8_t* w;
    const void* scale;
    void* out;
    int64_t rows, cols, block_h, block_w;
    int64_t scale_shape[2];    /* as found; the plan checks it */
    int32_t sdt;
    int32_t fast;              /* derived: 1 = 16 codes per lane with 16-byte loads, one scale and 16-byte stores; 0 = general path */
    int64_t scale_stride[2];   /* derived: in elements, 0 along a broadcast dimension */
    int64_t units_per_row;     /* derived: ceil(cols / 16) */
    int64_t first_block;       /* derived */
} ct_fp8block_item;            /* 14 64-bit words */
int64_t ct_fp8block_dequant_plan(ct_fp8block_item* items_host, int n);
int ct_fp8block_dequant_batch(const ct_fp8block_item* items_dev, int n, int64_t total_blocks, int odt, ct_stream_t stream);

/* FP8 block-quantized weights straight to mxfp4-pack-quantized for a TABLE of modules in ONE launch: the bytes of ct_fp8block_dequant_batch
 * (odt = xdt) followed by ct_rtn_mxfp4_quant_pack_batch, without the dense weight in between.  Per MX group (32 consecutive elements of a row):
 *   d[i] = rnd_xdt( f32(w[r, c + i]) * f32(scale[r / block_h, (c + i) / block_w]) ),  s = the MX scale of max |d| (calculate_qparams' MX branch),
 *   e8m0 = the stored exponent byte of s,  packed = the E2M1 nibbles of d / s (low nibble first).
 * w is float8_e4m3fn (rows, cols) row-major, packed uint8 (rows, cols / 2), e8m0 uint8 (rows, cols / 32); xdt (CT_BF16 or CT_F16: one per launch) is
 * the dense dtype that is never materialised.  The plan admits an item with cols % 32 == 0, block_w % 32 == 0 (no group straddles a scale block),
 * 16-byte aligned w and packed, and the scale shapes and dtypes of ct_fp8block_dequant_plan; anything else returns -1 with ct_last_error naming the
 * item.  A workgroup owns CT_FP8BLOCK_MX_GROUPS_PER_BLOCK consecutive groups of one item.  Protocol as the other batches. */
#define CT_FP8BLOCK_MX_GROUPS_PER_BLOCK 512
typedef struct ct_fp8block_mx_item {
    const uint8_t* w;
    const void* scale;
    uint8_t* packed;
    uint8_t* e8m0;
    int64_t rows, cols, block_h, block_w;
    int64_t scale_shape[2];    /* as found; the plan checks it */
    int32_t sdt;
    int32_t reserved;          /* derived: 0 */
    int64_t scale_stride[2];   /* derived: in elements, 0 along a broadcast dimension */
    int64_t units_per_row;     /* derived: cols / 32, the MX groups of a row */
    int64_t units;             /* derived: rows * units_per_row */
    int64_t first_block;       /* derived */
} ct_fp8block_mx_item;         /* 16 64-bit words */
int64_t ct_fp8block_mxfp4_plan(ct_fp8block_mx_item* items_host, int n);
int ct_fp8block_mxfp4_batch(const ct_fp8block_mx_item* items_dev, int n, int64_t total_blocks, int xdt, ct_stream_t stream);

/* FP8 block-quantized weights straight to mxfp8-quantized for a TABLE of modules in ONE launch: the bytes of ct_fp8block_dequant_batch (odt = xdt)
 * followed by the one-pass MXFP8 table (ct_rtn_quant_group8_batch, kind 4), without the dense weight in between.  Per MX group (32 consecutive
 * elements of a row): d[i] as above, s = the MXFP8 scale of max |d|, e8m0 = its stored exponent byte (code_table: the 65536-entry table
 * ct_mx_scale_compress reads, of the dense dtype, consulted for a non-finite scale), codes = float8_e4m3fn of d / s.
 * The row is ct_fp8block_mx_item with `packed` = the float8 codes (rows, cols); the plan admits what ct_fp8block_mxfp4_plan admits (cols % 32 == 0,
 * block_w % 32 == 0, 16-byte aligned w and codes, the scale shapes and dtypes of ct_fp8block_dequant_plan).  A workgroup owns
 * CT_FP8BLOCK_MXFP8_GROUPS_PER_BLOCK consecutive groups of one item. */
#define CT_FP8BLOCK_MXFP8_GROUPS_PER_BLOCK 512
int64_t ct_fp8block_mxfp8_plan(ct_fp8block_mx_item* items_host, int n);
int ct_fp8block_mxfp8_batch(const ct_fp8block_mx_item* items_dev, int n, int64_t total_blocks, int xdt, const uint8_t* code_table, ct_stream_t stream);

/* FP8 block-quantized weights straight to nvfp4-pack-quantized for a TABLE of modules in TWO launches over the same planned rows: the bytes of
 * ct_fp8block_dequant_batch (odt = xdt) followed by ct_rtn_nvfp4_amax_batch and ct_rtn_nvfp4_quant_pack_batch, without the dense weight in between.
 * ct_fp8block_nvfp4_amax_batch folds max |d| of every item into its `key` (one 32-bit word the caller has ZEROED on the stream);
 * ct_fp8block_nvfp4_batch derives the item's global scale from the key (generate_gparam), stores it in `global_scale` and writes, per group of 16
 * consecutive elements of a row, the float8_e4m3fn scale byte and the E2M1 nibbles (low nibble first).
 * packed is uint8 (rows, cols / 2), scale_f8 float8_e4m3fn (rows, cols / 16), global_scale float32 (1,).  The plan admits an item with cols % 16 == 0,
 * block_w % 16 == 0, 16-byte aligned w and packed, 4-byte aligned key and global_scale, and the scale shapes and dtypes of
 * ct_fp8block_dequant_plan.  A workgroup owns CT_FP8BLOCK_NV_GROUPS_PER_BLOCK consecutive groups of one item. */
#define CT_FP8BLOCK_NV_GROUPS_PER_BLOCK 1024
typedef struct ct_fp8block_nv_item {
    const uint8_t* w;
    const void* scale;
    uint8_t* packed;
    uint8_t* scale_f8;
    uint32_t* key;
    float* global_scale;
    int64_t rows, cols, block_h, block_w;
    int64_t scale_shape[2];    /* as found; the plan checks it */
    int32_t sdt;
    int32_t reserved;          /* derived: 0 */
    int64_t scale_stride[2];   /* derived: in elements, 0 along a broadcast dimension */
    int64_t units_per_row;     /* derived: cols / 16, the groups of a row */
    int64_t units;             /* derived: rows * units_per_row */
    int64_t first_block;       /* derived */
} ct_fp8block_nv_item;         /* 18 64-bit words */
int64_t ct_fp8block_nvfp4_plan(ct_fp8block_nv_item* items_host, int n);
int ct_fp8block_nvfp4_amax_batch(const ct_fp8block_nv_item* items_dev, int n, int64_t total_blocks, int xdt, ct_stream_t stream);
int ct_fp8block_nvfp4_batch(const ct_fp8block_nv_item* items_dev, int n, int64_t total_blocks, int xdt, ct_stream_t stream);

/* nvfp4-pack-quantized weights straight to mxfp4-pack-quantized for a TABLE of modules in ONE launch: the bytes of ct_fp4_unpack_dequant_batch
 * (group 16, odt = CT_BF16: the dtype the NVFP4 decompress always yields) followed by ct_rtn_mxfp4_quant_pack_batch, without the dense weight in
 * between.  Per MX group (32 consecutive elements of a row, two NVFP4 groups):
 *   d[i] = rnd_bf16( E2M1(packed_in nibble i) * fl32(f32(scale_f8 of i's group of 16) / global_scale[0]) ),  s = the MX scale of max |d|,
 *   e8m0 = the stored exponent byte of s,  packed_out = the E2M1 nibbles of d / s (low nibble first).
 * packed_in is uint8 (rows, cols / 2), scale_f8 float8_e4m3fn (rows, cols / 16), global_scale float32 (one element), packed_out uint8
 * (rows, cols / 2), e8m0 uint8 (rows, cols / 32), all contiguous.  The plan admits an item with positive sizes below 2^31, cols % 32 == 0, 16-byte
 * aligned packed_in and packed_out, a 2-byte aligned scale_f8 and a 4-byte aligned global_scale; anything else returns -1 with ct_last_error naming
 * the item.  A workgroup owns CT_NVFP4_MX_GROUPS_PER_BLOCK consecutive groups of one item and reads that item's global scale alone.  Protocol as the
 * other batches. */
#define CT_NVFP4_MX_GROUPS_PER_BLOCK 1024
typedef struct ct_nvfp4_mx_item {
    const uint8_t* packed_in;
    const uint8_t* scale_f8;
    const float* global_scale;
    uint8_t* packed_out;
    uint8_t* e8m0;
    int64_t rows, cols;
    int64_t units;             /* derived: rows * cols / 32, the MX groups */
    int64_t first_block;       /* derived */
} ct_nvfp4_mx_item;            /* 9 64-bit words */
int64_t ct_nvfp4_mxfp4_plan(ct_nvfp4_mx_item* items_host, int n);
int ct_nvfp4_mxfp4_batch(const ct_nvfp4_mx_item* items_dev, int n, int64_t total_blocks, ct_stream_t stream);

/* sparse-bitmask decompress: out = zeros; out[mask] = values.  row_offsets may be NULL only if
 * fixed_row_nnz >= 0 (every row holds exactly that many values: the 2:4 codec).  16-bit payloads with
 * cols % 32 == 0 and 32-bit payloads with cols % 16 == 0 (as pairs of halves) take the LDS-window
 * kernel; everything else the general one. */
int ct_bitmask_decompress(const void* values, int64_t values_len, const uint8_t* bitmask,
                          const int64_t* row_offsets, int64_t fixed_row_nnz, int dt, int64_t rows,
                          int64_t cols, void* out, ct_stream_t stream);
/* popcount of each bitmask row -> row_counts (to rebuild row_offsets when a checkpoint lacks them) */
int ct_bitmask_row_popcount(const uint8_t* bitmask, int64_t rows, int64_t cols, int64_t* row_counts,
                            ct_stream_t stream);

/* sparse-24-bitmask compress: keep the 2 largest-|x| of every 4 consecutive elements (ties:
 * lower index first; NaN largest); values (rows, cols/2); bitmask (rows, ceil(cols/8)) */
int ct_sparse24_compress(const void* x, int dt, int64_t rows, int64_t cols, void* values,
                         uint8_t* bitmask, ct_stream_t stream);
/* the 2:4 magnitude mask alone (mask_creator, utils/semi_structured_conversions.py:301-330) */
int ct_sparse24_mask(const void* x, int dt, int64_t numel, uint8_t* mask, ct_stream_t stream);

/* sparse_semi_structured_from_dense_cutlass   utils/semi_structured_conversions.py:66-197
 * dense (m, k) of CT_F16/CT_BF16 (meta int16) or CT_I8 (meta int32); sparse (m, k/2);
 * meta (m, k/(4*Q)) reordered, Q = 4 (int16) or 8 (int32) */
int ct_cutlass24_from_dense(const void* dense, int dt, int64_t m, int64_t k, void* sparse, void* meta,
                            ct_stream_t stream);
/* sparse_semi_structured_to_dense_cutlass   :204-298.  sparse (m, k) -> dense (m, 2k) */
int ct_cutlass24_to_dense(const void* sparse, int dt, const void* meta, int meta_itemsize, int64_t m,
                          int64_t k, void* dense, ct_stream_t stream);

/* marlin-24 front end, fused (restated Marlin24Compressor.compress): fp16 quantize
 * of a 2:4-sparse 16-bit weight (every op rounded to fp16, like quantize() on weight.to(fp16)),
 * 2:4 compression of the codes (utils/semi_structured_conversions.py:66-197 on the 16-bit flavour:
 * int16 metadata, reordered) without any full-size intermediate.  comp: int8 (m, k/2) kept codes
 * (no offset); meta: int16 (m, k/16) reordered; bad[0] != 0 afterwards if some quad had more than
 * two non-zero codes (the weight is not 2:4).  scale: (m, k/cdiv), zp nullable. */
/* the same front end with the marlin-24 tile permutation + int4 packing fused in (rows % 64 == 0,
 * cols % 256 == 0): weight -> packed int32 (cols/32, rows*2) + reordered int16 metadata in ONE pass. */
int ct_marlin24_compress_w4(const void* w, int wdt, const void* scale, int sdt, const void* zp, int zdt,
                            int64_t m, int64_t k, int64_t cdiv, int32_t* packed, int16_t* meta, int* bad,
                            ct_stream_t stream);
int ct_marlin24_quant_compress(const void* w, int wdt, const void* scale, int sdt, const void* zp, int zdt,
                               int64_t m, int64_t k, int64_t cdiv, int bits, int8_t* comp, int16_t* meta,
                               int* bad, ct_stream_t stream);
/* the whole restated Marlin24Compressor.compress for int4 in one host call: ct_marlin24_compress_w4 followed by
 * ct_marlin24_pack_scales_f16 (scale (m, k/cdiv) bf16 / fp16 -> scale_packed fp16 (k/cdiv, m); group_perm != 0 selects
 * scale_perm, 0 scale_perm_single).  clear_bad == 0 leaves *bad alone (the violation is OR-ed in): the caller owns a
 * pre-zeroed flag, e.g. one slot of a ring that is read back once per batch instead of once per tensor. */
int ct_marlin24_compress_w4_full(const void* w, int wdt, const void* scale, int sdt, const void* zp, int zdt,
                                 int64_t m, int64_t k, int64_t cdiv, int group_perm, int32_t* packed, int16_t* meta,
                                 void* scale_packed, int* bad, int clear_bad, ct_stream_t stream);

/* the same one-launch compress for a caller that must RAISE from the call when the weight is not 2:4 (upstream's
 * Marlin24Compressor.compress -> validate_sparsity_structure, historical sparse_quantized_compressors/marlin_24.py; the mask test is
 * utils/semi_structured_conversions.py / tensor_follows_mask_structure, utils/helpers.py:87-109): instead of a flag that is final only
 * when the stream has drained, the launch's last-reporting workgroup stores 1 (every quad of every row keeps at most two non-zero
 * codes) or 3 (violated) into *verdict_word at system scope as soon as every workgroup has evaluated its tiles — the caller zeroes
 * the word (pinned, device-mapped host memory: ct_mailbox_alloc) before the call and spins on it; outputs follow on `stream` as usual.
 *   workspace        CT_M24_VERDICT_WORKSPACE_BYTES of device memory on the stream's device, 128-byte aligned, owned by the CALLER
 *                    (as ct_bitmask_compress's): the workgroups count themselves in through it.  It must be all-zero when the launch
 *                    starts and is all-zero again once the verdict has been stored (the kernel orders its resets before that store),
 *                    so one zeroed allocation serves any number of consecutive calls.  One launch per workspace at a time: launches on
 *                    ONE stream may share a workspace without waiting (stream order separates them); launches that can overlap — other
 *                    streams, other host threads, other devices — need a workspace each, or must wait for the verdict in between.
 *                    The library keeps no device state: the entry is re-entrant like every other one (convert_checkpoint's worker
 *                    threads, entrypoints/convert/convert_checkpoint.py:129-132).
 *   clear_workspace  != 0: the call zeroes the workspace first (one hipMemsetAsync on `stream`) — the first use of an allocation
 *                    that is not known to be zero, or the use after a launch that did not finish.
 * CT_ERR_UNSUPPORTED for a layout the one-launch kernel does not take (use ct_marlin24_compress_w4_full + a stream wait). */
#define CT_M24_VERDICT_WORKSPACE_BYTES 8320
int ct_marlin24_compress_w4_verdict(const void* w, int wdt, const void* scale, int sdt, const void* zp, int zdt,
                                    int64_t m, int64_t k, int64_t cdiv, int group_perm, int32_t* packed, int16_t* meta,
                                    void* scale_packed, int64_t* verdict_word, void* workspace, int clear_workspace,
                                    ct_stream_t stream);

/* marlin-24 weight packing (historical Marlin24Compressor.pack_weight_24 with the table of
 * utils/permutations_24.py:20-45).  q: codes of dtype dt (CT_I32 / CT_I8 / float holding
 * integers), laid out (size_k, size_n) [transposed == 0] or as the un-transposed 2:4-compressed
 * matrix (size_n, size_k) [transposed == 1]; add_offset != 0 adds 2^(bits-1) to make the codes
 * unsigned.  packed: int32 (size_k/16, size_n*16*bits/32) */
int ct_marlin24_pack_weights(const void* q, int dt, int transposed, int add_offset, int64_t size_k,
                             int64_t size_n, int bits, int32_t* packed, ct_stream_t stream);
/* marlin-24 scale packing: scale (size_n, groups) 16-bit float -> transposed, permuted with
 * scale_perm (single == 0) or scale_perm_single (single != 0) of utils/permutations_24.py:46-53
 * -> (groups, size_n) */
int ct_marlin24_pack_scales(const void* scale, int dt, int64_t size_n, int64_t groups, int single,
                            void* out, ct_stream_t stream);
/* the same with the reference's `scale.to(torch.float16)` folded in: scale may be bfloat16, out is float16 */
int ct_marlin24_pack_scales_f16(const void* scale, int dt, int64_t size_n, int64_t groups, int single,
                                void* out, ct_stream_t stream);

/* ---------------------------------------------------------------------------- diagnostics
 * Exhaustive device-side check of the reciprocal fast path used by the bf16 fused kernels:
 * for every bf16 (x, s) pair in [s_lo_bits, s_hi_bits) x all 65536 x, compares
 * rnd_bf16(x * rcp(s)) with rnd_bf16(x / s).  mismatches[0] receives the count. */
/* the same for the fp16 quotient shortcut of ct_marlin24_quant_compress (reciprocal + one Newton step) */
int ct_selftest_f16_div(uint32_t s_lo_bits, uint32_t s_hi_bits, unsigned long long* mismatches,
                        ct_stream_t stream);
int ct_selftest_bf16_div(uint32_t s_lo_bits, uint32_t s_hi_bits, unsigned long long* mismatches,
                         ct_stream_t stream);
/* the quotients of the lean marlin-24 front end (ct_marlin24_compress_w4): mode 0 = fp16 x / fp16 scale by reciprocal +
 * Newton step, mode 1 = bf16 x / bf16 scale by ONE multiply with the reciprocal, mode 2 = the kernel's reciprocal (v_rcp_f32 + two
 * Newton steps) against the IEEE 1.0f / s, bit for bit; s bits in [s_lo_bits, s_hi_bits) */
int ct_selftest_m24_div(int mode, uint32_t s_lo_bits, uint32_t s_hi_bits, unsigned long long* mismatches,
                        ct_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CT_HIP_H */
