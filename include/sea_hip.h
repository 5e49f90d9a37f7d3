/*
 * sea_hip.h -- C ABI of libsea_hip.so: SEA sparse-attention hot path on MI355X (gfx950).
 *
 * Drop-in boundary for the reference's operator package
 *   src/models/perlin_attention/ops/__init__.py:1-7   (7 exported operators)
 * and for the sparse branch of PerlinAttention.forward
 *   src/models/perlin_attention/attention.py:774-947  (grouped top-k)
 *   src/models/perlin_attention/attention.py:1034-1042 (mask -> flat CSR)
 *   src/models/perlin_attention/attention.py:1158-1173 (SDDMM/softmax/elmul/SpMM)
 *   src/models/perlin_attention/attention.py:1236-1244 (average-pool mix)
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller;
 *   - the library allocates nothing persistent, frees nothing, keeps no global state except a
 *     thread-local last-error string; every call is asynchronous on `stream` (a hipStream_t);
 *   - return 0 on success, negative SEA_E* otherwise (no exception crosses the ABI);
 *   - tensors are addressed by ELEMENT strides; the innermost (feature / pixel) stride must be 1;
 *   - "flat CSR" is the reference's wire format (causal_resize_m_to_t.py:757-762): one CSR row per
 *     (batch, query) with column id = head*T_src + key, entries of a row grouped by ascending head,
 *     pixels ascending inside a head, keys DESCENDING inside a pixel (causal_resize_m_to_t.py:569).
 *     Internally indices are int32; `idx_bytes` = 8 selects int64 at the API edge (torch CSR).
 */
#ifndef SEA_HIP_H
#define SEA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version, returned by sea_version(); the Python binding refuses a library of another version (a stale .so next to newer
 * Python, or the other way round, through SEA_HIP_LIB).  History of INCOMPATIBLE changes of existing entry points:
 *   1  rounds 1-2
 *   2  round 3: sea_performer_causal_step (both forms) reads k / v / pos FROM THE LAST CHUNK BOUNDARY (T + t_base % C rows)
 *      and takes the state image at that boundary;  round 4: sea_predictor_mlp's w2_packed / vectors pad every decoder half to whole
 *      16-row tiles (identical for Wd % 16 == 0), sea_predictor_tail_select accepts probs = NULL and any T_m % 4 == 0 <= 512
 *   3  round 5: new entry points the binding requires (the z, fp32 and decode forms of the convolution, tail, selection and
 *      attention, sea_decode_cnn_tail_select, sea_predictor_tail_consts); the tail + selection takes a trailing
 *      `consts_tab` argument (NULL = the round-4 behaviour)
 *   4  one entry point per operator: the variants that were separate, suffixed entry points of sea_sparse_attention,
 *      sea_predictor_tail, sea_predictor_tail_select, sea_csr_emit, sea_causal_conv_c8, sea_performer_causal and
 *      sea_performer_causal_step are gone; each of these takes the variants' arguments instead (NULL / 0 / 1 = not wanted)
 *   5  one entry point per operator again: the decode step's per-sequence (*_ragged) and paged (*_paged) entries of
 *      sea_decode_stage, sea_performer_causal_step, sea_decode_cnn_tail_select, sea_sparse_attention and sea_csr_emit are
 *      gone; each of these takes their trailing arguments instead (stride 0 / NULL block table = the shared form); ABI 4 had
 *      also gained sea_decode_fork
 *   6  one entry point per operator once more: the multi-row (*_rows) entries of sea_decode_stage and
 *      sea_decode_cnn_tail_select and the sliced entry sea_cumavg_sliced, added beside ABI 5, are gone; sea_decode_stage takes
 *      `rows` (and [n, h, t] strides), sea_decode_cnn_tail_select takes `y1_scratch` and `rows` (NULL, 1 = the one-row form),
 *      sea_cumavg takes `n_slices, workspace, workspace_bytes` (1, NULL, 0 = one pass)
 *   7  one entry point per operator, the last one: sea_sparse_attention_bwd_gather is gone; sea_sparse_attention_bwd takes
 *      `workspace, workspace_bytes, form` (NULL, 0 where the atomic form runs) and no longer wants dk / dv zeroed, and
 *      sea_sparse_attention_bwd_workspace_bytes takes `dtype`, `D` and `form` too.  One alignment rule for both forms (q, k, v,
 *      dout, dq, dk, dv): the atomic form used to accept misaligned fp32 dout / dq / dk / dv
 *      */
#define SEA_ABI_VERSION 7

enum sea_dtype { SEA_F32 = 0, SEA_F16 = 1, SEA_BF16 = 2 };

enum sea_error {
  SEA_OK = 0,
  SEA_EINVAL = -1,      /* bad argument (null pointer, bad dtype, stride) */
  SEA_EUNSUPPORTED = -2,/* shape outside what the kernels are built for */
  SEA_ELAUNCH = -3      /* HIP launch error (see sea_last_error) */
};

typedef void* sea_stream_t; /* hipStream_t */

int sea_version(void);
const char* sea_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * a6  grouped top-k selection.
 * Replaces: PerlinAttention.forward "mask" region, attention.py:774-947 (torch.sort + int64 rank
 * scatter + compare) and the kernel-test helper ops/kernels/causal_topk_masking.py:3-77.
 *
 * For every (n, t) keep the keep[n*keep_stride_n + t] largest of the H*T_m pooled values
 * probs[n, :, t, :] (ties: lower flat index h*T_m+b first).  Writes
 *   bits      (N, T_dst, W) uint32, W = ceil(H*T_m/32): bit f of a row = pixel f kept;
 *   mask_out  optional (N, H, T_dst, T_m) fp32 0/1, contiguous  (= partial_attention_mask_before_interp);
 * and, for the interpolation that follows (target widths as causal_resize_m_to_t.py:951-955,
 * boundaries round_half_away(b*fp32(w/T_m)), per-pixel count clamped to max_k, :657-659),
 *   row_nnz   (N, T_dst) int32      entries row t will emit,
 *   head_off  (N, T_dst, H+1) int32 exclusive per-head offsets inside the row.
 * Limits: H*T_m <= 16384, T_m % 4 == 0.
 */
int sea_topk_select(const void* probs, int dtype,
                    int64_t N, int64_t H, int64_t T_dst, int64_t T_m,
                    int64_t stride_n, int64_t stride_h, int64_t stride_t,
                    const int32_t* keep, int64_t keep_stride_n,
                    int64_t T_src, int is_causal, int max_k,
                    uint32_t* bits, float* mask_out,
                    int32_t* row_nnz, int32_t* head_off,
                    sea_stream_t stream);

/* Same outputs as sea_topk_select, but from an existing 0/1 mask (N,H,T_dst,T_m) of `dtype`
 * (nonzero = kept).  Replaces the `n_pixels` pass of scan_col, causal_resize_m_to_t.py:657-659. */
int sea_mask_to_bits(const void* mask, int dtype,
                     int64_t N, int64_t H, int64_t T_dst, int64_t T_m,
                     int64_t stride_n, int64_t stride_h, int64_t stride_t,
                     int64_t T_src, int is_causal, int max_k,
                     uint32_t* bits, int32_t* row_nnz, int32_t* head_off,
                     sea_stream_t stream);

/* crow[n, 0..T_dst] = exclusive scan of row_nnz[n, :]  (replaces cumsum + `crow_indices[:,1:] = ...`,
 * causal_resize_m_to_t.py:664,672).  crow is int32 or int64 per idx_bytes. */
int sea_csr_row_scan(const int32_t* row_nnz, int64_t N, int64_t T_dst,
                     void* crow, int idx_bytes, sea_stream_t stream);

/* a7  emit the column indices (replaces nonzero() + __scan_col_4_compute,
 * causal_resize_m_to_t.py:493-572,724-746).  col has room for z_cap entries per batch item
 * (col_stride_n elements apart); entries at or beyond crow[n,T_dst] are left untouched.
 * values_out (optional, fp32, same shape as col) receives 1.0 for every emitted entry.
 * Ids are head * T_src + key; a pixel wider than max_k is thinned with the reference's fp32 stepping of those ids, exact
 * while H * T_src < 2^24 (else SEA_EUNSUPPORTED).
 * DECODE form, t_src_dev != NULL (a step captured as a HIP graph): the row widths follow *t_src_dev (device memory: the
 * current sequence length) and the column ids are head * T_src + key for a FIXED capacity T_src >= *t_src_dev (the K / V
 * caches' row count), so sea_sparse_attention is called with that same T_src; values_out must be NULL.  A thinned pixel is
 * stepped in fp32 on the KEY alone and the head offset is added as an integer, so the capacity changes no id: needs
 * H * T_src < 2^31 (int32 ids) and T_src < 2^24 (fp32-exact keys).  Where H * T_src < 2^24 the ids are the stateless
 * form's bit for bit.
 * A length PER SEQUENCE, t_src_stride > 0 (the decode form of a batch whose sequences sit at different positions; 0 = one
 * length for the batch): batch item n's rows follow t_src_dev[n * t_src_stride], ids are head * T_src + key with T_src the
 * capacity as above.  A non-zero stride with t_src_dev = NULL, or a negative one: SEA_EINVAL; with values_out:
 * SEA_EUNSUPPORTED.
 * A sequence that SITS OUT a decoding step (below, sea_decode_cnn_tail_select) has an empty crow row, written by that launch:
 * a row with crow[t] == crow[t + 1] returns before it reads its length, so nothing is emitted for it. */
int sea_csr_emit(const uint32_t* bits, const void* crow, const int32_t* head_off,
                 int64_t N, int64_t H, int64_t T_dst, int64_t T_m,
                 int64_t T_src, int is_causal, int max_k,
                 void* col, int idx_bytes, int64_t col_stride_n, int64_t z_cap,
                 float* values_out,
                 const int32_t* t_src_dev, /* decode form, or NULL */
                 int64_t t_src_stride,     /* per-sequence lengths, or 0 */
                 sea_stream_t stream);

/* Per-(row, head) offsets of a foreign flat CSR whose rows are grouped by ascending head
 * (replaces __flat_csr_sdbmm_tch_compute, flat_csr_sdbmm.py:48-127). */
int sea_csr_head_offsets(const void* crow, const void* col, int idx_bytes,
                         int64_t N, int64_t H, int64_t T_dst, int64_t T_src,
                         int64_t col_stride_n, int32_t* head_off, sea_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a9..a12  the four unfused CSR operators (1:1 with ops/__init__.py), values are fp32 (N, Z).
 */
/* flat_csr_masked_bmm, flat_csr_masked_bmm.py:137-195: values[n,e] = q[n,h,row,:] . k[n,h,key,:] */
int sea_csr_sddmm(const void* q, const void* k, int dtype,
                  int64_t N, int64_t H, int64_t T_dst, int64_t T_src, int64_t D,
                  const int64_t* q_strides /*[n,h,t]*/, const int64_t* k_strides /*[n,h,t]*/,
                  const void* crow, const void* col, int idx_bytes, int64_t col_stride_n,
                  float* values, sea_stream_t stream);

/* flat_csr_softmax, flat_csr_softmax.py:127-176: softmax over each (row, head) group of entries. */
int sea_csr_softmax(const float* in_values, float* out_values,
                    int64_t N, int64_t H, int64_t T_dst, int64_t T_src,
                    const void* crow, const void* col, int idx_bytes, int64_t col_stride_n,
                    sea_stream_t stream);

/* flat_csr_elmul, flat_csr_elmul.py:110-162: values[n,e] *= other[n,h,row,key]  (element strides,
 * stride 0 allowed -- the module passes a row-broadcast view, attention.py:1170-1171). */
int sea_csr_elmul(const float* in_values, float* out_values,
                  const void* other, int dtype, const int64_t* other_strides /*[n,h,t,s]*/,
                  int64_t N, int64_t H, int64_t T_dst, int64_t T_src,
                  const void* crow, const void* col, int idx_bytes, int64_t col_stride_n,
                  sea_stream_t stream);

/* flat_csr_sdbmm, flat_csr_sdbmm.py:323-439: out[n,h,row,:] = sum_e values[e] * v[n,h,key,:];
 * out is fp32 (N,H,T_dst,D) contiguous, as the reference (`torch.zeros` w/o dtype, :347). */
int sea_csr_spmm(const float* values, const void* v, int dtype,
                 int64_t N, int64_t H, int64_t T_dst, int64_t T_src, int64_t D,
                 const int64_t* v_strides /*[n,h,t]*/,
                 const void* crow, const void* col, int idx_bytes, int64_t col_stride_n,
                 const int32_t* head_off,
                 float* out, sea_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fused row-indexed sparse attention (the hot kernel): SDDMM + per-(row,head) softmax +
 * row scale + SpMM (+ optional average-pool mix) in one pass, one wavefront per (n, h, t).
 * Replaces the four launches of attention.py:1158-1173 and, with `avg`/`mix`, :1236-1237.
 *
 *   out[n,h,t,:] = rs * sum_e softmax_e(q.k_e) v_e            rs  = row_scale[n,h,t]  (or 1)
 *   if mix:  out = out*a + (1-a)*avg[n,h,t,:]                  a   = mix[n,h,t]
 *
 * crow/col are int32 (internal format), head_off as produced by sea_topk_select.
 * out has dtype out_dtype and arbitrary [n,h,t] element strides (so it can be written straight
 * into the (N, T, H*D) layout of attention.py:1279-1282).
 *
 * flags, low byte = kernel path:
 *   SEA_ATTN_AUTO    with a `block_path` plan (sea_attention_plan): the ONE kernel the plan's statistics favour for this
 *                    launch, decided on the device; without a plan: the gather kernels (the tile kernel pays off only
 *                    where neighbouring query rows share most of their keys);
 *   SEA_ATTN_GATHER  row-indexed gather kernels (sea_attn.hip): one lane group per (n,h,t) row walks the row's entries,
 *                    every K / V row is fetched per entry (L2-served); any dtype, any D <= 64*vec, duplicates counted;
 *   SEA_ATTN_TILE    MFMA tile kernel (sea_attn_tile.hip): a wave owns 16 (or 32) consecutive query rows of one (n,h),
 *                    turns their entries into a key bitmap in LDS, and for every 16-key tile that holds a kept key
 *                    runs K.Q^T, the masked online softmax and V^T.P^T on v_mfma_f32_16x16x32 with K/V rows fetched
 *                    once per tile -- the shape of the reference's flat_csr_sdbmm.py:141-313.  16-bit data,
 *                    D in {64, 80, 128}, no duplicate (row, column) pairs.  SEA_EUNSUPPORTED otherwise.
 *                    CONTRACT (differs from the gather kernels): every V row below T_src must be FINITE.  A key that
 *                    shares a 16-key tile with a kept key is staged and multiplied by an exact 0, and 0 * Inf = NaN
 *                    (the reference's dense branch matmul(probs, v), attention.py:1128, has the same property); K rows
 *                    may hold anything (their scores are replaced before use).  The gather kernels read kept keys only:
 *                    a kv-cache whose unused slots are uninitialised takes SEA_ATTN_GATHER (as DecodeSession does) or
 *                    zero-fills them;
 *   SEA_ATTN_KEYRANGE  the key-range form, for K + V per head beyond an XCD's L2 (see below); range_keys in bits 16..30;
 *   bits 4..7 (SEA_ATTN_ROW_POOL_SHIFT): log2 of the row pool of the fused gather form (ROW-POOL form below; 0 = none);
 *   bits 8..11: row tiles per wave for the tile kernel (1 or 2; 0 = default for the head size);
 *   bits 12..15: log2 of its key window (6..12; 0 = default 2048);
 *   bits 16..17 (SEA_ATTN_GRID_ORDER_SHIFT; every path but SEA_ATTN_KEYRANGE, the fused forms included): the order in which
 *                    the workgroups of an XCD take the row blocks of its (n, h) pairs -- a causal row block's work grows with
 *                    t.  0: pair after pair, t ascending; 1: pair after pair, t descending (the heaviest block first); 2: the
 *                    XCD's pairs G at a time, their row blocks interleaved, t descending, G = 1 << bits 18..19
 *                    (SEA_ATTN_GRID_GROUP_SHIFT; 1, 2 or 4: G pairs' K + V share the XCD's L2).  Another value: SEA_EINVAL.
 *                    Rows are independent: every output bit is that of order 0.  The forward prefill launches read the
 *                    field: the fused gather forms (bits != NULL) with and without pools, the wave-per-row kernel (rows
 *                    wider than 16 lanes) and the tile kernel.  The decode forms (t_src_dev), a launch of at most
 *                    sea_attention_few_rows() rows and the unfused lane-group form (bits == NULL, rows of up to 16 lanes)
 *                    keep order 0 whatever the field says.  A library without the field ignores the bits.
 *
 * probs_out (optional): fp32, laid out like `col` (row n at probs_out + n*probs_stride_n): entry e receives
 *   rs * softmax_e -- the values of `partial_attention_probs` after flat_csr_softmax + flat_csr_elmul
 *   (attention.py:1162-1171).  Served by the gather kernels (SEA_ATTN_TILE + probs_out is SEA_EUNSUPPORTED;
 *   SEA_ATTN_AUTO falls back to them).
 * block_path (optional): the buffer sea_attention_plan filled.
 *
 * FUSED form, bits != NULL (round 3): steps I + J of the hot path in ONE launch -- the nearest-neighbour interpolation of
 * the kept pixels (causal_resize_m_to_t.py:493-572,631-762) INSIDE the row-indexed sparse attention (flat_csr_masked_bmm /
 * softmax / elmul / sdbmm).  Each lane group of the gather kernels expands ITS (row, head)'s kept pixels to key columns --
 * sea_csr_emit's arithmetic bit for bit: fp32 scale = w_t / T_m, bounds round_half_away(b * scale), keys descending inside
 * a pixel, the reference's fp32 stepping for a pixel wider than max_k -- into a group-private list in LDS, writes the list
 * to `col` and walks it from LDS.  No separate sea_csr_emit launch, no column re-read from memory.  `flags` is not read
 * (the gather path) but for its row-pool field, block_path must be NULL without that field, probs_out is allowed.
 *   bits      (N, T_dst, ceil(H*T_m/32)) kept-pixel masks of sea_topk_select / sea_predictor_tail_select (T_m % 32 == 0);
 *             T_m, is_causal, max_k as for that launch.  With bits = NULL, T_m / is_causal / max_k / write_cols are not read;
 *   crow      from sea_csr_row_scan over that launch's row_nnz; head_off from the same launch;
 *   col       (N, col_stride_n) int32: OUTPUT -- after the launch it holds exactly what sea_csr_emit would have written.
 *   write_cols  0 (round 4): the expanded columns stay in LDS and `col` is NOT written (blocks whose key lists exceed the
 *             kernel's LDS list still pass through their part of it): the column array is an output nobody on the hot path
 *             reads -- 266 MB and ~50 us of the headline launch.  A caller that wants it later runs sea_csr_emit on the same
 *             bits / crow (bit-identical); the Python handle keeps its columns pending and does that on first access.
 * Rows of 4 lanes and rows wider than 16 lanes are SEA_EUNSUPPORTED: run sea_csr_emit + the plain form there.
 * sea_attention_few_rows(): for a launch of at most that many rows (N * H * T_dst: a decoding step) sea_csr_emit + the
 * plain form is the faster pair -- with T_dst <= 8 that kernel's idle lane groups first touch every K / V row the step
 * will gather, so the rows' dependent walks find them in cache (same arithmetic, bit for bit).
 *
 * KEY-RANGE form, flags & 0xff == SEA_ATTN_KEYRANGE (a fused form: bits != NULL; sea_attn_keyrange.hip).  The gather kernels
 * walk each query row's kept keys over the whole key axis, so every row block of a head drags the head's whole K and V through
 * the L2 (8 MB at 32 768 bf16 d = 64 keys against 4 MB per XCD).  Here the key axis [0, T_src) is cut into
 * n_ranges = ceil(T_src / range_keys) ranges (range_keys = bits 16..30 of flags, 1 .. 32767; n_ranges <= 64) and two ordinary
 * launches on `stream` do the work, stream order being the only hand-off (no flag, no atomics, no workgroup waits for another;
 * graph-capturable; the same bits from run to run):
 *   1. per (n, h, t, range) the online-softmax state -- running maximum m, sum l, unnormalised accumulator acc[D] -- over the
 *      kept pixels whose LOWEST key lies in the range (pixels are not split; a pixel's keys may run past the range's end).  Per
 *      entry exactly the fused gather form: the same expansion arithmetic, score and online softmax with the same keys in flight.
 *      Workgroups are numbered so that all row blocks of one ((n, h), range) are dispatched next to each other on that pair's XCD,
 *      ranges ascending; a causal row block that lies entirely below a range reads no K or V row.  Only kept keys are read (the
 *      gather kernels' contract).  A row's list of one range that exceeds its share of the kernel's LDS list (8192 entries per
 *      workgroup, shared out evenly to its 64 / 32 rows) passes through it in pieces, the state staying in registers;
 *   2. M = max_r m_r, L = sum_r l_r exp(m_r - M), A = sum_r acc_r exp(m_r - M) over the ranges in ascending order (a range that
 *      held nothing for a row contributes exactly nothing), then the gather kernel's epilogue: A / L * row_scale (0 where L = 0),
 *      the mix with avg, out_dtype, out_strides.
 * With one range (range_keys >= T_src) the result is the fused gather form's bit for bit; with more it agrees to fp32 rounding
 * (another summation order): per range one exp, one multiply and one add more per output element.
 *   probs_out / probs_stride_n carry the WORKSPACE (the per-entry probabilities are not available in this form): probs_out the
 *             16-byte aligned fp32 base, probs_stride_n the floats per batch item, >= H * n_ranges * T_dst * (D + 2) and, with
 *             N > 1, a multiple of 4; NULL or too small: SEA_EINVAL (the message gives the floats needed).  Caller-owned,
 *             contents undefined before and after;
 *   col       neither read nor written (the columns stay pending: sea_csr_emit writes them for whoever reads them);
 *   write_cols must be 0, block_path NULL (SEA_EINVAL), range_keys 0 is SEA_EINVAL.
 * 16-bit data with D = 64 or 128, fp32 with D = 32 or 64; T_m % 32 == 0; is_causal 0 or 1; H * T_src < 2^24 as in the fused
 * form.  bits == NULL, any other D (80 included), t_src_dev / block_table (no decode or paged form), write_cols != 0, more than
 * 64 ranges: SEA_EUNSUPPORTED, before anything is launched.
 *
 * ROW-POOL form of the fused launch, bits != NULL and (flags >> SEA_ATTN_ROW_POOL_SHIFT) & 0xf = log2(POOL) != 0 (the one
 * field of `flags` the fused gather form reads).  The gather kernels walk the rows of a wave in lockstep for as long as the
 * wave's longest row lasts, so they deal rows to waves by length; without this field every workgroup ranks its own 64 (rows
 * of 8 lanes, d = 80 included) or 32 (rows of 16 lanes) rows.  With it the entry issues two launches on `stream`, stream order
 * being the only hand-off (graph-capturable): a pre-pass in which one workgroup per (n, h, pool of POOL consecutive query
 * rows) counting-sorts the pool's rows by their entries, longest first, into the workspace, then the fused gather kernel
 * whose wave w of the pool's block b (of nb = POOL / rows per workgroup) takes the sorted slots (w * nb + b) * rows_per_wave
 * ...: a wave holds neighbours of the sorted order, a workgroup rows from the whole length range.  Which lane group walks a
 * row changes no bit of the result: context rows and `col` are exactly those of the launch without the field.
 *   block_path  the WORKSPACE (no plan exists in the fused form): 16-byte aligned uint16 base, probs_stride_n its elements per
 *             batch item, >= H * ceil(T_dst / POOL) * POOL.  Caller-owned; after the launch it holds, per (n, h, pool), the
 *             rows' offsets in the pool in the order they were dealt (a permutation of 0 .. POOL - 1, slots past T_dst last).
 *             NULL, misaligned or too small: SEA_EINVAL (the message gives the elements needed);
 *   POOL      a multiple of the form's rows per workgroup and at most 1024, else SEA_EUNSUPPORTED;
 *   probs_out must be NULL; the decode and paged forms (t_src_dev / block_table), the key-range and tile paths and bits == NULL
 *             are SEA_EUNSUPPORTED, before anything is launched.
 * A launch of at most sea_attention_few_rows() rows (N * H * T_dst) ignores the field and reads no workspace.
 *
 * DECODE form of the fused launch, bits and t_src_dev != NULL (round 5; SURVEY 8f-3, src/main/opt_generate.py:131,
 * PA/attention.py:410-426): a position of a graph-replayed decoding session has static kernel arguments, so the sequence
 * length the row widths follow is read from device memory (*t_src_dev, what the decode form of sea_csr_emit reads) while
 * T_src is the CAPACITY -- the row count of the K / V caches -- with which the column ids are encoded (head * T_src + key).
 * Thinned pixels are stepped as the decode form of sea_csr_emit steps them (the key alone: the capacity changes no id;
 * H * T_src < 2^31).  The stateless fused form steps head * T_src + key like the reference and, like sea_csr_emit, refuses
 * H * T_src >= 2^24 (SEA_EUNSUPPORTED).
 * T_dst <= 8 new rows per sequence; 16-bit d = 64 / 80 / 128 or fp32 d = 32 / 64 (the fused forms), else
 * SEA_EUNSUPPORTED (run the decode form of sea_csr_emit + the plain form).
 * probs_out is taken (every decode form: one length or one per sequence, paged or not, T_dst = 1 .. 8): entry e of a row
 * receives rs * softmax_e at the slot `col` has for it -- or would have: with write_cols = 0 the values are written all the
 * same -- with the plain form's expression, so the values are that form's bit for bit.  probs_stride_n >= col_stride_n
 * (SEA_EINVAL otherwise).  Only the slots of real entries are written: an empty head, the slots behind a row and a sequence
 * that sits out leave probs_out as it was (a caller that replays the launch keeps one buffer and never clears it).  The lane groups of a workgroup that have no row
 * touch the K / V rows of the expanded lists before the one group per row starts its dependent walk (what the unfused
 * kernel does from `col`).  Same arithmetic in the same order as sea_csr_emit + the plain form: the step stays bitwise
 * the stateless forward; the emit launch (or the emit phase of sea_decode_cnn_tail_select: pass col = NULL there) and the
 * crow -> col -> K / V load chain leave the position's critical path.
 *
 * A length PER SEQUENCE, t_src_stride > 0 (the decode form only; 0 = one length for the batch): sequence n's row widths follow
 * t_src_dev[n * t_src_stride]; T_src is the caches' capacity the ids are encoded with.  The gather path, no plan (probs_out
 * as in the decode form above); bits and t_src_dev are required (NULL: SEA_EINVAL, as is a negative stride).  Per workgroup the length is one scalar
 * load: the same kernels, the same bits per sequence as the shared-length form at that sequence's length.
 *
 * PAGED K / V, block_table != NULL (the one-row decode form with a length per sequence: T_dst = 1, 16-bit data, D in {64, 80,
 * 128}, T_m <= 256).  k / v are the K / V halves of a page pool (P, H, page_rows, D) with element strides [page, head, row];
 * sequence n's key r lives in page block_table[n * table_stride + r / page_rows] (int32, on the device) at row r % page_rows.
 * Keys and column ids stay logical: ids are head * T_src + key as in the contiguous form, and the context rows -- and, with
 * probs_out, the per-entry values -- are bitwise that form's.  page_rows: a power of two and a multiple of the Performer chunk of D (sea_performer_chunk_rows);
 * table_stride >= ceil(T_src / page_rows), at most 4096 pages per table row; the page stride must stay below 4 GB and a page
 * below 2 GB.  Null pointers, t_src_stride = 0, a bad page size or table stride: SEA_EINVAL; other dtypes / D / shapes:
 * SEA_EUNSUPPORTED.  Without a table, page_rows and table_stride must be 0 (else SEA_EINVAL).
 * A sequence that sits out the step (per-sequence decode form: t_src_dev[n * t_src_stride] < 0, see sea_decode_cnn_tail_select):
 * its workgroups read no block table entry, K or V row, write nothing to probs_out and store ZEROS to its output rows (no row
 * scale, no mix with avg) --
 * the one-row kernel in all its forms, the paged ones included, and the T_dst = 2 .. 8 lane-group forms.  The test is on the
 * length the workgroup loads anyway, at its first use: q, crow and head_off of the sequence (valid memory; crow / head_off as
 * the selection launch wrote its empty rows) may have been read by then.
 */
enum sea_attn_path { SEA_ATTN_AUTO = 0, SEA_ATTN_GATHER = 1, SEA_ATTN_TILE = 2, SEA_ATTN_KEYRANGE = 3 };
enum { SEA_ATTN_ROW_POOL_SHIFT = 4, SEA_ATTN_GRID_ORDER_SHIFT = 16, SEA_ATTN_GRID_GROUP_SHIFT = 18 };
int sea_sparse_attention(const void* q, const void* k, const void* v, int dtype,
                         int64_t N, int64_t H, int64_t T_dst, int64_t T_src, int64_t D,
                         const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                         const int32_t* crow, const int32_t* col, int64_t col_stride_n,
                         const int32_t* head_off,
                         const float* row_scale, /* (N,H,T_dst) contiguous or NULL */
                         const void* avg, const int64_t* avg_strides, /* dtype `dtype`, or NULL */
                         const float* mix,       /* (N,H,T_dst) contiguous or NULL */
                         void* out, int out_dtype, const int64_t* out_strides,
                         float* probs_out, int64_t probs_stride_n,
                         const uint8_t* block_path, /* buffer filled by sea_attention_plan, or NULL */
                         int flags,
                         const uint32_t* bits, int64_t T_m, int is_causal, int max_k, int write_cols, /* fused form */
                         const int32_t* t_src_dev, /* decode form, or NULL */
                         int64_t t_src_stride,     /* per-sequence lengths, or 0 */
                         const int32_t* block_table, int64_t table_stride, int64_t page_rows, /* paged K / V, or NULL, 0, 0 */
                         sea_stream_t stream);
int64_t sea_attention_few_rows(void);

/* Backward of the fused operator WITHOUT its epilogue (o = sum_e softmax_e(q.k_e) v_e; the caller applies row scale and mix
 * in its autograd framework): dQ, dK, dV from dO.  Reference shape: masked_mm.py:169-267 (gradients flow through the kept
 * entries only) + the dense branch's autograd (attention.py:1061-1133).  probs = the forward's probs_out with row_scale = NULL;
 * out / dout / dq fp32 (N,H,T_dst,D) contiguous; dk / dv fp32 (N,H,T_src,D) contiguous: every row is WRITTEN, in both forms --
 * the caller does not zero them.  dQ is a plain store per row and the same from run to run; dK / dV sum a key's entries in the
 * order the launch reached them and agree between runs to fp32 rounding, in both forms.
 * form:
 *   SEA_ATTN_BWD_GATHER  (round 3) no float atomics: dK / dV are gathered over the transposed pattern.  The library counts the
 *                        entries of every (n, head, key) column (int32 atomics), scans them into list starts, lets the row pass
 *                        (dQ) drop a 16-byte record {row, p, ds} into its key's list, and a column pass (one lane group per
 *                        key) sums dK = sum ds q_row, dV = sum p dO_row with plain stores.  Rows of up to 16 lanes (D <= 64
 *                        fp32, D <= 128 16-bit); wider rows: SEA_EUNSUPPORTED.  Needs `workspace`;
 *   SEA_ATTN_BWD_ATOMIC  the first form: dK / dV rows accumulated with fp32 atomics, cleared first by a hipMemsetAsync on
 *                        `stream` (graph-capturable).  Rows of up to 64 lanes.  workspace / workspace_bytes are not read
 *                        (NULL, 0);
 *   SEA_ATTN_BWD_AUTO    the gather form where it has kernels (rows of up to 16 lanes), the atomic form for wider rows: what a
 *                        caller passes; the library decides from dtype and D.  Another value: SEA_EINVAL.
 * workspace: caller-owned scratch of sea_sparse_attention_bwd_workspace_bytes(dtype, N, H, T_src, D, col_stride_n, form) bytes,
 * contents undefined before and after.  The query returns 0 where the atomic form runs and for arguments the entry refuses;
 * else 2 * 4 * ceil4(N * (H * T_src + 1)) bytes of list starts and cursors (ceil4: up to a multiple of 4) + max(16 * N *
 * col_stride_n, 128 * N) bytes of records.  Where the gather form runs, NULL or fewer bytes is SEA_EINVAL.
 * q, k, v, dout, dq, dk, dv -- and workspace where it is read -- are 16-byte aligned (SEA_EUNSUPPORTED).  Null pointers, a bad
 * dtype, shape or form: SEA_EINVAL; D, strides (multiples of the 16-byte fragment), alignment, a pinned form without kernels:
 * SEA_EUNSUPPORTED.  Every refusal comes before anything is launched or cleared. */
enum sea_attn_bwd_form { SEA_ATTN_BWD_AUTO = 0, SEA_ATTN_BWD_GATHER = 1, SEA_ATTN_BWD_ATOMIC = 2 };
int64_t sea_sparse_attention_bwd_workspace_bytes(int dtype, int64_t N, int64_t H, int64_t T_src, int64_t D,
                                                 int64_t col_stride_n, int form);
int sea_sparse_attention_bwd(const void* q, const void* k, const void* v, int dtype,
                             int64_t N, int64_t H, int64_t T_dst, int64_t T_src, int64_t D,
                             const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                             const int32_t* crow, const int32_t* col, int64_t col_stride_n, const int32_t* head_off,
                             const float* probs, int64_t probs_stride_n, const float* out, const float* dout,
                             float* dq, float* dk, float* dv, void* workspace, int64_t workspace_bytes, int form,
                             sea_stream_t stream);

/* Kernel-choice plan for SEA_ATTN_AUTO, made on the device (no host round trip, graph-capturable).  One byte per (n, h,
 * 16-row block): 1 where the block's entries per staged 16-key tile favour the MFMA tile kernel -- estimated from the
 * kept-pixel bit masks of sea_topk_select / sea_predictor_tail_select (`bits`, (N,T_dst,ceil(H*T_m/32))): entries the block
 * walks against the 16-key tiles it would stage, favourable when entries >= entries_per_tile * tiles (<= 0: 30) -- followed,
 * 4-byte aligned, by the int32 COUNT of such blocks: `block_path` holds ((N*H*ceil(T_dst/16) + 3) & ~3) + 4 bytes.
 * With a plan, sea_sparse_attention launches BOTH kernels over all rows; each reads the count, and ONE of them runs
 * the launch while the other's workgroups exit at once: the tile kernel when the favourable blocks' share exceeds 1/2
 * (D <= 80) or 13/20 (D = 128), else the gather kernels.  (Round 2 split a launch per block between the two kernels; since
 * the gather kernels deal their rows by length that mix is slower than the better kernel alone -- scripts/
 * sweep_plan_threshold.py -- and the bytes only feed the count.)  T_m % 32 == 0, H <= 64. */
int sea_attention_plan(const uint32_t* bits, int64_t N, int64_t H, int64_t T_dst, int64_t T_src, int64_t T_m,
                       int is_causal, float entries_per_tile, uint8_t* block_path, sea_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Bandwidth-bound estimator / epilogue pieces (the callers either side of the hot kernels).
 */
/* ChannelSplit + LayerNorm (+ optional GELU): out[n, c*S+i, t, :] = act(LN(x[n, c, t, i*W:(i+1)*W]) * gamma + beta).
 * S=2, activation=0 replaces ChannelSplit (attention.py:123-131) + cnn.lnorm1 (attention.py:266);
 * S=1, activation=1 (exact-erf GELU) replaces LayerNorm + GELU of attention_predictor_enc (attention.py:190-196).
 * x (N,C,T,S*W) and out (N,C*S,T,W) contiguous, dtype `dtype`; gamma/beta (W) of the same dtype. */
int sea_split_layernorm(const void* x, int dtype, int64_t N, int64_t C, int64_t T, int64_t S, int64_t W,
                        const void* gamma, const void* beta, float eps, int activation, void* out,
                        sea_stream_t stream);

/* Predictor tail in one pass: nearest upsample x`up` along the width + 1x1 conv (C -> H channels, zero pad 1
 * on the width) + area resize (T_m+2 -> T_m) + LayerNorm(T_m) + softmax(T_m).
 * Replaces cnn.keepres.upsam / conv4 / the KeepRes resize / cnn.lnorm2 (attention.py:271-281,
 * modules.py:42-55,77-92) and the softmax of attention.py:670-673.
 * y (N,C,T,W4) of `dtype` with FIVE element strides y_strides = {n, c, t, w, c8}: element (n,c,t,w) lives at
 * n*s[0] + (c/8)*s[4] + (c%8)*s[1] + t*s[2] + w*s[3].  Plain 4-D layouts have s[4] = 8*s[1] (NCHW: s[3] == 1;
 * NHWC: s[1] == 1); the C8 layout of sea_causal_conv_c8 has s[1] = 1, s[3] = 8, s[4] = 8*W4, s[2] = C*W4;
 * conv_wT (C, Hpad) FP32 = the conv weight transposed with the head axis zero-padded to Hpad = 8*ceil(H/8),
 * conv_b (Hpad) FP32 (both are read through the scalar cache); gamma/beta (T_m) of `dtype`;
 * conv_w16 (optional, may be NULL): (16*ceil(H/16), Cp) row-major copy of the weight in `dtype`, channels zero-padded
 * to Cp (multiple of 32) -- with it, 16-bit NHWC / C8 input takes the MFMA variant of the kernel;
 * probs and optional scores (pre-softmax) are (N,H,T,T_m) contiguous of `dtype`.
 * Requires W4*up == T_m, T_m <= 512, W4 a multiple of the 16-byte vector width.
 * z form, y = NULL and z != NULL: the same tail from z = the 1x1 convolution's output (N, T, H, W4) fp32, as the epilogue
 * of sea_causal_conv_c8 writes it (16-bit maps, W4 % 4 == 0; C, y_strides, conv_wT, conv_w16 and Cp are not read;
 * conv_b (>= H) fp32 is still needed: the zero-padded border pixels of the padded 1x1 convolution are the bias alone).
 * Exactly one of y and z is non-NULL, else SEA_EINVAL. */
int sea_predictor_tail(const void* y, const float* z, int dtype, int64_t N, int64_t C, int64_t H, int64_t T, int64_t W4,
                       int64_t up, int64_t T_m, const int64_t* y_strides,
                       const void* conv_wT, const void* conv_b, const void* conv_w16, int64_t Cp,
                       const void* gamma, const void* beta, float eps,
                       void* probs, void* scores, sea_stream_t stream);

/* Predictor tail + grouped top-k selection in one launch: sea_predictor_tail (MFMA variant, 16-bit
 * channels-last / C8 input) followed by sea_topk_select on the probability map it produces, with the map's values
 * handed over on chip -- the (N,H,T,T_m) map is never re-read, and `probs` MAY BE NULL (round 4): the map is then not
 * written at all (537 MB per step at OPT-1.3B x 8, stored only because the module returns it, attention.py:1343); a caller
 * that wants it later runs sea_predictor_tail on the same y (bit-identical values).  The selection's slow path (overfull
 * threshold bin, all-equal rows) works on the on-chip keys too.
 * Bit-identical to the two separate calls.  Requires W4 * up == T_m, T_m % 4 == 0, T_m <= 512, H <= 64, H * T_m <= 16384
 * (round 4: any predictor length -- the reference's own grid runs 64 / 96 / 128 / 256 / 384,
 * src/main/benchmark_opt_ablation.py:160-186, exp_long_context.py:152; T_m = 256 with H % 4 == 0 keeps the map in
 * registers, every other shape passes it through a flat LDS image of the row).  SEA_EUNSUPPORTED when the row's LDS plan
 * does not fit.  Arguments as in sea_predictor_tail (conv_w16 mandatory, no FP32 weight copy) and sea_topk_select
 * (keep / keep_stride_n / T_src / is_causal / max_k -> bits / row_nnz / head_off).
 * fp32 data (round 5, the reference's measurement protocol): dtype = SEA_F32 with T_m = 256 (W4 = 64, up = 4), H % 4 == 0,
 * H <= 32; `conv_w16` then carries sea_predictor_tail's conv_wT, the (C, Hpad) FP32 transposed weights (Cp ignored), probs is
 * mandatory (the fp32 map is always written) and the 1x1 convolution runs on the fp32 MFMA -- bit-identical to
 * sea_predictor_tail (fp32, channels-last / C8 input: the same device code) followed by sea_topk_select.
 * z form, y = NULL and z != NULL (round 5): the launch is fed with z (N, T, H, W4) fp32 = the 1x1 convolution's output from
 * the epilogue of sea_causal_conv_c8: the "z tile" of a row -- loads of y and of the weights, MFMAs, LDS stores: a third of
 * a row's life in this issue-bound kernel -- becomes a 16-byte-per-lane copy into LDS.  C, y_strides, conv_w16 and Cp are
 * not read; everything else (and every bit of the result) as with y; a caller that wants the map later runs the z form of
 * sea_predictor_tail on the same z.  Exactly one of y and z is non-NULL, else SEA_EINVAL.
 * DECODE form, t_src_dev != NULL (y only; 16-bit data; T_m = 256 with W4 = 64, up = 4 and H % 4 == 0 on the register-resident
 * kernel, or any T_m < 256 this launch serves on the general-length kernel, which reads the row's width from t_src_dev like
 * the first; anything else -- T_m = 256 with another H, T_m > 256 -- SEA_EUNSUPPORTED): the T rows are the LAST rows of sequences of
 * *t_src_dev tokens (device memory, for a step replayed as a HIP graph); `keep` is then the absolute table -- keep[i] = K of
 * the row that sees i+1 keys, for every position the session can reach (attention.py:849-866) -- and keep_stride_n / T_src
 * are not read.  crow_out (decode form only, T == 1; else NULL): (N, 2) int32 = [0, row total] per batch item, i.e. the
 * one-row CSR's crow -- the step then needs no sea_csr_row_scan launch. */
int sea_predictor_tail_select(const void* y, const float* z, int dtype, int64_t N, int64_t C, int64_t H, int64_t T,
                              int64_t W4, int64_t up, int64_t T_m, const int64_t* y_strides, const void* conv_b,
                              const void* conv_w16, int64_t Cp, const void* gamma, const void* beta, float eps,
                              void* probs, void* scores, const int32_t* keep, int64_t keep_stride_n,
                              int64_t T_src, const int32_t* t_src_dev, int is_causal, int max_k, uint32_t* bits,
                              int32_t* row_nnz, int32_t* head_off, int32_t* crow_out, const uint32_t* consts_tab,
                              sea_stream_t stream);

/* The per-pixel constants of the tail -- for every output pixel the <= 3 taps of the area resize, gamma, beta: (W4, up, T_m,
 * gamma, beta) only, the same for every row -- computed ONCE into tab (3 * 256 uint32, 16-byte aligned) instead of by every
 * row's workgroup (round 5).  Any T_m <= 256 with W4 * up == T_m (else SEA_EUNSUPPORTED, checked before the pointers): the
 * table is [3][64 E] words, E = ceil(T_m / 64) the pixels per lane of the kernel that reads it, so at most the 3 * 256 words
 * `tab` always has; pixels past T_m hold no tap.  The `consts_tab` argument of sea_predictor_tail_select (read by its T_m = 256
 * kernels; NULL = each row computes the table itself, as before: -3.5 % of the launch at OPT-1.3B x 8, -8 % at H = 12) and of
 * sea_decode_cnn_tail_select takes it (there optional at T_m = 256, MANDATORY below). */
int sea_predictor_tail_consts(int dtype, int64_t W4, int64_t up, int64_t T_m, const void* gamma, const void* beta,
                              uint32_t* tab, sea_stream_t stream);

/* A decoding step's predictor CNN + tail + selection + state advance in ONE launch (round 5; perlin_attention/decode.py).
 * A graph-replayed position used to run conv1, conv2 (each over the session's whole 25-row window), the decode form of
 * sea_predictor_tail_select and sea_c8_window_shift: four launches for one new row per sequence, each at its fixed cost.
 * Here one workgroup per sequence
 *   - computes conv1's new row from x rows t - 2 dil, t - dil (ring of the MLP's earlier rows) and t (`x_new`, which the MLP
 *     launch has just written), conv2's new row from the ring of conv1's rows -- bit for bit the rows sea_causal_conv_c8 writes
 *     (same operand placement and k order; weights read straight from the packed images, w1_packed / w2_packed / bias as for
 *     sea_causal_conv_c8 with Cin = Cout = C, 3 x 3, `dilation`, pad_w = dilation);
 *   - runs the decode form of sea_predictor_tail_select on that row (T_m = 4 W4, up = 4; keep_table over
 *     absolute rows; outputs bits (N,1,W), row_nnz (N,1), head_off (N,1,H+1), crow_out (N,2), optional probs (N,H,1,T_m));
 *   - files x_new and conv1's new row in their rings (slot = position % ring size: nothing is shifted) and, as the last
 *     workgroup to finish, advances counters = {rows seen (the new row's position), T_src of the step, T_src of the step JUST
 *     FINISHED}: counters[2] = counters[1], then counters[0] += 1, counters[1] += 1.  Launches behind this one in the same
 *     step (the decode form of sea_csr_emit) read their T_src from counters + 2.  `ticket` is one zero-initialised int32
 *     the library owns between calls.
 * `col` (optional, C <= 64): the step's CSR columns (N, col_stride_n) int32, ids = head * T_cap + key as the decode form of
 *   sea_csr_emit writes them, at most z_cap per item -- the emit of the one new row runs inside this launch too (one launch
 *   less per position); NULL = the caller runs that emit.
 * x_new (N, C/8, W4, 8); x_ring (N, ring_x, C/8, W4, 8); y1_ring (N, ring_y, C/8, W4, 8); y2 (N, C/8, W4, 8) scratch, all `dtype`
 * (16-bit); ring sizes > 2 * dilation.  C = 2 H <= 80, H % 4 == 0.
 * PREDICTOR LENGTH: T_m = 4 W4 with W4 % 8 == 0 and W4 <= 64 (a row is one pass of the row convolution), else SEA_EUNSUPPORTED.
 *   W4 = 64 (T_m = 256) keeps the tail's row in registers, and `consts_tab` is optional (NULL: the workgroup computes it).  W4 =
 *   16, 24, 32 (T_m = 64, 96, 128: the reference's grid) run the general-length tail -- E = ceil(T_m / 64) pixels per lane, the
 *   rounded row through a flat 16-bit LDS image, bit for bit the general-length kernel of sea_predictor_tail_select -- and read
 *   the per-pixel constants from `consts_tab` ONLY: the table of sea_predictor_tail_consts for this (W4, 4, T_m), 16-byte aligned,
 *   is mandatory there (without it: SEA_EUNSUPPORTED).  Other W4 < 64 are not instantiated (SEA_EUNSUPPORTED), as is a row
 *   whose z tile, flat image (2 H T_m bytes) and candidate list do not fit the LDS beside the kernel's static arrays (the weight
 *   image, dead before the tail, is overlaid: H = 40 at T_m = 128 fits).
 * A counter triple PER SEQUENCE, counter_stride > 0 (0 = the batch's one triple): sequence n's {seen, T_src, T_src just
 * finished} at counters + n * counter_stride (counter_stride >= 3, else SEA_EINVAL).  Workgroup n reads its own triple (ring
 * slots, row widths, the in-launch emit); the last workgroup advances all N triples as above.
 * SITTING OUT (per-sequence triples; DecodeSession.pause / release): a sequence whose triple is NEGATIVE takes no part in the
 * step.  The convention of every decode entry that takes per-sequence counters: the caller stores the bitwise complement of
 * each value, {~seen, ~T_src, ~T_src just finished} (reversible; -1 = ~0 for a slot that holds no sequence), a value no live
 * sequence reaches, and writes the plain values back to let it take part again.  Here workgroup n of such a sequence leaves
 * both rings alone, writes its selection as an EMPTY row (bits 0, head_off 0, row_nnz 0, crow_out {0, 0}; probs, y2 and col
 * keep what they held) and STILL takes its ticket; the last workgroup's advance leaves a negative triple as it is.
 *
 * MULTI-ROW form, y1_scratch != NULL: a step of `rows` new rows per sequence, rows in 1 .. 8 (speculative decoding: a draft's
 * tokens verified in one step; perlin_attention/decode.py, DecodeSession.from_sequences(..., max_step_rows=...)).  One workgroup
 * per (sequence n, row j) serves position t = counters[n * counter_stride] + j:
 *   - conv1's rows t - 2 dil, t - dil, t: those at positions >= seen (new in this step) are recomputed from x rows -- x_new's
 *     row (q - seen) for a position q >= seen, the x ring's slot q % ring_x below it -- into the workgroup's own two rows of
 *     y1_scratch (N, rows, 2, C/8, W4, 8), row t into the y1 ring; older ones are read from the y1 ring;
 *   - conv2's row t into y2 (N, rows, C/8, W4, 8), then the tail + selection of that row (keep_table[t], width t + 1): bits
 *     (N, rows, W), row_nnz (N, rows), head_off (N, rows, H+1), optional probs (N, H, rows, T_m).  No crow and no in-launch emit:
 *     crow_out and col must be NULL, col_stride_n / z_cap / T_cap 0 (else SEA_EINVAL); run sea_csr_row_scan on row_nnz;
 *   - x_new's row j joins the x ring at slot t % ring_x.
 * No data passes between the workgroups of a launch: the ring slots read (positions seen - 2 dil .. seen - 1) and written
 * (seen .. seen + rows - 1) are disjoint, which needs ring_x, ring_y >= 2 * dilation + rows (else SEA_EINVAL).  A session
 * that may drop rows of a step again (rewind) needs more: x_ring >= LB + max rows (the window it exports), y1_ring >=
 * 2 * dilation + max rows.  The last of the N * rows workgroups advances every triple: counters[2] = counters[0] + rows,
 * counters[0] += rows, counters[1] = counters[0] + 1 (rows = 1: what the one-row form does).  x_new (N, rows, C/8, W4, 8) dense.
 * Everything else, and the other refusals, as for the one-row form; rows outside 1 .. 8: SEA_EINVAL.  Without y1_scratch
 * (the one-row form) rows must be 1, else SEA_EINVAL.
 * A sequence that sits out (negative triple): each of its `rows` workgroups writes an empty row (the row scan behind the launch
 * then gives it an empty crow), touches neither ring nor scratch and takes its ticket; the advance skips the triple. */
int sea_decode_cnn_tail_select(const void* x_new, void* x_ring, void* y1_ring, void* y2, void* y1_scratch, int dtype, int64_t N,
                               int64_t rows, int64_t C, int64_t H, int64_t W4, int64_t ring_x, int64_t ring_y,
                               const void* w1_packed, const float* bias1, const void* w2_packed, const float* bias2, int64_t CinP,
                               int dilation, int pad_w, const void* conv_b, const void* conv_w16, int64_t Cp, const void* gamma,
                               const void* beta, float eps, void* probs, const int32_t* keep_table, int32_t* counters,
                               int32_t* ticket, int is_causal, int max_k, uint32_t* bits, int32_t* row_nnz,
                               int32_t* head_off, int32_t* crow_out, int32_t* col, int64_t col_stride_n, int64_t z_cap,
                               int64_t T_cap, const uint32_t* consts_tab, int64_t counter_stride, sea_stream_t stream);

/* Causal cumulative average out[n,h,t,:] = sum_{s<=t} v[n,h,s,:] / (t+1), fp32 accumulation.
 * Replaces `avg_v.cumsum(-2) / arange(1..T)` (attention.py:1220-1222).  out (N,H,T,D) contiguous.
 * n_slices > 1: the T rows are cut into n_slices slices (two launches: column totals per slice, then the averages
 * starting from the totals before a slice) -- for the few (n,h) pairs of a one-sequence-per-GPU shard.
 * workspace: N*H*n_slices*D floats, caller-owned; 16-bit data, D in {32,64,80,128}.  n_slices = 1: one pass, workspace may be
 * NULL (bytes 0). */
int sea_cumavg(const void* v, int dtype, int64_t N, int64_t H, int64_t T, int64_t D, const int64_t* v_strides,
               void* out, int64_t n_slices, void* workspace, int64_t workspace_bytes, sea_stream_t stream);

/* Channel-blocked ("C8") predictor CNN for 16-bit data.
 * C8 layout of a logical (N, C, T, W) activation, C % 8 == 0:  memory (N, T, C/8, W, 8) -- 16-byte blocks of 8
 * channels, consecutive pixels of a block adjacent (what an MFMA operand fragment reads contiguously).
 * sea_split_layernorm_c8: as sea_split_layernorm (no activation) but the result is written C8,
 *   out (N, T, C*S/8, W, 8) -- the layout the conv kernels below consume (16-bit data, and fp32 since round 5).
 * sea_causal_conv_c8: y = act(conv2d(x) + bias), square kernel `ksize` (1 or 3), dilation `dilation`, zero padding
 *   (ksize-1)*dilation rows on TOP only (causal along T, = CausalConv2d of modules.py:96-192 whose lower kernel
 *   rows are masked) and pad_w columns on both sides (width preserving).  x (N,T,Cin/8,W,8), y (N,T,Cout/8,W,8);
 *   w_packed (Cout, ksize*ksize*CinP) 16-bit = weight[co, ci, i, j] laid out [co][i*ksize+j][ci], ci zero-padded to
 *   CinP (Cin rounded up to 32); bias (Cout) FP32; relu != 0 fuses the ReLU that follows conv1/conv2
 *   (attention.py:271-276). */
int sea_split_layernorm_c8(const void* x, int dtype, int64_t N, int64_t C, int64_t T, int64_t S, int64_t W,
                           const void* gamma, const void* beta, float eps, void* out, sea_stream_t stream);
/* fp32 form, dtype = SEA_F32 (round 5): exact fp32 products and accumulation on v_mfma_f32_16x16x4_f32, for callers that
 * keep the reference's fp32 measurement protocol (src/main/benchmark_bert.py:196-239).  x (N,T,Cin/8,W,8), y (N,T,Cout/8,W,8)
 * fp32 in the same channel-blocked layout; w_packed (Cout, ksize*ksize, CinP) fp32 = weight[co, ci, i, j] laid out
 * [co][i*ksize+j][ci], ci zero-padded to CinP = Cin rounded up to 16; bias (Cout) fp32.  ksize 1 or 3, Cout <= 80;
 * SEA_EUNSUPPORTED when the fp32 weight image (16*ceil(Cout/16) x ksize^2 x CinP x 4 B) exceeds the 160 KB LDS, and with z.
 *
 * 1x1 epilogue, z != NULL (round 5, 16-bit data): the LAST (conv, ReLU) pair of the predictor CNN with the tail's 1x1
 * convolution in its epilogue.  `KeepRes` adds no residual (modules.py:42-55) and a 1x1 kernel commutes with the nearest
 * x`up` upsample that sits between the two (attention.py:266-281), so  z = W1 . relu(conv(x) + bias) + b1  can be formed
 * while the activation tile is still in the matrix pipe's registers: + ceil(H/16) * ceil(Cout/32) MFMAs per 16 pixels
 * (+5.5 % at 64 -> 64 channels, 32 heads).  ksize = 3, Cout <= 80; y may be NULL (the activation is then not written);
 *   conv1x1_w16 (16*ceil(H/16), Cp1) 16-bit row-major, zero padded, Cp1 = Cout rounded up to 32 (= sea_predictor_tail's
 *   conv_w16); conv1x1_b (>= H) fp32; z (N, T, H, W) fp32 -- what the z forms of sea_predictor_tail /
 *   sea_predictor_tail_select read.
 * The activation enters the product rounded to `dtype` exactly as the y store rounds it, with the operand placement and k
 * order of the tail kernels' own z stage: z is bit for bit what they compute from y.  z = NULL: no epilogue (conv1x1_w16,
 * Cp1, conv1x1_b and H are not read). */
int sea_causal_conv_c8(const void* x, int dtype, int64_t N, int64_t T, int64_t W, int64_t Cin, int64_t Cout,
                       const void* w_packed, int64_t CinP, const float* bias, int ksize, int dilation, int pad_w,
                       int relu, void* y, const void* conv1x1_w16, int64_t Cp1, const float* conv1x1_b, int64_t H,
                       float* z, sea_stream_t stream);

/* Predictor MLP of SEA's estimator in one launch, 16-bit data, bf16/f16 MFMA:
 *   enc  = GELU(LayerNorm_D1(x W1^T + b1))                      attention_predictor_enc      (attention.py:190-196)
 *   dec  = enc W2^T + b2, split into S = 2 halves of Wd = D2/2      attention_predictor_dec_row  (attention.py:123-131,623)
 *   y    = LayerNorm_Wd(dec half) * g2 + be2, written in the C8 layout of sea_causal_conv_c8 with channel = 2*h + half
 *                                                                   cnn.lnorm1                   (attention.py:266)
 *   gate = sigmoid(enc Wsc^T + bsc)  (2 values per row)             attention_predictor_dec_scaler (attention.py:1158-1166)
 * Every Linear / LayerNorm output is rounded to `dtype` exactly where the reference's module chain rounds it.
 * x (N,H,T,Din) of `dtype`, element strides x_strides[n,h,t], Din contiguous.
 * w1_packed: W1 (D1,Din) as MFMA A fragments  [ks][tile][lane][j] = W1[16*tile + lane%16][32*ks + 8*(lane/16) + j]
 *            (ks < ceil(Din/32), tile < D1/16, zero beyond Din);
 * w2_packed: [ks][tile][lane][j] = W2'[16*tile + lane%16][f(ks, lane/16, j)],  f(ks,g,j) = 16*(2*ks + j/4) + 4*g + j%4,
 *            ks < D1/32, tile <= 2*HT, HT = ceil(Wd/16), WdP = 16*HT, where W2' = the rows of W2 (D2,D1) with each half
 *            zero-padded to WdP rows (half s at rows s*WdP .. s*WdP+Wd-1; identical to W2 when Wd % 16 == 0), followed by
 *            one extra tile whose rows 0,1 are Wsc (2,D1);
 * vectors (fp32): b1[D1] g1[D1] be1[D1] b2[2*WdP] (padded like W2') g2[WdP] be2[WdP] (zero past Wd) bsc[2].
 * Outputs: x_c8 (N, T, H*2/8, Wd, 8) of `dtype`, batch items x_c8_stride_n elements apart (0 = dense; a decode session
 *   lets the one new row of every item land behind that item's CNN window); optional tpred (N,H,T,D1) of `dtype` (= enc); optional
 * row_scale / avg_scale (N,H,T) FP32 = gate[...,0] / gate[...,1].
 * Supported (D1, D2): D1 = 128 with any D2 % 16 == 0 up to 256 (round 4: every predictor length T_M = 2*D2 with
 * T_M % 32 == 0, the reference's grid of src/main/benchmark_opt_ablation.py:160-186 included), (160,128), (256,128)
 * (the weights must fit 160 KB of LDS, or stream: D1 = 256); H % 4 == 0; Din % 8 == 0. */
int sea_predictor_mlp(const void* x, int dtype, int64_t N, int64_t H, int64_t T, int64_t Din, const int64_t* x_strides,
                      int64_t D1, int64_t D2, const void* w1_packed, const void* w2_packed, const float* vectors,
                      float eps1, float eps2, void* x_c8, int64_t x_c8_stride_n, void* tpred, float* row_scale, float* avg_scale,
                      sea_stream_t stream);

/* Causal Performer of SEA's estimator in one launch, fp32 MFMA:
 *   phi(x) = relu(D^-1/4 x W^T) + 1e-3;  ctx_t = sum_{s<=t} (phi(q_t).phi(k_s)) V_s / (phi(q_t).(sum_{s<=t} phi(k_s) + 1e-6))
 * with V = [pos | v] (the learned causal value embedding concatenated in front of v, attention.py:506-510).
 * Replaces performer_pytorch.FastAttention(causal, generalized) as called at attention.py:556-572 plus the
 * concatenations at :506-510 and :577-590.  q,k,v (N,H,T,D) of `dtype` (element strides [n,h,t]), pos (>=T, D)
 * with row stride pos_stride, proj (nb, D) FP32.  out (N,H,T,3D) contiguous of `dtype` = [ctx_pos | ctx_v | v].
 * Supported: D in {64,80,128}, nb <= 80.
 * 16-bit data runs on 16-bit MFMA with split (hi+lo) operands (64-row chunks at D = 64, 32-row chunks
 * and two column blocks per wave at D = 80 / 128); those kernels can also emit avg_out (N,H,T,D) = cumsum_t(v)/(t+1),
 * the input of the mix step (attention.py:1220-1222) -- pass NULL otherwise (sea_performer_avg_supported says when it
 * may be non-NULL).  FP32 data: fp32 MFMA throughout.
 *
 * Sequence-parallel form, n_segments > 1.  One workgroup walks one (n, h) pair's rows in order, so N*H pairs
 * fill N*H compute units: the reference's configurations that put ONE sequence on a GPU (BASELINE configs 4-5: 32-40
 * pairs on 256 CUs) leave most of the chip idle.  With n_segments > 1 the T rows are cut into segments of whole
 * 64-row chunks; a first launch leaves every segment's state increment (sum phi(k)^T [pos|v], sum phi(k), sum v) in
 * `workspace`, the second starts each segment from the sum of the increments before it (added in segment order:
 * results are reproducible run to run; they differ from the one-segment kernel in fp32 summation order only).
 * sea_performer_plan proposes n_segments for a shape (1 when N*H already fills the chip) and the workspace size;
 * the caller owns the workspace (16-byte aligned, no initialisation needed).  n_segments = 1: one pass, workspace may be
 * NULL. */
int sea_performer_causal(const void* q, const void* k, const void* v, const void* pos, int dtype,
                         const float* proj, int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb,
                         const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                         int64_t pos_stride, void* out, void* avg_out, int64_t n_segments,
                         void* workspace, int64_t workspace_bytes, sea_stream_t stream);
/* 1 when sea_performer_causal* can also write `avg_out` (the cumulative average of v) for this head size, feature
 * count and dtype, else 0 -- the one predicate both sides of the ABI use (host arithmetic only). */
int sea_performer_avg_supported(int64_t D, int64_t nb, int dtype);
int sea_performer_plan(int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb, int dtype,
                       int64_t* n_segments, int64_t* workspace_bytes);

/* Stateful, CHUNK-ALIGNED form of the causal Performer for kv-cache decoding (role of the reference's
 * StatefulCausalPerformer, attention_state.py:43-140, called from attention.py:559-566 when pconfig.use_cache; parity
 * protocol test_perlin_opt_cache.py:7-32: cached decoding reproduces the stateless forward).  The T rows handed in CONTINUE
 * sequences of which t_base rows have been seen.  The kernels walk the rows in chunks of C = sea_performer_chunk_rows(...)
 * rows (64 for D = 64, 32 for D = 80 / 128); an image -- sea_performer_state_bytes(N,H,D,nb,dtype) bytes holding, per
 * (n,h), the kernel's own FP32 accumulators sum phi(k)^T [pos|v], sum phi(k), sum v -- is always the state at a CHUNK
 * BOUNDARY: state_in at c0 = floor(t_base / C) * C (NULL only at t_base = 0), state_out at floor((t_base + T) / C) * C.
 * The open chunk's old rows c0 .. t_base-1 are walked AGAIN:
 *   k, v, pos   point at ROW c0 of the caller's kv-cache / value embedding: T + t_base % C rows are read;
 *   q, out, avg_out point at the first NEW row: T rows.
 * Every new row is thereby computed by the very instruction sequence the one-pass kernel runs for it (same chunk, same
 * operand tiles, same summation order): outputs and images are BITWISE those of sea_performer_causal over the whole
 * sequence, however the sequence is cut into calls.  16-bit data, D in {64, 80, 128} (fp32 data: SEA_EUNSUPPORTED -- the
 * torch-side state of attention_state.py serves it).  state_in and state_out may alias when n_segments = 1.
 * n_segments / workspace as in sea_performer_causal (1 / NULL for the few rows of a decode step; a prefill may
 * cut: its image then sums the segments' increments in segment order).
 * DEVICE-position form, t_base_dev != NULL (a step replayed as a HIP graph, see below): t_base = *t_base_dev and the `t_base`
 * argument is not read.  k / v are then the BASES (row 0) of the kv-caches -- they already hold the new rows -- and pos the
 * BASE of the value embedding: the kernel finds the chunk boundary itself and walks the open chunk from there.  q / out /
 * avg_out: the T new rows.  state_in and state_out are both required and may be one image (updated in place; it changes
 * only when a chunk completes).  One segment: n_segments = 1 (else SEA_EUNSUPPORTED), workspace not read.
 * A position PER SEQUENCE, t_base_stride > 0 (the device-position form; 0 = one position for the batch): sequence n has seen
 * t_base_dev[n * t_base_stride] rows.  Its chunk boundary, cache rows, embedding rows and state image (the n-th contiguous H
 * images of state_in / state_out) follow from that.  t_base_dev NULL or a negative stride: SEA_EINVAL.
 * PAGED K / V, block_table != NULL (a position per sequence, one new row each: T = 1): k / v are the K / V halves of a page pool
 * (P, H, page_rows, D), strides [page, head, row].  Sequence n's open chunk c0 .. seen (c0 = floor(seen / C) * C) lies in page
 * block_table[n * table_stride + c0 / page_rows] from row c0 % page_rows on: page_rows is a power of two and a multiple of C,
 * so one table lookup per workgroup serves the step.  capacity: the logical rows a table row covers (table_stride >=
 * ceil(capacity / page_rows)).  Everything else as in the per-sequence form, bitwise.  A table with t_base_stride = 0, or
 * page_rows / table_stride / capacity non-zero without one: SEA_EINVAL.
 * A sequence that sits out the step (per-sequence form, 16-bit kernels: t_base_dev[n * t_base_stride] < 0, the convention of
 * sea_decode_cnn_tail_select): its workgroups return before their first q / K / V load, the state image untouched; its rows
 * of `out` and `avg_out` keep what they held (stale, never mixed into another sequence's rows).  The paged form has read
 * entry 0 of the sequence's table row by then (the index is clamped; the entry may be anything and is used for nothing). */
int64_t sea_performer_chunk_rows(int64_t D, int64_t nb, int dtype);
int64_t sea_performer_state_bytes(int64_t N, int64_t H, int64_t D, int64_t nb, int dtype);
int sea_performer_causal_step(const void* q, const void* k, const void* v, const void* pos, int dtype,
                              const float* proj, int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb,
                              const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                              int64_t pos_stride, void* out, void* avg_out, const void* state_in, void* state_out,
                              int64_t state_bytes, int64_t t_base, const int32_t* t_base_dev, int64_t t_base_stride,
                              int64_t n_segments, void* workspace, int64_t workspace_bytes,
                              const int32_t* block_table, int64_t table_stride, int64_t page_rows, int64_t capacity,
                              sea_stream_t stream);

/* ---- decode step with the position in DEVICE memory ------------------------------------------------------------------
 * The reference's generation loop (src/main/opt_generate.py:131 -> attention.py use_cache branches + attention_state.py)
 * runs one position per forward.  For a step that is captured ONCE as a HIP graph and replayed per token, nothing that
 * changes with the position may sit in kernel arguments: the decode forms of sea_performer_causal_step (t_base_dev),
 * sea_predictor_tail_select, sea_csr_emit and sea_sparse_attention (t_src_dev) read it from device memory instead (an int32
 * the captured step itself increments).  Everything else of the step -- predictor MLP, the two convolutions over the
 * cached window, row scan, fused attention over K / V caches of fixed capacity -- has static arguments already. */

/* Algorithmic bytes of one sea_sparse_attention launch:
 * Z*(2*D*s + 4) + N*H*T_dst*(2*D*s + 4).  Host-side helper, no device work. */
int64_t sea_sparse_attention_bytes(int64_t Z, int64_t N, int64_t H, int64_t T_dst, int64_t D, int elem_bytes);

/* Glue of a graph-replayed decoding step (round 4; perlin_attention/decode.py, reference loop src/main/opt_generate.py:131).
 * sea_decode_stage: the ONE launch of a step whose arguments change (rows = 1: the caller's new q / k / v rows, (N,H,1,D) with
 *   element strides {n, h, t} of which t is not read, feature stride 1, 16-byte aligned rows): q is copied into q_in (N,H,D),
 *   k / v are written into kv_cache (2,N,H,capacity,D) at row counters[0] (device int32: the rows the session's state has
 *   seen).  Replaces three input copies and an index_copy_ of the framework (four launches of ~4.5 us).
 *   A counter PER SEQUENCE, counter_stride > 0 (0 = one counter for the batch): sequence n's k / v rows go to cache row
 *   counters[n * counter_stride]; a sequence whose row lies outside the capacity writes nothing.  A negative stride: SEA_EINVAL.
 *   PAGED, block_table != NULL (with a counter per sequence): kv_cache is a page pool (2, pool_pages, H, page_rows, D) dense
 *   (K pages, then V pages: one page index for both); sequence n's k / v rows go to page block_table[n * table_stride +
 *   ctr / page_rows], row ctr % page_rows (ctr = counters[n * counter_stride]).  A row at or beyond `capacity`, or whose table
 *   entry is outside 0 .. pool_pages-1, writes nothing.  Page rule and refusals as for sea_sparse_attention's paged form; a
 *   table with counter_stride = 0, or page_rows / table_stride / pool_pages non-zero without one: SEA_EINVAL.
 *   A sequence that sits out the step (counter < 0, the convention of sea_decode_cnn_tail_select) is such a row: no k / v row
 *   is written and no table entry read; its q row is handed over and read by nobody.
 *   `rows` in 2 .. 8 (the stage of a multi-row step, see sea_decode_cnn_tail_select): q / k / v (N,H,rows,D) with element strides
 *   {n, h, t}; q is copied into q_in (N,H,rows,D) dense, k / v row j of sequence n into kv_cache (2,N,H,capacity,D) at row
 *   counters[n * counter_stride] + j (counter_stride 0: the batch's one counter).  A row at or beyond the capacity writes
 *   nothing; a sequence whose counter is negative sits out the step: none of its k / v rows is written (the test is on the
 *   counter, not on counter + j).  Contiguous caches only: with a block_table SEA_EUNSUPPORTED (paged K / V takes one row per
 *   step).  rows outside 1 .. 8: SEA_EINVAL.
 * sea_c8_window_shift: xs (N, rows, row_bytes) moved up by one row in place (xs[n, r] = xs[n, r + 1]): the predictor CNN's
 *   window after a step whose MLP wrote the new row behind it (sea_predictor_mlp with x_c8_stride_n).  `counters` (optional):
 *   two device int32 advanced by one by the same launch -- the LAST of a step, so every reader of the step is done. */
int sea_decode_stage(const void* q, const void* k, const void* v, int dtype, int64_t N, int64_t H, int64_t rows, int64_t D,
                     const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                     void* q_in, void* kv_cache, int64_t capacity, const int32_t* counters, int64_t counter_stride,
                     const int32_t* block_table, int64_t table_stride, int64_t page_rows, int64_t pool_pages,
                     sea_stream_t stream);
int sea_c8_window_shift(void* xs, int64_t N, int64_t rows, int64_t row_bytes, int32_t* counters, sea_stream_t stream);

/* Fork / beam reorder of a paged ragged session's slots, between two steps (perlin_attention/decode.py: DecodeSession.fork and
 * reorder).  `moves`: DEVICE int32 (M, 5), one row per destination slot: {src, dst, src_open, dst_open, stage}.  Destination
 * dst continues as a copy of slot src; it receives
 *   - src's Performer image slice (sea_performer_state_bytes(1, H, D, nb, dtype) bytes at slot * that in `image`),
 *   - src's x_ring and y1_ring slices (x_ring_bytes / y1_ring_bytes per slot, each a multiple of 16),
 *   - src's counter row (three int32 at slot * counter_stride, counter_stride >= 3),
 *   - a block-table row: src's entries below its open index o = seen >> log2(page_rows) (seen = src's first counter), then
 *     dst_open at o, then -1 up to ceil(capacity / page_rows) entries,
 *   - when src_open >= 0 and dst_open >= 0: pool page dst_open := pool page src_open, K and V, all page_rows rows
 *     (kv_pool (2, pool_pages, H, page_rows, D) dense; src_open is src's page at index o, -1 when src has none).
 * SNAPSHOT semantics: every destination gets its source's state as it was before the call, also when that source is the
 * destination of another move (a beam swap, a cycle).  Such a move names a staging slot, stage in 0 .. n_staged-1 (else -1):
 * a first launch copies those sources' image, rings, counters and table rows into `staging` (n_staged slots of
 * img_bytes + x_ring_bytes + y1_ring_bytes + 16 + 16 * ceil(ceil(capacity / page_rows) / 4) bytes each), a second writes
 * every destination.  The first launch is skipped when n_staged = 0.  No host synchronisation.
 * The device contents of `moves` cannot be checked here; the caller guarantees:
 *   - destinations are distinct, and no move has src == dst,
 *   - a move whose source is the destination of another move has a staging slot of its own,
 *   - destination open pages are distinct, and held by no slot before the call (so no source page is written),
 *   - the block table, pool and counters describe the host's view of the session (the table rows name pool pages).
 * Out-of-range slots, stage indices and pages in `moves` skip the item instead of writing out of bounds.
 * This is the only entry that writes one slot's state from another's; it must not run concurrently with a step of the same
 * session (call it in the step's stream, between steps).  Null pointers (staging: when n_staged > 0), M outside 1 .. N,
 * n_staged outside 0 .. M, a counter_stride below 3, a bad page size / table stride / pool, a staging buffer too small:
 * SEA_EINVAL; other dtypes / D, ring bytes that are not whole 16-byte chunks, unaligned buffers: SEA_EUNSUPPORTED.
 * A source that sits out steps (negative counters = the complement of its values, sea_decode_cnn_tail_select): the counters
 * are copied as they are -- the copy sits out too -- and the open page index is taken from the DECODED `seen` (~counter).  The
 * kernel decodes; the caller passes the slot's open page in `moves` as for any source. */
int sea_decode_fork(const int32_t* moves, int64_t M, int64_t n_staged, int dtype, int64_t N, int64_t H, int64_t D, int64_t nb,
                    void* image, void* x_ring, int64_t x_ring_bytes, void* y1_ring, int64_t y1_ring_bytes,
                    int32_t* counters, int64_t counter_stride, int32_t* block_table, int64_t table_stride, int64_t capacity,
                    void* kv_pool, int64_t page_rows, int64_t pool_pages, void* staging, int64_t staging_bytes,
                    sea_stream_t stream);

/* Extending ONE slot of a ragged session by many rows between two steps (perlin_attention/decode.py: DecodeSession.extend).
 * The rows themselves are the module's cached forward over the new rows, which reads contiguous K / V; these two entries move
 * the slot's rows between its pages and a contiguous buffer and file the forward's result into the slot.  Grid-stride loops
 * over 16-byte chunks, no LDS, no flag between workgroups, no host synchronisation.  Additive: the ABI version stays.
 *
 * sea_decode_gather_rows: rows [r0, r1) of sequence `slot`, K and V, from kv_pool (2, pool_pages, H, page_rows, D) into `out`
 *   (2, H, out_rows, D) dense, row r at out row r - r0, through the sequence's block-table row (block_table + slot *
 *   table_stride, on the device).  A row whose table entry is outside 0 .. pool_pages-1 is skipped (its out row keeps what
 *   it held); r0 == r1 launches nothing.  Null pointers, a bad page size / table stride / pool (as for sea_decode_stage's paged
 *   form), a slot outside 0 .. N-1, r0 > r1, r0 < 0, r1 > capacity, out_rows < r1 - r0: SEA_EINVAL; other dtypes than f16 /
 *   bf16, D outside {64, 80, 128}, unaligned buffers: SEA_EUNSUPPORTED.
 *
 * sea_decode_append_rows: slot `slot` stood at `seen` rows and now stands at t = seen + rows.  ONE launch writes
 *   - K / V rows seen .. t-1 into the slot's pages through its table row: row seen + i of head h is read at
 *     k_rows + h * k_strides[0] + i * k_strides[1] elements (v alike; feature stride 1, 16-byte aligned rows).  kv_pool NULL
 *     (a contiguous session: its rows lie in its cache already): no K / V part, and k_rows / v_rows / the strides /
 *     block_table are not read (block_table, table_stride, page_rows, pool_pages must be NULL / 0).  A row at or beyond
 *     `capacity`, or whose table entry is outside the pool, is skipped, as in sea_decode_stage;
 *   - the x ring: `window` (window_rows, row_bytes) dense holds the predictor CNN's input rows of positions t - window_rows ..
 *     t-1; each goes to ring row position % x_ring_rows of the slot's slice (x_ring (N, x_ring_rows, row_bytes)); the other
 *     ring rows keep what they held;
 *   - the y1 ring: `conv1_rows` (window_rows, row_bytes) is the first convolution over that window; its last keep_rows rows
 *     (positions t - keep_rows .. t-1: the rows whose taps lie inside the window) go to ring row position % y1_ring_rows,
 *     EVERY other row of the slot's ring slice is zeroed (what seeding a slot of length t leaves);
 *   - the Performer image: sea_performer_state_bytes(1, H, D, nb, dtype) bytes from image_src into the slot's slice of `image`;
 *   - the counter row: counters[slot * counter_stride + 0 .. 2] = {ctr_seen, ctr_tsrc, ctr_done}, as the host gives them
 *     (plain {t, t + 1, t}, or the bitwise complement of each for a slot that sits out steps).
 *   Every written chunk is written by exactly one work item and no item reads what another writes.  It must not run
 *   concurrently with a step of the same session (call it in the step's stream, between steps).
 *   Null pointers, a slot outside 0 .. N-1, a counter_stride below 3, rows < 1 or seen + rows > capacity (r0 > r1), a window
 *   that does not fit the rings (window_rows outside 1 .. min(x_ring_rows, t), keep_rows outside 0 .. min(window_rows,
 *   y1_ring_rows - 1)), a bad page size / table stride / pool: SEA_EINVAL; other dtypes / D, image or ring rows that are not
 *   whole 16-byte chunks, unaligned rows or strides: SEA_EUNSUPPORTED. */
int sea_decode_gather_rows(const void* kv_pool, int dtype, int64_t N, int64_t H, int64_t D, int64_t capacity,
                           const int32_t* block_table, int64_t table_stride, int64_t page_rows, int64_t pool_pages,
                           int64_t slot, int64_t r0, int64_t r1, void* out, int64_t out_rows, sea_stream_t stream);
int sea_decode_append_rows(int dtype, int64_t slot, int64_t N, int64_t H, int64_t D, int64_t nb, int64_t seen, int64_t rows,
                           int64_t capacity, const void* k_rows, const void* v_rows, const int64_t* k_strides,
                           const int64_t* v_strides, void* kv_pool, const int32_t* block_table, int64_t table_stride,
                           int64_t page_rows, int64_t pool_pages, const void* window, int64_t window_rows,
                           const void* conv1_rows, int64_t keep_rows, int64_t row_bytes, void* x_ring, int64_t x_ring_rows,
                           void* y1_ring, int64_t y1_ring_rows, const void* image_src, void* image, int32_t* counters,
                           int64_t counter_stride, int32_t ctr_seen, int32_t ctr_tsrc, int32_t ctr_done, sea_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SEA_HIP_H */
