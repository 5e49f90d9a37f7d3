/*
 * sea_hip_context_grad.h -- the sparse context branch under autograd in libsea_hip.so (MI355X, gfx950): what lies between the sparse
 * product o = sum_e softmax_e(q . k_e) v_e and the (N, T, H D) context, forwards and backwards, beside the inference ABI of sea_hip.h,
 * the distillation losses of sea_hip_train.h and the gradient headers (sea_hip_estimator_grad.h, sea_hip_estimator_grad_seg.h,
 * sea_hip_predictor_grad.h, sea_hip_predictor_cnn_grad.h, sea_hip_predictor_mlp_grad.h).
 *
 * None of those headers is touched by anything here: these entries are additive, carry a version of their own and follow the same
 * conventions -- plain pointers and element counts, every pointer DEVICE memory owned by the caller (v_strides: host), nothing
 * allocated or kept, every call asynchronous on `stream`, 0 on success and a negative SEA_E* otherwise with the text in
 * sea_last_error().
 */
#ifndef SEA_HIP_CONTEXT_GRAD_H
#define SEA_HIP_CONTEXT_GRAD_H

#include "sea_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of the entries in this header, returned by sea_context_grad_version().
 *   1  scale, mix and cumulative average around the sparse product: T_dst = T_src, D in {64, 80, 128}, fp32 / fp16 / bf16 */
#define SEA_CONTEXT_GRAD_ABI_VERSION 1

int sea_context_grad_version(void);

/* ---------------------------------------------------------------------------------------------
 * The expression, per (n, h, t), with a = mix, rs = row_scale (1 when null) and r16 the rounding to `dtype`:
 *   avg[t]  = r16( (v[0] + ... + v[t]) / (t + 1) )                       fp32 sums, a true fp32 division
 *   ctx[n, t, h D : (h + 1) D] = (o[t] rs) a + (1 - a) avg[t]            stored as `out_dtype`
 * and its gradient, g = d ctx, r16 passed as the identity:
 *   d_o[t]  = a rs g[t]          d_row_scale[t] = a (g[t] . o[t])          d_mix[t] = g[t] . (rs o[t] - avg[t])
 *   dv[t]   = dv_attn[t] + sum_{s >= t} w[s],   w[s] = (1 - a_s) g[s] / (s + 1)
 * where d_o is the `dout` sea_sparse_attention_bwd takes and dv_attn the dv it returns.
 *
 * Every scan along T is cut into chunks of 64 rows: a launch of grid (N H, ceil(T / 64)) writes one column sum per chunk to the
 * workspace, and every workgroup of the launch after it adds the sums of the chunks before its own in ascending order (behind its
 * own in descending order, for the suffix sum) and scans its 64 rows in LDS.  No floating-point atomics, one summation order, grids
 * that depend on the shape alone: the same inputs give the same bits, and sea_context_mix_bwd recomputes the very avg
 * sea_context_mix_fwd mixed in -- it is saved nowhere.
 *
 * v (N, H, T, D) of `dtype` with element strides v_strides = {n, h, t} (D contiguous); o, d_o, dv_attn fp32 (N, H, T, D) contiguous;
 * ctx, g (N, T, H D) contiguous of `out_dtype`; row_scale (or null), mix, d_row_scale (or null), d_mix (or null) fp32 (N, H, T)
 * contiguous; dv (N, H, T, D) contiguous of `dtype`.
 * workspace: sea_context_grad_workspace_bytes(N, H, T, D, backward) = (backward ? 2 : 1) * N * H * ceil(T / 64) * D * 4 bytes,
 * 16-byte aligned.  Forward: contents irrelevant before and after.  Backward: sea_context_mix_bwd writes it, sea_context_dv_finish
 * reads it -- the caller keeps it untouched between the two (sea_sparse_attention_bwd, with a workspace of its own, runs between).
 * Limits: sea_context_grad_supported -- T_dst == T_src, 0 < T < 2^24, D in {64, 80, 128}, SEA_F32 / SEA_F16 / SEA_BF16 for both.
 *
 * Refusals, all before any launch; sea_last_error() names the entry and the argument.
 *   SEA_EINVAL        a null pointer that is not optional, a shape that is not positive, a pointer that is not 16-byte aligned (the
 *                     (N, H, T) fp32 vectors: 4), a v stride that is not a multiple of 16 bytes, a workspace that is too short
 *   SEA_EUNSUPPORTED  an unknown dtype code, another D, T >= 2^24
 */
int sea_context_grad_supported(int64_t T_dst, int64_t T_src, int64_t D, int dtype, int out_dtype);   /* 1 / 0; host arithmetic only */
int64_t sea_context_grad_workspace_bytes(int64_t N, int64_t H, int64_t T, int64_t D, int backward);  /* 0: no kernel */

/* c1  forward: the chunk sums of v, then average, rounding, scale, mix, permute and cast in one pass over o, v and ctx */
int sea_context_mix_fwd(const void* v, const int64_t* v_strides, const float* o, const float* row_scale, const float* mix, int dtype,
                        int out_dtype, int64_t N, int64_t H, int64_t T, int64_t D, void* ctx, void* workspace, int64_t workspace_bytes,
                        sea_stream_t stream);

/* c2  backward, before sea_sparse_attention_bwd: the chunk sums of v and of w, then d_o, d_row_scale and d_mix */
int sea_context_mix_bwd(const void* v, const int64_t* v_strides, const float* o, const void* g, const float* row_scale,
                        const float* mix, int dtype, int out_dtype, int64_t N, int64_t H, int64_t T, int64_t D, float* d_o,
                        float* d_row_scale, float* d_mix, void* workspace, int64_t workspace_bytes, sea_stream_t stream);

/* c3  backward, after sea_sparse_attention_bwd: dv = dv_attn + the suffix sum of w (recomputed from g and mix), in `dtype` */
int sea_context_dv_finish(const void* g, const float* mix, const float* dv_attn, int dtype, int out_dtype, int64_t N, int64_t H,
                          int64_t T, int64_t D, void* dv, const void* workspace, int64_t workspace_bytes, sea_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SEA_HIP_CONTEXT_GRAD_H */
