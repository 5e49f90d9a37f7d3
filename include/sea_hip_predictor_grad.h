/*
 * sea_hip_predictor_grad.h -- gradients of the predictor's kernels in libsea_hip.so (MI355X, gfx950), beside the inference ABI of
 * sea_hip.h, the distillation losses of sea_hip_train.h and the Performer's backward of sea_hip_estimator_grad.h.
 *
 * None of those headers is touched by anything here: these entries are additive, carry a version of their own and follow the same
 * conventions -- plain pointers and sizes, every pointer DEVICE memory owned by the caller (stride arrays are host memory), nothing
 * allocated or kept, every call asynchronous on `stream`, 0 on success and a negative SEA_E* otherwise with the text in
 * sea_last_error(), tensors addressed by ELEMENT strides.
 */
#ifndef SEA_HIP_PREDICTOR_GRAD_H
#define SEA_HIP_PREDICTOR_GRAD_H

#include "sea_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of the entries in this header, returned by sea_predictor_grad_version().
 *   1  the backward of the predictor tail (sea_predictor_tail), up = 4, T_m <= 256 */
#define SEA_PREDICTOR_GRAD_ABI_VERSION 1

int sea_predictor_grad_version(void);

/* ---------------------------------------------------------------------------------------------
 * p1  backward of sea_predictor_tail: upsample (1, up) -> 1x1 convolution padded by one pixel -> area resize to T_m -> LayerNorm
 *     -> softmax, for the scores s and the probabilities p it returns.
 *
 * Per (n, t) row, with Wp = up W4 + 2 and M the (T_m x (W4 + 1)) matrix of the padded nearest upsample followed by the area
 * taps (xs = floor(j Wp / T_m), xe = ceil((j + 1) Wp / T_m), weight 1 / (xe - xs); column W4 is the zero-padded border, which
 * carries the bias alone), the forward is
 *   z = W y (H x W4),  a = [z | 0] M^T,  mu, rstd over j,  xh = (a - mu) rstd,  s = gamma xh + beta,  p = softmax(s)
 * (the bias shifts every pixel of a row alike and the LayerNorm removes it: it does not enter, and its gradient is zero), and
 * given g_s = grad of s and g_p = grad of p
 *   ds = g_s + p (.) (g_p - sum_j g_p p)          d gamma += sum_h ds (.) xh          d beta += sum_h ds
 *   da = rstd (gamma ds - mean_j(gamma ds) - xh mean_j(gamma ds (.) xh))
 *   dz = (da M)[:, :W4]          d y = W^T dz (C x W4)          d W += dz y^T (H x C)
 * Nothing of the forward is kept: one 256-thread workgroup walks a contiguous block of rows, computes z, a, mu, rstd, xh (and p
 * when g_p is given) again, writes d y row by row, and keeps d W in MFMA accumulators and d gamma / d beta in registers until its
 * block ends; a second launch adds the blocks' parts in block order.  No atomics, one summation order, and a block size that
 * depends on the shapes alone: the same inputs give the same bits on every device.  All arithmetic is fp32 (the three products on
 * v_mfma_f32_16x16x4_f32); 16-bit data is converted as it is loaded.
 *
 * y (N, C, T, W4) of `dtype` (SEA_F32 / SEA_F16 / SEA_BF16) with y_strides[4] = {n, c, t, w} in elements, the innermost of them
 * (w or c) 1, rows 16-byte aligned (the base pointer and every other stride).  conv_w (H, C) fp32, contiguous: what the forward
 * was given (for 16-bit data: the weight rounded to the data type).  gamma, beta (T_m) of `dtype`.  g_scores, g_probs
 * (N, H, T, T_m) of `dtype`, contiguous; either may be null, not both.  d_y (N, C, T, W4) of `dtype`, contiguous; d_w (H, C),
 * d_gamma (T_m), d_beta (T_m) fp32; every element of the four outputs is written.
 * workspace: sea_predictor_tail_bwd_workspace_bytes(...) bytes, 16-byte aligned, contents irrelevant before and after.
 * Limits: sea_predictor_tail_bwd_supported (up = 4, W4 up = T_m, T_m a multiple of 32 up to 256, H <= 64, C <= 128 with
 * C % 8 == 0, the three dtypes), N T < 2^31.
 *
 * Refusals, all before any launch; sea_last_error() names the entry and the argument.
 *   SEA_EINVAL        a null pointer that is not optional, both gradients null, a shape that is not positive, strides that are
 *                     negative or let elements overlap, a base pointer or stride that is not 16-byte aligned, a workspace that
 *                     is too short
 *   SEA_EUNSUPPORTED  an unknown dtype code, shapes outside the predicate, a layout with neither w nor c innermost, N T beyond
 *                     the limit
 */
int sea_predictor_tail_bwd_supported(int64_t C, int64_t H, int64_t W4, int64_t up, int64_t T_m, int dtype);   /* 1 / 0; host arithmetic only */
int64_t sea_predictor_tail_bwd_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t T, int64_t W4, int64_t up, int64_t T_m, int dtype);   /* 0: no kernel */
int sea_predictor_tail_bwd(const void* y, int dtype, int64_t N, int64_t C, int64_t H, int64_t T, int64_t W4, int64_t up, int64_t T_m,
                           const int64_t* y_strides, const float* conv_w, const void* gamma, const void* beta, float eps,
                           const void* g_scores, const void* g_probs, void* d_y, float* d_w, float* d_gamma, float* d_beta,
                           void* workspace, int64_t workspace_bytes, sea_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SEA_HIP_PREDICTOR_GRAD_H */
