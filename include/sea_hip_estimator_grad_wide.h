/*
 * sea_hip_estimator_grad_wide.h -- the causal Performer's backward for the wide heads (D = 80 and 128) in libsea_hip.so (MI355X,
 * gfx950), beside sea_hip_estimator_grad.h (D = 64) and sea_hip_estimator_grad_seg.h (its row segments).
 *
 * Those headers and the others are not touched by anything here: these entries are additive, carry a version of their own and
 * follow the same conventions -- plain pointers and sizes, every pointer DEVICE memory owned by the caller (stride arrays are
 * host memory), nothing allocated or kept, every call asynchronous on `stream`, 0 on success and a negative SEA_E* otherwise with
 * the text in sea_last_error(), tensors addressed by ELEMENT strides with an innermost stride of 1.
 */
#ifndef SEA_HIP_ESTIMATOR_GRAD_WIDE_H
#define SEA_HIP_ESTIMATOR_GRAD_WIDE_H

#include "sea_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of the entries in this header, returned by sea_estimator_grad_wide_version().
 *   1  sea_performer_causal_bwd_wide */
#define SEA_ESTIMATOR_GRAD_WIDE_ABI_VERSION 1

int sea_estimator_grad_wide_version(void);

/* ---------------------------------------------------------------------------------------------
 * w1  the backward of sea_performer_causal for D = 80 and D = 128: what sea_performer_causal_bwd computes for D = 64, argument
 * for argument -- d_q, d_k, d_v (N,H,T,D, contiguous, the data type) and d_pos (T,D, fp32) from q, k, v, pos, the fp32 projection
 * the forward was given and grad_out (N,H,T,3D, contiguous, the data type).  Nothing of the forward is saved.
 *
 * The NBP x 2D state of that backward does not fit the LDS beside its tiles at these head sizes.  Everything in it is linear in
 * the 2D value columns [pos | v], so they are split: workgroup (n h, half) of each sweep carries the NBP x D state of its D
 * columns (half 0: pos, half 1: v), computes the feature maps and the denominators itself, and writes
 *   half 0: its part of d_pos per (n, h);  half 1: d_v;  both: fp32 partial rows of d_q (forward sweep) and d_k (reverse sweep).
 * One closing launch adds the two partial images (half 0 + half 1), casts them to the data type and adds the d_pos parts in the
 * order of (n, h).  Rows run in chunks of 32.  No floating-point atomics: the same inputs give the same bits.
 *
 * sea_performer_causal_bwd_wide_supported: 1 for D in {80, 128}, 1 <= nb <= 80 and dtype among SEA_F32 / SEA_F16 / SEA_BF16 --
 * the (D, nb, dtype) the forward has a form for at these head sizes -- and 0 elsewhere; D = 64 stays with sea_performer_causal_bwd.
 * Limits: T < 2^24, N*H < 2^31.  Alignment as there: 16-byte-aligned rows of q, k, v, pos, proj, grad_out and the outputs.
 *
 * workspace: sea_performer_causal_bwd_wide_workspace_bytes(...) bytes, 16-byte aligned, contents irrelevant before and after;
 * 0 where there is no kernel.  With P = N*H and every term rounded up to 16 bytes:
 *     2 * P * T * 2 * 4       the row scalars 1 / den and g_h . num_h / den^2 of each half
 *   + 2 * (2 * P * T * D * 4) the two fp32 partial images of d_q, then those of d_k
 *   + P * T * D * 4           the d_pos parts
 *
 * Refusals, all before any launch, naming the entry and the argument:
 *   SEA_EINVAL        a null pointer, a shape below 1, negative strides or rows that overlap, misaligned rows, a short or
 *                     misaligned workspace
 *   SEA_EUNSUPPORTED  an unknown dtype, D outside {80, 128} (64 included), nb > 80, T >= 2^24 or N*H >= 2^31
 */
int sea_performer_causal_bwd_wide_supported(int64_t D, int64_t nb, int dtype);
int64_t sea_performer_causal_bwd_wide_workspace_bytes(int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb, int dtype);
int sea_performer_causal_bwd_wide(const void* q, const void* k, const void* v, const void* pos, int dtype, const float* proj,
                                  int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb,
                                  const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides, int64_t pos_stride,
                                  const void* grad_out, void* d_q, void* d_k, void* d_v, float* d_pos,
                                  void* workspace, int64_t workspace_bytes, sea_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SEA_HIP_ESTIMATOR_GRAD_WIDE_H */
