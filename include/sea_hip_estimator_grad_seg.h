/*
 * sea_hip_estimator_grad_seg.h -- the row-segmented form of the causal Performer's backward in libsea_hip.so (MI355X, gfx950),
 * beside sea_hip_estimator_grad.h.
 *
 * That header and the others are not touched by anything here: these entries are additive, carry a version of their own and
 * follow the same conventions -- plain pointers and sizes, every pointer DEVICE memory owned by the caller (stride arrays are
 * host memory), nothing allocated or kept, every call asynchronous on `stream`, 0 on success and a negative SEA_E* otherwise with
 * the text in sea_last_error(), tensors addressed by ELEMENT strides with an innermost stride of 1.
 */
#ifndef SEA_HIP_ESTIMATOR_GRAD_SEG_H
#define SEA_HIP_ESTIMATOR_GRAD_SEG_H

#include "sea_hip_estimator_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of the entries in this header, returned by sea_estimator_grad_seg_version().
 *   1  sea_performer_causal_bwd over row segments */
#define SEA_ESTIMATOR_GRAD_SEG_ABI_VERSION 1

int sea_estimator_grad_seg_version(void);

/* ---------------------------------------------------------------------------------------------
 * s1  sea_performer_causal_bwd with the rows of every (n, h) cut into segments that run as workgroups of their own.
 *
 * The rows are cut into whole chunks of 64.  With nc = ceil(T / 64) and `requested` >= 1:
 *   cps = ceil(nc / min(requested, nc))   chunks per segment
 *   Sg  = ceil(nc / cps)                  the effective count, what sea_performer_causal_bwd_seg_count returns
 * and segment j owns the chunks [j cps, min(nc, (j + 1) cps)): only the last one may hold the partial chunk.
 *
 * The state a chunk needs is a sum over the rows before it (S, z) or after it (R, r), so with Sg > 1 a segment's own part of
 * that sum is computed by a launch of its own and handed over through the workspace:
 *   1  segments 0 .. Sg-2:  dS_j = sum b^T V, dz_j = sum b over the segment's rows
 *   2  the forward sweep of sea_performer_causal_bwd over the grid (N H, Sg); segment j starts from the sum of dS_j', dz_j'
 *      over j' < j, added in ascending j'
 *   3  segments 1 .. Sg-1:  dR_j = sum a^T G, dr_j = sum a^T e (from the row scalars launch 2 wrote)
 *   4  the reverse sweep over the same grid; segment j starts from the sum of dR_j', dr_j' over j' > j, added in descending j'
 *   5  the reduction of d_pos over (n, h), as it is
 * No floating-point atomics and no waiting between workgroups: every dependency is a launch boundary on `stream`, every sum has
 * one order, the same inputs and the same `segments` give the same bits.  With Sg = 1 the launches are exactly those of
 * sea_performer_causal_bwd, and so are the bits.
 *
 * Arguments, layouts, alignment and limits are those of sea_performer_causal_bwd (D = 64, 1 <= nb <= 80, the three dtypes,
 * T < 2^24, N*H < 2^31); `segments` is the requested count, any value >= 1 (larger than nc: one chunk per segment).
 * workspace: sea_performer_causal_bwd_seg_workspace_bytes(...) bytes -- those of sea_performer_causal_bwd plus
 * 2 * N*H * Sg * (NBP * 2D + NBP) fp32 with NBP = 48 for nb <= 48 and 80 above -- 16-byte aligned, contents irrelevant before and after.
 *
 * Refusals, all before any launch: those of sea_performer_causal_bwd under this entry's name, and SEA_EINVAL for segments < 1.
 */
int64_t sea_performer_causal_bwd_seg_count(int64_t T, int64_t requested);            /* Sg; 0 for T < 1 or requested < 1 */
int64_t sea_performer_causal_bwd_seg_workspace_bytes(int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb, int dtype,
                                                     int64_t segments);                                  /* 0: no kernel */
int sea_performer_causal_bwd_seg(const void* q, const void* k, const void* v, const void* pos, int dtype, const float* proj,
                                 int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb,
                                 const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides, int64_t pos_stride,
                                 const void* grad_out, void* d_q, void* d_k, void* d_v, float* d_pos,
                                 int64_t segments, void* workspace, int64_t workspace_bytes, sea_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SEA_HIP_ESTIMATOR_GRAD_SEG_H */
