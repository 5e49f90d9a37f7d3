/*
 * sea_hip_estimator_grad.h -- gradients of the estimator's kernels in libsea_hip.so (MI355X, gfx950), beside the inference ABI
 * of sea_hip.h and the distillation losses of sea_hip_train.h.
 *
 * Neither of those headers is touched by anything here: these entries are additive, carry a version of their own and follow
 * the same conventions -- plain pointers and sizes, every pointer DEVICE memory owned by the caller (stride arrays are host
 * memory), nothing allocated or kept, every call asynchronous on `stream`, 0 on success and a negative SEA_E* otherwise with
 * the text in sea_last_error(), tensors addressed by ELEMENT strides with an innermost stride of 1.
 */
#ifndef SEA_HIP_ESTIMATOR_GRAD_H
#define SEA_HIP_ESTIMATOR_GRAD_H

#include "sea_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of the entries in this header, returned by sea_estimator_grad_version().
 *   1  the backward of the causal Performer (sea_performer_causal), D = 64 with up to 80 features */
#define SEA_ESTIMATOR_GRAD_ABI_VERSION 1

int sea_estimator_grad_version(void);

/* ---------------------------------------------------------------------------------------------
 * g1  backward of sea_performer_causal (one segment or many: the gradient does not depend on how the forward cut the rows).
 *
 * With s = D^-1/4, a_t = relu(s q_t W^T) + 1e-3, b_t = relu(s k_t W^T) + 1e-3, V_t = [pos_t | v_t] (E = 2D wide), the forward is
 *   S_t = sum_{u<=t} b_u (x) V_u,  z_t = sum_{u<=t} b_u,  num_t = a_t S_t,  den_t = a_t . (z_t + 1e-6),
 *   out_t = [num_t / den_t | v_t]                                                       (3D wide)
 * and, given g_t = grad_out[n,h,t,:], with G_t = g_t[:E] / den_t and e_t = -(g_t[:E] . num_t) / den_t^2:
 *   d a_t = sum_{u<=t} (G_t . V_u + e_t) b_u + e_t 1e-6            d b_u = sum_{t>=u} (G_t . V_u + e_t) a_t
 *   d V_u = sum_{t>=u} (a_t . b_u) G_t
 *   d_q = s (d a (.) [q W^T > 0]) W,  d_k likewise,  d_v = d V[:, D:E] + g[:, E:],  d_pos[t] = sum over (n,h) of d V[:, :D]
 * Nothing of the forward is kept: a forward sweep over the rows computes a, b, S, den and num again and writes d_q and two fp32
 * per row to the workspace, a reverse sweep writes d_k, d_v and a per-(n,h) part of d_pos to the workspace, and a third launch
 * adds those parts in the order of (n,h).  No atomics, one summation order: the same inputs give the same bits.
 * All arithmetic is fp32 (v_mfma_f32_16x16x4_f32); 16-bit data is converted as it is loaded.  `proj` (nb, D) is fp32 and
 * contiguous and holds what the forward was given (for 16-bit data: the projection rounded to the data type).
 *
 * q, k, v (N,H,T,D) and pos (>= T rows of D) of `dtype` (SEA_F32 / SEA_F16 / SEA_BF16), strides[3] = {n, h, t} in elements,
 * rows 16-byte aligned (base pointer and every stride).  grad_out (N,H,T,3D), d_q, d_k, d_v (N,H,T,D) are contiguous, of
 * `dtype` and 16-byte aligned; d_pos (T,D) is fp32, contiguous; every element of the four outputs is written.
 * workspace: sea_performer_causal_bwd_workspace_bytes(...) bytes, 16-byte aligned, contents irrelevant before and after.
 * Limits: sea_performer_causal_bwd_supported (D = 64, 1 <= nb <= 80, the three dtypes), T < 2^24, N*H < 2^31.
 *
 * Refusals, all before any launch; sea_last_error() names the entry and the argument.
 *   SEA_EINVAL        a null pointer, a shape that is not positive, strides that are negative or let rows overlap, a base
 *                     pointer or stride that is not 16-byte aligned, a workspace that is too short
 *   SEA_EUNSUPPORTED  an unknown dtype code, a D or nb without a kernel, T or N*H beyond the limits
 */
int sea_performer_causal_bwd_supported(int64_t D, int64_t nb, int dtype);          /* 1 / 0; host arithmetic only */
int64_t sea_performer_causal_bwd_workspace_bytes(int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb, int dtype);   /* 0: no kernel */
int sea_performer_causal_bwd(const void* q, const void* k, const void* v, const void* pos, int dtype, const float* proj,
                             int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb,
                             const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides, int64_t pos_stride,
                             const void* grad_out, void* d_q, void* d_k, void* d_v, float* d_pos,
                             void* workspace, int64_t workspace_bytes, sea_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SEA_HIP_ESTIMATOR_GRAD_H */
