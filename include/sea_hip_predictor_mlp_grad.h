/*
 * sea_hip_predictor_mlp_grad.h -- the gradient of the predictor MLP (sea_predictor_mlp) in libsea_hip.so (MI355X, gfx950), beside the
 * inference ABI of sea_hip.h, the distillation losses of sea_hip_train.h, the Performer's backward of sea_hip_estimator_grad.h, the
 * tail's backward of sea_hip_predictor_grad.h and the CNN pairs' backward of sea_hip_predictor_cnn_grad.h.
 *
 * None of those headers is touched by anything here: these entries are additive, carry a version of their own and follow the same
 * conventions -- plain pointers and element counts, every pointer DEVICE memory owned by the caller (x_strides: host), nothing
 * allocated or kept, every call asynchronous on `stream`, 0 on success and a negative SEA_E* otherwise with the text in
 * sea_last_error().
 */
#ifndef SEA_HIP_PREDICTOR_MLP_GRAD_H
#define SEA_HIP_PREDICTOR_MLP_GRAD_H

#include "sea_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of the entries in this header, returned by sea_predictor_mlp_grad_version().
 *   1  the backward of sea_predictor_mlp without its gates: D1 = 128, D2 <= 128, Din <= 256, 16-bit data */
#define SEA_PREDICTOR_MLP_GRAD_ABI_VERSION 1

int sea_predictor_mlp_grad_version(void);

/* ---------------------------------------------------------------------------------------------
 * m1  backward of x_c8, tpred = sea_predictor_mlp(x): Linear(Din -> D1), LayerNorm(D1), erf GELU (= tpred), Linear(D1 -> D2), the two
 *     halves of Wd = D2 / 2 features LayerNorm'ed (x_c8, channel 2 h + half).  The two gate outputs are not part of it.
 *
 * Per row (n, h, t), r16 = the rounding to `dtype` the forward applies, treated straight-through:
 *   recomputed from x with the forward's expressions: a1 = r16(W1 x + b1), xh1 = (a1 - mean1) rstd1, u = xh1 g1 + be1,
 *     enc = r16(gelu(u)) (the forward's bits), dec = r16(W2 enc + b2), per half xh2 = (dec - mean2) rstd2
 *   d_g2[w] += g_y xh2      d_be2[w] += g_y      dxh2 = g_y g2      d_dec = rstd2 (dxh2 - mean(dxh2) - xh2 mean(dxh2 xh2))
 *   d_b2 += d_dec           d_w2 += d_dec (x) enc                  d_enc = W2^T d_dec (+ g_tpred)
 *   d_u = d_enc (Phi(u) + u phi(u))      d_g1 += d_u xh1      d_be1 += d_u      dxh1 = d_u g1
 *   d_a1 = rstd1 (dxh1 - mean(dxh1) - xh1 mean(dxh1 xh1))      d_b1 += d_a1      d_w1 += d_a1 (x) x      d_x = W1^T d_a1
 * Every sum is fp32; d_dec and d_a1 are rounded once to `dtype` where they become matrix operands.
 * Launches: a pack of the transposed weight images into the workspace; the row kernel (recompute + the whole per-row chain in
 * registers; enc, d_dec, d_a1 to the workspace, the LayerNorm parameters' gradients as one part per workgroup); d_x (skipped when
 * d_x is null); the weight-gradient kernel (split-K over the rows, d_b1 / d_b2 as one more column); a reduce that adds the parts in
 * block order.  No atomics, grids and block sizes that depend on the shapes alone: the same inputs give the same bits.
 *
 * x (N, H, T, Din) of `dtype` with element strides x_strides = {n, h, t} (Din contiguous); g_y the gradient of x_c8, dense C8
 * (N, T, H/4, Wd, 8); g_tpred the gradient of tpred, dense (N, H, T, D1), or null.  w1_packed, w2_packed, vectors: the images
 * sea_predictor_mlp takes, eps1 / eps2 its constants.  d_x of `dtype` with x's strides, or null.  fp32 outputs, every element
 * written: d_w1 (D1, Din), d_b1, d_g1, d_be1 (D1), d_w2 (D2, D1), d_b2 (D2), d_g2, d_be2 (Wd).
 * workspace: sea_predictor_mlp_bwd_workspace_bytes(...) bytes, 16-byte aligned, contents irrelevant before and after.
 * Limits: sea_predictor_mlp_bwd_supported -- D1 = 128, D2 % 16 == 0 and 16 <= D2 <= 128, H % 4 == 0, Din % 32 == 0 and Din <= 256,
 * SEA_F16 / SEA_BF16 -- and N H T < 2^30.
 *
 * Refusals, all before any launch; sea_last_error() names the entry and the argument.
 *   SEA_EINVAL        a null pointer that is not optional (g_tpred and d_x are), a shape that is not positive, a pointer that is not
 *                     16-byte aligned (fp32 outputs: 4), a stride that is not a multiple of 8 elements, a workspace that is too short
 *   SEA_EUNSUPPORTED  an unknown dtype code, fp32 data, shapes outside the predicate, N H T beyond the limit
 */
int sea_predictor_mlp_bwd_supported(int64_t D1, int64_t D2, int64_t H, int64_t Din, int dtype);   /* 1 / 0; host arithmetic only */
int64_t sea_predictor_mlp_bwd_workspace_bytes(int64_t N, int64_t H, int64_t T, int64_t Din, int64_t D1, int64_t D2, int dtype);   /* 0: no kernel */
int sea_predictor_mlp_bwd(const void* x, const int64_t* x_strides, const void* g_y, const void* g_tpred, int dtype, int64_t N, int64_t H,
                          int64_t T, int64_t Din, int64_t D1, int64_t D2, const void* w1_packed, const void* w2_packed,
                          const float* vectors, float eps1, float eps2, void* d_x, float* d_w1, float* d_b1, float* d_g1, float* d_be1,
                          float* d_w2, float* d_b2, float* d_g2, float* d_be2, void* workspace, int64_t workspace_bytes,
                          sea_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SEA_HIP_PREDICTOR_MLP_GRAD_H */
