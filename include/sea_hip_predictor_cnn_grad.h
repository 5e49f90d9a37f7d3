/*
 * sea_hip_predictor_cnn_grad.h -- gradients of the predictor CNN's (convolution, ReLU) pairs in libsea_hip.so (MI355X, gfx950),
 * beside the inference ABI of sea_hip.h, the distillation losses of sea_hip_train.h, the Performer's backward of
 * sea_hip_estimator_grad.h and the tail's backward of sea_hip_predictor_grad.h.
 *
 * None of those headers is touched by anything here: these entries are additive, carry a version of their own and follow the same
 * conventions -- plain pointers and element counts, every pointer DEVICE memory owned by the caller, nothing allocated or kept,
 * every call asynchronous on `stream`, 0 on success and a negative SEA_E* otherwise with the text in sea_last_error().
 */
#ifndef SEA_HIP_PREDICTOR_CNN_GRAD_H
#define SEA_HIP_PREDICTOR_CNN_GRAD_H

#include "sea_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of the entries in this header, returned by sea_predictor_cnn_grad_version().
 *   1  the backward of sea_causal_conv_c8 with its ReLU: 3 x 3, C -> C channels, dilation 1 or 2, W <= 64, 16-bit data */
#define SEA_PREDICTOR_CNN_GRAD_ABI_VERSION 1

int sea_predictor_cnn_grad_version(void);

/* ---------------------------------------------------------------------------------------------
 * c1  backward of y = relu(conv(x) + b), the dilated causal 3 x 3 layer of sea_causal_conv_c8 (relu = 1), on C8 activations.
 *
 * With d = dilation = pad_w, Wt (C, C, 3, 3) the live kernel rows, x (N, T, C/8, W, 8), y the forward's own output, g the
 * gradient of y (all C8, dense, of `dtype`):
 *   dp = g (.) (y > 0)                                          (applied as the operands are staged; never written to memory)
 *   d_b[co]         = sum_{n,t,w} dp[n,co,t,w]
 *   d_x[n,ci,t,w]   = sum_{co,i,j} Wt[co,ci,i,j] dp[n,co,t+(2-i)d, w-(j-1)d]      (rows >= T and columns outside [0,W): zero)
 *   d_w[co,ci,i,j]  = sum_{n,t,w} dp[n,co,t,w] x[n,ci,t-(2-i)d, w+(j-1)d]          (rows < 0 and columns outside [0,W): zero)
 * Launches: a pack of the transposed, tap-flipped weight image [ci][tap][co] into the workspace; the data-gradient kernel (the
 * forward with the channel axes swapped: v_mfma_f32_16x16x32 on an LDS ring of 2d+1 masked dp rows, skipped when d_x is null);
 * the weight-gradient kernel (a split-K GEMM with the pixel axis as K, operands turned by the transposing LDS reads, the
 * accumulators resident across a block of rows, d_b from the same staged rows); a reduce launch that adds the blocks' parts in
 * block order.  No atomics, a block size that depends on the shapes alone: the same inputs give the same bits.  Products are
 * exact (16-bit operands, fp32 accumulate), all sums fp32.
 *
 * w_packed: the forward's image (C, 9 CinP) [co][tap][ci], CinP = C rounded up to 32.  d_x C8 of `dtype` or null; d_w fp32
 * (C, C, 3, 3), d_b fp32 (C): every element is written.
 * workspace: sea_causal_conv_relu_bwd_workspace_bytes(...) bytes, 16-byte aligned, contents irrelevant before and after.
 * Limits: sea_causal_conv_relu_bwd_supported -- ksize = 3, C % 8 == 0 with the forward's weight image within its 160 KB
 * (C <= 80), dilation 1 or 2 with pad_w = dilation, W % 8 == 0, W <= 64, SEA_F16 / SEA_BF16 -- and N T < 2^30.
 *
 * Refusals, all before any launch; sea_last_error() names the entry and the argument.
 *   SEA_EINVAL        a null pointer that is not optional, a shape that is not positive, CinP that is not C rounded up to 32, a
 *                     pointer that is not 16-byte aligned, a workspace that is too short
 *   SEA_EUNSUPPORTED  an unknown dtype code, fp32 data, shapes outside the predicate, N T beyond the limit
 */
int sea_causal_conv_relu_bwd_supported(int64_t C, int64_t W, int ksize, int dilation, int pad_w, int dtype);   /* 1 / 0; host arithmetic only */
int64_t sea_causal_conv_relu_bwd_workspace_bytes(int64_t N, int64_t T, int64_t W, int64_t C, int dilation, int dtype);   /* 0: no kernel */
int sea_causal_conv_relu_bwd(const void* x, const void* y, const void* g, int dtype, int64_t N, int64_t T, int64_t W, int64_t C,
                             const void* w_packed, int64_t CinP, int dilation, int pad_w, void* d_x, float* d_w, float* d_b,
                             void* workspace, int64_t workspace_bytes, sea_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SEA_HIP_PREDICTOR_CNN_GRAD_H */
