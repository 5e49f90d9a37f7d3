/*
 * sea_hip_predictor_mlp_f32.h -- the predictor MLP for fp32 data in one launch, in libsea_hip.so (MI355X, gfx950), beside the inference
 * ABI of sea_hip.h (whose sea_predictor_mlp takes 16-bit data only) and the training-side headers.
 *
 * None of those headers is touched by anything here: these entries are additive, carry a version of their own and follow the same
 * conventions -- plain pointers and element counts, every pointer DEVICE memory owned by the caller (x_strides: host), nothing
 * allocated or kept, every call asynchronous on `stream`, 0 on success and a negative SEA_E* otherwise with the text in
 * sea_last_error().
 */
#ifndef SEA_HIP_PREDICTOR_MLP_F32_H
#define SEA_HIP_PREDICTOR_MLP_F32_H

#include "sea_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of the entries in this header, returned by sea_predictor_mlp_f32_version().
 *   1  sea_predictor_mlp on fp32 data: D1 = 128, Din = 192 (d = 64), D2 in {16, 32, 48, 64, 128}, H % 4 == 0 */
#define SEA_PREDICTOR_MLP_F32_ABI_VERSION 1

int sea_predictor_mlp_f32_version(void);

/* ---------------------------------------------------------------------------------------------
 * f1  x_c8, tpred, row_scale, avg_scale = the predictor MLP of an fp32 estimator, one launch, every product on v_mfma_f32_16x16x4_f32
 *     (true fp32: operands, accumulators and every intermediate; nothing is rounded to 16 bit anywhere).
 *
 * Per row (n, h, t):
 *   tpred = gelu_erf(LayerNorm_D1(W1 x + b1) g1 + be1)          attention_predictor_enc: Linear + LayerNorm + GELU
 *   dec   = W2 tpred + b2                                        attention_predictor_dec_row's Linear
 *   y[half][w] = LayerNorm_Wd(dec[half Wd .. half Wd + Wd)) g2 + be2, half in {0, 1}, Wd = D2 / 2      ChannelSplit(2) + cnn.lnorm1
 *   row_scale, avg_scale = sigmoid(Ws tpred + bs)                attention_predictor_dec_scaler and the sigmoid of its two outputs
 * y is stored in the channel-blocked C8 layout the convolutions read: x_c8 (N, T, 2 H / 8, Wd, 8) with channel 2 h + half; batch items
 * x_c8_stride_n elements apart (0: dense).  tpred (N, H, T, D1) dense, or null (not stored).  row_scale, avg_scale (N, H, T).
 * LayerNorm statistics are two-pass fp32 sums, the biased variance, rsqrt(var + eps).
 *
 * x (N, H, T, Din) fp32 with element strides x_strides = {n, h, t} (Din contiguous).
 * w1_packed  [D1 / 16][Din / 16][64 lanes][4]: lane 16 g + i of fragment (tile, kb) holds W1[16 tile + i][16 kb + 4 g + j], j = 0 .. 3
 * w2_packed  [D2 / 16][D1 / 16][64 lanes][4]:  the same packing of W2
 * vectors    b1[D1] g1[D1] be1[D1] b2[D2] g2[Wd] be2[Wd] Ws[2][D1] bs[2]
 * Limits: sea_predictor_mlp_f32_supported -- D1 = 128, Din = 192, D2 in {16, 32, 48, 64, 128}, H % 4 == 0 -- and N H T < 2^31 - 64.
 *
 * Refusals, all before any launch; sea_last_error() names the entry and the argument.
 *   SEA_EINVAL        a null pointer that is not optional (tpred is), a shape that is not positive, x, w1_packed, w2_packed, vectors,
 *                     x_c8 or tpred not 16-byte aligned (row_scale, avg_scale: 4), a stride of x that is not a multiple of 4 elements,
 *                     an x_c8_stride_n that is neither 0 nor at least one dense item in whole 16-byte blocks
 *   SEA_EUNSUPPORTED  shapes outside the predicate, N H T beyond the limit
 */
int sea_predictor_mlp_f32_supported(int64_t D1, int64_t D2, int64_t H, int64_t Din);   /* 1 / 0; host arithmetic only */
int sea_predictor_mlp_f32(const float* x, int64_t N, int64_t H, int64_t T, int64_t Din, const int64_t* x_strides, int64_t D1, int64_t D2,
                          const float* w1_packed, const float* w2_packed, const float* vectors, float eps1, float eps2, float* x_c8,
                          int64_t x_c8_stride_n, float* tpred, float* row_scale, float* avg_scale, sea_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SEA_HIP_PREDICTOR_MLP_F32_H */
