/*
 * sea_hip_train.h -- training-side entries of libsea_hip.so (MI355X, gfx950), beside the inference ABI of sea_hip.h.
 *
 * The inference ABI (sea_hip.h, SEA_ABI_VERSION) is not touched by anything here: these entries are additive, carry a version
 * of their own and follow the same conventions -- plain pointers and sizes, every pointer DEVICE memory owned by the caller
 * (stride arrays are host memory), nothing allocated or kept, every call asynchronous on `stream`, 0 on success and a negative
 * SEA_E* otherwise with the text in sea_last_error(), tensors addressed by ELEMENT strides with an innermost stride of 1.
 */
#ifndef SEA_HIP_TRAIN_H
#define SEA_HIP_TRAIN_H

#include "sea_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of the entries in this header, returned by sea_train_version().
 *   1  sea_kd_estimator_loss, sea_kd_estimator_loss_bwd */
#define SEA_TRAIN_ABI_VERSION 1

int sea_train_version(void);

/* ---------------------------------------------------------------------------------------------
 * t1  distillation loss of the estimator, causal and unpadded (row t sees keys 0 .. t of T).
 * Replaces, for the estimator term: PerlinAttention.forward's  _kl_and_mse(resize_from_m_to_t(est), truth)  -- the gather
 * of the T_m-wide score map out to (N,H,T,T), two masked fills, log_softmax, two softmaxes, kl_div and mse_loss.
 *
 * Key s of row t reads pixel  pix(t,s) = clamp(floor((fp32(s+1) - 0.5) / fp32(t+1) * fp32(T_m) - 1e-4), 0, T_m)  (fp32, IEEE
 * operations: ops/resize_dense.py), non-decreasing in s, so the keys of a pixel are contiguous; c_b keys read pixel b.  Per row,
 * with e_b the estimator score and x_s the teacher's score, both as fp32:
 *   p_b = exp(e_b - m_e) / S,  m_e = max over the pixels with c_b > 0,  S = sum_b c_b exp(e_b - m_e)
 *   tgt_s = softmax over s <= t of x_s,   G_b = sum over the keys of pixel b of tgt_s
 *   row_kl[n,h,t]  = sum_s tgt_s (log tgt_s - log p_pix(s))       (a key with tgt_s == 0 adds 0)
 *   row_mse[n,h,t] = sum_s (p_pix(s) - tgt_s)^2
 *   pix_tgt[n,h,t,b] = G_b  (exactly 0 where c_b == 0),   row_stats[n,h,t] = { m_e, log S }
 * The loss is  0.1 * sum(row_kl) / R + sum(row_mse) / (R * T),  R = N*H*T; the caller reduces the row values.
 *
 * est (N,H,T,T_m) and truth (N,H,T,T): fp32 / fp16 / bf16 independently, strides[3] = {n, h, t} in elements, rows 16-byte
 * aligned (base pointer and every stride).  Only keys s <= t are read, apart from the rest of the 16-byte chunk that holds key
 * t where that chunk lies inside the row; nothing read past t reaches a result.  The four outputs are fp32 and contiguous.
 * No atomics, one summation order: the same inputs give the same bits.
 * Limits: T_m % 4 == 0, T_m <= 512, T <= 16384 (SEA_EUNSUPPORTED otherwise, before any launch).
 */
int sea_kd_estimator_loss(const void* est, int est_dtype, const int64_t* est_strides,
                          const void* truth, int truth_dtype, const int64_t* truth_strides,
                          int64_t N, int64_t H, int64_t T, int64_t T_m,
                          float* row_kl, float* row_mse, float* pix_tgt, float* row_stats,
                          sea_stream_t stream);

/* t2  its gradient with respect to est; T_m wide, the teacher's scores are not read again.  With P_b = c_b p_b (c_b again from
 * pix, p_b from est and row_stats), G_b = pix_tgt and Q = sum_b p_b (P_b - G_b):
 *   d_est[n,h,t,b] = g * ( 0.1 / R * (P_b - G_b) + 2 / (R * T) * (p_b (P_b - G_b) - P_b Q) ),   exactly 0 where c_b == 0
 * g = *grad_loss, the upstream gradient of the scalar loss: a DEVICE fp32 (no host synchronisation).  d_est is contiguous
 * (N,H,T,T_m) in est's dtype.  Same limits as t1. */
int sea_kd_estimator_loss_bwd(const void* est, int est_dtype, const int64_t* est_strides,
                              const float* pix_tgt, const float* row_stats, const float* grad_loss,
                              int64_t N, int64_t H, int64_t T, int64_t T_m,
                              void* d_est, sea_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SEA_HIP_TRAIN_H */
