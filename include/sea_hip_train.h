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
 *   1  the distillation losses as they were added, one entry per operator AND per form of the teacher: seven entries
 *      (sea_kd_estimator_loss[_qk], sea_kd_estimator_loss_bwd, sea_kd_score_loss[_qk], sea_kd_score_loss[_qk]_bwd)
 *   2  one entry per operator, as in sea_hip.h: the three _qk entries are gone, t1, t3 and t4 take the teacher in either form
 *      (NULL for the form that is not given, "the teacher" below), and all four refuse by one rule ("refusals" below: in t1 /
 *      t2 an unknown dtype code is now SEA_EUNSUPPORTED and a misaligned row SEA_EINVAL).  What the kernels compute is
 *      unchanged, bit for bit */
#define SEA_TRAIN_ABI_VERSION 2

int sea_train_version(void);

/* ---------------------------------------------------------------------------------------------
 * t1  distillation loss of the estimator, causal and unpadded (row t sees keys 0 .. t of T).
 * Replaces, for the estimator term: PerlinAttention.forward's  _kl_and_mse(resize_from_m_to_t(est), truth)  -- the gather
 * of the T_m-wide score map out to (N,H,T,T), two masked fills, log_softmax, two softmaxes, kl_div and mse_loss.
 *
 * Key s of row t reads pixel  pix(t,s) = clamp(floor((fp32(s+1) - 0.5) / fp32(t+1) * fp32(T_m) - 1e-4), 0, T_m)  (fp32, IEEE
 * operations: ops/resize_dense.py), non-decreasing in s, so the keys of a pixel are contiguous; c_b keys read pixel b.  Per row,
 * with e_b the estimator score and x_s the teacher's score ("the teacher" below), both as fp32:
 *   p_b = exp(e_b - m_e) / S,  m_e = max over the pixels with c_b > 0,  S = sum_b c_b exp(e_b - m_e)
 *   tgt_s = softmax over s <= t of x_s,   G_b = sum over the keys of pixel b of tgt_s
 *   row_kl[n,h,t]  = sum_s tgt_s (log tgt_s - log p_pix(s))       (a key with tgt_s == 0 adds 0)
 *   row_mse[n,h,t] = sum_s (p_pix(s) - tgt_s)^2
 *   pix_tgt[n,h,t,b] = G_b  (exactly 0 where c_b == 0),   row_stats[n,h,t] = { m_e, log S }
 * The loss is  0.1 * sum(row_kl) / R + sum(row_mse) / (R * T),  R = N*H*T; the caller reduces the row values.
 *
 * est (N,H,T,T_m): fp32 / fp16 / bf16, independent of the teacher's type, strides[3] = {n, h, t} in elements, rows 16-byte
 * aligned (base pointer and every stride).  The four outputs are fp32 and contiguous.
 * Limits: T_m % 4 == 0, T_m <= 512, 1 <= T <= 16384.
 * With the factored teacher another kernel runs (the tile body of t3, the teacher's tile alone): pix_tgt is cleared on `stream`
 * before the launch, row_stats is 8-byte aligned, and the sums S and G_b are taken in another order, so the two forms agree on
 * the same scores to rounding, not bit for bit.  The outputs mean the same, and t2 is the backward of either.
 */
int sea_kd_estimator_loss(const void* est, int est_dtype, const int64_t* est_strides,
                          const void* truth, int truth_dtype, const int64_t* truth_strides,
                          const void* teacher_q, const void* teacher_k, int teacher_dtype,
                          const int64_t* teacher_q_strides, const int64_t* teacher_k_strides,
                          int64_t N, int64_t H, int64_t T, int64_t T_m, int64_t D,
                          float* row_kl, float* row_mse, float* pix_tgt, float* row_stats,
                          sea_stream_t stream);

/* t2  its gradient with respect to est; T_m wide, the teacher is not read again in either form.  With P_b = c_b p_b (c_b again
 * from pix, p_b from est and row_stats), G_b = pix_tgt and Q = sum_b p_b (P_b - G_b):
 *   d_est[n,h,t,b] = g * ( 0.1 / R * (P_b - G_b) + 2 / (R * T) * (p_b (P_b - G_b) - P_b Q) ),   exactly 0 where c_b == 0
 * g = *grad_loss, the upstream gradient of the scalar loss: a DEVICE fp32 (no host synchronisation).  d_est is contiguous
 * (N,H,T,T_m) in est's dtype.  Same limits as t1. */
int sea_kd_estimator_loss_bwd(const void* est, int est_dtype, const int64_t* est_strides,
                              const float* pix_tgt, const float* row_stats, const float* grad_loss,
                              int64_t N, int64_t H, int64_t T, int64_t T_m,
                              void* d_est, sea_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * t3  distillation loss of the student's own scores, causal and unpadded, T_dst == T_src == T (row t sees keys 0 .. t).
 * Replaces, for the student-score term: PerlinAttention's  _kl_and_mse(q_for_score @ k_for_score^T, truth)  -- the (N,H,T,T)
 * score tensor, two masked fills, log_softmax, two softmaxes, kl_div and mse_loss.
 *
 * Per (n,h) and row t, over the keys s <= t, with S_ts = q_t . k_s accumulated in fp32 from the 16-bit inputs (the torch form
 * rounds q k^T to the data type first: the kernels keep the fp32 accumulator) and x_ts the teacher's score as fp32:
 *   p_s = softmax over s <= t of S_ts,   tgt_s = softmax over s <= t of x_ts
 *   row_kl[n,h,t]  = sum_s tgt_s (log tgt_s - log p_s)            (a key with tgt_s == 0 adds 0)
 *   row_mse[n,h,t] = sum_s (p_s - tgt_s)^2                         (key by key, never the expanded form)
 *   row_q[n,h,t]   = sum_s p_s (p_s - tgt_s)
 *   row_stats[n,h,t] = { max_s S_ts, log sum_s exp(S_ts - max), max_s x_ts, log sum_s exp(x_ts - max) }
 * The loss is  0.1 * sum(row_kl) / R + sum(row_mse) / (R * T),  R = N*H*T; the caller reduces the row values.
 *
 * q, k (N,H,T,D): fp16 or bf16, both of `qk_dtype`, each with strides[3] = {n, h, t} in elements, innermost stride 1, rows
 * 16-byte aligned (base pointer and every stride).  Columns of q / k past D are never read (D = 80: the padded k-step).  The
 * four outputs are fp32 and contiguous, row_stats 16-byte aligned.
 * A factored teacher must have the student's type, teacher_dtype == qk_dtype: one tile body serves both products, and a teacher
 * holding the student's bits gives row_kl = row_mse = row_q = 0 exactly.
 * Limits: D in {64, 80, 128}, 1 <= T <= 16384, 16-bit q / k.
 */
int sea_kd_score_loss(const void* q, const void* k, int qk_dtype, const int64_t* q_strides, const int64_t* k_strides,
                      const void* truth, int truth_dtype, const int64_t* truth_strides,
                      const void* teacher_q, const void* teacher_k, int teacher_dtype,
                      const int64_t* teacher_q_strides, const int64_t* teacher_k_strides,
                      int64_t N, int64_t H, int64_t T, int64_t D,
                      float* row_kl, float* row_mse, float* row_q, float* row_stats,
                      sea_stream_t stream);

/* t4  its gradient with respect to q and k: two launches (a pass over the query blocks for d_q, one over the key blocks for
 * d_k), both computing S again and reading the causal half of truth again, as t3 reads it (factored: computing the teacher's
 * tile again).  With p_s and tgt_s from row_stats:
 *   dS_ts = g * ( 0.1 / R * (p_s - tgt_s) + 2 / (R * T) * (p_s (p_s - tgt_s) - p_s row_q[t]) ),   0 for s > t
 *   d_q[n,h,t,:] = sum over s <= t of dS_ts k_s,      d_k[n,h,s,:] = sum over t >= s of dS_ts q_t
 * g = *grad_loss, the upstream gradient of the scalar loss: a DEVICE fp32 (no host synchronisation).  dS enters the matrix
 * instructions as a 16-bit hi + lo pair, the sums are fp32.  d_q and d_k are contiguous (N,H,T,D) in q's dtype, 8-byte aligned,
 * every element written.  Same limits as t3. */
int sea_kd_score_loss_bwd(const void* q, const void* k, int qk_dtype, const int64_t* q_strides, const int64_t* k_strides,
                          const void* truth, int truth_dtype, const int64_t* truth_strides,
                          const void* teacher_q, const void* teacher_k, int teacher_dtype,
                          const int64_t* teacher_q_strides, const int64_t* teacher_k_strides,
                          const float* row_q, const float* row_stats, const float* grad_loss,
                          int64_t N, int64_t H, int64_t T, int64_t D,
                          void* d_q, void* d_k, sea_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The teacher and the refusals, for all of the above.  t1, t3 and t4 take the teacher's scores in exactly one of two forms:
 *   the tensor  truth (N,H,T,T), fp32 / fp16 / bf16 (`truth_dtype`), truth_strides[3] = {n, h, t}.  teacher_q, teacher_k and
 *               their stride arrays must all be NULL (SEA_EINVAL otherwise: the teacher is given twice); teacher_dtype is not
 *               looked at, nor is D in t1.  Only keys s <= t are read, apart from the rest of a 16-byte chunk that holds such a
 *               key where that chunk lies inside the row's T elements; nothing read past t reaches a result.
 *   FACTORED    truth == NULL and teacher_q, teacher_k (N,H,T,D), whose product the tensor is (teacher_q already carries the
 *               teacher's scaling): fp16 or bf16, both of `teacher_dtype`, each with strides[3] = {n, h, t}, D in {64, 80, 128}.
 *               truth_dtype and truth_strides are not looked at; every teacher_* pointer is required, and a NULL teacher_q is
 *               reported with the remark that truth is NULL too.  Columns past D are never read (D = 80: the last k-step of the
 *               matrix instruction is padded with zero fragments).  With this form no T x T tensor exists in a training step,
 *               neither in the library nor in its caller.
 * Factored, x_ts = teacher_q_t . teacher_k_s is accumulated in fp32 from the 16-bit inputs, tile by tile on the matrix
 * instructions, and is NOT rounded to the data type -- the decision t3 states for the student's scores.  A caller that used to
 * hand over the teacher's own bmm result (rounded to 16 bits) therefore gets other row values than from the tensor, by far more
 * than the kernels' error; against the unrounded product the forms and the accuracy are the same.
 *
 * Refusals, the same in all four entries and all before any launch or memset; sea_last_error() names the entry and the argument.
 *   SEA_EINVAL        a null pointer, a shape that is not positive, strides that are negative or let rows overlap, a base
 *                     pointer or stride that is not 16-byte aligned (every tensor is read in 16-byte chunks; innermost stride
 *                     1), a misaligned output, a teacher given twice
 *   SEA_EUNSUPPORTED  what the kernels have no form for: an unknown dtype code, fp32 where 16-bit data is needed, D, T, T_m
 *                     beyond the limits, a grid of 2^31 workgroups or more, a factored teacher of another type than the student
 * No atomics, one summation order: the same inputs give the same bits.
 */

#ifdef __cplusplus
}
#endif

#endif /* SEA_HIP_TRAIN_H */
