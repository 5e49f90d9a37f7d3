// Distillation loss of the estimator (include/sea_hip_train.h): 0.1 KL + MSE between the softmax of the T_M-wide score map
// stretched over the causal keys of each row and the softmax of the teacher's scores, without a T x T tensor.  gfx950 only.
//
// Replaces, for the estimator term of PerlinAttention.forward:
//   ops/resize_dense.py  resize_from_m_to_t   gather of the (N,H,T,T_M) scores out to (N,H,T,T)
//   attention.py         _kl_and_mse          two masked fills, log_softmax, two softmaxes, kl_div, mse_loss (fp32 copies)
//
// Inside a pixel every key has the same logit, and the keys of a pixel are contiguous (pix is non-decreasing in s), so a row
// needs the key counts c_b, the teacher's probability mass per pixel G_b and a few scalars: the forward reads the causal half
// of the teacher's scores once, the backward is T_M wide.
#include "sea_common.hpp"
#include "sea_kd.hpp"                 // kd_pix, kd_first, KD_MAX_TM, KD_MAX_T, the host checks
#include "../../include/sea_hip_train.h"

namespace sea {

constexpr int KD_FIRST_SLOTS = KD_MAX_TM + 8;     // first key of pixels 0 .. T_M (one past the last), padded to 16 bytes

// LDS slot of key s, in elements of the teacher's own type (the row is kept as it was loaded: 16-bit scores take half the
// LDS of an fp32 copy, and the LDS a row takes is what bounds the waves per CU): one pad dword per 32 dwords.  In the pixel
// pass neighbouring lanes walk neighbouring pixels, i.e. addresses a pixel width apart (1 .. T / T_M keys); unpadded, a width
// of 16 dwords puts the 32 lanes of a half wave on two banks.
template <typename TX> __device__ inline int kd_slot(int s) {
  if constexpr (sizeof(TX) == 4) return s + (s >> 5);
  else return s + 2 * (s >> 6);
}
inline size_t kd_lds_bytes(int64_t T, size_t elem) {
  const size_t row = elem == 4 ? (size_t)(T + (T >> 5) + 8) * 4 : (size_t)(T + 2 * (T >> 6) + 16) * 2;
  return (size_t)(KD_FIRST_SLOTS + KD_MAX_TM) * 4 + row;
}

struct KdParams {
  const void* est;
  const void* truth;
  int64_t esn, esh, est_t, xsn, xsh, xst;
  int N, H, T, T_M;
  float* row_kl;
  float* row_mse;
  float* pix_tgt;
  float* row_stats;
};

// One row on one wave.  LDS: first[] (first key of every pixel), e[] (the row of estimator scores), x[] (the teacher's
// scores of keys 0 .. t, padded slots).  Every sum has one order: a lane's own terms ascending, then wave_sum.
template <typename TE, typename TX>
__device__ inline void kd_row(const KdParams& p, int n, int h, int t, int* s_first, float* s_e, TX* s_x, int lane) {
  constexpr int VEC = Elem<TX>::VEC;
  const int T_M = p.T_M;
  const float len = (float)(t + 1), tm = (float)T_M;
  const int64_t r = ((int64_t)n * p.H + h) * p.T + t;
  const TX* x = reinterpret_cast<const TX*>(p.truth) + n * p.xsn + h * p.xsh + (int64_t)t * p.xst;
  const TE* e = reinterpret_cast<const TE*>(p.est) + n * p.esn + h * p.esh + (int64_t)t * p.est_t;

  for (int b = lane; b <= T_M; b += 64) s_first[b] = kd_first(b, t, len, tm, T_M);
#pragma unroll 4
  for (int b = lane; b < T_M; b += 64) s_e[b] = Elem<TE>::to_f(e[b]);

  // pass 1: keys 0 .. t in 16-byte chunks, row maximum, copy to LDS.  A chunk is loaded whole only where it lies inside
  // the row's T elements (the one that holds key t may reach past t: those values are dropped here); what is left of a row
  // whose length is no multiple of the chunk goes element by element.
  float mx = -INFINITY;
  const int nchunks = t / VEC + 1;
  const int nwhole = p.T / VEC;
  const int nvec = nchunks < nwhole ? nchunks : nwhole;
#pragma unroll 4
  for (int c = lane; c < nvec; c += 64) {
    const int s0 = c * VEC;
    float f[VEC];
    const uint4 raw = *reinterpret_cast<const uint4*>(x + s0);
    unpack16<TX>(raw, f);
    const TX* rx = reinterpret_cast<const TX*>(&raw);
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      if (s0 + j <= t) {
        mx = fmaxf(mx, f[j]);
        s_x[kd_slot<TX>(s0 + j)] = rx[j];
      }
  }
  if (nchunks > nvec) {
    const int s = nvec * VEC + lane;
    if (lane < VEC && s <= t) {
      const TX raw = x[s];
      mx = fmaxf(mx, Elem<TX>::to_f(raw));
      s_x[kd_slot<TX>(s)] = raw;
    }
  }
  mx = wave_max(mx);
  __syncthreads();

  // the estimator's softmax over the keys, from the pixels: m_e over the pixels that hold keys, S = sum c_b exp(e_b - m_e)
  float me = -INFINITY;
  for (int b = lane; b < T_M; b += 64)
    if (s_first[b + 1] > s_first[b]) me = fmaxf(me, s_e[b]);
  me = wave_max(me);
  float S = 0.f;
  for (int b = lane; b < T_M; b += 64) {
    const int c = s_first[b + 1] - s_first[b];
    if (c > 0) S += (float)c * expf(s_e[b] - me);
  }
  S = wave_sum(S);

  // pass 2: the teacher's softmax denominator
  // (four keys per step: the LDS reads and the exps of a step do not wait for each other; the additions keep their order)
  float z = 0.f;
  {
    int s = lane;
    for (; s + 192 <= t; s += 256) {
      float ex[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) ex[j] = expf(Elem<TX>::to_f(s_x[kd_slot<TX>(s + 64 * j)]) - mx);
#pragma unroll
      for (int j = 0; j < 4; ++j) z += ex[j];
    }
    for (; s <= t; s += 64) z += expf(Elem<TX>::to_f(s_x[kd_slot<TX>(s)]) - mx);
  }
  z = wave_sum(z);
  const float log_z = logf(z), inv_z = 1.0f / z, log_s = logf(S), inv_s = 1.0f / S;

  // pass 3: whole pixels per lane, the keys of a pixel ascending
  float kl = 0.f, mse = 0.f;
  float* g_out = p.pix_tgt + r * T_M;
  for (int b = lane; b < T_M; b += 64) {
    const int a0 = s_first[b], a1 = s_first[b + 1];
    float G = 0.f;
    if (a1 > a0) {
      const float de = s_e[b] - me;
      const float pb = expf(de) * inv_s, lp = de - log_s;
      float klb = 0.f, mb = 0.f;
      auto add_key = [&](float d, float tg) {
        G += tg;
        klb += tg > 0.f ? tg * ((d - log_z) - lp) : 0.f;
        const float df = pb - tg;
        mb += df * df;
      };
      int s = a0;
      for (; s + 4 <= a1; s += 4) {                 // four keys per step, as in pass 2
        float d[4], tg[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = Elem<TX>::to_f(s_x[kd_slot<TX>(s + j)]) - mx;
#pragma unroll
        for (int j = 0; j < 4; ++j) tg[j] = expf(d[j]) * inv_z;
#pragma unroll
        for (int j = 0; j < 4; ++j) add_key(d[j], tg[j]);
      }
      for (; s < a1; ++s) {
        const float d = Elem<TX>::to_f(s_x[kd_slot<TX>(s)]) - mx;
        add_key(d, expf(d) * inv_z);
      }
      kl += klb;
      mse += mb;
    }
    g_out[b] = G;
  }
  kl = wave_sum(kl);
  mse = wave_sum(mse);
  if (lane == 0) {
    p.row_kl[r] = kl;
    p.row_mse[r] = mse;
    p.row_stats[2 * r] = me;
    p.row_stats[2 * r + 1] = log_s;
  }
}

// One wave per workgroup, rows t = T - 1 - i and t = i of one (n, h): causal rows grow with t, the pair always holds T + 1
// keys, so every workgroup of the launch carries the same work.
template <typename TE, typename TX>
__global__ __launch_bounds__(64) void kd_loss_fwd_kernel(KdParams p) {
  extern __shared__ __align__(16) uint32_t kd_lds[];
  int* s_first = reinterpret_cast<int*>(kd_lds);
  float* s_e = reinterpret_cast<float*>(kd_lds + KD_FIRST_SLOTS);
  TX* s_x = reinterpret_cast<TX*>(kd_lds + KD_FIRST_SLOTS + KD_MAX_TM);
  const int lane = threadIdx.x;
  const int half = (p.T + 1) >> 1;
  const int pair = blockIdx.x / half, i = blockIdx.x - pair * half;
  const int n = pair / p.H, h = pair - n * p.H;
  const int t_long = p.T - 1 - i;
  kd_row<TE, TX>(p, n, h, t_long, s_first, s_e, s_x, lane);
  if (i != t_long) {
    __syncthreads();
    kd_row<TE, TX>(p, n, h, i, s_first, s_e, s_x, lane);
  }
}

// Backward: one wave per row, T_M wide (at most 8 pixels per lane, kept in registers between the two steps).
template <typename TE>
__global__ __launch_bounds__(256) void kd_loss_bwd_kernel(const TE* est, int64_t esn, int64_t esh, int64_t est_t,
                                                         const float* pix_tgt, const float* row_stats, const float* grad_loss,
                                                         int H, int T, int T_M, int64_t R, float k_kl, float k_mse, TE* d_est) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int64_t nh = r / T;
  const int t = (int)(r - nh * T), n = (int)(nh / H), h = (int)(nh - (int64_t)n * H);
  const float len = (float)(t + 1), tm = (float)T_M;
  const TE* e = est + n * esn + h * esh + (int64_t)t * est_t;
  const float* G = pix_tgt + r * T_M;
  const float me = row_stats[2 * r], log_s = row_stats[2 * r + 1];
  const float g = *grad_loss;
  float pb[8], Pb[8], Db[8];                      // p_b, P_b = c_b p_b, P_b - G_b
  bool held[8];
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int b = j * 64 + lane;
    pb[j] = Pb[j] = Db[j] = 0.f;
    held[j] = false;
    if (b < T_M) {
      const int c = kd_first(b + 1, t, len, tm, T_M) - kd_first(b, t, len, tm, T_M);
      if (c > 0) {
        held[j] = true;
        pb[j] = expf((Elem<TE>::to_f(e[b]) - me) - log_s);
        Pb[j] = (float)c * pb[j];
        Db[j] = Pb[j] - G[b];
        q += pb[j] * Db[j];
      }
    }
  }
  q = wave_sum(q);
  TE* out = d_est + r * T_M;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int b = j * 64 + lane;
    if (b < T_M) out[b] = from_f<TE>(held[j] ? g * (k_kl * Db[j] + k_mse * (pb[j] * Db[j] - Pb[j] * q)) : 0.f);
  }
}

// What t1 and t2 check alike: est, the shape and the limits.  `block_rows`: rows per workgroup of the kernel that will run
static int kd_check_est(const char* nm, const void* est, int est_dtype, const int64_t* est_strides, int64_t N, int64_t H,
                        int64_t T, int64_t T_m, int block_rows) {
  int rc = kd_check_nulls(nm, {KdArg{"est", est}, {"est_strides", est_strides}});
  if (rc == SEA_OK) rc = kd_check_dtype(nm, "est_dtype", "est", est_dtype, true);
  if (rc == SEA_OK) rc = kd_check_shape(nm, N, H, T, block_rows);
  if (rc == SEA_OK) rc = kd_check_tm(nm, T_m);
  if (rc == SEA_OK) rc = kd_check_rows(nm, {KdRows{"est", est, est_strides, T_m, est_dtype}});
  return rc;
}

template <typename TE, typename TX> static int kd_launch_fwd(const char* nm, const KdParams& p, hipStream_t s) {
  const size_t lds = kd_lds_bytes(p.T, sizeof(TX));
  if (lds > 48 * 1024) {                           // (fp32 scores from T = 10909 on; 16-bit rows never get there)
    static DevOnce once;
    if (once.first()) SEA_MAX_LDS((kd_loss_fwd_kernel<TE, TX>), kd_lds_bytes(KD_MAX_T, sizeof(TX)));
  }
  const int64_t blocks = (int64_t)p.N * p.H * ((p.T + 1) / 2);
  hipLaunchKernelGGL((kd_loss_fwd_kernel<TE, TX>), dim3((unsigned)blocks), dim3(64), lds, s, p);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}
template <typename TE> static int kd_launch_fwd_x(const char* nm, int truth_dtype, const KdParams& p, hipStream_t s) {
  if (truth_dtype == SEA_F32) return kd_launch_fwd<TE, float>(nm, p, s);
  if (truth_dtype == SEA_F16) return kd_launch_fwd<TE, __half>(nm, p, s);
  return kd_launch_fwd<TE, __hip_bfloat16>(nm, p, s);
}

template <typename TE>
static int kd_launch_bwd(const char* nm, const void* est, const int64_t* es, const float* pix_tgt, const float* row_stats,
                         const float* grad_loss, int64_t N, int64_t H, int64_t T, int64_t T_m, void* d_est, hipStream_t s) {
  const int64_t R = N * H * T;
  const float k_kl = (float)(0.1 / (double)R), k_mse = (float)(2.0 / ((double)R * (double)T));
  hipLaunchKernelGGL((kd_loss_bwd_kernel<TE>), dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const TE*>(est),
                     es[0], es[1], es[2], pix_tgt, row_stats, grad_loss, (int)H, (int)T, (int)T_m, R, k_kl, k_mse,
                     reinterpret_cast<TE*>(d_est));
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}

}  // namespace sea

using namespace sea;

extern "C" int sea_train_version(void) { return SEA_TRAIN_ABI_VERSION; }

extern "C" int sea_kd_estimator_loss(const void* est, int est_dtype, const int64_t* est_strides, const void* truth, int truth_dtype,
                                     const int64_t* truth_strides, const void* teacher_q, const void* teacher_k, int teacher_dtype,
                                     const int64_t* teacher_q_strides, const int64_t* teacher_k_strides, int64_t N, int64_t H,
                                     int64_t T, int64_t T_m, int64_t D, float* row_kl, float* row_mse, float* pix_tgt,
                                     float* row_stats, sea_stream_t stream) {
  const char* nm = "sea_kd_estimator_loss";
  const bool factored = !truth;                    // then the tile kernel runs, and D is the teacher's head size
  int rc = kd_check_est(nm, est, est_dtype, est_strides, N, H, T, T_m, factored ? KS_TILE : 2);
  if (rc == SEA_OK && factored) rc = kd_check_head(nm, D);
  if (rc == SEA_OK)
    rc = kd_check_teacher(nm, truth, truth_dtype, truth_strides, teacher_q, teacher_k, teacher_dtype, teacher_q_strides,
                          teacher_k_strides, -1, T, D);
  if (rc == SEA_OK)
    rc = kd_check_nulls(nm, {KdArg{"row_kl", row_kl}, {"row_mse", row_mse}, {"pix_tgt", pix_tgt}, {"row_stats", row_stats}});
  if (rc != SEA_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (factored) {
    SEA_REQUIRE(((uintptr_t)row_stats & 7) == 0, SEA_EINVAL, "%s: row_stats must be 8-byte aligned", nm);
    return kdq_launch_fwd(nm, est, est_dtype, est_strides, teacher_q, teacher_k, teacher_dtype, teacher_q_strides,
                          teacher_k_strides, N, H, T, T_m, D, row_kl, row_mse, pix_tgt, row_stats, s);
  }
  KdParams p;
  p.est = est;
  p.truth = truth;
  p.esn = est_strides[0]; p.esh = est_strides[1]; p.est_t = est_strides[2];
  p.xsn = truth_strides[0]; p.xsh = truth_strides[1]; p.xst = truth_strides[2];
  p.N = (int)N; p.H = (int)H; p.T = (int)T; p.T_M = (int)T_m;
  p.row_kl = row_kl; p.row_mse = row_mse; p.pix_tgt = pix_tgt; p.row_stats = row_stats;
  if (est_dtype == SEA_F32) return kd_launch_fwd_x<float>(nm, truth_dtype, p, s);
  if (est_dtype == SEA_F16) return kd_launch_fwd_x<__half>(nm, truth_dtype, p, s);
  return kd_launch_fwd_x<__hip_bfloat16>(nm, truth_dtype, p, s);
}

extern "C" int sea_kd_estimator_loss_bwd(const void* est, int est_dtype, const int64_t* est_strides, const float* pix_tgt,
                                         const float* row_stats, const float* grad_loss, int64_t N, int64_t H, int64_t T,
                                         int64_t T_m, void* d_est, sea_stream_t stream) {
  const char* nm = "sea_kd_estimator_loss_bwd";
  int rc = kd_check_est(nm, est, est_dtype, est_strides, N, H, T, T_m, 2);
  if (rc == SEA_OK)
    rc = kd_check_nulls(nm, {KdArg{"pix_tgt", pix_tgt}, {"row_stats", row_stats}, {"grad_loss", grad_loss}, {"d_est", d_est}});
  if (rc != SEA_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (est_dtype == SEA_F32) return kd_launch_bwd<float>(nm, est, est_strides, pix_tgt, row_stats, grad_loss, N, H, T, T_m, d_est, s);
  if (est_dtype == SEA_F16) return kd_launch_bwd<__half>(nm, est, est_strides, pix_tgt, row_stats, grad_loss, N, H, T, T_m, d_est, s);
  return kd_launch_bwd<__hip_bfloat16>(nm, est, est_strides, pix_tgt, row_stats, grad_loss, N, H, T, T_m, d_est, s);
}
