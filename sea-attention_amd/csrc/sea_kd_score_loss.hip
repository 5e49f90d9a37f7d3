// Distillation loss of the student's own scores (include/sea_hip_train.h, t3 / t4): 0.1 KL + MSE between the softmax of q k^T
// over the causal keys of each row and the softmax of the teacher's scores, without a T x T tensor.  gfx950 only.
//
// Replaces, for the student-score term of PerlinAttention (`_forward_dense`, `_dense_attention_by_head_chunks`):
//   torch.matmul(q_for_score, k_for_score^T)     the (N,H,T,T) scores, rounded to 16 bits
//   attention.py  _kl_and_mse                    two masked fills, log_softmax, two softmaxes, kl_div, mse_loss (fp32 copies)
//
// One tile body serves the three kernels.  A wave OWNS 16 indices (queries in the forward and in the backward's row pass, keys
// in its column pass) and SWEEPS the other side in tiles of 64 staged in LDS for the four waves of the workgroup.  The score
// tile is  (swept x own) = swept_tile . own^T  on v_mfma_f32_16x16x32: the accumulator has the own index on the lane (lane & 15)
// and the swept index in the registers.  Which swept index a row of the A operand stands for is free, so row i of sub-tile c is
// swept index 16 (i >> 2) + 4 c + (i & 3): lane l then holds the SIXTEEN CONSECUTIVE swept indices 16 (l >> 4) .. + 15 of its own
// index.  In the forward and the row pass those are consecutive keys of one query: the teacher's scores come straight from
// global memory in 16-byte chunks, already in the accumulator's lane map, and never pass through LDS.  The same sixteen values
// are, eight at a time, the B operand of the gradient's MFMA (k = 8 (l >> 4) + j stands for swept index 16 (l >> 4) + 8 u + j in
// k-step u; the A operand is read from a transposed LDS image with the same numbering), so dS never leaves registers either.
//
// The teacher may come factored (truth == NULL: `KsQK` in place of the type of the score tensor): its q and k of the student's
// type and head size.  Then the teacher's tile is staged in a second row image beside the student's, the teacher's own
// fragments are loaded like the student's, and x is a second score tile in the same lane map -- same indexing, same
// instructions, so a teacher that holds the student's bits gives the student's scores bit for bit.  Nothing T x T is read.
// The estimator's term with the factored teacher (t1, `kdq_fwd_kernel` below) runs on the same tile body with the teacher's tile
// alone.
#include <type_traits>

#include "sea_common.hpp"
#include "sea_kd.hpp"                 // kd_pix, kd_first, KS_TILE, the host checks
#include "../../include/sea_hip_train.h"

namespace sea {

constexpr int KS_THREADS = 256;

typedef __attribute__((ext_vector_type(8))) __bf16 ks_bf8;
typedef __attribute__((ext_vector_type(8))) _Float16 ks_h8;
typedef __attribute__((ext_vector_type(4))) float ks_f4;

template <typename T> struct KsX;
template <> struct KsX<__hip_bfloat16> {
  static constexpr float DS_SCALE = 1.0f;
  __device__ static inline ks_f4 mfma(const uint4& a, const uint4& b, ks_f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ks_bf8, a), __builtin_bit_cast(ks_bf8, b), c, 0, 0, 0);
  }
};
template <> struct KsX<__half> {
  // dS is at most 0.1 + 4 / T in magnitude and falls with the row length; times 2^12 its hi + lo halves stay clear of fp16's
  // subnormals (a power of two: taken out again exactly with the upstream gradient)
  static constexpr float DS_SCALE = 4096.0f;
  __device__ static inline ks_f4 mfma(const uint4& a, const uint4& b, ks_f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(ks_h8, a), __builtin_bit_cast(ks_h8, b), c, 0, 0, 0);
  }
};

template <int D> struct KsGeo {
  static constexpr int KK = (D + 31) / 32;         // k-steps of the score MFMA; at D = 80 half of the third is zero fragments
  static constexpr int DT = D / 16;                // 16-wide column tiles of dQ / dK
  static constexpr int CH = D / 8;                 // 16-byte chunks per row
  static constexpr int RST = D + 8;                // row image: elements per row (16 bytes of padding)
  static constexpr int TST = KS_TILE + 8;          // transposed image: elements per column of the tile
};

__device__ inline float ks_xor16_max(float v) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ inline float ks_xor32_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
// over the four lanes l & 15 + {0, 16, 32, 48} that share an own index; every one of them ends with the same bits
__device__ inline float ks_own_max(float v) { return ks_xor32_max(ks_xor16_max(v)); }
__device__ inline float ks_own_sum(float v) { return xor32_sum(xor16_sum(v)); }

// in place of the score tensor's element type: the teacher is q_t, k_t (KsParams::tq, tk), of the student's type T
struct KsQK {};
template <typename TX> constexpr bool ks_is_qk = std::is_same<TX, KsQK>::value;

// a * b rounded to fp32, never fused into a following addition (the build contracts by default and honours this pragma)
__device__ inline float ks_mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

struct KsParams {
  const void* q;
  const void* k;
  const void* truth;
  int64_t qsn, qsh, qst, ksn, ksh, kst, xsn, xsh, xst;
  int N, H, T;
  float* row_kl;
  float* row_mse;
  float* row_q;
  float* row_stats;
  const float* grad_loss;
  void* d_q;
  void* d_k;
  const void* tq;                                  // the factored teacher (KsQK): truth is null.  (Last: the fields above keep
  const void* tk;                                  // their places in the kernel arguments)
  int64_t tqsn, tqsh, tqst, tksn, tksh, tkst;
};

// Rows i0 .. i0 + 63 of `src` (stride `st` elements) into LDS: the row image and, for the gradient's A operand, the transposed
// one.  Rows at or past T are zero and are not loaded.  Consecutive lanes take consecutive rows.
template <typename T, int D, bool TR>
__device__ inline void ks_stage(const T* src, int64_t st, int i0, int Tn, unsigned short* s_row, unsigned short* s_tr) {
  using G = KsGeo<D>;
#pragma unroll
  for (int ch = threadIdx.x; ch < KS_TILE * G::CH; ch += KS_THREADS) {
    const int row = ch & (KS_TILE - 1), cc = ch >> 6;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i0 + row < Tn) v = *reinterpret_cast<const uint4*>(src + (int64_t)(i0 + row) * st + cc * 8);
    *reinterpret_cast<uint4*>(s_row + row * G::RST + cc * 8) = v;
    if constexpr (TR) {
      const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) s_tr[(cc * 8 + j) * G::TST + row] = (unsigned short)(d[j >> 1] >> (16 * (j & 1)));
    }
  }
}

// the lane's own fragments (B operand of the score MFMA): row `idx` of `src`, columns 32 kk + 8 (l >> 4) .. + 7; zero past D
// (the padded k-step at 80) and for an index at or past T -- neither is read
template <typename T, int D>
__device__ inline void ks_own_frags(const T* src, int64_t st, int idx, int Tn, int lane, uint4 (&own)[KsGeo<D>::KK]) {
#pragma unroll
  for (int kk = 0; kk < KsGeo<D>::KK; ++kk) {
    const int col = kk * 32 + 8 * (lane >> 4);
    own[kk] = make_uint4(0u, 0u, 0u, 0u);
    if (idx < Tn && col < D) own[kk] = *reinterpret_cast<const uint4*>(src + (int64_t)idx * st + col);
  }
}

// score tile: s[e], e = 0 .. 15, is  swept(16 (l >> 4) + e) . own(l & 15)
template <typename T, int D>
__device__ inline void ks_scores(const unsigned short* s_row, const uint4 (&own)[KsGeo<D>::KK], int lane, float (&s)[16]) {
  using G = KsGeo<D>;
  const int li = lane & 15, g = lane >> 4;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int row = 16 * (li >> 2) + 4 * c + (li & 3);
    ks_f4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < G::KK; ++kk) {
      const int col = kk * 32 + 8 * g;
      uint4 f = make_uint4(0u, 0u, 0u, 0u);
      if (D % 32 == 0 || col < D) f = *reinterpret_cast<const uint4*>(s_row + row * G::RST + col);
      a = KsX<T>::mfma(f, own[kk], a);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) s[4 * c + r] = a[r];
  }
}

// The teacher's scores of query t (row pointer `xrow`), keys s0 .. s0 + 15, as fp32.  Only chunks with a key <= t are touched;
// a chunk is loaded whole only where it lies inside the row's T elements (what it holds past t is dropped by the caller's
// mask), the rest goes element by element up to t.  t < 0: nothing is read.
template <typename TX>
__device__ inline void ks_truth_keys(const TX* xrow, int t, int Tn, int s0, float (&x)[16]) {
  constexpr int VEC = Elem<TX>::VEC;
#pragma unroll
  for (int c = 0; c < 16 / VEC; ++c) {
    const int s = s0 + c * VEC;
    float f[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) f[j] = 0.f;
    if (s <= t) {
      if (s + VEC <= Tn) {
        const uint4 raw = *reinterpret_cast<const uint4*>(xrow + s);
        unpack16<TX>(raw, f);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          if (s + j <= t) f[j] = Elem<TX>::to_f(xrow[s + j]);
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) x[c * VEC + j] = f[j];
  }
}

// The per-tile prologue of a sweep that stages one swept tile and reads nothing else: barrier, tile `i0 / 64` of `src` into
// `s_row`, barrier, the score tile.  (The score kernels keep their own lines: they stage a second tile or a transposed image,
// and issue the loads of truth between staging and the second barrier, so that they are in flight during it.)
template <typename T, int D>
__device__ inline void ks_sweep_tile(const T* src, int64_t st, int i0, int Tn, unsigned short* s_row,
                                     const uint4 (&own)[KsGeo<D>::KK], int lane, float (&s)[16]) {
  __syncthreads();
  ks_stage<T, D, false>(src, st, i0, Tn, s_row, nullptr);
  __syncthreads();
  ks_scores<T, D>(s_row, own, lane, s);
}

// The finish of sweep 1 across the four lanes of an own index: from a lane's running maximum m and its sum l of exp(score - m)
// over its keys, and the row's maximum M = ks_own_max(m), the row's sum of exp(score - M).  A lane that met no key <= t adds 0.
// (The update inside the sweep stays written out where it is: folded into a helper it moved the forward's register allocation.)
__device__ inline float ks_online_sum(float m, float l, float M) { return ks_own_sum(m > -INFINITY ? l * expf(m - M) : 0.f); }

// block -> (index of the 64-block of own indices, (n, h)).  All (n, h) of one block index are neighbours in the grid, and the
// grid starts with the longest sweeps (the causal triangle: block b of the queries sweeps b + 1 key tiles, block b of the keys
// sweeps NB - b query tiles), so the launch ends on the short ones.
template <bool COL, typename P> __device__ inline void ks_block(const P& p, int& ob, int& n, int& h) {
  const int NH = p.N * p.H, NB = (p.T + KS_TILE - 1) / KS_TILE;
  const int i = blockIdx.x / NH, nh = blockIdx.x - i * NH;
  ob = COL ? i : NB - 1 - i;
  n = nh / p.H;
  h = nh - n * p.H;
}

// ---- forward -----------------------------------------------------------------------------------------------------------------
template <typename T, typename TX, int D>
__global__ __launch_bounds__(KS_THREADS) void ks_fwd_kernel(KsParams p) {
  using G = KsGeo<D>;
  constexpr bool QK = ks_is_qk<TX>;
  __shared__ __align__(16) unsigned short s_row[KS_TILE * G::RST];
  __shared__ __align__(16) unsigned short s_xrow[QK ? KS_TILE * G::RST : 8];   // the teacher's k tile (KsQK only)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
  int rb, n, h;
  ks_block<false>(p, rb, n, h);
  const T* q = reinterpret_cast<const T*>(p.q) + n * p.qsn + h * p.qsh;
  const T* k = reinterpret_cast<const T*>(p.k) + n * p.ksn + h * p.ksh;
  const int t = rb * KS_TILE + 16 * w + li;
  const bool own_ok = t < p.T;
  const int tv = own_ok ? t : -1;                  // no key is <= -1: a query past T reads and adds nothing
  const TX* xrow = nullptr;
  const T* tk = nullptr;
  uint4 own[G::KK], xown[G::KK];
  ks_own_frags<T, D>(q, p.qst, t, p.T, lane, own);
  if constexpr (QK) {
    tk = reinterpret_cast<const T*>(p.tk) + n * p.tksn + h * p.tksh;
    ks_own_frags<T, D>(reinterpret_cast<const T*>(p.tq) + n * p.tqsn + h * p.tqsh, p.tqst, t, p.T, lane, xown);
  } else {
    xrow = reinterpret_cast<const TX*>(p.truth) + n * p.xsn + h * p.xsh + (int64_t)(own_ok ? t : 0) * p.xst;
  }

  // sweep 1: running maximum and sum of both softmaxes, per lane over its keys
  float ms = -INFINITY, ls = 0.f, mx = -INFINITY, lx = 0.f;
  for (int tile = 0; tile <= rb; ++tile) {
    const int s0 = tile * KS_TILE + 16 * g;
    __syncthreads();
    ks_stage<T, D, false>(k, p.kst, tile * KS_TILE, p.T, s_row, nullptr);
    if constexpr (QK) ks_stage<T, D, false>(tk, p.tkst, tile * KS_TILE, p.T, s_xrow, nullptr);
    float xv[16], sv[16];
    if constexpr (!QK) ks_truth_keys<TX>(xrow, tv, p.T, s0, xv);
    __syncthreads();
    ks_scores<T, D>(s_row, own, lane, sv);
    if constexpr (QK) ks_scores<T, D>(s_xrow, xown, lane, xv);
    float ts = -INFINITY, tx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const bool ok = s0 + e <= tv;
      sv[e] = ok ? sv[e] : -INFINITY;
      xv[e] = ok ? xv[e] : -INFINITY;
      ts = fmaxf(ts, sv[e]);
      tx = fmaxf(tx, xv[e]);
    }
    const float ns = fmaxf(ms, ts), nx = fmaxf(mx, tx);
    if (ns > -INFINITY) {                          // (the lane has met a key <= t: both maxima are finite from here on)
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        a += expf(sv[e] - ns);
        b += expf(xv[e] - nx);
      }
      ls = ls * expf(ms - ns) + a;
      lx = lx * expf(mx - nx) + b;
      ms = ns;
      mx = nx;
    }
  }
  const float M = ks_own_max(ms), MX = ks_own_max(mx);
  const float L = ks_online_sum(ms, ls, M), LX = ks_online_sum(mx, lx, MX);
  const float inv_l = 1.0f / L, log_l = logf(L), inv_lx = 1.0f / LX, log_lx = logf(LX);

  // sweep 2: the scores again, both probabilities, the three row sums key by key
  float kl = 0.f, mse = 0.f, rq = 0.f;
  for (int tile = 0; tile <= rb; ++tile) {
    const int s0 = tile * KS_TILE + 16 * g;
    __syncthreads();
    ks_stage<T, D, false>(k, p.kst, tile * KS_TILE, p.T, s_row, nullptr);
    if constexpr (QK) ks_stage<T, D, false>(tk, p.tkst, tile * KS_TILE, p.T, s_xrow, nullptr);
    float xv[16], sv[16];
    if constexpr (!QK) ks_truth_keys<TX>(xrow, tv, p.T, s0, xv);
    __syncthreads();
    ks_scores<T, D>(s_row, own, lane, sv);
    if constexpr (QK) ks_scores<T, D>(s_xrow, xown, lane, xv);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (s0 + e <= tv) {
        const float ds = sv[e] - M, dx = xv[e] - MX;
        float pe = expf(ds) * inv_l, tg = expf(dx) * inv_lx;
        if constexpr (QK) {
          // both products rounded on their own: left to contraction, pe - tg becomes fma(a, b, -(c d)), which is the rounding
          // error of c d and not 0 for a teacher row that equals the student's bit for bit
          pe = ks_mul_rn(expf(ds), inv_l);
          tg = ks_mul_rn(expf(dx), inv_lx);
        }
        kl += tg > 0.f ? tg * ((dx - log_lx) - (ds - log_l)) : 0.f;
        const float df = pe - tg;
        mse += df * df;
        rq += pe * df;
      }
    }
  }
  kl = ks_own_sum(kl);
  mse = ks_own_sum(mse);
  rq = ks_own_sum(rq);
  if (own_ok && g == 0) {
    const int64_t r = ((int64_t)n * p.H + h) * p.T + t;
    p.row_kl[r] = kl;
    p.row_mse[r] = mse;
    p.row_q[r] = rq;
    *reinterpret_cast<float4*>(p.row_stats + 4 * r) = make_float4(M, log_l, MX, log_lx);
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------
// COL = false, the row pass: own = queries, sweeps the key tiles 0 .. rb, dQ^T += K^T . dS^T.
// COL = true, the column pass: own = keys, sweeps the query tiles kb .. NB - 1, dK^T += Q^T . dS.
// Both: the score tile again, p and tgt from row_stats, dS (without g / R, times DS_SCALE) as hi + lo 16-bit halves.
template <typename T, typename TX, int D, bool COL>
__global__ __launch_bounds__(KS_THREADS) void ks_bwd_kernel(KsParams p) {
  using G = KsGeo<D>;
  using X = KsX<T>;
  __shared__ __align__(16) unsigned short s_row[KS_TILE * G::RST];
  constexpr bool QK = ks_is_qk<TX>;
  __shared__ __align__(16) unsigned short s_tr[D * G::TST];
  __shared__ __align__(16) unsigned short s_xrow[QK ? KS_TILE * G::RST : 8];   // the teacher's swept tile (KsQK only): no transposed image
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
  int ob, n, h;
  ks_block<COL>(p, ob, n, h);
  const int NB = (p.T + KS_TILE - 1) / KS_TILE;
  const T* q = reinterpret_cast<const T*>(p.q) + n * p.qsn + h * p.qsh;
  const T* k = reinterpret_cast<const T*>(p.k) + n * p.ksn + h * p.ksh;
  const TX* x = nullptr;
  const T* tq = nullptr;
  const T* tk = nullptr;
  if constexpr (QK) {
    tq = reinterpret_cast<const T*>(p.tq) + n * p.tqsn + h * p.tqsh;
    tk = reinterpret_cast<const T*>(p.tk) + n * p.tksn + h * p.tksh;
  } else {
    x = reinterpret_cast<const TX*>(p.truth) + n * p.xsn + h * p.xsh;
  }
  const int64_t r0 = ((int64_t)n * p.H + h) * p.T;
  const int o = ob * KS_TILE + 16 * w + li;        // the lane's own index
  const bool own_ok = o < p.T;
  uint4 own[G::KK], xown[G::KK];
  ks_own_frags<T, D>(COL ? k : q, COL ? p.kst : p.qst, o, p.T, lane, own);
  if constexpr (QK) ks_own_frags<T, D>(COL ? tk : tq, COL ? p.tkst : p.tqst, o, p.T, lane, xown);
  const float k_kl = 0.1f * X::DS_SCALE, k_mse = 2.0f / (float)p.T * X::DS_SCALE;

  float4 st_own = make_float4(0.f, 0.f, 0.f, 0.f);
  float rq_own = 0.f;
  if (!COL && own_ok) {
    st_own = *reinterpret_cast<const float4*>(p.row_stats + 4 * (r0 + o));
    rq_own = p.row_q[r0 + o];
  }
  const TX* xrow = nullptr;                                   // row pass, score tensor only
  if constexpr (!QK) xrow = x + (int64_t)(own_ok ? o : 0) * p.xst;

  ks_f4 out[G::DT];
#pragma unroll
  for (int dt = 0; dt < G::DT; ++dt) out[dt] = ks_f4{0.f, 0.f, 0.f, 0.f};

  const int tile_lo = COL ? ob : 0, tile_hi = COL ? NB - 1 : ob;
  for (int tile = tile_lo; tile <= tile_hi; ++tile) {
    const int i0 = tile * KS_TILE + 16 * g;        // the lane's first swept index
    __syncthreads();
    ks_stage<T, D, true>(COL ? q : k, COL ? p.qst : p.kst, tile * KS_TILE, p.T, s_row, s_tr);
    if constexpr (QK) ks_stage<T, D, false>(COL ? tq : tk, COL ? p.tqst : p.tkst, tile * KS_TILE, p.T, s_xrow, nullptr);
    float xv[16], sv[16], u[16];
    bool ok[16];
    if constexpr (!COL) {
      if constexpr (!QK) ks_truth_keys<TX>(xrow, own_ok ? o : -1, p.T, i0, xv);
#pragma unroll
      for (int e = 0; e < 16; ++e) ok[e] = own_ok && i0 + e <= o;
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int t = i0 + e;
        ok[e] = t < p.T && o <= t;                 // (o <= t < T: the key is inside too)
        if constexpr (!QK) xv[e] = ok[e] ? Elem<TX>::to_f(x[(int64_t)t * p.xst + o]) : 0.f;
      }
    }
    __syncthreads();
    ks_scores<T, D>(s_row, own, lane, sv);
    if constexpr (QK) ks_scores<T, D>(s_xrow, xown, lane, xv);   // either pass: (swept x own) of the teacher, the student's lane map
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float4 st = st_own;
      float rq = rq_own;
      if constexpr (COL) {
        if (ok[e]) {
          st = *reinterpret_cast<const float4*>(p.row_stats + 4 * (r0 + i0 + e));
          rq = p.row_q[r0 + i0 + e];
        }
      }
      float v = 0.f;
      if (ok[e]) {
        const float pe = expf((sv[e] - st.x) - st.y), tg = expf((xv[e] - st.z) - st.w);
        const float df = pe - tg;
        v = k_kl * df + k_mse * (pe * df - pe * rq);
      }
      u[e] = v;
    }
    // dS as the B operand: element j of k-step uu is swept index 16 g + 8 uu + j, the numbering of the transposed image
    uint4 bh[2], bl[2];
#pragma unroll
    for (int uu = 0; uu < 2; ++uu) {
      uint32_t hi[4], lo[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float a = u[8 * uu + 2 * j], b = u[8 * uu + 2 * j + 1];
        const T ah = from_f<T>(a), bhh = from_f<T>(b);
        hi[j] = (uint32_t)__builtin_bit_cast(unsigned short, ah) | ((uint32_t)__builtin_bit_cast(unsigned short, bhh) << 16);
        lo[j] = pack2<T>(a - Elem<T>::to_f(ah), b - Elem<T>::to_f(bhh));
      }
      bh[uu] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
      bl[uu] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    }
#pragma unroll
    for (int dt = 0; dt < G::DT; ++dt) {
#pragma unroll
      for (int uu = 0; uu < 2; ++uu) {
        const uint4 a = *reinterpret_cast<const uint4*>(s_tr + (16 * dt + li) * G::TST + 16 * g + 8 * uu);
        out[dt] = X::mfma(a, bh[uu], out[dt]);
        out[dt] = X::mfma(a, bl[uu], out[dt]);
      }
    }
  }
  // out[dt][r] = d(own = l & 15, column 16 dt + 4 (l >> 4) + r): four 16-bit values, one 8-byte store
  if (own_ok) {
    const int64_t R = (int64_t)p.N * p.H * p.T;
    const float scale = *p.grad_loss * (float)(1.0 / ((double)R * (double)X::DS_SCALE));
    T* dst = reinterpret_cast<T*>(COL ? p.d_k : p.d_q) + (r0 + o) * D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < G::DT; ++dt) {
      const uint2 pk = make_uint2(pack2<T>(out[dt][0] * scale, out[dt][1] * scale), pack2<T>(out[dt][2] * scale, out[dt][3] * scale));
      *reinterpret_cast<uint2*>(dst + 16 * dt) = pk;
    }
  }
}

// ---- the estimator's term on the tile body (t1 with the factored teacher) ---------------------------------------------------
// Same outputs as sea_kd_loss.hip's forward (t1: row_kl, row_mse, pix_tgt, row_stats = {m_e, log S}; t2 then runs unchanged), the
// teacher's scores recomputed from q_t, k_t instead of read.  A workgroup owns 64 queries and sweeps the key tiles 0 .. rb twice.
//   before the sweeps  every wave takes its 16 queries one at a time, 64 lanes over the T_M pixels: c_b from kd_first, m_e and S
//                      in kd_row's own order (so row_stats carries t1's bits), left on the lanes of the query
//   sweep 1            the teacher's row maximum and log sum exp, as the score forward takes them
//   sweep 2            x again, tgt_s, pix(t, s) by kd_pix itself (the fp32 IEEE formula, evaluated per key), row_kl and row_mse
//                      key by key, and G_b
// G_b without a table and without atomics: a pixel's keys are contiguous, so a lane's 16 keys fall into segments of equal
// pixel.  A segment with a neighbour on both sides inside the lane is a whole pixel and is stored as it is.  The lane's first
// and last segment may go on in the neighbouring lane or tile: they are handed down the four lanes of the query in key order
// (shuffles; all four lanes do the same arithmetic on the same values) into a carry (pixel, sum) that every lane keeps and
// that crosses to the next tile in registers; the carry is stored when the pixel changes and after the last tile.  Every held
// pixel is stored exactly once, in one summation order (the keys of a lane ascending, then the lanes and tiles ascending); the
// host zeroes pix_tgt on the stream first, which is what leaves the empty pixels exactly 0.
struct KdqParams {
  const void* est;
  const void* tq;
  const void* tk;
  int64_t esn, esh, est_t, tqsn, tqsh, tqst, tksn, tksh, tkst;
  int N, H, T, T_M;
  float* row_kl;
  float* row_mse;
  float* pix_tgt;
  float* row_stats;
};

template <typename TE, typename T, int D>
__global__ __launch_bounds__(KS_THREADS) void kdq_fwd_kernel(KdqParams p) {
  using G = KsGeo<D>;
  __shared__ __align__(16) unsigned short s_row[KS_TILE * G::RST];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
  int rb, n, h;
  ks_block<false>(p, rb, n, h);
  const T* tq = reinterpret_cast<const T*>(p.tq) + n * p.tqsn + h * p.tqsh;
  const T* tk = reinterpret_cast<const T*>(p.tk) + n * p.tksn + h * p.tksh;
  const TE* est = reinterpret_cast<const TE*>(p.est) + n * p.esn + h * p.esh;
  const int T_M = p.T_M;
  const float tm = (float)T_M;
  const int t = rb * KS_TILE + 16 * w + li;
  const bool own_ok = t < p.T;
  const int tv = own_ok ? t : -1;                  // no key is <= -1: a query past T reads and adds nothing
  const int64_t r = ((int64_t)n * p.H + h) * p.T + (own_ok ? t : 0);
  uint4 own[G::KK];
  ks_own_frags<T, D>(tq, p.tqst, t, p.T, lane, own);

  // the estimator's softmax over the keys, from the pixels (at most 8 per lane): kd_row's order, one query at a time
  float me_own = 0.f, inv_s_own = 0.f, log_s_own = 0.f;
  for (int qi = 0; qi < 16; ++qi) {
    const int tt = rb * KS_TILE + 16 * w + qi;
    if (tt >= p.T) break;                          // (the same for the whole wave)
    const float len = (float)(tt + 1);
    const TE* e = est + (int64_t)tt * p.est_t;
    float ev[8], cn[8];
    float me = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int b = j * 64 + lane;
      ev[j] = cn[j] = 0.f;
      if (b < T_M) {
        const int c = kd_first(b + 1, tt, len, tm, T_M) - kd_first(b, tt, len, tm, T_M);
        if (c > 0) {
          cn[j] = (float)c;
          ev[j] = Elem<TE>::to_f(e[b]);
          me = fmaxf(me, ev[j]);
        }
      }
    }
    me = wave_max(me);
    float S = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (cn[j] > 0.f) S += cn[j] * expf(ev[j] - me);
    S = wave_sum(S);
    if (li == qi) {
      me_own = me;
      inv_s_own = 1.0f / S;
      log_s_own = logf(S);
    }
  }

  // sweep 1: running maximum and sum of the teacher's softmax, per lane over its keys
  float mx = -INFINITY, lx = 0.f;
  for (int tile = 0; tile <= rb; ++tile) {
    const int s0 = tile * KS_TILE + 16 * g;
    float xv[16];
    ks_sweep_tile<T, D>(tk, p.tkst, tile * KS_TILE, p.T, s_row, own, lane, xv);
    float tx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      xv[e] = s0 + e <= tv ? xv[e] : -INFINITY;
      tx = fmaxf(tx, xv[e]);
    }
    const float nx = fmaxf(mx, tx);
    if (nx > -INFINITY) {
      float b = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) b += expf(xv[e] - nx);
      lx = lx * expf(mx - nx) + b;
      mx = nx;
    }
  }
  const float MX = ks_own_max(mx);
  const float LX = ks_online_sum(mx, lx, MX);
  const float inv_lx = 1.0f / LX, log_lx = logf(LX);

  // sweep 2
  const float len = (float)(t + 1);
  const TE* erow = est + (int64_t)(own_ok ? t : 0) * p.est_t;
  float* g_out = p.pix_tgt + r * T_M;
  float kl = 0.f, mse = 0.f;
  int cb = -1;                                     // the carry: pixel and the sum of its keys so far (the same on the four lanes)
  float cv = 0.f;
  for (int tile = 0; tile <= rb; ++tile) {
    const int s0 = tile * KS_TILE + 16 * g;
    float xv[16], ee[16];
    int px[16];
    ks_sweep_tile<T, D>(tk, p.tkst, tile * KS_TILE, p.T, s_row, own, lane, xv);
    // the pixels of the lane's keys (< T_M for a key <= t; held below it for the addresses' sake) and, where the pixel changes,
    // its estimator score: all loads issued before the first is used
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int b = kd_pix(s0 + e, len, tm, T_M);
      px[e] = b < T_M ? b : T_M - 1;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const bool fresh = s0 + e <= tv && (e == 0 || px[e] != px[e - 1]);
      ee[e] = fresh ? Elem<TE>::to_f(erow[px[e]]) : 0.f;
    }
    int fb = -1, lb = -1, sb = -1;                 // pixel of the lane's first, last and current segment
    float fv = 0.f, lv = 0.f, sv = 0.f, pb = 0.f, lp = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (s0 + e <= tv) {
        if (px[e] != sb) {
          if (sb >= 0) {
            if (fb < 0) {
              fb = sb;
              fv = sv;
            } else {
              g_out[sb] = sv;                      // a whole pixel
            }
          }
          sb = px[e];
          sv = 0.f;
          const float de = ee[e] - me_own;
          pb = expf(de) * inv_s_own;
          lp = de - log_s_own;
        }
        const float dx = xv[e] - MX;
        const float tg = expf(dx) * inv_lx;
        sv += tg;
        kl += tg > 0.f ? tg * ((dx - log_lx) - lp) : 0.f;
        const float df = pb - tg;
        mse += df * df;
      }
    }
    if (sb >= 0) {
      if (fb < 0) {
        fb = sb;
        fv = sv;
      } else {
        lb = sb;
        lv = sv;
      }
    }
    // down the four lanes of the query, in key order
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int src = li + 16 * rr;
      const int ofb = __shfl(fb, src), olb = __shfl(lb, src);
      const float ofv = __shfl(fv, src), olv = __shfl(lv, src);
      if (ofb >= 0) {
        if (ofb == cb) {
          cv += ofv;
        } else {
          if (cb >= 0 && g == 0) g_out[cb] = cv;
          cb = ofb;
          cv = ofv;
        }
        if (olb >= 0) {
          if (g == 0) g_out[cb] = cv;
          cb = olb;
          cv = olv;
        }
      }
    }
  }
  if (cb >= 0 && g == 0) g_out[cb] = cv;
  kl = ks_own_sum(kl);
  mse = ks_own_sum(mse);
  if (own_ok && g == 0) {
    p.row_kl[r] = kl;
    p.row_mse[r] = mse;
    *reinterpret_cast<float2*>(p.row_stats + 2 * r) = make_float2(me_own, log_s_own);
  }
}


// ---- host ---------------------------------------------------------------------------------------------------------------------
template <typename T, typename TX, int D> static int ks_launch(const char* nm, bool bwd, const KsParams& p, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)p.N * p.H * ((p.T + KS_TILE - 1) / KS_TILE)));
  if (!bwd) {
    hipLaunchKernelGGL((ks_fwd_kernel<T, TX, D>), grid, dim3(KS_THREADS), 0, s, p);
    SEA_CHECK_LAUNCH(nm);
  } else {
    hipLaunchKernelGGL((ks_bwd_kernel<T, TX, D, false>), grid, dim3(KS_THREADS), 0, s, p);
    SEA_CHECK_LAUNCH(nm);
    hipLaunchKernelGGL((ks_bwd_kernel<T, TX, D, true>), grid, dim3(KS_THREADS), 0, s, p);
    SEA_CHECK_LAUNCH(nm);
  }
  return SEA_OK;
}
template <typename T, typename TX> static int ks_launch_d(const char* nm, bool bwd, int64_t D, const KsParams& p, hipStream_t s) {
  if (D == 64) return ks_launch<T, TX, 64>(nm, bwd, p, s);
  if (D == 80) return ks_launch<T, TX, 80>(nm, bwd, p, s);
  return ks_launch<T, TX, 128>(nm, bwd, p, s);
}
template <typename T>
static int ks_launch_x(const char* nm, bool bwd, int truth_dtype, int64_t D, const KsParams& p, hipStream_t s) {
  if (truth_dtype == SEA_F32) return ks_launch_d<T, float>(nm, bwd, D, p, s);
  if (truth_dtype == SEA_F16) return ks_launch_d<T, __half>(nm, bwd, D, p, s);
  return ks_launch_d<T, __hip_bfloat16>(nm, bwd, D, p, s);
}
static int ks_dispatch(const char* nm, bool bwd, int qk_dtype, int truth_dtype, int64_t D, const KsParams& p, hipStream_t s) {
  if (p.truth) {
    if (qk_dtype == SEA_F16) return ks_launch_x<__half>(nm, bwd, truth_dtype, D, p, s);
    return ks_launch_x<__hip_bfloat16>(nm, bwd, truth_dtype, D, p, s);
  }
  if (qk_dtype == SEA_F16) return ks_launch_d<__half, KsQK>(nm, bwd, D, p, s);         // the factored teacher: the student's type
  return ks_launch_d<__hip_bfloat16, KsQK>(nm, bwd, D, p, s);
}

// What t3 and t4 share: every check of the inputs and the kernel arguments made of them.  The entry adds its own outputs to `p`
static int ks_inputs(const char* nm, const void* q, const void* k, int qk_dtype, const int64_t* q_strides, const int64_t* k_strides,
                     const void* truth, int truth_dtype, const int64_t* truth_strides, const void* tq, const void* tk,
                     int teacher_dtype, const int64_t* tq_strides, const int64_t* tk_strides, int64_t N, int64_t H, int64_t T,
                     int64_t D, KsParams& p) {
  int rc = kd_check_nulls(nm, {KdArg{"q", q}, {"k", k}, {"q_strides", q_strides}, {"k_strides", k_strides}});
  if (rc == SEA_OK) rc = kd_check_dtype(nm, "qk_dtype", "q / k", qk_dtype, false);
  if (rc == SEA_OK) rc = kd_check_shape(nm, N, H, T, KS_TILE);
  if (rc == SEA_OK) rc = kd_check_head(nm, D);
  if (rc == SEA_OK)
    rc = kd_check_teacher(nm, truth, truth_dtype, truth_strides, tq, tk, teacher_dtype, tq_strides, tk_strides, qk_dtype, T, D);
  if (rc == SEA_OK) rc = kd_check_rows(nm, {KdRows{"q", q, q_strides, D, qk_dtype}, {"k", k, k_strides, D, qk_dtype}});
  if (rc != SEA_OK) return rc;
  p = {};
  p.q = q; p.k = k;
  p.qsn = q_strides[0]; p.qsh = q_strides[1]; p.qst = q_strides[2];
  p.ksn = k_strides[0]; p.ksh = k_strides[1]; p.kst = k_strides[2];
  if (truth) {
    p.truth = truth;
    p.xsn = truth_strides[0]; p.xsh = truth_strides[1]; p.xst = truth_strides[2];
  } else {                                         // (truth stays null: what ks_dispatch picks the KsQK kernels by)
    p.tq = tq; p.tk = tk;
    p.tqsn = tq_strides[0]; p.tqsh = tq_strides[1]; p.tqst = tq_strides[2];
    p.tksn = tk_strides[0]; p.tksh = tk_strides[1]; p.tkst = tk_strides[2];
  }
  p.N = (int)N; p.H = (int)H; p.T = (int)T;
  return SEA_OK;
}

template <typename TE, typename T> static int kdq_launch_d(const char* nm, int64_t D, const KdqParams& p, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)p.N * p.H * ((p.T + KS_TILE - 1) / KS_TILE)));
  if (D == 64) hipLaunchKernelGGL((kdq_fwd_kernel<TE, T, 64>), grid, dim3(KS_THREADS), 0, s, p);
  else if (D == 80) hipLaunchKernelGGL((kdq_fwd_kernel<TE, T, 80>), grid, dim3(KS_THREADS), 0, s, p);
  else hipLaunchKernelGGL((kdq_fwd_kernel<TE, T, 128>), grid, dim3(KS_THREADS), 0, s, p);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}
template <typename TE> static int kdq_launch(const char* nm, int teacher_dtype, int64_t D, const KdqParams& p, hipStream_t s) {
  if (teacher_dtype == SEA_F16) return kdq_launch_d<TE, __half>(nm, D, p, s);
  return kdq_launch_d<TE, __hip_bfloat16>(nm, D, p, s);
}

int kdq_launch_fwd(const char* nm, const void* est, int est_dtype, const int64_t* est_strides, const void* tq, const void* tk,
                   int teacher_dtype, const int64_t* tq_strides, const int64_t* tk_strides, int64_t N, int64_t H, int64_t T,
                   int64_t T_m, int64_t D, float* row_kl, float* row_mse, float* pix_tgt, float* row_stats, hipStream_t s) {
  KdqParams p = {};
  p.est = est; p.tq = tq; p.tk = tk;
  p.esn = est_strides[0]; p.esh = est_strides[1]; p.est_t = est_strides[2];
  p.tqsn = tq_strides[0]; p.tqsh = tq_strides[1]; p.tqst = tq_strides[2];
  p.tksn = tk_strides[0]; p.tksh = tk_strides[1]; p.tkst = tk_strides[2];
  p.N = (int)N; p.H = (int)H; p.T = (int)T; p.T_M = (int)T_m;
  p.row_kl = row_kl; p.row_mse = row_mse; p.pix_tgt = pix_tgt; p.row_stats = row_stats;
  // the empty pixels' zeros: the kernel stores the held pixels only, each exactly once
  const hipError_t e = hipMemsetAsync(pix_tgt, 0, (size_t)(N * H * T * T_m) * sizeof(float), s);
  SEA_REQUIRE(e == hipSuccess, SEA_ELAUNCH, "%s: clearing pix_tgt failed: %s", nm, hipGetErrorString(e));
  if (est_dtype == SEA_F32) return kdq_launch<float>(nm, teacher_dtype, D, p, s);
  if (est_dtype == SEA_F16) return kdq_launch<__half>(nm, teacher_dtype, D, p, s);
  return kdq_launch<__hip_bfloat16>(nm, teacher_dtype, D, p, s);
}

}  // namespace sea

using namespace sea;

extern "C" int sea_kd_score_loss(const void* q, const void* k, int qk_dtype, const int64_t* q_strides, const int64_t* k_strides,
                                 const void* truth, int truth_dtype, const int64_t* truth_strides, const void* teacher_q,
                                 const void* teacher_k, int teacher_dtype, const int64_t* teacher_q_strides,
                                 const int64_t* teacher_k_strides, int64_t N, int64_t H, int64_t T, int64_t D, float* row_kl,
                                 float* row_mse, float* row_q, float* row_stats, sea_stream_t stream) {
  const char* nm = "sea_kd_score_loss";
  KsParams p;
  int rc = ks_inputs(nm, q, k, qk_dtype, q_strides, k_strides, truth, truth_dtype, truth_strides, teacher_q, teacher_k,
                     teacher_dtype, teacher_q_strides, teacher_k_strides, N, H, T, D, p);
  if (rc == SEA_OK)
    rc = kd_check_nulls(nm, {KdArg{"row_kl", row_kl}, {"row_mse", row_mse}, {"row_q", row_q}, {"row_stats", row_stats}});
  if (rc != SEA_OK) return rc;
  SEA_REQUIRE(((uintptr_t)row_stats & 15) == 0, SEA_EINVAL, "%s: row_stats must be 16-byte aligned", nm);
  p.row_kl = row_kl; p.row_mse = row_mse; p.row_q = row_q; p.row_stats = row_stats;
  return ks_dispatch(nm, false, qk_dtype, truth_dtype, D, p, (hipStream_t)stream);
}

extern "C" int sea_kd_score_loss_bwd(const void* q, const void* k, int qk_dtype, const int64_t* q_strides, const int64_t* k_strides,
                                     const void* truth, int truth_dtype, const int64_t* truth_strides, const void* teacher_q,
                                     const void* teacher_k, int teacher_dtype, const int64_t* teacher_q_strides,
                                     const int64_t* teacher_k_strides, const float* row_q, const float* row_stats,
                                     const float* grad_loss, int64_t N, int64_t H, int64_t T, int64_t D, void* d_q, void* d_k,
                                     sea_stream_t stream) {
  const char* nm = "sea_kd_score_loss_bwd";
  KsParams p;
  int rc = ks_inputs(nm, q, k, qk_dtype, q_strides, k_strides, truth, truth_dtype, truth_strides, teacher_q, teacher_k,
                     teacher_dtype, teacher_q_strides, teacher_k_strides, N, H, T, D, p);
  if (rc == SEA_OK)
    rc = kd_check_nulls(nm,
                        {KdArg{"row_q", row_q}, {"row_stats", row_stats}, {"grad_loss", grad_loss}, {"d_q", d_q}, {"d_k", d_k}});
  if (rc != SEA_OK) return rc;
  SEA_REQUIRE(((uintptr_t)row_stats & 15) == 0 && ((uintptr_t)d_q & 7) == 0 && ((uintptr_t)d_k & 7) == 0, SEA_EINVAL,
              "%s: row_stats must be 16-byte aligned, d_q and d_k 8-byte aligned", nm);
  p.row_q = const_cast<float*>(row_q); p.row_stats = const_cast<float*>(row_stats);
  p.grad_loss = grad_loss; p.d_q = d_q; p.d_k = d_k;
  return ks_dispatch(nm, true, qk_dtype, truth_dtype, D, p, (hipStream_t)stream);
}
