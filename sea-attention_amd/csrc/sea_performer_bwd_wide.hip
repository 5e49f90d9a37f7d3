// Backward of the causal Performer for the wide heads D = 80 / 128, gfx950: include/sea_hip_estimator_grad_wide.h, entry w1;
// DESIGN 5.10b.  The mathematics is that of sea_performer_bwd.hip (D = 64), whose NBP x 2D state does not fit the LDS here.
//
// Everything is linear in the E = 2D value columns V = [pos | v], so they are split over two workgroups.  Half h (0: the pos
// columns, 1: the v columns; V_h, g_h, S_h, R_h all D wide), a = phi(q), b = phi(k), A = tril(a b^T), den = A 1 + a (z + 1e-6):
//   num_h = A V_h + a S_h        G_h = g_h / den        e_h = -(g_h . num_h) / den^2            B_h = tril(G_h V_h^T + e_h 1^T)
//   forward sweep (S_h, z)       da_h = B_h b + G_h S_h^T + e_h (z + 1e-6)^T             then  S_h += b^T V_h,  z += sum b
//   reverse sweep (R_h, r_h)     dV_h = A^T G_h + b R_h,   db_h = B_h^T a + V_h R_h^T + 1 r_h^T   then  R_h += a^T G_h,  r_h += a^T e_h
//   dq_h = s (da_h (.) [q W^T > 0]) W,  dk_h likewise       dq = dq_0 + dq_1,  dk = dk_0 + dk_1
//   dpos = sum over (n, h) of dV_0,   dv = dV_1 + g[:, 2D:]
// Two launches on the grid (N H, 2) of one 512-thread workgroup (8 waves) each, walking chunks of C = 32 rows:
// performer_bwd_wide_fwd writes the fp32 partial dq_h and the row scalars 1 / den, g_h . num_h / den^2 of its half;
// performer_bwd_wide_rev reads them back and writes the fp32 partial dk_h and, half 0, its pair's part of dpos, half 1, dv.
// performer_bwd_wide_close adds half 0 + half 1, casts, and adds the dpos parts in the order of (n, h).  Both halves compute the
// feature maps and den: that is the price; a one-sequence step gets twice the workgroups.  No atomics: the same bits every run.
// Every product is fp32 on v_mfma_f32_16x16x4_f32; 16-bit data is widened on load.
//
// LDS plan (fp32; PerfWidePlan; bytes at D = 128 NBT = 5 / D = 128 NBT = 3 / D = 80 NBT = 5 / D = 80 NBT = 3):
//   state  NBP x (D + 4)   42240 / 25344 / 26880 / 16128   S_h or R_h, resident for the whole walk
//   W      NBP x (D + 4)   the same                        the projection, resident (the D = 64 kernel stages it twice per chunk)
//   P, Kf  32 x (NBP + 4)  10752 / 6656 each               a and b; the masked da overwrites a (forward), the masked db b (reverse)
//   V, G   32 x (D + 4)    16896 / 10752 each              Q and K staged for the feature maps; then V_h and G_h
//   A, B   32 x 36         4608 each                       the two lower-triangular tiles
//   small  z or r, 1 / den, e, the partial sums of den (32 x 16) and g . num (32 x D / 16), the ReLU ballots
// 152960 / 110720 / 109568 / 79616 bytes: one workgroup per CU.  A padded feature and a padded row of the last chunk are ZERO in
// a and b (their phi would be 1e-3), in G, e and V, and their mask bits are clear.
// Compiled without packed fp32 arithmetic (_build.FILE_FLAGS).
#include <algorithm>
#include "sea_common.hpp"
#include "../../include/sea_hip_estimator_grad_wide.h"

namespace sea {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
#define SEA_WIDE_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

struct PerfWideParams {
  const void *q, *k, *v, *pos, *g;
  const float* W;
  void* dv;
  float* rowstat;      // (2, N*H, T, 2): 1 / den, g_h . num_h / den^2
  float* dq_part;      // (2, N*H, T, D)
  float* dk_part;      // (2, N*H, T, D)
  float* dpos_part;    // (N*H, T, D)
  int64_t qs[3], ks[3], vs[3], pos_stride, pairs;
  int H, T, nb;
};

template <int D_, int NBT>
struct PerfWidePlan {
  static constexpr int D = D_, C = 32, NTH = 512, NW = 8, NCB = D / 16, NDP = 16;     // NDP: partial sums of den per row
  static constexpr int NBP = 16 * NBT, LDP = NBP + 4, LDV = D + 4, LDT = C + 4;
  static constexpr int oState = 0, oW = oState + NBP * LDV, oP = oW + NBP * LDV, oK = oP + C * LDP, oV = oK + C * LDP;
  static constexpr int oG = oV + C * LDV, oA = oG + C * LDV, oB = oA + C * LDT, oSum = oB + C * LDT, oInv = oSum + NBP;
  static constexpr int oE = oInv + C, oPart = oE + C, oPartG = oPart + C * NDP, oMask = oPartG + C * NCB;
  static constexpr int floats = oMask + 2 * NBT * 4 * 2;            // 2 row blocks x NBT x 4 ballots of 8 bytes
  static constexpr int lds_bytes = floats * 4;
  static_assert(D % 16 == 0 && C * NDP == NTH, "column blocks of 16; one den partial per thread");
  static_assert(oMask % 2 == 0, "ballots are 8-byte aligned");
  static_assert(lds_bytes <= 160 * 1024, "LDS");
};

// C rows x D of a row-major global tensor into LDS as fp32, scaled per row; rows at or beyond `rows` become zero
template <typename T, typename P, typename F>
__device__ inline void wide_stage(float* dst, const T* src, int64_t rstride, int t0, int rows, F scale) {
  constexpr int VEC = Elem<T>::VEC, ppr = P::D / VEC;
  for (int idx = threadIdx.x; idx < P::C * ppr; idx += P::NTH) {
    const int r = idx / ppr, c = (idx - r * ppr) * VEC;
    float f[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) f[j] = 0.f;
    float sc = 0.f;
    if (r < rows) {
      const uint4 raw = *reinterpret_cast<const uint4*>(src + (int64_t)(t0 + r) * rstride + c);
      unpack16<T>(raw, f);
      sc = scale(r);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) dst[r * P::LDV + c + j] = (r < rows) ? f[j] * sc : 0.f;
  }
}

// phi(Q) -> sP, phi(K) -> sKf from the staged chunk; wave wv owns matrix wv & 1, row block (wv >> 1) & 1 and the feature blocks
// of parity wv >> 2.  The ReLU mask of matrix `mask_of` (0: Q, 1: K) is kept as one ballot per (row block, feature block, register).
template <typename P, int NBT>
__device__ inline void wide_feature_maps(const float* sQ, const float* sKr, const float* sW, float* sP, float* sKf,
                                         unsigned long long* sMask, int mask_of, int rows, int nb, float cnorm) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  const int which = wv & 1, ib = (wv >> 1) & 1, par = wv >> 2;
  constexpr int NJ = (NBT + 1) / 2;
  const float* src = which ? sKr : sQ;
  f4 acc[NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) acc[i] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int ks = 0; ks < P::D / 4; ++ks) {
    const float a = src[(ib * 16 + li) * P::LDV + ks * 4 + lg];
#pragma unroll
    for (int i = 0; i < NJ; ++i)
      if (par + 2 * i < NBT) acc[i] = SEA_WIDE_MFMA(a, sW[((par + 2 * i) * 16 + li) * P::LDV + ks * 4 + lg], acc[i]);
  }
  float* dst = which ? sKf : sP;
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    const int jb = par + 2 * i, col = jb * 16 + li;
    if (jb < NBT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ib * 16 + lg * 4 + r;
        const bool live = col < nb && row < rows;
        dst[row * P::LDP + col] = live ? fmaxf(cnorm * acc[i][r], 0.f) + 1e-3f : 0.f;
        const unsigned long long m = __ballot(live && acc[i][r] > 0.f);
        if (which == mask_of && lane == 0) sMask[(ib * NBT + jb) * 4 + r] = m;
      }
    }
  }
}

// the three lower 16 x 16 tiles of X Y^T (X, Y: 32 x K in LDS), + add[row], zero above the diagonal -> sT (32 x LDT); waves 0..2
template <typename P, typename ADD>
__device__ inline void wide_tril(float* sT, const float* sXm, int ldx, const float* sYm, int ldy, int K, ADD add) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  if (wv >= 3) return;
  const int ib = wv > 0, jb = wv > 1;
  f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int ks = 0; ks < K / 4; ++ks)
    acc = SEA_WIDE_MFMA(sXm[(ib * 16 + li) * ldx + ks * 4 + lg], sYm[(jb * 16 + li) * ldy + ks * 4 + lg], acc);
  const int col = jb * 16 + li;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = ib * 16 + lg * 4 + r;
    sT[row * P::LDT + col] = (col <= row) ? acc[r] + add(row) : 0.f;
  }
}

// state[f][col] += sum over the chunk rows of F[row][f] * X[row][col]   (NBP x D; the NBT x NCB tiles dealt to the waves)
template <typename P, int NBT>
__device__ inline void wide_state_update(float* sS, const float* sF, const float* sXm) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  for (int tile = wv; tile < NBT * P::NCB; tile += P::NW) {
    const int fb = tile / P::NCB, cb = tile - fb * P::NCB;
    f4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = sS[(fb * 16 + lg * 4 + r) * P::LDV + cb * 16 + li];
#pragma unroll
    for (int ks = 0; ks < P::C / 4; ++ks)
      acc = SEA_WIDE_MFMA(sF[(ks * 4 + lg) * P::LDP + fb * 16 + li], sXm[(ks * 4 + lg) * P::LDV + cb * 16 + li], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) sS[(fb * 16 + lg * 4 + r) * P::LDV + cb * 16 + li] = acc[r];
  }
}

// out[t0 + row][0..D) = cnorm * (sDm (32 x NBP, already masked) W) as fp32, rows below `rows`
template <typename P>
__device__ inline void wide_project_back(float* out, const float* sDm, const float* sW, int t0, int rows, float cnorm) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  for (int tile = wv; tile < 2 * P::NCB; tile += P::NW) {
    const int ib = tile / P::NCB, cb = tile - ib * P::NCB;
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int ks = 0; ks < P::NBP / 4; ++ks)
      acc = SEA_WIDE_MFMA(sDm[(ib * 16 + li) * P::LDP + ks * 4 + lg], sW[(ks * 4 + lg) * P::LDV + cb * 16 + li], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ib * 16 + lg * 4 + r;
      if (row < rows) out[(int64_t)(t0 + row) * P::D + cb * 16 + li] = cnorm * acc[r];
    }
  }
}

// state, its vector and the resident projection (rows at or beyond nb zero) before the walk
template <typename P>
__device__ inline void wide_prologue(float* sState, float* sVec, float* sW, const float* W, int nb) {
  for (int i = threadIdx.x; i < P::NBP * P::LDV; i += P::NTH) {
    const int r = i / P::LDV, c = i - r * P::LDV;
    sState[i] = 0.f;
    sW[i] = (r < nb && c < P::D) ? W[r * P::D + c] : 0.f;
  }
  if (threadIdx.x < P::NBP) sVec[threadIdx.x] = 0.f;
}

template <typename T, int D_, int NBT>
__global__ __launch_bounds__(512) void performer_bwd_wide_fwd(PerfWideParams p) {
  using P = PerfWidePlan<D_, NBT>;
  constexpr int D = P::D, C = P::C, NBP = P::NBP, LDP = P::LDP, LDV = P::LDV, LDT = P::LDT, NW = P::NW, NCB = P::NCB, NDP = P::NDP;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *sS = smem + P::oState, *sW = smem + P::oW, *sP = smem + P::oP, *sKf = smem + P::oK, *sV = smem + P::oV, *sG = smem + P::oG;
  float *sA = smem + P::oA, *sB = smem + P::oB, *sZ = smem + P::oSum, *sInv = smem + P::oInv, *sE = smem + P::oE;
  float *sPart = smem + P::oPart, *sPartG = smem + P::oPartG;
  unsigned long long* sMask = reinterpret_cast<unsigned long long*>(smem + P::oMask);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int nh = blockIdx.x, hf = blockIdx.y, n = nh / p.H, h = nh - n * p.H, T_ = p.T;
  const T* qb = reinterpret_cast<const T*>(p.q) + n * p.qs[0] + h * p.qs[1];
  const T* kb = reinterpret_cast<const T*>(p.k) + n * p.ks[0] + h * p.ks[1];
  const T* xb = hf ? reinterpret_cast<const T*>(p.v) + n * p.vs[0] + h * p.vs[1] : reinterpret_cast<const T*>(p.pos);
  const int64_t xstride = hf ? p.vs[2] : p.pos_stride;
  const T* gb = reinterpret_cast<const T*>(p.g) + (int64_t)nh * T_ * (3 * D) + hf * D;     // this half's D columns of a 3D-wide row
  float* dqp = p.dq_part + ((int64_t)hf * p.pairs + nh) * T_ * D;
  float* rs = p.rowstat + ((int64_t)hf * p.pairs + nh) * T_ * 2;
  const float cnorm = powf((float)D, -0.25f);
  auto one = [](int) { return 1.f; };

  wide_prologue<P>(sS, sZ, sW, p.W, p.nb);
  __syncthreads();

  for (int t0 = 0; t0 < T_; t0 += C) {
    const int rows = min(C, T_ - t0);
    // ---- 1: Q -> the V region, K -> the G region; a, b and the mask of q
    wide_stage<T, P>(sV, qb, p.qs[2], t0, rows, one);
    wide_stage<T, P>(sG, kb, p.ks[2], t0, rows, one);
    __syncthreads();
    wide_feature_maps<P, NBT>(sV, sG, sW, sP, sKf, sMask, 0, rows, p.nb, cnorm);
    __syncthreads();
    // ---- 2: A = tril(a b^T); V_h
    wide_tril<P>(sA, sP, LDP, sKf, LDP, NBP, [](int) { return 0.f; });
    wide_stage<T, P>(sV, xb, xstride, t0, rows, one);
    __syncthreads();
    // ---- 3: den = A 1 + a . (z + 1e-6) and g_h . num_h with num_h = A V_h + a S_h, neither stored
    {
      const int row = tid & (C - 1), part = tid / C;
      float s = 0.f;
      for (int c = part * (C / NDP); c < (part + 1) * (C / NDP); ++c) s += (c <= row) ? sA[row * LDT + c] : 0.f;
      constexpr int per = (NBP + NDP - 1) / NDP;
      for (int f = part * per; f < min(NBP, (part + 1) * per); ++f) s = fmaf(sP[row * LDP + f], sZ[f] + 1e-6f, s);
      sPart[row * NDP + part] = s;
    }
    for (int tile = wv; tile < 2 * NCB; tile += NW) {
      const int ib = tile / NCB, cb = tile - ib * NCB;
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < 4 * (ib + 1); ++ks)
        acc = SEA_WIDE_MFMA(sA[(ib * 16 + li) * LDT + ks * 4 + lg], sV[(ks * 4 + lg) * LDV + cb * 16 + li], acc);
#pragma unroll 4
      for (int ks = 0; ks < NBP / 4; ++ks)
        acc = SEA_WIDE_MFMA(sP[(ib * 16 + li) * LDP + ks * 4 + lg], sS[(ks * 4 + lg) * LDV + cb * 16 + li], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ib * 16 + lg * 4 + r;
        float s = (row < rows) ? Elem<T>::to_f(gb[(int64_t)(t0 + row) * (3 * D) + cb * 16 + li]) * acc[r] : 0.f;
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
        if (li == 0) sPartG[row * NCB + cb] = s;
      }
    }
    __syncthreads();
    if (tid < C) {
      float den = 0.f, gn = 0.f;
#pragma unroll
      for (int i = 0; i < NDP; ++i) den += sPart[tid * NDP + i];
#pragma unroll
      for (int i = 0; i < NCB; ++i) gn += sPartG[tid * NCB + i];
      float inv = 0.f, c = 0.f;
      if (tid < rows) {
        inv = 1.f / den;
        c = gn * inv * inv;
        rs[(int64_t)(t0 + tid) * 2] = inv;
        rs[(int64_t)(t0 + tid) * 2 + 1] = c;
      }
      sInv[tid] = inv;
      sE[tid] = -c;
    }
    __syncthreads();
    // ---- 4: G_h = g_h / den -> the G region; B = tril(G_h V_h^T + e_h)
    wide_stage<T, P>(sG, gb, 3 * D, t0, rows, [&](int r) { return sInv[r]; });
    __syncthreads();
    wide_tril<P>(sB, sG, LDV, sV, LDV, D, [&](int row) { return sE[row]; });
    __syncthreads();
    // ---- 5: da_h = B b + G_h S_h^T + e_h (z + 1e-6), masked, over a (nothing reads a any more)
    for (int tile = wv; tile < 2 * NBT; tile += NW) {
      const int ib = tile / NBT, fb = tile - ib * NBT;
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < 4 * (ib + 1); ++ks)
        acc = SEA_WIDE_MFMA(sB[(ib * 16 + li) * LDT + ks * 4 + lg], sKf[(ks * 4 + lg) * LDP + fb * 16 + li], acc);
#pragma unroll 4
      for (int ks = 0; ks < D / 4; ++ks)
        acc = SEA_WIDE_MFMA(sG[(ib * 16 + li) * LDV + ks * 4 + lg], sS[(fb * 16 + li) * LDV + ks * 4 + lg], acc);
      const float zf = sZ[fb * 16 + li] + 1e-6f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ib * 16 + lg * 4 + r;
        const bool on = (sMask[(ib * NBT + fb) * 4 + r] >> lane) & 1ull;
        sP[row * LDP + fb * 16 + li] = on ? fmaf(sE[row], zf, acc[r]) : 0.f;
      }
    }
    __syncthreads();
    // ---- 6: S_h += b^T V_h, z += sum b; dq_h = s da_h W
    wide_state_update<P, NBT>(sS, sKf, sV);
    if (tid < NBP) {
      float s = sZ[tid];
      for (int r = 0; r < C; ++r) s += sKf[r * LDP + tid];
      sZ[tid] = s;
    }
    wide_project_back<P>(dqp, sP, sW, t0, rows, cnorm);
    __syncthreads();                                                 // the next chunk's Q and K go where V_h and G_h are read
  }
}

template <typename T, int D_, int NBT>
__global__ __launch_bounds__(512) void performer_bwd_wide_rev(PerfWideParams p) {
  using P = PerfWidePlan<D_, NBT>;
  constexpr int D = P::D, C = P::C, NBP = P::NBP, LDP = P::LDP, LDV = P::LDV, LDT = P::LDT, NW = P::NW, NCB = P::NCB;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *sR = smem + P::oState, *sW = smem + P::oW, *sP = smem + P::oP, *sKf = smem + P::oK, *sV = smem + P::oV, *sG = smem + P::oG;
  float *sA = smem + P::oA, *sB = smem + P::oB, *sr = smem + P::oSum, *sInv = smem + P::oInv, *sE = smem + P::oE;
  unsigned long long* sMask = reinterpret_cast<unsigned long long*>(smem + P::oMask);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int nh = blockIdx.x, hf = blockIdx.y, n = nh / p.H, h = nh - n * p.H, T_ = p.T;
  const T* qb = reinterpret_cast<const T*>(p.q) + n * p.qs[0] + h * p.qs[1];
  const T* kb = reinterpret_cast<const T*>(p.k) + n * p.ks[0] + h * p.ks[1];
  const T* xb = hf ? reinterpret_cast<const T*>(p.v) + n * p.vs[0] + h * p.vs[1] : reinterpret_cast<const T*>(p.pos);
  const int64_t xstride = hf ? p.vs[2] : p.pos_stride;
  const T* g0 = reinterpret_cast<const T*>(p.g) + (int64_t)nh * T_ * (3 * D);
  const T* gb = g0 + hf * D;
  float* dkp = p.dk_part + ((int64_t)hf * p.pairs + nh) * T_ * D;
  T* dvb = reinterpret_cast<T*>(p.dv) + (int64_t)nh * T_ * D;
  float* dpp = p.dpos_part + (int64_t)nh * T_ * D;
  const float* rs = p.rowstat + ((int64_t)hf * p.pairs + nh) * T_ * 2;
  const float cnorm = powf((float)D, -0.25f);
  auto one = [](int) { return 1.f; };

  wide_prologue<P>(sR, sr, sW, p.W, p.nb);
  __syncthreads();

  for (int t0 = ((T_ - 1) / C) * C; t0 >= 0; t0 -= C) {              // the partial chunk first
    const int rows = min(C, T_ - t0);
    // ---- 1: Q -> the V region, K -> the G region; a, b and the mask of k; the row scalars of this half
    wide_stage<T, P>(sV, qb, p.qs[2], t0, rows, one);
    wide_stage<T, P>(sG, kb, p.ks[2], t0, rows, one);
    if (tid < C) {
      sInv[tid] = (tid < rows) ? rs[(int64_t)(t0 + tid) * 2] : 0.f;
      sE[tid] = (tid < rows) ? -rs[(int64_t)(t0 + tid) * 2 + 1] : 0.f;
    }
    __syncthreads();
    wide_feature_maps<P, NBT>(sV, sG, sW, sP, sKf, sMask, 1, rows, p.nb, cnorm);
    __syncthreads();
    // ---- 2: A = tril(a b^T); V_h and G_h = g_h / den
    wide_tril<P>(sA, sP, LDP, sKf, LDP, NBP, [](int) { return 0.f; });
    wide_stage<T, P>(sV, xb, xstride, t0, rows, one);
    wide_stage<T, P>(sG, gb, 3 * D, t0, rows, [&](int r) { return sInv[r]; });
    __syncthreads();
    // ---- 3: dV_h = A^T G_h + b R_h leaves from the registers: the dpos part (half 0) or dv (half 1)
    for (int tile = wv; tile < 2 * NCB; tile += NW) {
      const int ib = tile / NCB, cb = tile - ib * NCB;
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      for (int ks = 4 * ib; ks < C / 4; ++ks)                        // rows t of the blocks at and below the diagonal
        acc = SEA_WIDE_MFMA(sA[(ks * 4 + lg) * LDT + ib * 16 + li], sG[(ks * 4 + lg) * LDV + cb * 16 + li], acc);
#pragma unroll 4
      for (int ks = 0; ks < NBP / 4; ++ks)
        acc = SEA_WIDE_MFMA(sKf[(ib * 16 + li) * LDP + ks * 4 + lg], sR[(ks * 4 + lg) * LDV + cb * 16 + li], acc);
      const int col = cb * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ib * 16 + lg * 4 + r;
        if (row < rows) {
          const int64_t t = t0 + row;
          if (hf == 0) dpp[t * D + col] = acc[r];
          else dvb[t * D + col] = from_f<T>(acc[r] + Elem<T>::to_f(g0[t * (3 * D) + 2 * D + col]));
        }
      }
    }
    // ---- 4: B = tril(G_h V_h^T + e_h)
    wide_tril<P>(sB, sG, LDV, sV, LDV, D, [&](int row) { return sE[row]; });
    __syncthreads();
    // ---- 5: db_h = B^T a + V_h R_h^T + r_h, masked, over b (every wave is past step 3)
    for (int tile = wv; tile < 2 * NBT; tile += NW) {
      const int ib = tile / NBT, fb = tile - ib * NBT;
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      for (int ks = 4 * ib; ks < C / 4; ++ks)
        acc = SEA_WIDE_MFMA(sB[(ks * 4 + lg) * LDT + ib * 16 + li], sP[(ks * 4 + lg) * LDP + fb * 16 + li], acc);
#pragma unroll 4
      for (int ks = 0; ks < D / 4; ++ks)
        acc = SEA_WIDE_MFMA(sV[(ib * 16 + li) * LDV + ks * 4 + lg], sR[(fb * 16 + li) * LDV + ks * 4 + lg], acc);
      const float rf = sr[fb * 16 + li];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool on = (sMask[(ib * NBT + fb) * 4 + r] >> lane) & 1ull;
        sKf[(ib * 16 + lg * 4 + r) * LDP + fb * 16 + li] = on ? acc[r] + rf : 0.f;
      }
    }
    __syncthreads();
    // ---- 6: R_h += a^T G_h, r_h += a^T e_h; dk_h = s db_h W
    wide_state_update<P, NBT>(sR, sP, sG);
    if (tid < NBP) {
      float s = sr[tid];
      for (int r = 0; r < C; ++r) s = fmaf(sP[r * LDP + tid], sE[r], s);
      sr[tid] = s;
    }
    wide_project_back<P>(dkp, sKf, sW, t0, rows, cnorm);
    __syncthreads();                                                 // the next chunk's Q, K and scalars go where these are read
  }
}

// dq = dq_0 + dq_1 and dk = dk_0 + dk_1 (half 0 first) cast to the data type; dpos = the parts in the order of (n, h)
template <typename T>
__global__ __launch_bounds__(256) void performer_bwd_wide_close(const float* dq_part, const float* dk_part, const float* dpos_part,
                                                                T* dq, T* dk, float* dpos, int64_t total, int64_t pairs, int64_t TD) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    dq[i] = from_f<T>(dq_part[i] + dq_part[total + i]);
    dk[i] = from_f<T>(dk_part[i] + dk_part[total + i]);
    if (i < TD) {
      float s = 0.f;
      for (int64_t j = 0; j < pairs; ++j) s += dpos_part[j * TD + i];
      dpos[i] = s;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// the (D, nb, dtype) sea_performer.hip's perf_form has a kernel form for at the wide head sizes
bool wide_supported(int64_t D, int64_t nb, int dtype) {
  return (D == 80 || D == 128) && nb >= 1 && nb <= 80 && (dtype == SEA_F32 || dtype == SEA_F16 || dtype == SEA_BF16);
}

int64_t align16(int64_t b) { return (b + 15) / 16 * 16; }
int64_t rowstat_bytes(int64_t pairs, int64_t T) { return align16(2 * pairs * T * 2 * (int64_t)sizeof(float)); }
int64_t image_bytes(int64_t pairs, int64_t T, int64_t D) { return align16(pairs * T * D * (int64_t)sizeof(float)); }

template <typename T, int D, int NBT>
int launch_wide(const PerfWideParams& p, void* d_q, void* d_k, float* d_pos, hipStream_t s) {
  using P = PerfWidePlan<D, NBT>;
  static DevOnce once;
  if (once.first()) {
    SEA_MAX_LDS((performer_bwd_wide_fwd<T, D, NBT>), P::lds_bytes);
    SEA_MAX_LDS((performer_bwd_wide_rev<T, D, NBT>), P::lds_bytes);
  }
  const char* nm = "sea_performer_causal_bwd_wide";
  const dim3 grid((unsigned)p.pairs, 2);
  hipLaunchKernelGGL((performer_bwd_wide_fwd<T, D, NBT>), grid, dim3(512), P::lds_bytes, s, p);
  SEA_CHECK_LAUNCH(nm);
  hipLaunchKernelGGL((performer_bwd_wide_rev<T, D, NBT>), grid, dim3(512), P::lds_bytes, s, p);
  SEA_CHECK_LAUNCH(nm);
  const int64_t total = p.pairs * p.T * D;
  const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 1 << 20);
  hipLaunchKernelGGL((performer_bwd_wide_close<T>), dim3(blocks), dim3(256), 0, s, p.dq_part, p.dk_part, p.dpos_part,
                     reinterpret_cast<T*>(d_q), reinterpret_cast<T*>(d_k), d_pos, total, p.pairs, (int64_t)p.T * D);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}

template <typename T>
int launch_wide_form(const PerfWideParams& p, int64_t D, void* d_q, void* d_k, float* d_pos, hipStream_t s) {
  if (D == 80) return p.nb <= 48 ? launch_wide<T, 80, 3>(p, d_q, d_k, d_pos, s) : launch_wide<T, 80, 5>(p, d_q, d_k, d_pos, s);
  return p.nb <= 48 ? launch_wide<T, 128, 3>(p, d_q, d_k, d_pos, s) : launch_wide<T, 128, 5>(p, d_q, d_k, d_pos, s);
}

}  // namespace
}  // namespace sea

using namespace sea;

extern "C" int sea_estimator_grad_wide_version(void) { return SEA_ESTIMATOR_GRAD_WIDE_ABI_VERSION; }

extern "C" int sea_performer_causal_bwd_wide_supported(int64_t D, int64_t nb, int dtype) { return wide_supported(D, nb, dtype) ? 1 : 0; }

extern "C" int64_t sea_performer_causal_bwd_wide_workspace_bytes(int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb, int dtype) {
  if (N <= 0 || H <= 0 || T <= 0 || !wide_supported(D, nb, dtype)) return 0;
  return rowstat_bytes(N * H, T) + 2 * image_bytes(2 * N * H, T, D) + image_bytes(N * H, T, D);
}

extern "C" int sea_performer_causal_bwd_wide(const void* q, const void* k, const void* v, const void* pos, int dtype, const float* proj,
                                             int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb,
                                             const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                             int64_t pos_stride, const void* grad_out, void* d_q, void* d_k, void* d_v, float* d_pos,
                                             void* workspace, int64_t workspace_bytes, sea_stream_t stream) {
  const char* nm = "sea_performer_causal_bwd_wide";
#define SEA_WIDE_NONNULL(x) SEA_REQUIRE((x) != nullptr, SEA_EINVAL, "%s: " #x " is null", nm)
  SEA_WIDE_NONNULL(q); SEA_WIDE_NONNULL(k); SEA_WIDE_NONNULL(v); SEA_WIDE_NONNULL(pos); SEA_WIDE_NONNULL(proj);
  SEA_WIDE_NONNULL(q_strides); SEA_WIDE_NONNULL(k_strides); SEA_WIDE_NONNULL(v_strides);
  SEA_WIDE_NONNULL(grad_out); SEA_WIDE_NONNULL(d_q); SEA_WIDE_NONNULL(d_k); SEA_WIDE_NONNULL(d_v); SEA_WIDE_NONNULL(d_pos);
  SEA_WIDE_NONNULL(workspace);
#undef SEA_WIDE_NONNULL
  SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: unknown dtype %d", nm, dtype);
  SEA_REQUIRE(N > 0 && H > 0 && T > 0 && D > 0 && nb > 0, SEA_EINVAL, "%s: bad shape N=%lld H=%lld T=%lld D=%lld nb=%lld", nm,
              (long long)N, (long long)H, (long long)T, (long long)D, (long long)nb);
  SEA_REQUIRE(D == 80 || D == 128, SEA_EUNSUPPORTED, "%s: D=%lld has no wide backward kernel (D = 80 or 128; 64: sea_performer_causal_bwd)",
              nm, (long long)D);
  SEA_REQUIRE(nb <= 80, SEA_EUNSUPPORTED, "%s: nb=%lld has no backward kernel (nb <= 80)", nm, (long long)nb);
  SEA_REQUIRE(T < (1ll << 24) && N * H < (1ll << 31), SEA_EUNSUPPORTED, "%s: T=%lld or N*H=%lld beyond the limits", nm, (long long)T,
              (long long)(N * H));
  const int64_t vec = dtype == SEA_F32 ? 4 : 8;
  struct In { const char* name; const void* base; const int64_t* s; };
  const In ins[3] = {{"q", q, q_strides}, {"k", k, k_strides}, {"v", v, v_strides}};
  for (const In& t : ins) {
    SEA_REQUIRE(t.s[0] >= 0 && t.s[1] >= 0 && t.s[2] >= D, SEA_EINVAL, "%s: bad %s strides {%lld, %lld, %lld}", nm, t.name,
                (long long)t.s[0], (long long)t.s[1], (long long)t.s[2]);
    SEA_REQUIRE(((uintptr_t)t.base & 15) == 0 && t.s[0] % vec == 0 && t.s[1] % vec == 0 && t.s[2] % vec == 0, SEA_EINVAL,
                "%s: %s rows must be 16-byte aligned", nm, t.name);
  }
  SEA_REQUIRE(pos_stride >= D, SEA_EINVAL, "%s: bad pos stride %lld", nm, (long long)pos_stride);
  SEA_REQUIRE(((uintptr_t)pos & 15) == 0 && pos_stride % vec == 0, SEA_EINVAL, "%s: pos rows must be 16-byte aligned", nm);
  SEA_REQUIRE(((uintptr_t)proj & 15) == 0, SEA_EINVAL, "%s: proj rows must be 16-byte aligned", nm);
  SEA_REQUIRE(((uintptr_t)grad_out & 15) == 0, SEA_EINVAL, "%s: grad_out rows must be 16-byte aligned", nm);
  SEA_REQUIRE((((uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_pos) & 15) == 0, SEA_EINVAL,
              "%s: d_q, d_k, d_v, d_pos rows must be 16-byte aligned", nm);
  const int64_t need = sea_performer_causal_bwd_wide_workspace_bytes(N, H, T, D, nb, dtype);
  SEA_REQUIRE(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need, SEA_EINVAL,
              "%s: workspace of %lld bytes needed (16-byte aligned), got %lld", nm, (long long)need, (long long)workspace_bytes);

  PerfWideParams p;
  p.q = q; p.k = k; p.v = v; p.pos = pos; p.g = grad_out; p.W = proj; p.dv = d_v;
  char* ws = reinterpret_cast<char*>(workspace);
  p.rowstat = reinterpret_cast<float*>(ws);
  p.dq_part = reinterpret_cast<float*>(ws + rowstat_bytes(N * H, T));
  p.dk_part = reinterpret_cast<float*>(ws + rowstat_bytes(N * H, T) + image_bytes(2 * N * H, T, D));
  p.dpos_part = reinterpret_cast<float*>(ws + rowstat_bytes(N * H, T) + 2 * image_bytes(2 * N * H, T, D));
  for (int i = 0; i < 3; ++i) { p.qs[i] = q_strides[i]; p.ks[i] = k_strides[i]; p.vs[i] = v_strides[i]; }
  p.pos_stride = pos_stride; p.pairs = N * H;
  p.H = (int)H; p.T = (int)T; p.nb = (int)nb;
  hipStream_t s = (hipStream_t)stream;
  return dtype == SEA_F32 ? launch_wide_form<float>(p, D, d_q, d_k, d_pos, s)
       : dtype == SEA_F16 ? launch_wide_form<__half>(p, D, d_q, d_k, d_pos, s)
                          : launch_wide_form<__hip_bfloat16>(p, D, d_q, d_k, d_pos, s);
}
