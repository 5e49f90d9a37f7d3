// Backward of the causal Performer (sea_performer_causal), gfx950: include/sea_hip_estimator_grad.h, entry g1.
//
// Nothing of the forward is saved.  With a = phi(q), b = phi(k), V = [pos | v] (E = 2D wide), S / z the running state and k-sum
// BEFORE a chunk, G = g[:E] / den, e = -(g[:E] . num) / den^2 (the gradient of the column of ones that carries the denominator):
//   per chunk of C rows        A = tril(a b^T)                 B = tril(G V^T + e 1^T)
//   forward sweep   (S, z)     da = B b + G S^T + e (z + 1e-6)^T          then  S += b^T V,  z += sum b
//   reverse sweep   (R, r)     dV = A^T G + b R,   db = B^T a + V R^T + 1 r^T      then  R += a^T G,  r += a^T e
//   dq = s (da (.) [q W^T > 0]) W,  dk likewise,  dv = dV[:, D:] + g[:, E:],  dpos = sum over (n, h) of dV[:, :D]
// Two launches of one 512-thread workgroup (8 waves) per (n, h): performer_bwd_fwd_sweep walks the chunks upwards, computes den
// and num again, writes dq and the two row scalars 1 / den and g . ctx / den to the workspace; performer_bwd_rev_sweep walks them
// downwards from the partial chunk, reads the scalars, writes dk, dv and this pair's part of dpos.  performer_bwd_dpos adds the
// parts in the order of (n, h).  No atomics.  Every product is fp32 on v_mfma_f32_16x16x4_f32; 16-bit data is widened on load.
//
// LDS plan (D = 64, C = 64, NBP = 16 NBT features, fp32; bytes at NBT = 5 / 3), DESIGN 5.10:
//   state   NBP x 132   42240 / 25344    S (forward sweep) or R (reverse sweep), resident for the whole walk
//   P       64 x max(NBP + 4, 68)  21504 / 17408    a; then the B tile (forward) ; then the masked da
//   Kf      same                                      b; then the B tile (reverse)
//   V       64 x 132    33792            Q and K staging (2 x 64 x 66); V; the A tile and then the masked db (reverse)
//   G       64 x 132    33792            W (NBP x 68) across the chunk boundary; the A tile (forward); G
//   small   z or r, 1 / den, e, two 64 x 8 partial-sum tables, the ReLU masks (one 64-bit ballot per tile register)
// 158400 bytes at NBT = 5, 130752 at NBT = 3: one workgroup per CU either way.  A padded feature and a padded row of the last
// chunk are ZERO in a and b (their phi would be 1e-3), G, e and V of a padded row are zero, and the masks are clear there.
#include "sea_common.hpp"
#include "../../include/sea_hip_estimator_grad.h"

namespace sea {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
#define SEA_BWD_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

struct PerfBwdParams {
  const void *q, *k, *v, *pos, *g;
  const float* W;
  void *dq, *dk, *dv;
  float* rowstat;      // (N*H, T, 2): 1 / den, g . ctx / den
  float* dpos_part;    // (N*H, T, D)
  int64_t qs[3], ks[3], vs[3], pos_stride;
  int H, T, nb;
};

template <int NBT>
struct PerfBwdPlan {
  static constexpr int D = 64, E = 128, C = 64, NTH = 512, NW = 8;
  static constexpr int NBP = 16 * NBT, LDP = NBP + 4, LDV = E + 4, LDX = 66, LDT = 68, LDW = 68;
  static constexpr int RQ = C * (LDP > LDT ? LDP : LDT);
  static constexpr int oState = 0, oP = oState + NBP * LDV, oK = oP + RQ, oV = oK + RQ, oG = oV + C * LDV;
  static constexpr int oSum = oG + C * LDV, oInv = oSum + NBP, oE = oInv + C, oPart = oE + C, oPartG = oPart + C * 8;
  static constexpr int oMask = oPartG + C * 8;                       // 4 * NBT * 4 ballots of 8 bytes
  static constexpr int floats = oMask + 4 * NBT * 4 * 2;
  static constexpr int lds_bytes = floats * 4;
  static_assert(2 * C * LDX <= C * LDV && NBP * LDW <= C * LDV && C * LDT <= C * LDV, "overlays of the V / G regions");
  static_assert(oMask % 2 == 0, "ballots are 8-byte aligned");
  static_assert(lds_bytes <= 160 * 1024, "LDS");
};

// C rows x ncols of a row-major global tensor into LDS as fp32, scaled per row; rows at or beyond `rows` become zero
template <typename T, typename F>
__device__ inline void stage_rows(float* dst, int ld, const T* src, int64_t rstride, int t0, int rows, int ncols, F scale) {
  constexpr int VEC = Elem<T>::VEC;
  const int ppr = ncols / VEC;
  for (int idx = threadIdx.x; idx < 64 * ppr; idx += 512) {
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
    for (int j = 0; j < VEC; ++j) dst[r * ld + c + j] = (r < rows) ? f[j] * sc : 0.f;
  }
}

template <int NBT>
__device__ inline void stage_w(float* sW, const float* W, int nb) {
  using P = PerfBwdPlan<NBT>;
  for (int i = threadIdx.x; i < P::NBP * P::LDW; i += P::NTH) {
    const int r = i / P::LDW, c = i - r * P::LDW;
    sW[i] = (r < nb && c < P::D) ? W[r * P::D + c] : 0.f;
  }
}

// phi(Q) -> sP, phi(K) -> sKf from the staged chunk (sX: Q then K, 64 x LDX each) and sW; one (matrix, row block) per wave.
// The ReLU mask of matrix `mask_of` (0: Q, 1: K) is kept as one ballot per (row block, feature block, register).
template <int NBT>
__device__ inline void feature_maps(const float* sX, const float* sW, float* sP, float* sKf, unsigned long long* sMask, int mask_of,
                                    int rows, int nb, float cnorm) {
  using P = PerfBwdPlan<NBT>;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  const int which = wv >> 2, ib = wv & 3;
  const float* src = sX + which * P::C * P::LDX;
  f4 acc[NBT];
#pragma unroll
  for (int jb = 0; jb < NBT; ++jb) acc[jb] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int ks = 0; ks < P::D / 4; ++ks) {
    const float a = src[(ib * 16 + li) * P::LDX + ks * 4 + lg];
#pragma unroll
    for (int jb = 0; jb < NBT; ++jb) acc[jb] = SEA_BWD_MFMA(a, sW[(jb * 16 + li) * P::LDW + ks * 4 + lg], acc[jb]);
  }
  float* dst = which ? sKf : sP;
#pragma unroll
  for (int jb = 0; jb < NBT; ++jb) {
    const int col = jb * 16 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ib * 16 + lg * 4 + r;
      const bool live = col < nb && row < rows;
      dst[row * P::LDP + col] = live ? fmaxf(cnorm * acc[jb][r], 0.f) + 1e-3f : 0.f;
      const unsigned long long m = __ballot(live && acc[jb][r] > 0.f);
      if (which == mask_of && lane == 0) sMask[(ib * NBT + jb) * 4 + r] = m;
    }
  }
}

// lower-triangular 16 x 16 tiles of X Y^T (X, Y: 64 x K in LDS), + add[row], zero above the diagonal -> sT (64 x LDT)
template <int NBT, typename ADD>
__device__ inline void tril_tiles(float* sT, const float* sXm, int ldx, const float* sYm, int ldy, int K, ADD add) {
  using P = PerfBwdPlan<NBT>;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  for (int tile = wv; tile < 10; tile += P::NW) {
    int ib = 0, rem = tile;
    while (rem > ib) { rem -= ib + 1; ++ib; }
    const int jb = rem;
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < K / 4; ++ks)
      acc = SEA_BWD_MFMA(sXm[(ib * 16 + li) * ldx + ks * 4 + lg], sYm[(jb * 16 + li) * ldy + ks * 4 + lg], acc);
    const int col = jb * 16 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ib * 16 + lg * 4 + r;
      sT[row * P::LDT + col] = (col <= row) ? acc[r] + add(row) : 0.f;
    }
  }
}

// state[f][col] += sum over the chunk rows of F[row][f] * X[row][col]   (NBP x E; wave wv owns column block wv)
template <int NBT>
__device__ inline void state_update(float* sS, const float* sF, const float* sXm) {
  using P = PerfBwdPlan<NBT>;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int fb = 0; fb < NBT; ++fb) {
    f4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = sS[(fb * 16 + lg * 4 + r) * P::LDV + wv * 16 + li];
#pragma unroll 4
    for (int ks = 0; ks < P::C / 4; ++ks)
      acc = SEA_BWD_MFMA(sF[(ks * 4 + lg) * P::LDP + fb * 16 + li], sXm[(ks * 4 + lg) * P::LDV + wv * 16 + li], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) sS[(fb * 16 + lg * 4 + r) * P::LDV + wv * 16 + li] = acc[r];
  }
}

// out[t0 + row][0..D) = cnorm * (sDm (64 x NBP, already masked) W), rows below `rows`
template <typename T, int NBT>
__device__ inline void project_back(T* out, const float* sDm, const float* sW, int t0, int rows, float cnorm) {
  using P = PerfBwdPlan<NBT>;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  for (int tile = wv; tile < 16; tile += P::NW) {
    const int ib = tile >> 2, cb = tile & 3;
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int ks = 0; ks < P::NBP / 4; ++ks)
      acc = SEA_BWD_MFMA(sDm[(ib * 16 + li) * P::LDP + ks * 4 + lg], sW[(ks * 4 + lg) * P::LDW + cb * 16 + li], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ib * 16 + lg * 4 + r;
      if (row < rows) out[(int64_t)(t0 + row) * P::D + cb * 16 + li] = from_f<T>(cnorm * acc[r]);
    }
  }
}

template <typename T, int NBT>
__global__ __launch_bounds__(512) void performer_bwd_fwd_sweep(PerfBwdParams p) {
  using P = PerfBwdPlan<NBT>;
  constexpr int D = P::D, E = P::E, C = P::C, NBP = P::NBP, LDP = P::LDP, LDV = P::LDV, LDT = P::LDT, NW = P::NW;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *sS = smem + P::oState, *sP = smem + P::oP, *sKf = smem + P::oK, *sV = smem + P::oV, *sG = smem + P::oG;
  float *sZ = smem + P::oSum, *sInv = smem + P::oInv, *sE = smem + P::oE, *sPart = smem + P::oPart, *sPartG = smem + P::oPartG;
  unsigned long long* sMask = reinterpret_cast<unsigned long long*>(smem + P::oMask);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int nh = blockIdx.x, n = nh / p.H, h = nh - n * p.H, T_ = p.T;
  const T* qb = reinterpret_cast<const T*>(p.q) + n * p.qs[0] + h * p.qs[1];
  const T* kb = reinterpret_cast<const T*>(p.k) + n * p.ks[0] + h * p.ks[1];
  const T* vb = reinterpret_cast<const T*>(p.v) + n * p.vs[0] + h * p.vs[1];
  const T* pb = reinterpret_cast<const T*>(p.pos);
  const T* gb = reinterpret_cast<const T*>(p.g) + (int64_t)nh * T_ * (3 * D);
  T* dqb = reinterpret_cast<T*>(p.dq) + (int64_t)nh * T_ * D;
  float* rs = p.rowstat + (int64_t)nh * T_ * 2;
  const float cnorm = powf((float)D, -0.25f);
  auto one = [](int) { return 1.f; };

  for (int i = tid; i < NBP * LDV; i += P::NTH) sS[i] = 0.f;
  if (tid < NBP) sZ[tid] = 0.f;
  stage_w<NBT>(sG, p.W, p.nb);                                       // W sits in the G region across the chunk boundary
  __syncthreads();

  for (int t0 = 0; t0 < T_; t0 += C) {
    const int rows = min(C, T_ - t0);
    // ---- 1: Q, K -> the V region; a, b and the mask of q
    stage_rows<T>(sV, P::LDX, qb, p.qs[2], t0, rows, D, one);
    stage_rows<T>(sV + C * P::LDX, P::LDX, kb, p.ks[2], t0, rows, D, one);
    __syncthreads();
    feature_maps<NBT>(sV, sG, sP, sKf, sMask, 0, rows, p.nb, cnorm);
    __syncthreads();
    // ---- 2: A = tril(a b^T) -> the G region (W is done); V = [pos | v]
    tril_tiles<NBT>(sG, sP, LDP, sKf, LDP, NBP, [](int) { return 0.f; });
    stage_rows<T>(sV, LDV, pb, p.pos_stride, t0, rows, D, one);
    stage_rows<T>(sV + D, LDV, vb, p.vs[2], t0, rows, D, one);
    __syncthreads();
    // ---- 3: den = A 1 + a . (z + 1e-6) and g . num with num = A V + a S, neither stored
    {
      const int row = tid & 63, part = tid >> 6;
      float s = 0.f;
      for (int c = part * 8; c < part * 8 + 8; ++c) s += (c <= row) ? sG[row * LDT + c] : 0.f;
      constexpr int per = (NBP + 7) / 8;
      for (int f = part * per; f < min(NBP, (part + 1) * per); ++f) s = fmaf(sP[row * LDP + f], sZ[f] + 1e-6f, s);
      sPart[row * 8 + part] = s;
    }
    for (int ib = 0; ib < 4; ++ib) {                                 // wave wv owns column block wv of the E columns
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < 4 * (ib + 1); ++ks)
        acc = SEA_BWD_MFMA(sG[(ib * 16 + li) * LDT + ks * 4 + lg], sV[(ks * 4 + lg) * LDV + wv * 16 + li], acc);
#pragma unroll 4
      for (int ks = 0; ks < NBP / 4; ++ks)
        acc = SEA_BWD_MFMA(sP[(ib * 16 + li) * LDP + ks * 4 + lg], sS[(ks * 4 + lg) * LDV + wv * 16 + li], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ib * 16 + lg * 4 + r;
        float s = (row < rows) ? Elem<T>::to_f(gb[(int64_t)(t0 + row) * (3 * D) + wv * 16 + li]) * acc[r] : 0.f;
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
        if (li == 0) sPartG[row * 8 + wv] = s;
      }
    }
    __syncthreads();
    if (tid < C) {
      float den = 0.f, gn = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) { den += sPart[tid * 8 + i]; gn += sPartG[tid * 8 + i]; }
      float inv = 0.f, c = 0.f;
      if (tid < rows) {
        inv = 1.f / den;
        c = gn * inv * inv;                                          // g . ctx / den
        rs[(int64_t)(t0 + tid) * 2] = inv;
        rs[(int64_t)(t0 + tid) * 2 + 1] = c;
      }
      sInv[tid] = inv;
      sE[tid] = -c;
    }
    __syncthreads();
    // ---- 4: G = g[:E] / den -> the G region (A is done); B = tril(G V^T + e) -> the P region (a is done)
    stage_rows<T>(sG, LDV, gb, 3 * D, t0, rows, E, [&](int r) { return sInv[r]; });
    __syncthreads();
    tril_tiles<NBT>(sP, sG, LDV, sV, LDV, E, [&](int row) { return sE[row]; });
    __syncthreads();
    // ---- 5: da = B b + G S^T + e (z + 1e-6), masked, held in registers until every wave has read B
    constexpr int NT = (4 * NBT + NW - 1) / NW;
    f4 da[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wv + NW * i;
      da[i] = f4{0.f, 0.f, 0.f, 0.f};
      if (tile < 4 * NBT) {
        const int ib = tile / NBT, fb = tile - ib * NBT;
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < 4 * (ib + 1); ++ks)
          acc = SEA_BWD_MFMA(sP[(ib * 16 + li) * LDT + ks * 4 + lg], sKf[(ks * 4 + lg) * LDP + fb * 16 + li], acc);
#pragma unroll 4
        for (int ks = 0; ks < E / 4; ++ks)
          acc = SEA_BWD_MFMA(sG[(ib * 16 + li) * LDV + ks * 4 + lg], sS[(fb * 16 + li) * LDV + ks * 4 + lg], acc);
        const float zf = sZ[fb * 16 + li] + 1e-6f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool on = (sMask[(ib * NBT + fb) * 4 + r] >> lane) & 1ull;
          da[i][r] = on ? fmaf(sE[ib * 16 + lg * 4 + r], zf, acc[r]) : 0.f;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wv + NW * i;
      if (tile < 4 * NBT) {
        const int ib = tile / NBT, fb = tile - ib * NBT;
#pragma unroll
        for (int r = 0; r < 4; ++r) sP[(ib * 16 + lg * 4 + r) * LDP + fb * 16 + li] = da[i][r];
      }
    }
    // ---- 6: S += b^T V, z += sum b
    state_update<NBT>(sS, sKf, sV);
    if (tid < NBP) {
      float s = sZ[tid];
      for (int r = 0; r < C; ++r) s += sKf[r * LDP + tid];
      sZ[tid] = s;
    }
    __syncthreads();
    // ---- 7: W -> the G region (G is done), dq = s da W
    stage_w<NBT>(sG, p.W, p.nb);
    __syncthreads();
    project_back<T, NBT>(dqb, sP, sG, t0, rows, cnorm);
    // (the barrier after the next chunk's staging stands between these reads of da and the next a)
  }
}

template <typename T, int NBT>
__global__ __launch_bounds__(512) void performer_bwd_rev_sweep(PerfBwdParams p) {
  using P = PerfBwdPlan<NBT>;
  constexpr int D = P::D, E = P::E, C = P::C, NBP = P::NBP, LDP = P::LDP, LDV = P::LDV, LDT = P::LDT, NW = P::NW;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *sR = smem + P::oState, *sP = smem + P::oP, *sKf = smem + P::oK, *sV = smem + P::oV, *sG = smem + P::oG;
  float *sr = smem + P::oSum, *sInv = smem + P::oInv, *sE = smem + P::oE;
  unsigned long long* sMask = reinterpret_cast<unsigned long long*>(smem + P::oMask);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int nh = blockIdx.x, n = nh / p.H, h = nh - n * p.H, T_ = p.T;
  const T* qb = reinterpret_cast<const T*>(p.q) + n * p.qs[0] + h * p.qs[1];
  const T* kb = reinterpret_cast<const T*>(p.k) + n * p.ks[0] + h * p.ks[1];
  const T* vb = reinterpret_cast<const T*>(p.v) + n * p.vs[0] + h * p.vs[1];
  const T* pb = reinterpret_cast<const T*>(p.pos);
  const T* gb = reinterpret_cast<const T*>(p.g) + (int64_t)nh * T_ * (3 * D);
  T* dkb = reinterpret_cast<T*>(p.dk) + (int64_t)nh * T_ * D;
  T* dvb = reinterpret_cast<T*>(p.dv) + (int64_t)nh * T_ * D;
  float* dpp = p.dpos_part + (int64_t)nh * T_ * D;
  const float* rs = p.rowstat + (int64_t)nh * T_ * 2;
  const float cnorm = powf((float)D, -0.25f);
  auto one = [](int) { return 1.f; };

  for (int i = tid; i < NBP * LDV; i += P::NTH) sR[i] = 0.f;
  if (tid < NBP) sr[tid] = 0.f;
  stage_w<NBT>(sG, p.W, p.nb);
  __syncthreads();

  for (int t0 = ((T_ - 1) / C) * C; t0 >= 0; t0 -= C) {              // the partial chunk first
    const int rows = min(C, T_ - t0);
    // ---- 1: Q, K -> the V region; a, b and the mask of k
    stage_rows<T>(sV, P::LDX, qb, p.qs[2], t0, rows, D, one);
    stage_rows<T>(sV + C * P::LDX, P::LDX, kb, p.ks[2], t0, rows, D, one);
    __syncthreads();
    feature_maps<NBT>(sV, sG, sP, sKf, sMask, 1, rows, p.nb, cnorm);
    if (tid < C) {
      sInv[tid] = (tid < rows) ? rs[(int64_t)(t0 + tid) * 2] : 0.f;
      sE[tid] = (tid < rows) ? -rs[(int64_t)(t0 + tid) * 2 + 1] : 0.f;
    }
    __syncthreads();
    // ---- 2: A = tril(a b^T) -> the V region (the staging is done); G = g[:E] / den -> the G region (W is done)
    tril_tiles<NBT>(sV, sP, LDP, sKf, LDP, NBP, [](int) { return 0.f; });
    stage_rows<T>(sG, LDV, gb, 3 * D, t0, rows, E, [&](int r) { return sInv[r]; });
    __syncthreads();
    // ---- 3: dV = A^T G + b R: dpos part and dv leave from the registers (wave wv owns column block wv)
    for (int ib = 0; ib < 4; ++ib) {
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      for (int ks = 4 * ib; ks < C / 4; ++ks)                        // rows t of the blocks at and below the diagonal
        acc = SEA_BWD_MFMA(sV[(ks * 4 + lg) * LDT + ib * 16 + li], sG[(ks * 4 + lg) * LDV + wv * 16 + li], acc);
#pragma unroll 4
      for (int ks = 0; ks < NBP / 4; ++ks)
        acc = SEA_BWD_MFMA(sKf[(ib * 16 + li) * LDP + ks * 4 + lg], sR[(ks * 4 + lg) * LDV + wv * 16 + li], acc);
      const int col = wv * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ib * 16 + lg * 4 + r;
        if (row < rows) {
          const int64_t t = t0 + row;
          if (col < D) dpp[t * D + col] = acc[r];
          else dvb[t * D + col - D] = from_f<T>(acc[r] + Elem<T>::to_f(gb[t * (3 * D) + E + col - D]));
        }
      }
    }
    __syncthreads();
    // ---- 4: V -> the V region (A is done); B = tril(G V^T + e) -> the Kf region (b is done)
    stage_rows<T>(sV, LDV, pb, p.pos_stride, t0, rows, D, one);
    stage_rows<T>(sV + D, LDV, vb, p.vs[2], t0, rows, D, one);
    __syncthreads();
    tril_tiles<NBT>(sKf, sG, LDV, sV, LDV, E, [&](int row) { return sE[row]; });
    __syncthreads();
    // ---- 5: db = B^T a + V R^T + r, masked, held in registers until every wave has read V
    constexpr int NT = (4 * NBT + NW - 1) / NW;
    f4 db[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wv + NW * i;
      db[i] = f4{0.f, 0.f, 0.f, 0.f};
      if (tile < 4 * NBT) {
        const int ib = tile / NBT, fb = tile - ib * NBT;
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
        for (int ks = 4 * ib; ks < C / 4; ++ks)
          acc = SEA_BWD_MFMA(sKf[(ks * 4 + lg) * LDT + ib * 16 + li], sP[(ks * 4 + lg) * LDP + fb * 16 + li], acc);
#pragma unroll 4
        for (int ks = 0; ks < E / 4; ++ks)
          acc = SEA_BWD_MFMA(sV[(ib * 16 + li) * LDV + ks * 4 + lg], sR[(fb * 16 + li) * LDV + ks * 4 + lg], acc);
        const float rf = sr[fb * 16 + li];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool on = (sMask[(ib * NBT + fb) * 4 + r] >> lane) & 1ull;
          db[i][r] = on ? acc[r] + rf : 0.f;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wv + NW * i;
      if (tile < 4 * NBT) {
        const int ib = tile / NBT, fb = tile - ib * NBT;
#pragma unroll
        for (int r = 0; r < 4; ++r) sV[(ib * 16 + lg * 4 + r) * LDP + fb * 16 + li] = db[i][r];
      }
    }
    // ---- 6: R += a^T G, r += a^T e
    state_update<NBT>(sR, sP, sG);
    if (tid < NBP) {
      float s = sr[tid];
      for (int r = 0; r < C; ++r) s = fmaf(sP[r * LDP + tid], sE[r], s);
      sr[tid] = s;
    }
    __syncthreads();
    // ---- 7: W -> the G region (G is done), dk = s db W
    stage_w<NBT>(sG, p.W, p.nb);
    __syncthreads();
    project_back<T, NBT>(dkb, sV, sG, t0, rows, cnorm);
    __syncthreads();                                                 // db is read from the V region, which the next staging writes
  }
}

__global__ __launch_bounds__(256) void performer_bwd_dpos(const float* part, float* dpos, int64_t pairs, int64_t TD) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= TD) return;
  float s = 0.f;
  for (int64_t j = 0; j < pairs; ++j) s += part[j * TD + i];        // the order of (n, h): the same bits every run
  dpos[i] = s;
}

template <typename T, int NBT>
int launch_bwd(const PerfBwdParams& p, int64_t pairs, hipStream_t s) {
  using P = PerfBwdPlan<NBT>;
  static DevOnce once;
  if (once.first()) {
    SEA_MAX_LDS((performer_bwd_fwd_sweep<T, NBT>), P::lds_bytes);
    SEA_MAX_LDS((performer_bwd_rev_sweep<T, NBT>), P::lds_bytes);
  }
  hipLaunchKernelGGL((performer_bwd_fwd_sweep<T, NBT>), dim3((unsigned)pairs), dim3(512), P::lds_bytes, s, p);
  hipLaunchKernelGGL((performer_bwd_rev_sweep<T, NBT>), dim3((unsigned)pairs), dim3(512), P::lds_bytes, s, p);
  return SEA_OK;
}

template <typename T>
int launch_bwd_nbt(const PerfBwdParams& p, int64_t pairs, hipStream_t s) {
  return p.nb <= 48 ? launch_bwd<T, 3>(p, pairs, s) : launch_bwd<T, 5>(p, pairs, s);
}

bool bwd_supported(int64_t D, int64_t nb, int dtype) {
  return D == 64 && nb >= 1 && nb <= 80 && (dtype == SEA_F32 || dtype == SEA_F16 || dtype == SEA_BF16);
}

int64_t align16(int64_t b) { return (b + 15) / 16 * 16; }
int64_t rowstat_bytes(int64_t N, int64_t H, int64_t T) { return align16(N * H * T * 2 * (int64_t)sizeof(float)); }

}  // namespace
}  // namespace sea

using namespace sea;

extern "C" int sea_estimator_grad_version(void) { return SEA_ESTIMATOR_GRAD_ABI_VERSION; }

extern "C" int sea_performer_causal_bwd_supported(int64_t D, int64_t nb, int dtype) { return bwd_supported(D, nb, dtype) ? 1 : 0; }

extern "C" int64_t sea_performer_causal_bwd_workspace_bytes(int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb, int dtype) {
  if (N <= 0 || H <= 0 || T <= 0 || !bwd_supported(D, nb, dtype)) return 0;
  return rowstat_bytes(N, H, T) + align16(N * H * T * D * (int64_t)sizeof(float));
}

extern "C" int sea_performer_causal_bwd(const void* q, const void* k, const void* v, const void* pos, int dtype, const float* proj,
                                        int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb,
                                        const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                        int64_t pos_stride, const void* grad_out, void* d_q, void* d_k, void* d_v, float* d_pos,
                                        void* workspace, int64_t workspace_bytes, sea_stream_t stream) {
  const char* nm = "sea_performer_causal_bwd";
#define SEA_BWD_NONNULL(x) SEA_REQUIRE((x) != nullptr, SEA_EINVAL, "%s: " #x " is null", nm)
  SEA_BWD_NONNULL(q); SEA_BWD_NONNULL(k); SEA_BWD_NONNULL(v); SEA_BWD_NONNULL(pos); SEA_BWD_NONNULL(proj);
  SEA_BWD_NONNULL(q_strides); SEA_BWD_NONNULL(k_strides); SEA_BWD_NONNULL(v_strides);
  SEA_BWD_NONNULL(grad_out); SEA_BWD_NONNULL(d_q); SEA_BWD_NONNULL(d_k); SEA_BWD_NONNULL(d_v); SEA_BWD_NONNULL(d_pos);
  SEA_BWD_NONNULL(workspace);
#undef SEA_BWD_NONNULL
  SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: unknown dtype %d", nm, dtype);
  SEA_REQUIRE(N > 0 && H > 0 && T > 0 && D > 0 && nb > 0, SEA_EINVAL, "%s: bad shape N=%lld H=%lld T=%lld D=%lld nb=%lld", nm,
              (long long)N, (long long)H, (long long)T, (long long)D, (long long)nb);
  SEA_REQUIRE(D == 64, SEA_EUNSUPPORTED, "%s: D=%lld has no backward kernel (D = 64)", nm, (long long)D);
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
  const int64_t need = sea_performer_causal_bwd_workspace_bytes(N, H, T, D, nb, dtype);
  SEA_REQUIRE(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need, SEA_EINVAL,
              "%s: workspace of %lld bytes needed (16-byte aligned), got %lld", nm, (long long)need, (long long)workspace_bytes);

  PerfBwdParams p;
  p.q = q; p.k = k; p.v = v; p.pos = pos; p.g = grad_out; p.W = proj; p.dq = d_q; p.dk = d_k; p.dv = d_v;
  p.rowstat = reinterpret_cast<float*>(workspace);
  p.dpos_part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + rowstat_bytes(N, H, T));
  for (int i = 0; i < 3; ++i) { p.qs[i] = q_strides[i]; p.ks[i] = k_strides[i]; p.vs[i] = v_strides[i]; }
  p.pos_stride = pos_stride;
  p.H = (int)H; p.T = (int)T; p.nb = (int)nb;
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == SEA_F32 ? launch_bwd_nbt<float>(p, N * H, s)
               : dtype == SEA_F16 ? launch_bwd_nbt<__half>(p, N * H, s) : launch_bwd_nbt<__hip_bfloat16>(p, N * H, s);
  if (rc != SEA_OK) return rc;
  SEA_CHECK_LAUNCH(nm);
  const int64_t TD = T * D;
  hipLaunchKernelGGL(performer_bwd_dpos, dim3((unsigned)((TD + 255) / 256)), dim3(256), 0, s, p.dpos_part, d_pos, N * H, TD);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}
