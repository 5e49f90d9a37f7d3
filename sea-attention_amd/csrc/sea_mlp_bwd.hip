// Backward of the predictor MLP (csrc/sea_mlp.hip), gfx950, 16-bit data: include/sea_hip_predictor_mlp_grad.h, entry m1.
//
// The chain per row x = performer_value[n, h, t, :] (r16 = round to the data type, the modules' 16-bit outputs):
//   a1 = r16(W1 x + b1)   xh1 = (a1 - mean1) rstd1   u = xh1 g1 + be1   enc = r16(gelu_erf(u))
//   dec = r16(W2 enc + b2)   per half s: xh2 = (dec_s - mean2) rstd2   y[2h+s] = r16(xh2 g2 + be2)
// Nothing of it is saved: the backward recomputes it from x with the forward's own expressions (predictor_mlp_kernel), so the
// recomputed enc has the forward's bits, and differentiates with the roundings straight-through.
//
// Launches (no atomics; every grid and block size is a function of the shapes alone, so the same inputs give the same bits):
//   mlp_bwd_pack_kernel   the transposed weight images as MFMA A fragments into the head of the workspace, from the forward's own
//                         images: W2T (M = D1, K = the 2 WdP padded decoder rows, K permuted as the forward's decoder image so that
//                         a packed accumulator IS the B operand) and W1T (M = Din, K = D1, natural K: its B operand comes from memory).
//   mlp_bwd_row_kernel    persistent workgroups of 4 waves (one per SIMD, 512 registers each), W1, W2 (without the gate tile),
//                         W2T and the fp32 vectors in LDS (112.5 KB at Din = 192, Wd = 64).  A wave owns 16 consecutive rows of the flattened (n, t, h) order (the
//                         forward's PACK order) and keeps the whole chain in registers: products are computed TRANSPOSED
//                         (D^T = W . X^T), a lane holds 4 consecutive features of ONE row, a LayerNorm reduction is an in-lane sum
//                         plus two cross-lane adds, and a rounded, packed accumulator is the next product's B operand:
//                         d_dec -> W2T . d_dec^T -> d_enc with no LDS transpose.  g_y is read from C8 in the lane's own 4-byte
//                         (split 0, split 1) pairs.  Writes enc, d_dec, d_a1 (16 bit) to the workspace; the LayerNorm gains' and
//                         biases' gradients stay in registers per lane across the workgroup's items, are added over the 16 lanes of a
//                         DPP row, then over the waves in wave order, and leave as one part per workgroup.
//   mlp_bwd_dx_kernel     d_x = W1T . d_a1^T, the 48 KB W1T image in LDS, d_a1 rows loaded as the forward loads x; skipped when
//                         d_x is null.
//   mlp_bwd_wgrad_kernel  split-K GEMMs with the rows as K: dW1 = d_a1^T x (grid y = 0), dW2 = d_dec^T enc (y = 1).  32-row slabs of
//                         both operands go global -> registers -> LDS in a C8-like image [feature block][row][8] and are turned by
//                         ds_read_b64_tr_b16 (8 consecutive rows of one feature per lane); the next slab's loads fly under the
//                         current slab's MFMAs; a ragged slab is zero-filled.  Wave w owns the 16 output rows of M tile w and all
//                         N tiles, accumulators resident across the block's rows; one more N tile whose B operand is the constant
//                         1 gives the column sums d_b1 / d_b2 out of the same staged operand.
//                         Rows per block: mlp_bwd_wgrad_rows(rows) = max(256, 32 ceil(rows / 8192)).
//   mlp_bwd_reduce        adds the parts in block order and writes the outputs in the modules' own row order (halves un-padded).
#include "sea_common.hpp"
#include "../../include/sea_hip_predictor_mlp_grad.h"

namespace sea {
namespace {

typedef __attribute__((ext_vector_type(4))) float mf4;
typedef __attribute__((ext_vector_type(8))) __bf16 mbf8;
typedef __attribute__((ext_vector_type(8))) _Float16 mh8;
typedef short mb_s4 __attribute__((ext_vector_type(4)));

template <typename T> __device__ inline mf4 mb_mfma(const uint4& a, const uint4& b, mf4 c);
template <> __device__ inline mf4 mb_mfma<__hip_bfloat16>(const uint4& a, const uint4& b, mf4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mbf8, a), __builtin_bit_cast(mbf8, b), c, 0, 0, 0);
}
template <> __device__ inline mf4 mb_mfma<__half>(const uint4& a, const uint4& b, mf4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(mh8, a), __builtin_bit_cast(mh8, b), c, 0, 0, 0);
}
template <typename T> __device__ inline float mb_round16(float x) { return Elem<T>::to_f(from_f<T>(x)); }
// the 16-bit pattern in the low half of v as a float
template <typename T> __device__ inline float mb_lo16(uint32_t v) {
  return Elem<T>::to_f(__builtin_bit_cast(T, (unsigned short)(v & 0xffffu)));
}
template <typename T> __device__ inline void mb_unpack4(const uint2& v, float (&f)[4]) {
  f[0] = mb_lo16<T>(v.x); f[1] = mb_lo16<T>(v.x >> 16); f[2] = mb_lo16<T>(v.y); f[3] = mb_lo16<T>(v.y >> 16);
}
// sum over the 16 lanes of a DPP row (lanes 16 g .. 16 g + 15: the 16 rows of a tile that hold the same features)
__device__ inline float mb_row16_sum(float v) {
  v += __uint_as_float(dpp_u32<0xB1>(__float_as_uint(v)));
  v += __uint_as_float(dpp_u32<0x4E>(__float_as_uint(v)));
  v += __uint_as_float(dpp_u32<0x141>(__float_as_uint(v)));
  v += __uint_as_float(dpp_u32<0x140>(__float_as_uint(v)));
  return v;
}

constexpr int MB_D1 = 128, MB_NT1 = 8, MB_KS2 = 4, MB_WAVES = 8, MB_THREADS = MB_WAVES * 64, MB_MAX_GRID = 256;
// the row kernel runs 4 waves per workgroup, one per SIMD: the chain's accumulators (a1, d_enc, the four vector gradients: 200
// registers at Wd = 64) with the fragments in flight do not fit the 256 registers two waves per SIMD leave each, and no
// instantiation may touch scratch
constexpr int MB_ROW_WAVES = 4, MB_ROW_THREADS = MB_ROW_WAVES * 64;
constexpr int MB_MAX_LDS = 160 * 1024;
constexpr int MB_SLAB = 32, MB_BS = MB_SLAB * 16 + 16;        // rows of a slab; bytes of one 8-feature block of it in LDS (+16: banks)

struct MlpBwdParams {
  const void* x;            // (N, H, T, Din), Din contiguous
  int64_t xs_n, xs_h, xs_t;
  const void* gy;           // C8 (N, T, H/4, Wd, 8)
  const void* gtp;          // optional (N, H, T, D1)
  const void *w1p, *w2p;    // the forward's images
  const float* vec;         // b1[D1] g1[D1] be1[D1] b2[2 WdP] g2[WdP] be2[WdP] (bsc[2])
  void *w2t, *w1t;          // workspace: [HT][8][64][8], [4][Din/16][64][8]
  void *enc, *ddec, *da1;   // workspace: (rows, D1), (rows, 2 WdP), (rows, D1)
  float* rpart;             // (row grid, 2 D1 + 2 WdP): dg1, dbe1, dg2, dbe2
  float* wpart;             // (wgrad blocks, D1 (Din + 1) + 2 WdP (D1 + 1)): [dW1 | db1], [dW2 | db2] on padded decoder rows
  void* dx;
  int N, H, T, Din, KS1, Wd, HT, rows, wrows, wblocks, rgrid;
  float eps1, eps2;
};

// ---- the row kernel ------------------------------------------------------------------------------------------------------
template <typename T, int HT>
__global__ __launch_bounds__(MB_ROW_THREADS) void mlp_bwd_row_kernel(MlpBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NT1 = MB_NT1, D1 = MB_D1, KS2 = MB_KS2, NT2 = 2 * HT, D2P = NT2 * 16, WdP = HT * 16;
  constexpr int NVEC = 3 * D1 + D2P + 2 * WdP, NV = 2 * D1 + 2 * WdP;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int Wd = p.Wd;
  T* sW1 = reinterpret_cast<T*>(smem);                                   // KS1 * NT1 fragments of 512 elements
  T* sW2 = sW1 + (size_t)p.KS1 * NT1 * 512;                              // KS2 * NT2
  T* sW2T = sW2 + (size_t)KS2 * NT2 * 512;                               // HT * NT1
  float* sV = reinterpret_cast<float*>(sW2T + (size_t)HT * NT1 * 512);
  {
    const uint4* g1 = reinterpret_cast<const uint4*>(p.w1p);
    const uint4* g2 = reinterpret_cast<const uint4*>(p.w2p);
    const uint4* g3 = reinterpret_cast<const uint4*>(p.w2t);
    for (int i = threadIdx.x; i < p.KS1 * NT1 * 64; i += MB_ROW_THREADS) reinterpret_cast<uint4*>(sW1)[i] = g1[i];
    for (int i = threadIdx.x; i < KS2 * NT2 * 64; i += MB_ROW_THREADS) {     // the forward's image has NT2 + 1 tiles per k-step: the gates
      const int ks = i / (NT2 * 64);
      reinterpret_cast<uint4*>(sW2)[i] = g2[i + ks * 64];
    }
    for (int i = threadIdx.x; i < HT * NT1 * 64; i += MB_ROW_THREADS) reinterpret_cast<uint4*>(sW2T)[i] = g3[i];
    for (int i = threadIdx.x; i < NVEC; i += MB_ROW_THREADS) sV[i] = p.vec[i];
  }
  __syncthreads();
  const float* sB1 = sV, *sG1 = sV + D1, *sE1 = sV + 2 * D1;
  const float* sB2 = sV + 3 * D1, *sG2 = sB2 + D2P;
  const T* w1l = sW1 + lane * 8;
  const T* w2l = sW2 + lane * 8;
  const T* w2tl = sW2T + lane * 8;

  // this lane's share of the vector gradients: features 16 i + 4 lg + r, summed over its rows of every item
  float accG1[NT1][4], accB1[NT1][4], accG2[HT][4], accB2[HT][4];
#pragma unroll
  for (int i = 0; i < NT1; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) { accG1[i][r] = 0.f; accB1[i][r] = 0.f; }
#pragma unroll
  for (int i = 0; i < HT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) { accG2[i][r] = 0.f; accB2[i][r] = 0.f; }

  const int nitems = (p.rows + 15) >> 4;
  const int C8 = p.H >> 2;
#pragma unroll 1
  for (int base = blockIdx.x * MB_ROW_WAVES; base < nitems; base += gridDim.x * MB_ROW_WAVES) {
    const int item = base + wv;
    if (item >= nitems) continue;                                        // (wave-uniform; no barrier inside the loop)
    const int R = item * 16 + li;
    const bool hok = R < p.rows;
    const int Rc = hok ? R : 0;
    const int nt_ = Rc / p.H, h = Rc - nt_ * p.H;
    const int n = nt_ / p.T, t = nt_ - n * p.T;
    const T* xr = reinterpret_cast<const T*>(p.x) + n * p.xs_n + h * p.xs_h + t * p.xs_t + 8 * lg;

    // ---- product 1: a1^T = W1 . x^T (the forward's order) ---------------------------------------------
    mf4 acc1[NT1];
#pragma unroll
    for (int i = 0; i < NT1; ++i) acc1[i] = mf4{0.f, 0.f, 0.f, 0.f};
    {
      uint4 xf[8];
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        xf[ks] = make_uint4(0, 0, 0, 0);
        if (ks < p.KS1 && hok) xf[ks] = *reinterpret_cast<const uint4*>(xr + 32 * ks);
      }
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        if (ks < p.KS1) {
          const T* wk = w1l + (size_t)ks * NT1 * 512;
#pragma unroll
          for (int i = 0; i < NT1; ++i)
            acc1[i] = mb_mfma<T>(*reinterpret_cast<const uint4*>(wk + i * 512), xf[ks], acc1[i]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    // the gradient of y: the lane's (split 0, split 1) pair of pixel w = 16 i + 4 lg + r is 4 bytes of block h / 4.  Rows past the
    // end and padded pixels: zero, which makes every gradient of such a row an exact zero below
    uint32_t gp[HT][4];
    {
      const T* gb = reinterpret_cast<const T*>(p.gy) + (((int64_t)n * p.T + t) * C8 + (h >> 2)) * ((int64_t)Wd * 8) + (h & 3) * 2;
#pragma unroll
      for (int i = 0; i < HT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          gp[i][r] = 0u;
          if (hok && i * 16 + lg * 4 < Wd) gp[i][r] = *reinterpret_cast<const uint32_t*>(gb + (i * 16 + lg * 4 + r) * 8);
        }
    }
    // ---- bias, round, LayerNorm(D1) + GELU, round: the forward's expressions --------------------------
    uint4 tb[KS2];
    float mean1, rstd1;
    {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NT1; ++i) {
        const float4 b = *reinterpret_cast<const float4*>(sB1 + i * 16 + lg * 4);
        acc1[i][0] = mb_round16<T>(acc1[i][0] + b.x); acc1[i][1] = mb_round16<T>(acc1[i][1] + b.y);
        acc1[i][2] = mb_round16<T>(acc1[i][2] + b.z); acc1[i][3] = mb_round16<T>(acc1[i][3] + b.w);
        s += (acc1[i][0] + acc1[i][1]) + (acc1[i][2] + acc1[i][3]);
      }
      s = xor32_sum(xor16_sum(s));
      mean1 = s * (1.0f / (float)D1);
      float q2 = 0.f;
#pragma unroll
      for (int i = 0; i < NT1; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float d = acc1[i][r] - mean1; q2 += d * d; }
      q2 = xor32_sum(xor16_sum(q2));
      rstd1 = rsqrtf(q2 * (1.0f / (float)D1) + p.eps1);
#pragma unroll
      for (int i = 0; i < NT1; ++i) {
        const float4 g = *reinterpret_cast<const float4*>(sG1 + i * 16 + lg * 4);
        const float4 e = *reinterpret_cast<const float4*>(sE1 + i * 16 + lg * 4);
        float o[4] = {(acc1[i][0] - mean1) * rstd1 * g.x + e.x, (acc1[i][1] - mean1) * rstd1 * g.y + e.y,
                      (acc1[i][2] - mean1) * rstd1 * g.z + e.z, (acc1[i][3] - mean1) * rstd1 * g.w + e.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = gelu_erf(o[r]);
        const uint32_t p0 = pack2<T>(o[0], o[1]), p1 = pack2<T>(o[2], o[3]);
        if (i & 1) { tb[i >> 1].z = p0; tb[i >> 1].w = p1; } else { tb[i >> 1].x = p0; tb[i >> 1].y = p1; }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (hok) {                                                          // enc for the weight-gradient launch
        T* ep = reinterpret_cast<T*>(p.enc) + (int64_t)R * D1 + lg * 4;
#pragma unroll
        for (int i = 0; i < NT1; ++i)
          *reinterpret_cast<uint2*>(ep + i * 16) = (i & 1) ? make_uint2(tb[i >> 1].z, tb[i >> 1].w) : make_uint2(tb[i >> 1].x, tb[i >> 1].y);
      }
    }
    // ---- product 2: dec^T = W2 . enc^T ------------------------------------------------------------------
    mf4 acc2[NT2];
#pragma unroll
    for (int i = 0; i < NT2; ++i) acc2[i] = mf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks) {
      const T* wk = w2l + (size_t)ks * NT2 * 512;
#pragma unroll
      for (int i = 0; i < NT2; ++i)
        acc2[i] = mb_mfma<T>(*reinterpret_cast<const uint4*>(wk + i * 512), tb[ks], acc2[i]);
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- per half: LayerNorm(Wd) forward statistics, then its backward; d_dec replaces dec in acc2 -----
    const float invWd = 1.0f / (float)Wd;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < HT; ++i) {
        mf4& a = acc2[hf * HT + i];
        const float4 b = *reinterpret_cast<const float4*>(sB2 + (hf * HT + i) * 16 + lg * 4);
        a[0] = mb_round16<T>(a[0] + b.x); a[1] = mb_round16<T>(a[1] + b.y); a[2] = mb_round16<T>(a[2] + b.z); a[3] = mb_round16<T>(a[3] + b.w);
        s += (a[0] + a[1]) + (a[2] + a[3]);
      }
      s = xor32_sum(xor16_sum(s));                                        // (padded features are exact zeros here)
      const float mean = s * invWd;
      float q2 = 0.f;
#pragma unroll
      for (int i = 0; i < HT; ++i) {
        if (i * 16 + lg * 4 < Wd) {                                       // a lane's 4 features are real or padding together
#pragma unroll
          for (int r = 0; r < 4; ++r) { const float d = acc2[hf * HT + i][r] - mean; q2 += d * d; }
        }
      }
      q2 = xor32_sum(xor16_sum(q2));
      const float rstd = rsqrtf(q2 * invWd + p.eps2);
      float s1 = 0.f, s2 = 0.f;                                           // sum dxh, sum dxh xh2 over the real features
#pragma unroll
      for (int i = 0; i < HT; ++i) {
        const float4 g = *reinterpret_cast<const float4*>(sG2 + i * 16 + lg * 4);
        const float gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gv = mb_lo16<T>(hf == 0 ? gp[i][r] : gp[i][r] >> 16);   // zero on padded pixels and rows past the end
          const float xh = (acc2[hf * HT + i][r] - mean) * rstd;
          accG2[i][r] += gv * xh; accB2[i][r] += gv;
          const float dxh = gv * gg[r];
          s1 += dxh; s2 += dxh * xh;
        }
      }
      s1 = xor32_sum(xor16_sum(s1)) * invWd; s2 = xor32_sum(xor16_sum(s2)) * invWd;
#pragma unroll
      for (int i = 0; i < HT; ++i) {
        const float4 g = *reinterpret_cast<const float4*>(sG2 + i * 16 + lg * 4);
        const float gg[4] = {g.x, g.y, g.z, g.w};
        const bool real = i * 16 + lg * 4 < Wd;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gv = mb_lo16<T>(hf == 0 ? gp[i][r] : gp[i][r] >> 16);
          const float xh = (acc2[hf * HT + i][r] - mean) * rstd;
          acc2[hf * HT + i][r] = real ? rstd * (gv * gg[r] - s1 - xh * s2) : 0.f;
        }
      }
    }
    // d_dec rounded once: the B operand of product 3 (tiles 2 ks, 2 ks + 1 = the k-step's 8 values) and the workspace row
    uint4 dd[HT];
#pragma unroll
    for (int ks = 0; ks < HT; ++ks)
      dd[ks] = make_uint4(pack2<T>(acc2[2 * ks][0], acc2[2 * ks][1]), pack2<T>(acc2[2 * ks][2], acc2[2 * ks][3]),
                          pack2<T>(acc2[2 * ks + 1][0], acc2[2 * ks + 1][1]), pack2<T>(acc2[2 * ks + 1][2], acc2[2 * ks + 1][3]));
    if (hok) {
      T* dp = reinterpret_cast<T*>(p.ddec) + (int64_t)R * D2P + lg * 4;
#pragma unroll
      for (int ks = 0; ks < HT; ++ks) {
        *reinterpret_cast<uint2*>(dp + (2 * ks) * 16) = make_uint2(dd[ks].x, dd[ks].y);
        *reinterpret_cast<uint2*>(dp + (2 * ks + 1) * 16) = make_uint2(dd[ks].z, dd[ks].w);
      }
    }
    // ---- product 3: d_enc^T = W2T . d_dec^T (+ the gradient of tpred) -----------------------------------
    mf4 acc3[NT1];
#pragma unroll
    for (int i = 0; i < NT1; ++i) acc3[i] = mf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < HT; ++ks) {
      const T* wk = w2tl + (size_t)ks * NT1 * 512;
#pragma unroll
      for (int i = 0; i < NT1; ++i)
        acc3[i] = mb_mfma<T>(*reinterpret_cast<const uint4*>(wk + i * 512), dd[ks], acc3[i]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (p.gtp != nullptr && hok) {
      const T* tp = reinterpret_cast<const T*>(p.gtp) + (((int64_t)n * p.H + h) * p.T + t) * D1 + lg * 4;
#pragma unroll
      for (int i = 0; i < NT1; ++i) {
        float f[4];
        mb_unpack4<T>(*reinterpret_cast<const uint2*>(tp + i * 16), f);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc3[i][r] += f[r];
      }
    }
    // ---- GELU and LayerNorm(D1) backward; dxh1 replaces d_enc in acc3, then d_a1 -------------------------
    {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < NT1; ++i) {
        const float4 g = *reinterpret_cast<const float4*>(sG1 + i * 16 + lg * 4);
        const float4 e = *reinterpret_cast<const float4*>(sE1 + i * 16 + lg * 4);
        const float gg[4] = {g.x, g.y, g.z, g.w}, ee[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float xh = (acc1[i][r] - mean1) * rstd1;
          const float u = (acc1[i][r] - mean1) * rstd1 * gg[r] + ee[r];
          const float cdf = 0.5f * (1.0f + erf_as(u * 0.70710678118654752f));
          const float pdf = 0.3989422804014327f * __builtin_amdgcn_exp2f(u * u * (-0.5f * 1.4426950408889634f));
          const float du = acc3[i][r] * (cdf + u * pdf);
          accG1[i][r] += du * xh; accB1[i][r] += du;
          const float dxh = du * gg[r];
          s1 += dxh; s2 += dxh * xh;
          acc3[i][r] = dxh;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      s1 = xor32_sum(xor16_sum(s1)) * (1.0f / (float)D1); s2 = xor32_sum(xor16_sum(s2)) * (1.0f / (float)D1);
      T* ap = reinterpret_cast<T*>(p.da1) + (int64_t)R * D1 + lg * 4;
#pragma unroll
      for (int i = 0; i < NT1; ++i) {
        float d[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = rstd1 * (acc3[i][r] - s1 - (acc1[i][r] - mean1) * rstd1 * s2);
        if (hok) *reinterpret_cast<uint2*>(ap + i * 16) = make_uint2(pack2<T>(d[0], d[1]), pack2<T>(d[2], d[3]));
      }
    }
  }

  // ---- the workgroup's part: lanes of a DPP row, then the waves in wave order --------------------------
  __syncthreads();                                                       // every wave is done with the weights
  float* sRed = reinterpret_cast<float*>(smem);                          // [wave][NV]
#pragma unroll
  for (int i = 0; i < NT1; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = mb_row16_sum(accG1[i][r]), b = mb_row16_sum(accB1[i][r]);
      if (li == 0) { sRed[wv * NV + i * 16 + lg * 4 + r] = a; sRed[wv * NV + D1 + i * 16 + lg * 4 + r] = b; }
    }
#pragma unroll
  for (int i = 0; i < HT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = mb_row16_sum(accG2[i][r]), b = mb_row16_sum(accB2[i][r]);
      if (li == 0) { sRed[wv * NV + 2 * D1 + i * 16 + lg * 4 + r] = a; sRed[wv * NV + 2 * D1 + WdP + i * 16 + lg * 4 + r] = b; }
    }
  __syncthreads();
  for (int i = threadIdx.x; i < NV; i += MB_ROW_THREADS) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < MB_ROW_WAVES; ++w) s += sRed[w * NV + i];
    p.rpart[(int64_t)blockIdx.x * NV + i] = s;
  }
}

// ---- d_x = W1T . d_a1^T ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(MB_THREADS) void mlp_bwd_dx_kernel(MlpBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int MT = p.Din >> 4;                                             // tiles of Din: 2 .. 16
  for (int i = threadIdx.x; i < 4 * MT * 64; i += MB_THREADS) reinterpret_cast<uint4*>(smem)[i] = reinterpret_cast<const uint4*>(p.w1t)[i];
  __syncthreads();
  const T* wl = reinterpret_cast<const T*>(smem) + lane * 8;
  const int nitems = (p.rows + 15) >> 4;
#pragma unroll 1
  for (int base = blockIdx.x * MB_WAVES; base < nitems; base += gridDim.x * MB_WAVES) {
    const int item = base + wv;
    if (item >= nitems) continue;
    const int R = item * 16 + li;
    const bool hok = R < p.rows;
    const int Rc = hok ? R : 0;
    const int nt_ = Rc / p.H, h = Rc - nt_ * p.H;
    const int n = nt_ / p.T, t = nt_ - n * p.T;
    uint4 bf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf[ks] = make_uint4(0, 0, 0, 0);
      if (hok) bf[ks] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.da1) + (int64_t)R * MB_D1 + 32 * ks + 8 * lg);
    }
    T* xo = reinterpret_cast<T*>(p.dx) + n * p.xs_n + h * p.xs_h + t * p.xs_t + lg * 4;
#pragma unroll 4
    for (int mt = 0; mt < MT; ++mt) {
      mf4 acc = mf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        acc = mb_mfma<T>(*reinterpret_cast<const uint4*>(wl + (size_t)(ks * MT + mt) * 512), bf[ks], acc);
      if (hok) *reinterpret_cast<uint2*>(xo + mt * 16) = make_uint2(pack2<T>(acc[0], acc[1]), pack2<T>(acc[2], acc[3]));
    }
  }
}

// ---- the weight gradients ------------------------------------------------------------------------------------------------
// one fragment out of a slab image [feature block][row][8]: features 16 tile .. + 16 x rows r0 .. r0 + 8, lane li <-> feature
// (the transposing read of conv_relu_wgrad_kernel; scripts/micro/tr_read_check.hip has the semantics)
__device__ __forceinline__ uint4 mb_tr_frag(const char* slab, int blk0, int r0) {
  const int i = threadIdx.x & 15, q = i >> 2, pp = i & 3;
  const char* a = slab + (blk0 + (pp >> 1)) * MB_BS + (r0 + q) * 16 + (pp & 1) * 8;
  const mb_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mb_s4 __attribute__((address_space(3)))*)(a));
  const mb_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mb_s4 __attribute__((address_space(3)))*)(a + 64));
  const uint2 l = __builtin_bit_cast(uint2, lo), h = __builtin_bit_cast(uint2, hi);
  return make_uint4(l.x, l.y, h.x, h.y);
}

// LDS: the A slab (M / 8 blocks) then the B slab (Nc / 8 blocks), MB_BS bytes per block: 25 344 bytes at M = 128, Nc = 256.
template <typename T>
__global__ __launch_bounds__(MB_THREADS) void mlp_bwd_wgrad_kernel(MlpBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NTMAX = 16;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
  const bool first = blockIdx.y == 0;                                    // dW1 = d_a1^T x, else dW2 = d_dec^T enc
  const int D2P = p.HT * 32;
  const int M = first ? MB_D1 : D2P, Nc = first ? p.Din : MB_D1;
  const int MB8 = M >> 3, NB8 = Nc >> 3, MT = M >> 4, NT = Nc >> 4;
  const T* A = reinterpret_cast<const T*>(first ? p.da1 : p.ddec);
  char* sA = smem;
  char* sB = smem + MB8 * MB_BS;
  const int r0 = (int)blockIdx.x * p.wrows, r1 = min(p.rows, r0 + p.wrows);

  // a thread's units of a slab: A unit tid (row tid / MB8, block tid % MB8), B units tid and tid + 512
  uint4 av, bv[2];
  auto load = [&](int s0) {
    av = make_uint4(0, 0, 0, 0);
    if (tid < MB_SLAB * MB8) {
      const int rr = tid / MB8, blk = tid - rr * MB8;
      if (s0 + rr < r1) av = *reinterpret_cast<const uint4*>(A + (int64_t)(s0 + rr) * M + blk * 8);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int u = tid + MB_THREADS * k, rr = u / NB8, blk = u - rr * NB8, R = s0 + rr;
      bv[k] = make_uint4(0, 0, 0, 0);
      if (u < MB_SLAB * NB8 && R < r1) {
        if (first) {
          const int nt_ = R / p.H, h = R - nt_ * p.H, n = nt_ / p.T, t = nt_ - n * p.T;
          bv[k] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.x) + n * p.xs_n + h * p.xs_h + t * p.xs_t + blk * 8);
        } else {
          bv[k] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.enc) + (int64_t)R * MB_D1 + blk * 8);
        }
      }
    }
  };
  auto put = [&]() {
    if (tid < MB_SLAB * MB8) {
      const int rr = tid / MB8, blk = tid - rr * MB8;
      *reinterpret_cast<uint4*>(sA + blk * MB_BS + rr * 16) = av;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int u = tid + MB_THREADS * k, rr = u / NB8, blk = u - rr * NB8;
      if (u < MB_SLAB * NB8) *reinterpret_cast<uint4*>(sB + blk * MB_BS + rr * 16) = bv[k];
    }
  };
  mf4 acc[NTMAX + 1];
#pragma unroll
  for (int k = 0; k <= NTMAX; ++k) acc[k] = mf4{0.f, 0.f, 0.f, 0.f};
  const uint32_t one2 = pack2<T>(1.0f, 1.0f);
  const uint4 ones = make_uint4(one2, one2, one2, one2);

  load(r0);
#pragma unroll 1
  for (int s0 = r0; s0 < r1; s0 += MB_SLAB) {
    put();
    __syncthreads();
    if (s0 + MB_SLAB < r1) load(s0 + MB_SLAB);                           // in flight under this slab's MFMAs
    if (wv < MT) {                                                       // (wave-uniform)
      const uint4 a = mb_tr_frag(sA, 2 * wv, lg * 8);
#pragma unroll
      for (int nt = 0; nt < NTMAX; ++nt)
        if (nt < NT) acc[nt] = mb_mfma<T>(a, mb_tr_frag(sB, 2 * nt, lg * 8), acc[nt]);
      acc[NTMAX] = mb_mfma<T>(a, ones, acc[NTMAX]);                      // the column sums: d_b
    }
    __syncthreads();
  }
  // D: rows 4 lg + r = A's features (output rows), column li = B's feature; one more column for d_b
  const int PW1 = MB_D1 * (p.Din + 1);
  float* part = p.wpart + (int64_t)blockIdx.x * (PW1 + D2P * (MB_D1 + 1)) + (first ? 0 : PW1);
  if (wv < MT) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* prow = part + (int64_t)(wv * 16 + lg * 4 + r) * (Nc + 1);
#pragma unroll
      for (int nt = 0; nt < NTMAX; ++nt)
        if (nt < NT) prow[nt * 16 + li] = acc[nt][r];
      if (li == 0) prow[Nc] = acc[NTMAX][r];
    }
  }
}

// W2T[ks][m][lane][j] = W2[f(ks, lg, j)][16 m + li], f the forward's K permutation, on the padded decoder rows (the padding rows
// of the forward's image are zero); W1T[ks][mt][lane][j] = W1[32 ks + 8 lg + j][16 mt + li].  Both read from the forward's images.
__global__ __launch_bounds__(256) void mlp_bwd_pack_kernel(const unsigned short* w1p, const unsigned short* w2p, unsigned short* w2t,
                                                           unsigned short* w1t, int HT, int MT1) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int n2 = HT * MB_NT1 * 512, n1 = 4 * MT1 * 512;
  if (idx >= n2 + n1) return;
  const int e = idx < n2 ? idx : idx - n2;
  const int j = e & 7, lane = (e >> 3) & 63, li = lane & 15, lg = lane >> 4, frag = e >> 9;
  if (idx < n2) {
    const int ks = frag / MB_NT1, m = frag - ks * MB_NT1;
    const int R = 16 * (2 * ks + (j >> 2)) + 4 * lg + (j & 3), c = 16 * m + li;
    const int ks_ = c >> 5, j_ = ((c >> 4) & 1) * 4 + (c & 3), lg_ = (c & 15) >> 2;
    w2t[e] = w2p[(((int64_t)ks_ * (2 * HT + 1) + (R >> 4)) * 64 + lg_ * 16 + (R & 15)) * 8 + j_];
  } else {
    const int ks = frag / MT1, mt = frag - ks * MT1;
    const int R = 32 * ks + 8 * lg + j, c = 16 * mt + li;
    w1t[e] = w1p[(((int64_t)(c >> 5) * MB_NT1 + (R >> 4)) * 64 + ((c & 31) >> 3) * 16 + (R & 15)) * 8 + (c & 7)];
  }
}

struct MlpBwdOut { float *d_w1, *d_b1, *d_g1, *d_be1, *d_w2, *d_b2, *d_g2, *d_be2; };

// every output element: the sum of its parts in block order
__global__ __launch_bounds__(256) void mlp_bwd_reduce(MlpBwdParams p, MlpBwdOut o) {
  const int D1 = MB_D1, Din = p.Din, Wd = p.Wd, WdP = p.HT * 16, D2 = 2 * Wd;
  const int NV = 2 * D1 + 2 * WdP;
  const int64_t PW1 = (int64_t)D1 * (Din + 1), PW = PW1 + 2 * WdP * (D1 + 1);
  int i = blockIdx.x * 256 + threadIdx.x;
  const float* src; int64_t stride; int count; float* dst;
  if (i < D1 * Din) { src = p.wpart + (i / Din) * (Din + 1) + i % Din; stride = PW; count = p.wblocks; dst = o.d_w1 + i; }
  else if ((i -= D1 * Din) < D1) { src = p.wpart + i * (Din + 1) + Din; stride = PW; count = p.wblocks; dst = o.d_b1 + i; }
  else if ((i -= D1) < D1) { src = p.rpart + i; stride = NV; count = p.rgrid; dst = o.d_g1 + i; }
  else if ((i -= D1) < D1) { src = p.rpart + D1 + i; stride = NV; count = p.rgrid; dst = o.d_be1 + i; }
  else if ((i -= D1) < D2 * D1) {
    const int Rr = i / D1, pr = (Rr / Wd) * WdP + Rr % Wd;
    src = p.wpart + PW1 + (int64_t)pr * (D1 + 1) + i % D1; stride = PW; count = p.wblocks; dst = o.d_w2 + i;
  } else if ((i -= D2 * D1) < D2) {
    const int pr = (i / Wd) * WdP + i % Wd;
    src = p.wpart + PW1 + (int64_t)pr * (D1 + 1) + D1; stride = PW; count = p.wblocks; dst = o.d_b2 + i;
  } else if ((i -= D2) < Wd) { src = p.rpart + 2 * D1 + i; stride = NV; count = p.rgrid; dst = o.d_g2 + i; }
  else if ((i -= Wd) < Wd) { src = p.rpart + 2 * D1 + WdP + i; stride = NV; count = p.rgrid; dst = o.d_be2 + i; }
  else return;
  float s = 0.f;
  for (int b = 0; b < count; ++b) s += src[b * stride];
  *dst = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
bool mlp_bwd_supported(int64_t D1, int64_t D2, int64_t H, int64_t Din, int dtype) {
  return D1 == MB_D1 && D2 % 16 == 0 && D2 >= 16 && D2 <= 128 && H > 0 && H % 4 == 0 && Din > 0 && Din % 32 == 0 && Din <= 256 &&
         (dtype == SEA_F16 || dtype == SEA_BF16);
}
// rows of one weight-gradient block: the shapes alone decide it, so the parts and their sum are the same on every device
int64_t mlp_bwd_wgrad_rows(int64_t rows) {
  const int64_t r = 32 * ((rows + 8191) / 8192);
  return r < 256 ? 256 : r;
}
int64_t mlp_bwd_row_grid(int64_t rows) {
  const int64_t g = ((rows + 15) / 16 + MB_ROW_WAVES - 1) / MB_ROW_WAVES;
  return g > MB_MAX_GRID ? MB_MAX_GRID : g;
}
struct MlpBwdLayout { int64_t w2t, w1t, enc, ddec, da1, rpart, wpart, total; };
MlpBwdLayout mlp_bwd_layout(int64_t rows, int64_t Din, int64_t D2) {
  const int64_t HT = (D2 / 2 + 15) / 16, WdP = HT * 16;
  const int64_t wcap = (rows + 255) / 256 > MB_MAX_GRID ? MB_MAX_GRID : (rows + 255) / 256;   // >= the blocks of any split, monotone
  MlpBwdLayout l;
  int64_t o = 0;
  l.w2t = o; o += HT * MB_NT1 * 1024;
  l.w1t = o; o += 4 * (Din / 16) * 1024;
  l.enc = o; o += rows * MB_D1 * 2;
  l.ddec = o; o += rows * 2 * WdP * 2;
  l.da1 = o; o += rows * MB_D1 * 2;
  l.rpart = o; o += mlp_bwd_row_grid(rows) * (2 * MB_D1 + 2 * WdP) * 4;
  l.wpart = o; o += wcap * (MB_D1 * (Din + 1) + 2 * WdP * (MB_D1 + 1)) * 4;
  l.total = o;
  return l;
}

template <typename T, int HT>
int launch_row(const MlpBwdParams& p, hipStream_t s) {
  const size_t lds = ((size_t)p.KS1 * MB_NT1 + (size_t)MB_KS2 * 2 * HT + (size_t)HT * MB_NT1) * 1024 +
                     (size_t)(3 * MB_D1 + 4 * HT * 16) * sizeof(float);
  static DevOnce once;
  if (once.first()) SEA_MAX_LDS((mlp_bwd_row_kernel<T, HT>), MB_MAX_LDS);
  hipLaunchKernelGGL((mlp_bwd_row_kernel<T, HT>), dim3((unsigned)p.rgrid), dim3(MB_ROW_THREADS), lds, s, p);
  return SEA_OK;
}
template <typename T>
int launch_all(const MlpBwdParams& p, const MlpBwdOut& o, hipStream_t s, const char* nm) {
  const int MT1 = p.Din / 16, D2 = 2 * p.Wd;
  const int npack = (p.HT * MB_NT1 + 4 * MT1) * 512;
  hipLaunchKernelGGL(mlp_bwd_pack_kernel, dim3((unsigned)((npack + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const unsigned short*>(p.w1p), reinterpret_cast<const unsigned short*>(p.w2p),
                     reinterpret_cast<unsigned short*>(p.w2t), reinterpret_cast<unsigned short*>(p.w1t), p.HT, MT1);
  SEA_CHECK_LAUNCH(nm);
  int rc = p.HT == 1 ? launch_row<T, 1>(p, s) : p.HT == 2 ? launch_row<T, 2>(p, s) : p.HT == 3 ? launch_row<T, 3>(p, s)
                                                                                                 : launch_row<T, 4>(p, s);
  if (rc != SEA_OK) return rc;
  SEA_CHECK_LAUNCH(nm);
  if (p.dx != nullptr) {
    static DevOnce once;
    if (once.first()) SEA_MAX_LDS((mlp_bwd_dx_kernel<T>), MB_MAX_LDS);
    hipLaunchKernelGGL((mlp_bwd_dx_kernel<T>), dim3((unsigned)p.rgrid), dim3(MB_THREADS), (size_t)4 * MT1 * 1024, s, p);
    SEA_CHECK_LAUNCH(nm);
  }
  hipLaunchKernelGGL((mlp_bwd_wgrad_kernel<T>), dim3((unsigned)p.wblocks, 2), dim3(MB_THREADS), (size_t)(MB_D1 / 8 + 256 / 8) * MB_BS, s, p);
  SEA_CHECK_LAUNCH(nm);
  const int nout = MB_D1 * p.Din + 3 * MB_D1 + D2 * MB_D1 + D2 + 2 * p.Wd;
  hipLaunchKernelGGL(mlp_bwd_reduce, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, s, p, o);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}

}  // namespace
}  // namespace sea

using namespace sea;

extern "C" int sea_predictor_mlp_grad_version(void) { return SEA_PREDICTOR_MLP_GRAD_ABI_VERSION; }

extern "C" int sea_predictor_mlp_bwd_supported(int64_t D1, int64_t D2, int64_t H, int64_t Din, int dtype) {
  return mlp_bwd_supported(D1, D2, H, Din, dtype) ? 1 : 0;
}

extern "C" int64_t sea_predictor_mlp_bwd_workspace_bytes(int64_t N, int64_t H, int64_t T, int64_t Din, int64_t D1, int64_t D2, int dtype) {
  if (N <= 0 || H <= 0 || T <= 0 || !mlp_bwd_supported(D1, D2, H, Din, dtype)) return 0;
  if (N >= (1ll << 30) || T >= (1ll << 30) || H >= (1ll << 30) || N * T >= (1ll << 30) || N * T * H >= (1ll << 30)) return 0;
  return mlp_bwd_layout(N * H * T, Din, D2).total;
}

extern "C" int sea_predictor_mlp_bwd(const void* x, const int64_t* x_strides, const void* g_y, const void* g_tpred, int dtype, int64_t N,
                                     int64_t H, int64_t T, int64_t Din, int64_t D1, int64_t D2, const void* w1_packed,
                                     const void* w2_packed, const float* vectors, float eps1, float eps2, void* d_x, float* d_w1,
                                     float* d_b1, float* d_g1, float* d_be1, float* d_w2, float* d_b2, float* d_g2, float* d_be2,
                                     void* workspace, int64_t workspace_bytes, sea_stream_t stream) {
  const char* nm = "sea_predictor_mlp_bwd";
#define SEA_MB_NONNULL(a) SEA_REQUIRE((a) != nullptr, SEA_EINVAL, "%s: " #a " is null", nm)
  SEA_MB_NONNULL(x); SEA_MB_NONNULL(x_strides); SEA_MB_NONNULL(g_y); SEA_MB_NONNULL(w1_packed); SEA_MB_NONNULL(w2_packed);
  SEA_MB_NONNULL(vectors); SEA_MB_NONNULL(d_w1); SEA_MB_NONNULL(d_b1); SEA_MB_NONNULL(d_g1); SEA_MB_NONNULL(d_be1);
  SEA_MB_NONNULL(d_w2); SEA_MB_NONNULL(d_b2); SEA_MB_NONNULL(d_g2); SEA_MB_NONNULL(d_be2); SEA_MB_NONNULL(workspace);
#undef SEA_MB_NONNULL
  SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: unknown dtype %d", nm, dtype);
  SEA_REQUIRE(dtype != SEA_F32, SEA_EUNSUPPORTED, "%s: fp32 data has no backward kernel (16-bit data only)", nm);
  SEA_REQUIRE(N > 0 && H > 0 && T > 0 && Din > 0 && D1 > 0 && D2 > 0, SEA_EINVAL,
              "%s: bad shape N=%lld H=%lld T=%lld Din=%lld D1=%lld D2=%lld", nm, (long long)N, (long long)H, (long long)T, (long long)Din,
              (long long)D1, (long long)D2);
  SEA_REQUIRE(mlp_bwd_supported(D1, D2, H, Din, dtype), SEA_EUNSUPPORTED,
              "%s: (D1=%lld, D2=%lld, H=%lld, Din=%lld) has no backward kernel (D1 = 128, D2 %% 16 == 0 in 16 .. 128, H %% 4 == 0, "
              "Din %% 32 == 0 up to 256)", nm, (long long)D1, (long long)D2, (long long)H, (long long)Din);
  const int64_t need = sea_predictor_mlp_bwd_workspace_bytes(N, H, T, Din, D1, D2, dtype);
  SEA_REQUIRE(need > 0, SEA_EUNSUPPORTED, "%s: N*H*T beyond the limit of 2^30 rows", nm);
  SEA_REQUIRE((((uintptr_t)x | (uintptr_t)g_y | (uintptr_t)g_tpred | (uintptr_t)w1_packed | (uintptr_t)w2_packed | (uintptr_t)vectors |
                (uintptr_t)d_x) & 15) == 0, SEA_EINVAL, "%s: x, g_y, g_tpred, w1_packed, w2_packed, vectors, d_x must be 16-byte aligned", nm);
  SEA_REQUIRE(x_strides[0] % 8 == 0 && x_strides[1] % 8 == 0 && x_strides[2] % 8 == 0, SEA_EINVAL,
              "%s: x_strides must be multiples of 8 elements", nm);
  SEA_REQUIRE((((uintptr_t)d_w1 | (uintptr_t)d_b1 | (uintptr_t)d_g1 | (uintptr_t)d_be1 | (uintptr_t)d_w2 | (uintptr_t)d_b2 |
                (uintptr_t)d_g2 | (uintptr_t)d_be2) & 3) == 0, SEA_EINVAL, "%s: the fp32 outputs must be 4-byte aligned", nm);
  SEA_REQUIRE(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need, SEA_EINVAL,
              "%s: workspace of %lld bytes needed (16-byte aligned), got %lld", nm, (long long)need, (long long)workspace_bytes);

  const int64_t rows = N * H * T;
  const MlpBwdLayout l = mlp_bwd_layout(rows, Din, D2);
  char* ws = reinterpret_cast<char*>(workspace);
  MlpBwdParams p;
  p.x = x; p.xs_n = x_strides[0]; p.xs_h = x_strides[1]; p.xs_t = x_strides[2];
  p.gy = g_y; p.gtp = g_tpred; p.w1p = w1_packed; p.w2p = w2_packed; p.vec = vectors;
  p.w2t = ws + l.w2t; p.w1t = ws + l.w1t; p.enc = ws + l.enc; p.ddec = ws + l.ddec; p.da1 = ws + l.da1;
  p.rpart = reinterpret_cast<float*>(ws + l.rpart); p.wpart = reinterpret_cast<float*>(ws + l.wpart);
  p.dx = d_x;
  p.N = (int)N; p.H = (int)H; p.T = (int)T; p.Din = (int)Din; p.KS1 = (int)(Din / 32); p.Wd = (int)(D2 / 2);
  p.HT = (int)((D2 / 2 + 15) / 16); p.rows = (int)rows;
  p.wrows = (int)mlp_bwd_wgrad_rows(rows); p.wblocks = (int)((rows + p.wrows - 1) / p.wrows); p.rgrid = (int)mlp_bwd_row_grid(rows);
  p.eps1 = eps1; p.eps2 = eps2;
  const MlpBwdOut o{d_w1, d_b1, d_g1, d_be1, d_w2, d_b2, d_g2, d_be2};
  hipStream_t s = (hipStream_t)stream;
  return dtype == SEA_BF16 ? launch_all<__hip_bfloat16>(p, o, s, nm) : launch_all<__half>(p, o, s, nm);
}
