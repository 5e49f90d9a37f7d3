// SEA predictor MLP for fp32 data in one launch, hand-written for gfx950 (v_mfma_f32_16x16x4_f32: true fp32, nothing reduced).
//
// The fp32 twin of predictor_mlp_kernel (sea_mlp.hip), include/sea_hip_predictor_mlp_f32.h.  For fp32 x (N, H, T, 192), d = 64:
//   attention_predictor_enc         Linear(192 -> 128) + LayerNorm(128) + erf GELU       = tpred
//   attention_predictor_dec_row     Linear(128 -> D2) + ChannelSplit(2)
//   cnn.lnorm1                      LayerNorm(Wd = D2 / 2) on every split, stored in the C8 layout of the convolutions
//   attention_predictor_dec_scaler  Linear(128 -> 2) + sigmoid                           = row_scale, avg_scale
// which otherwise are three library GEMMs, two LayerNorm launches, a re-layout copy and their fp32 round trips through HBM.
//
// WORK SPLIT.  Persistent workgroups of 8 waves, one per compute unit (the grid is sized from the device's CU count).  A workgroup
// walks items of ROWS = 32 consecutive rows of the flattened (n, t, h) order -- sea_mlp.hip's PACK rule for every H: with H % 16 == 0
// a 16-row tile is 16 heads of one token anyway, with H = 12 every tile but the launch's last is full; H % 4 == 0 keeps each group of
// 4 rows inside one token, so a group is one whole 8-channel block (4 heads x 2 splits) of the C8 output.  Rows past the end are zeros
// on load and skipped on store.
//   Both products are computed TRANSPOSED, D^T = W . X^T (A = weights, B = activations), and split over the waves by OUTPUT FEATURE:
//   wave w owns features 16 w .. 16 w + 15 of the encoder and (w < D2 / 16) of the decoder, for all 32 rows.  In the 16x16x4
//   accumulator lane 16 g + i then holds features 4 g .. 4 g + 3 of the tile for row i.
//
// REGISTERS.  A wave's weight slices never change, so they live in registers for the lifetime of the workgroup, loaded once from
// the host-packed fragment images: W1 16 x 192 = 48 VGPRs per lane, W2 16 x 128 = 32.  (The 16-bit kernel's plan -- weight images in
// LDS -- does not carry over: W1 is 96 KB in fp32.  Keeping W1 in LDS and only W2 in registers was the first plan; with the feature
// split a wave reads nothing but ITS 12 KB of W1, 8 waves at 2 per SIMD have 256 VGPRs each, and the registers cost no LDS read per
// MFMA block and leave the LDS to 32-row tiles: half the barriers per row of a 16-row tile.)  K is walked in blocks of 16: for block
// kb a lane reads ONE float4 of a row's activations, x[i][16 kb + 4 g + j], j = 0 .. 3, and MFMA step j of the block multiplies the
// k set {16 kb + 4 g + j : g}; the host packs the weights with the same permutation (lane 16 g + i, element j = W[16 w + i][16 kb + 4 g + j]).
//
// LDS PLAN (floats; rows padded by 4 so that the 16 rows a float4 read touches fall in 16 different bank groups):
//   xs    2 x 32 x 196   the x tile, double-buffered: the next item's rows are requested at the top of a step (global -> registers),
//                        and written to the other buffer after the decoder product                                          50 176 B
//   enc   32 x 132       the encoder tile, passed through LDS ONCE: written as W1 x + b1 by the feature-owning waves, normalised in
//                        place by a half-wave per row (LayerNorm statistics, GELU, the gates' two dot products, the tpred store),
//                        then read as the B operand of the decoder product                                                    16 896 B
//   dec   32 x 132       W2 tpred + b2, for lnorm1's statistics (8 lanes per (row, split)) and the transposing C8 store      16 896 B
//   stat  64 x 2         (mean, rstd) of every (row, split)                                                                     512 B
//   ln1   2 x 64         lnorm1's weight and bias                                                                                512 B
// Four barriers per item: after enc is written, after it is normalised, after dec (and the next x tile) is written, after stat.
#include "sea_common.hpp"
#include "../../include/sea_hip_predictor_mlp_f32.h"

namespace sea {

typedef __attribute__((ext_vector_type(4))) float qf4;

constexpr int F_D1 = 128, F_DIN = 192, F_WAVES = 8, F_THREADS = F_WAVES * 64, F_ROWS = 32, F_RT = F_ROWS / 16;
constexpr int F_KB1 = F_DIN / 16, F_KB2 = F_D1 / 16;
constexpr int F_XSTR = F_DIN + 4, F_ESTR = F_D1 + 4;
constexpr int F_XCH = F_ROWS * (F_DIN / 4) / F_THREADS;                  // float4 chunks of an x tile per thread
constexpr int F_LDS_X = 2 * F_ROWS * F_XSTR, F_LDS_ENC = F_ROWS * F_ESTR, F_LDS_DEC = F_ROWS * F_ESTR, F_LDS_STAT = 2 * F_ROWS * 2,
              F_LDS_LN1 = 2 * 64;
constexpr int F_LDS_BYTES = (F_LDS_X + F_LDS_ENC + F_LDS_DEC + F_LDS_STAT + F_LDS_LN1) * (int)sizeof(float);
static_assert(F_LDS_BYTES <= 160 * 1024, "the LDS plan at the top of this file");
static_assert(F_ROWS * (F_DIN / 4) % F_THREADS == 0 && F_D1 == 16 * F_WAVES && F_ROWS == 2 * 16, "tile / workgroup shape");

struct MlpF32Params {
  const float* x;            // (N, H, T, 192), last axis contiguous
  int64_t xs_n, xs_h, xs_t;  // element strides, multiples of 4
  const float* w1p;          // [8][12][64][4]
  const float* w2p;          // [NT2][8][64][4]
  const float* vec;          // b1[128] g1[128] be1[128] b2[D2] g2[Wd] be2[Wd] Ws[2][128] bs[2]
  float* x_c8;               // (N, T, H / 4, Wd, 8)
  float* tpred;              // optional (N, H, T, 128)
  float* row_scale;          // (N, H, T)
  float* avg_scale;          // (N, H, T)
  int H, T;
  int total_rows, nitems;    // N H T (< 2^31 - 64), ceil(total_rows / 32)
  float eps1, eps2;
  int64_t xc8_n;             // element stride between batch items of x_c8
};

// sum over the 32 lanes of a half-wave (lanes 0 .. 31 and 32 .. 63 apart), every lane of the half ends with it
__device__ inline float half_sum(float v) {
  v += __uint_as_float(dpp_u32<0xB1>(__float_as_uint(v)));               // quad_perm [1,0,3,2]
  v += __uint_as_float(dpp_u32<0x4E>(__float_as_uint(v)));               // quad_perm [2,3,0,1]
  v += __uint_as_float(dpp_u32<0x141>(__float_as_uint(v)));              // row_half_mirror
  v += __uint_as_float(dpp_u32<0x140>(__float_as_uint(v)));              // row_mirror
  return xor16_sum(v);
}
// sum over each group of 8 consecutive lanes
__device__ inline float oct_sum(float v) {
  v += __uint_as_float(dpp_u32<0xB1>(__float_as_uint(v)));
  v += __uint_as_float(dpp_u32<0x4E>(__float_as_uint(v)));
  v += __uint_as_float(dpp_u32<0x141>(__float_as_uint(v)));
  return v;
}

// the x tile of `item`: thread's chunk u is float4 (c % 48) of row c / 48, c = tid + 512 u; rows past the end are zeros
__device__ inline void mlp_f32_load_x(const MlpF32Params& p, int item, int tid, float4 (&xr)[F_XCH]) {
#pragma unroll
  for (int u = 0; u < F_XCH; ++u) {
    const int c = tid + u * F_THREADS, r = c / (F_DIN / 4), c4 = c - r * (F_DIN / 4);
    const int R = item * F_ROWS + r;
    xr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (R < p.total_rows) {
      const int nt = R / p.H, h = R - nt * p.H, n = nt / p.T, t = nt - n * p.T;
      xr[u] = *reinterpret_cast<const float4*>(p.x + n * p.xs_n + h * p.xs_h + t * p.xs_t + 4 * c4);
    }
  }
}
__device__ inline void mlp_f32_put_x(float* xb, int tid, const float4 (&xr)[F_XCH]) {
#pragma unroll
  for (int u = 0; u < F_XCH; ++u) {
    const int c = tid + u * F_THREADS, r = c / (F_DIN / 4), c4 = c - r * (F_DIN / 4);
    *reinterpret_cast<float4*>(xb + r * F_XSTR + 4 * c4) = xr[u];
  }
}

template <int NT2>
__global__ __launch_bounds__(F_THREADS) void predictor_mlp_f32_kernel(MlpF32Params p) {
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  constexpr int D2 = 16 * NT2, Wd = D2 / 2;
  static_assert(NT2 >= 1 && NT2 <= F_WAVES && Wd % 8 == 0 && Wd <= 64, "decoder tiles: one per wave, lnorm1 on 8 lanes per split");
  float* xs = fsm;
  float* enc = xs + F_LDS_X;
  float* dec = enc + F_LDS_ENC;
  float* stat = dec + F_LDS_DEC;
  float* ln1 = stat + F_LDS_STAT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  constexpr int OFF_B2 = 3 * F_D1, OFF_G2 = OFF_B2 + D2, OFF_E2 = OFF_G2 + Wd, OFF_WS = OFF_E2 + Wd, OFF_BS = OFF_WS + 2 * F_D1;

  // ---- once per workgroup: this wave's weight slices and this lane's vector pieces into registers ----------------------------
  qf4 w1r[F_KB1], w2r[F_KB2];
#pragma unroll
  for (int kb = 0; kb < F_KB1; ++kb) w1r[kb] = *reinterpret_cast<const qf4*>(p.w1p + ((size_t)(wv * F_KB1 + kb) * 64 + lane) * 4);
  qf4 b2v = qf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < F_KB2; ++kb) w2r[kb] = qf4{0.f, 0.f, 0.f, 0.f};
  if (wv < NT2) {
#pragma unroll
    for (int kb = 0; kb < F_KB2; ++kb) w2r[kb] = *reinterpret_cast<const qf4*>(p.w2p + ((size_t)(wv * F_KB2 + kb) * 64 + lane) * 4);
    b2v = *reinterpret_cast<const qf4*>(p.vec + OFF_B2 + 16 * wv + 4 * lg);
  }
  const qf4 b1v = *reinterpret_cast<const qf4*>(p.vec + 16 * wv + 4 * lg);
  const int hj = tid & 31, hwv = tid >> 5;                               // LayerNorm(128) phase: lane of / index of the half-wave
  const float4 g1v = *reinterpret_cast<const float4*>(p.vec + F_D1 + 4 * hj);
  const float4 e1v = *reinterpret_cast<const float4*>(p.vec + 2 * F_D1 + 4 * hj);
  const float4 ws0 = *reinterpret_cast<const float4*>(p.vec + OFF_WS + 4 * hj);
  const float4 ws1 = *reinterpret_cast<const float4*>(p.vec + OFF_WS + F_D1 + 4 * hj);
  const float bs0 = p.vec[OFF_BS], bs1 = p.vec[OFF_BS + 1];
  if (tid < Wd) { ln1[tid] = p.vec[OFF_G2 + tid]; ln1[64 + tid] = p.vec[OFF_E2 + tid]; }
  const int C8 = p.H >> 2;

  float4 xr[F_XCH];
  int item = blockIdx.x;                                                 // (launcher: gridDim.x <= nitems)
  mlp_f32_load_x(p, item, tid, xr);
  mlp_f32_put_x(xs, tid, xr);
  __syncthreads();

  for (int buf = 0; item < p.nitems; item += gridDim.x, buf ^= 1) {
    const int next = item + gridDim.x;
    if (next < p.nitems) mlp_f32_load_x(p, next, tid, xr);               // in flight under product 1
    // ---- product 1: enc^T = W1 . x^T, this wave's 16 features of the 32 rows --------------------------------------------------
    const float* xc = xs + buf * (F_ROWS * F_XSTR) + li * F_XSTR + 4 * lg;
    qf4 acc1[F_RT];
#pragma unroll
    for (int rt = 0; rt < F_RT; ++rt) acc1[rt] = qf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < F_KB1; ++kb) {
#pragma unroll
      for (int rt = 0; rt < F_RT; ++rt) {
        const qf4 b = *reinterpret_cast<const qf4*>(xc + rt * 16 * F_XSTR + 16 * kb);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc1[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1r[kb][j], b[j], acc1[rt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int rt = 0; rt < F_RT; ++rt)
      *reinterpret_cast<qf4*>(enc + (rt * 16 + li) * F_ESTR + 16 * wv + 4 * lg) = acc1[rt] + b1v;
    __syncthreads();
    // ---- LayerNorm(128) + GELU in place, a half-wave per row; tpred and the two gates leave from here ----------------------------
#pragma unroll
    for (int it = 0; it < F_ROWS / 16; ++it) {
      const int row = hwv + 16 * it;
      float* er = enc + row * F_ESTR + 4 * hj;
      const float4 a = *reinterpret_cast<const float4*>(er);
      const float mean = half_sum((a.x + a.y) + (a.z + a.w)) * (1.0f / (float)F_D1);
      const float d0 = a.x - mean, d1 = a.y - mean, d2 = a.z - mean, d3 = a.w - mean;
      const float var = half_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) * (1.0f / (float)F_D1);
      const float rstd = rsqrtf(var + p.eps1);
      float4 o;
      o.x = gelu_erf(d0 * rstd * g1v.x + e1v.x); o.y = gelu_erf(d1 * rstd * g1v.y + e1v.y);
      o.z = gelu_erf(d2 * rstd * g1v.z + e1v.z); o.w = gelu_erf(d3 * rstd * g1v.w + e1v.w);
      *reinterpret_cast<float4*>(er) = o;
      const float s0 = half_sum((o.x * ws0.x + o.y * ws0.y) + (o.z * ws0.z + o.w * ws0.w)) + bs0;
      const float s1 = half_sum((o.x * ws1.x + o.y * ws1.y) + (o.z * ws1.z + o.w * ws1.w)) + bs1;
      const int R = item * F_ROWS + row;
      if (R < p.total_rows) {
        const int nt = R / p.H, h = R - nt * p.H, n = nt / p.T, t = nt - n * p.T;
        const int64_t orow = ((int64_t)n * p.H + h) * p.T + t;
        if (p.tpred) *reinterpret_cast<float4*>(p.tpred + orow * F_D1 + 4 * hj) = o;
        if (hj == 0) {
          p.row_scale[orow] = 1.0f / (1.0f + __expf(-s0));
          p.avg_scale[orow] = 1.0f / (1.0f + __expf(-s1));
        }
      }
    }
    __syncthreads();
    // ---- product 2: dec^T = W2 . tpred^T, waves 0 .. NT2 - 1 ------------------------------------------------------------------------
    if (wv < NT2) {
      const float* ec = enc + li * F_ESTR + 4 * lg;
      qf4 acc2[F_RT];
#pragma unroll
      for (int rt = 0; rt < F_RT; ++rt) acc2[rt] = qf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < F_KB2; ++kb) {
#pragma unroll
        for (int rt = 0; rt < F_RT; ++rt) {
          const qf4 b = *reinterpret_cast<const qf4*>(ec + rt * 16 * F_ESTR + 16 * kb);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc2[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2r[kb][j], b[j], acc2[rt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int rt = 0; rt < F_RT; ++rt)
        *reinterpret_cast<qf4*>(dec + (rt * 16 + li) * F_ESTR + 16 * wv + 4 * lg) = acc2[rt] + b2v;
    }
    // the next item's rows into the other x buffer (last read a whole step ago, two barriers before it is read again)
    if (next < p.nitems) mlp_f32_put_x(xs + (buf ^ 1) * (F_ROWS * F_XSTR), tid, xr);
    __syncthreads();
    // ---- lnorm1 statistics: 8 lanes per (row, split) ---------------------------------------------------------------------------------
    {
      const int pr = tid >> 3, j8 = tid & 7;                            // pair = 2 row + split
      const float* dr = dec + (pr >> 1) * F_ESTR + (pr & 1) * Wd + j8;
      float v[NT2];
      float s = 0.f;
#pragma unroll
      for (int m = 0; m < NT2; ++m) { v[m] = dr[8 * m]; s += v[m]; }
      const float mean = oct_sum(s) * (1.0f / (float)Wd);
      float q = 0.f;
#pragma unroll
      for (int m = 0; m < NT2; ++m) { const float d = v[m] - mean; q += d * d; }
      const float rstd = rsqrtf(oct_sum(q) * (1.0f / (float)Wd) + p.eps2);
      if (j8 == 0) { stat[2 * pr] = mean; stat[2 * pr + 1] = rstd; }
    }
    __syncthreads();
    // ---- C8 store: group q of 4 rows = one (n, t, 4-head block) = Wd x 8 contiguous floats; a thread writes 2 heads x 2 splits ------
#pragma unroll
    for (int u = 0; u < (F_ROWS * D2 / 4 + F_THREADS - 1) / F_THREADS; ++u) {
      const int c = tid + u * F_THREADS;
      const int q = c / (2 * Wd), rem = c - q * (2 * Wd), w = rem >> 1, hh = rem & 1;
      const int ra = 4 * q + 2 * hh;
      const int Rq = item * F_ROWS + 4 * q;                              // total_rows % 4 == 0: a group is whole or absent
      if (c < F_ROWS * D2 / 4 && Rq < p.total_rows) {
        const float* da = dec + ra * F_ESTR + w;
        const float4 sa = *reinterpret_cast<const float4*>(stat + 4 * ra);        // (mean, rstd) of (ra, 0), (ra, 1)
        const float4 sb = *reinterpret_cast<const float4*>(stat + 4 * ra + 4);    //              of (ra + 1, 0), (ra + 1, 1)
        const float g = ln1[w], e = ln1[64 + w];
        float4 o;
        o.x = (da[0] - sa.x) * sa.y * g + e;
        o.y = (da[Wd] - sa.z) * sa.w * g + e;
        o.z = (da[F_ESTR] - sb.x) * sb.y * g + e;
        o.w = (da[F_ESTR + Wd] - sb.z) * sb.w * g + e;
        const int nt = Rq / p.H, h = Rq - nt * p.H, n = nt / p.T, t = nt - n * p.T;
        float* yb = p.x_c8 + n * p.xc8_n + ((int64_t)t * C8 + (h >> 2)) * (Wd * 8);
        *reinterpret_cast<float4*>(yb + w * 8 + hh * 4) = o;
      }
    }
    // (no barrier here: the next step writes enc first, last read before the third barrier above; dec, stat and the x buffer
    //  this step read are written again only behind the next step's barriers)
  }
}

}  // namespace sea

using namespace sea;

// compute units of the current device, asked once per device (the persistent grid is sized by it)
static int mlp_f32_device_cus() {
  static int cus[64];
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) return 256;
  int c = __atomic_load_n(&cus[d & 63], __ATOMIC_RELAXED);
  if (c <= 0) {
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || c <= 0) c = 256;
    __atomic_store_n(&cus[d & 63], c, __ATOMIC_RELAXED);
  }
  return c;
}

// the one predicate, on both sides of the ABI
static bool mlp_f32_shape_ok(int64_t D1, int64_t D2, int64_t H, int64_t Din) {
  return D1 == F_D1 && Din == F_DIN && (D2 == 16 || D2 == 32 || D2 == 48 || D2 == 64 || D2 == 128) && H > 0 && H % 4 == 0;
}

extern "C" int sea_predictor_mlp_f32_version(void) { return SEA_PREDICTOR_MLP_F32_ABI_VERSION; }

extern "C" int sea_predictor_mlp_f32_supported(int64_t D1, int64_t D2, int64_t H, int64_t Din) { return mlp_f32_shape_ok(D1, D2, H, Din) ? 1 : 0; }

template <int NT2>
static int launch_mlp_f32(const MlpF32Params& p, hipStream_t s) {
  static DevOnce once;
  if (once.first()) SEA_MAX_LDS((predictor_mlp_f32_kernel<NT2>), F_LDS_BYTES);
  const int cus = mlp_f32_device_cus();
  const int blocks = p.nitems < cus ? p.nitems : cus;                    // persistent: one workgroup per compute unit
  hipLaunchKernelGGL((predictor_mlp_f32_kernel<NT2>), dim3((unsigned)blocks), dim3(F_THREADS), F_LDS_BYTES, s, p);
  return SEA_OK;
}

extern "C" int sea_predictor_mlp_f32(const float* x, int64_t N, int64_t H, int64_t T, int64_t Din, const int64_t* x_strides, int64_t D1,
                                     int64_t D2, const float* w1_packed, const float* w2_packed, const float* vectors, float eps1,
                                     float eps2, float* x_c8, int64_t x_c8_stride_n, float* tpred, float* row_scale, float* avg_scale,
                                     sea_stream_t stream) {
  const char* nm = "sea_predictor_mlp_f32";
#define SEA_F32_NONNULL(a) SEA_REQUIRE((a) != nullptr, SEA_EINVAL, "%s: " #a " is null", nm)
  SEA_F32_NONNULL(x); SEA_F32_NONNULL(x_strides); SEA_F32_NONNULL(w1_packed); SEA_F32_NONNULL(w2_packed); SEA_F32_NONNULL(vectors);
  SEA_F32_NONNULL(x_c8); SEA_F32_NONNULL(row_scale); SEA_F32_NONNULL(avg_scale);
#undef SEA_F32_NONNULL
  SEA_REQUIRE(N > 0 && H > 0 && T > 0 && Din > 0 && D1 > 0 && D2 > 0, SEA_EINVAL, "%s: bad shape", nm);
  SEA_REQUIRE(mlp_f32_shape_ok(D1, D2, H, Din), SEA_EUNSUPPORTED,
              "%s: (D1=%lld, D2=%lld, H=%lld, Din=%lld) is outside sea_predictor_mlp_f32_supported: D1 = 128, Din = 192, D2 in {16, 32, 48, "
              "64, 128}, H %% 4 == 0", nm, (long long)D1, (long long)D2, (long long)H, (long long)Din);
  SEA_REQUIRE(N < (1ll << 31) && T < (1ll << 31) && N * H < (1ll << 31) && N * H * T < (1ll << 31) - 64, SEA_EUNSUPPORTED,
              "%s: N*H*T must stay below 2^31 - 64 rows", nm);
  SEA_REQUIRE((((uintptr_t)x | (uintptr_t)w1_packed | (uintptr_t)w2_packed | (uintptr_t)vectors | (uintptr_t)x_c8 | (uintptr_t)tpred) & 15) == 0,
              SEA_EINVAL, "%s: x, w1_packed, w2_packed, vectors, x_c8, tpred must be 16-byte aligned", nm);
  SEA_REQUIRE((((uintptr_t)row_scale | (uintptr_t)avg_scale) & 3) == 0, SEA_EINVAL, "%s: row_scale, avg_scale must be 4-byte aligned", nm);
  SEA_REQUIRE(x_strides[0] % 4 == 0 && x_strides[1] % 4 == 0 && x_strides[2] % 4 == 0, SEA_EINVAL,
              "%s: x_strides must be multiples of 4 elements (16-byte rows)", nm);
  const int64_t dense_n = T * (H / 4) * (D2 / 2) * 8;
  SEA_REQUIRE(x_c8_stride_n == 0 || (x_c8_stride_n >= dense_n && x_c8_stride_n % 4 == 0), SEA_EINVAL,
              "%s: x_c8_stride_n must be 0 (dense) or >= %lld elements in whole 16-byte blocks", nm, (long long)dense_n);
  MlpF32Params p;
  p.x = x; p.xs_n = x_strides[0]; p.xs_h = x_strides[1]; p.xs_t = x_strides[2];
  p.w1p = w1_packed; p.w2p = w2_packed; p.vec = vectors;
  p.x_c8 = x_c8; p.tpred = tpred; p.row_scale = row_scale; p.avg_scale = avg_scale;
  p.H = (int)H; p.T = (int)T;
  p.total_rows = (int)(N * H * T);
  p.nitems = (int)((N * H * T + F_ROWS - 1) / F_ROWS);
  p.eps1 = eps1; p.eps2 = eps2;
  p.xc8_n = x_c8_stride_n ? x_c8_stride_n : dense_n;
  hipStream_t s = (hipStream_t)stream;
  int rc;                                                                // (a failed attribute call has set its own text)
  switch (D2) {
    case 16: rc = launch_mlp_f32<1>(p, s); break;
    case 32: rc = launch_mlp_f32<2>(p, s); break;
    case 48: rc = launch_mlp_f32<3>(p, s); break;
    case 64: rc = launch_mlp_f32<4>(p, s); break;
    default: rc = launch_mlp_f32<8>(p, s); break;                        // 128: the predicate leaves nothing else
  }
  if (rc != SEA_OK) return rc;
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}
