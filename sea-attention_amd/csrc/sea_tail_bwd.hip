// Backward of the predictor tail (sea_predictor_tail), gfx950: include/sea_hip_predictor_grad.h, entry p1.
//
// Nothing of the forward is saved.  Per (n, t) row, with M the (T_m x (W4 + 1)) matrix of the padded nearest upsample and the area
// taps (tail_consts_fill's table), column W4 the zero-padded border:
//   z = W y,  a = [z | 0] M^T,  xh = (a - mu) rstd,  s = gamma xh + beta,  p = softmax(s)        (the bias cancels in xh)
//   ds = g_s + p (.) (g_p - sum_j g_p p),  d gamma += ds (.) xh,  d beta += ds
//   da = rstd (gamma ds - mean_j(gamma ds) - xh mean_j(gamma ds (.) xh)),  dz = (da M)[:, :W4],  dy = W^T dz,  dW += dz y^T
// tail_bwd_kernel: one 256-thread workgroup walks rows_per_block consecutive rows.  Per row: the C x W4 tile of y into LDS as
// fp32; z on the MFMA; one wave per head for a .. da, the lane owning one 16-byte piece of the g rows; dz as a gather of da over
// the <= 8 output pixels whose windows touch a source pixel (weights in registers, computed once from the table); dy^T = dz^T W
// on the MFMA into LDS and out with 16-byte stores; dW += dz y^T into accumulators that live across the rows.  d gamma / d beta
// stay in per-lane registers.  At the end of the block both go to the workspace; tail_bwd_reduce adds the blocks' parts in block
// order.  No atomics.  Every product is fp32 on v_mfma_f32_16x16x4_f32; 16-bit data is widened on load.
//
// LDS plan (floats; HP, CP, WP = H, C, W4 rounded up to 16), DESIGN 5.11:
//   Y    CP x (WP + 4)   the y tile, zero in its padding (written once)         DY   the same, dy of the row before it leaves
//   W    HP x (CP + 4)   the weights, resident                                  Z    HP x (W4 + 3), [W4] = [W4 + 1] = 0
//   DZ   HP x (WP + 4)   dz, zero in its padding                                tab  3 x 256 words (taps, gamma, beta)
//   U    4 x 256         da of the head a wave is on                            red  4 x 2 x 256, the waves' d gamma / d beta at the end
// 153 344 bytes at H = 64, C = 128, W4 = 64; 76 160 at H = 32, C = 64, W4 = 64 (two workgroups per CU).
#include <utility>
#include "sea_common.hpp"
#include "sea_tail.hpp"
#include "../../include/sea_hip_predictor_grad.h"

namespace sea {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
#define SEA_TB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

constexpr int TB_TMAX = 256;      // T_m of the predicate: one 16-byte piece of a row per lane, a table of 256 pixels
constexpr int TB_SLOTS = 8;       // output pixels whose windows can touch one source pixel: 4 T_m / Wp + 2 < 6, from jlo = first - 1

struct TailBwdParams {
  const void *y, *gamma, *beta, *gs, *gp;
  const float* w;                 // (H, C)
  void* dy;
  float* part;                    // (blocks, H C + 2 T_m)
  int64_t ys_n, ys_c, ys_t, ys_w, rows;
  float eps;
  int C, H, T, W4, T_M, rows_per_block;
};

struct TailBwdPlan {
  int HP, CP, WP, LDY, LDW, LDZ, LDD;
  int oY, oDY, oW, oZ, oDZ, oTab, oU, oRed, floats;
  __host__ __device__ constexpr TailBwdPlan(int H, int C, int W4)
      : HP((H + 15) / 16 * 16), CP((C + 15) / 16 * 16), WP((W4 + 15) / 16 * 16), LDY(WP + 4), LDW(CP + 4), LDZ(W4 + 3), LDD(WP + 4),
        oY(0), oDY(oY + CP * LDY), oW(oDY + CP * LDY), oZ(oW + HP * LDW), oDZ(oZ + HP * LDZ), oTab(oDZ + HP * LDD),
        oU(oTab + TAIL_TAB_ROWS * TB_TMAX), oRed(oU + 4 * TB_TMAX), floats(oRed + 4 * 2 * TB_TMAX) {}
  __host__ __device__ constexpr size_t bytes() const { return (size_t)floats * sizeof(float); }
};
static_assert(TailBwdPlan(64, 128, 64).bytes() <= 160 * 1024, "LDS at the predicate's largest shape");

// rows per workgroup: the shapes alone decide it (not the device), so the parts and their sum are the same everywhere
__host__ inline int64_t tail_bwd_block_rows(int64_t rows) {
  const int64_t r = (rows + 1023) / 1024;
  return r < 8 ? 8 : r > 32 ? 32 : r;
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void tail_bwd_kernel(TailBwdParams p) {
  constexpr int VEC = Elem<T>::VEC;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TailBwdPlan L(p.H, p.C, p.W4);
  float *sY = smem + L.oY, *sDY = smem + L.oDY, *sW = smem + L.oW, *sZ = smem + L.oZ, *sDZ = smem + L.oDZ;
  float *sU = smem + L.oU, *sRed = smem + L.oRed;
  uint32_t* sTab = reinterpret_cast<uint32_t*>(smem + L.oTab);
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
  const int H = p.H, C = p.C, W4 = p.W4, T_M = p.T_M;
  const int HT = L.HP / 16, CT = L.CP / 16, WT = L.WP / 16;

  // ---- once per block: the weights, the zero padding of Y / DZ / Z, the table of taps
  for (int i = tid; i < L.HP * L.LDW; i += 256) {
    const int r = i / L.LDW, c = i - r * L.LDW;
    sW[i] = (r < H && c < C) ? p.w[r * C + c] : 0.f;
  }
  for (int i = tid; i < L.CP * L.LDY; i += 256) sY[i] = 0.f;
  for (int i = tid; i < L.HP * L.LDD; i += 256) sDZ[i] = 0.f;
  for (int i = tid; i < L.HP * L.LDZ; i += 256) sZ[i] = 0.f;
  {
    TailParams tp{};
    tp.gamma = p.gamma; tp.beta = p.beta; tp.W4 = W4; tp.UP = 4; tp.T_M = T_M;
    tail_consts_fill<T>(tp, sTab, TB_TMAX);
  }
  __syncthreads();

  // ---- a lane's constants: its VEC output pixels (one 16-byte piece of a row), and as source pixel `lane` the weights of the gather
  const bool act = lane * VEC < T_M;                       // T_m % VEC == 0: a lane is all in or all out
  uint32_t pk[VEC];
  float gam[VEC], bet[VEC], rcnt[VEC], dgam[VEC], dbet[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const int j = act ? lane * VEC + e : 0;
    const uint32_t w = sTab[j];
    pk[e] = act ? w : (uint32_t)(W4 + 1) * 0x100401u;      // out: three unused taps, count 0
    gam[e] = act ? __uint_as_float(sTab[TB_TMAX + j]) : 0.f;
    bet[e] = act ? __uint_as_float(sTab[2 * TB_TMAX + j]) : 0.f;
    const uint32_t cnt = pk[e] >> 30;
    rcnt[e] = cnt == 1 ? 1.0f : cnt == 2 ? 0.5f : cnt == 3 ? (1.0f / 3.0f) : 0.f;
    dgam[e] = 0.f; dbet[e] = 0.f;
  }
  int jlo = 0;
  float wt[TB_SLOTS];
#pragma unroll
  for (int i = 0; i < TB_SLOTS; ++i) wt[i] = 0.f;
  if (lane < W4) {
    jlo = max(0, ((4 * lane + 1) * T_M) / (4 * W4 + 2) - 1);
#pragma unroll
    for (int i = 0; i < TB_SLOTS; ++i) {
      const int j = jlo + i;
      if (j < T_M) {
        const uint32_t w = sTab[j], cnt = w >> 30;
        int hits = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) hits += ((int)__builtin_amdgcn_ubfe(w, 10 * k, 10) == lane) ? 1 : 0;
        wt[i] = (float)hits * (cnt == 1 ? 1.0f : cnt == 2 ? 0.5f : cnt == 3 ? (1.0f / 3.0f) : 0.f);
      }
    }
  }

  f4 accW[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) accW[i] = f4{0.f, 0.f, 0.f, 0.f};
  const float invT = 1.0f / (float)T_M;
  const T* gs = reinterpret_cast<const T*>(p.gs);
  const T* gp = reinterpret_cast<const T*>(p.gp);

  const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block;
  const int64_t r1 = r0 + p.rows_per_block < p.rows ? r0 + p.rows_per_block : p.rows;
  for (int64_t row = r0; row < r1; ++row) {
    const int64_t n = row / p.T, t = row - n * p.T;
    // ---- 1: the y tile, from either layout
    const T* yb = reinterpret_cast<const T*>(p.y) + n * p.ys_n + t * p.ys_t;
    if (p.ys_w == 1) {
      const int ppr = W4 / VEC;
      for (int idx = tid; idx < C * ppr; idx += 256) {
        const int c = idx / ppr, w0 = (idx - c * ppr) * VEC;
        float f[VEC];
        unpack16<T>(*reinterpret_cast<const uint4*>(yb + (int64_t)c * p.ys_c + w0), f);
#pragma unroll
        for (int j = 0; j < VEC; ++j) sY[c * L.LDY + w0 + j] = f[j];
      }
    } else {
      const int ppr = C / VEC;
      for (int idx = tid; idx < W4 * ppr; idx += 256) {
        const int w = idx / ppr, c0 = (idx - w * ppr) * VEC;
        float f[VEC];
        unpack16<T>(*reinterpret_cast<const uint4*>(yb + (int64_t)w * p.ys_w + c0), f);
#pragma unroll
        for (int j = 0; j < VEC; ++j) sY[(c0 + j) * L.LDY + w] = f[j];
      }
    }
    __syncthreads();
    // ---- 2: z = W y (HP x WP tiles), rows of heads, columns of pixels
    for (int tile = wv; tile < HT * WT; tile += 4) {
      const int ht = tile / WT, wb = tile - ht * WT;
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < L.CP / 4; ++ks)
        acc = SEA_TB_MFMA(sW[(ht * 16 + li) * L.LDW + ks * 4 + lg], sY[(ks * 4 + lg) * L.LDY + wb * 16 + li], acc);
      const int px = wb * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (px < W4) sZ[(ht * 16 + lg * 4 + r) * L.LDZ + px] = acc[r];
    }
    __syncthreads();
    // ---- 3: one wave per head: a, mu, rstd, xh, (p), ds, da, dz
    for (int h = wv; h < H; h += 4) {
      const float* zr = sZ + h * L.LDZ;
      float xh[VEC], ds[VEC];
      float s1 = 0.f;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        xh[e] = (zr[__builtin_amdgcn_ubfe(pk[e], 0, 10)] + zr[__builtin_amdgcn_ubfe(pk[e], 10, 10)] +
                 zr[__builtin_amdgcn_ubfe(pk[e], 20, 10)]) * rcnt[e];
        s1 += xh[e];
      }
      const float mean = wave_sum(s1) * invT;
      float s2 = 0.f;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        xh[e] = act ? xh[e] - mean : 0.f;
        s2 = fmaf(xh[e], xh[e], s2);
      }
      const float rstd = 1.0f / sqrtf(wave_sum(s2) * invT + p.eps);
#pragma unroll
      for (int e = 0; e < VEC; ++e) { xh[e] *= rstd; ds[e] = 0.f; }
      const int64_t gbase = ((n * H + h) * p.T + t) * T_M + lane * VEC;
      if (gs) {
        uint4 raw = make_uint4(0, 0, 0, 0);
        if (act) raw = *reinterpret_cast<const uint4*>(gs + gbase);
        unpack16<T>(raw, ds);
      }
      if (gp) {
        uint4 raw = make_uint4(0, 0, 0, 0);
        if (act) raw = *reinterpret_cast<const uint4*>(gp + gbase);
        float pr[VEC], gv[VEC];
        unpack16<T>(raw, gv);
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          pr[e] = fmaf(gam[e], xh[e], bet[e]);
          if (act) mx = fmaxf(mx, pr[e]);
        }
        mx = wave_max(mx);
        float se = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          pr[e] = act ? expf(pr[e] - mx) : 0.f;
          se += pr[e];
        }
        const float inv = 1.0f / wave_sum(se);
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          pr[e] *= inv;
          dot = fmaf(gv[e], pr[e], dot);
        }
        dot = wave_sum(dot);
#pragma unroll
        for (int e = 0; e < VEC; ++e) ds[e] = fmaf(pr[e], gv[e] - dot, ds[e]);
      }
      float m1 = 0.f, m2 = 0.f;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        dgam[e] = fmaf(ds[e], xh[e], dgam[e]);
        dbet[e] += ds[e];
        ds[e] *= gam[e];
        m1 += ds[e];
        m2 = fmaf(ds[e], xh[e], m2);
      }
      m1 = wave_sum(m1) * invT;
      m2 = wave_sum(m2) * invT;
      float* su = sU + wv * TB_TMAX;
      if (act) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) su[lane * VEC + e] = rstd * (ds[e] - m1 - xh[e] * m2);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();                     // da of this head is in U for the lanes that gather it
      if (lane < W4) {
        float dz = 0.f;
#pragma unroll
        for (int i = 0; i < TB_SLOTS; ++i) dz = fmaf(wt[i], su[min(jlo + i, T_M - 1)], dz);   // (a slot past T_m has weight 0)
        sDZ[h * L.LDD + lane] = dz;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();                     // U is read before the next head writes it
    }
    __syncthreads();
    // ---- 4: dW += dz y^T (HP x CP tiles, summed over the pixels), in accumulators that live across the rows
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wv + 4 * i;
      if (tile < HT * CT) {
        const int ht = tile / CT, cb = tile - ht * CT;
        for (int ks = 0; ks < L.WP / 4; ++ks)
          accW[i] = SEA_TB_MFMA(sDZ[(ht * 16 + li) * L.LDD + ks * 4 + lg], sY[(cb * 16 + li) * L.LDY + ks * 4 + lg], accW[i]);
      }
    }
    // ---- 5: dy^T = dz^T W (WP x CP tiles, summed over the heads): a lane ends with four consecutive pixels of one channel
    for (int tile = wv; tile < WT * CT; tile += 4) {
      const int wb = tile / CT, cb = tile - wb * CT;
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < L.HP / 4; ++ks)
        acc = SEA_TB_MFMA(sDZ[(ks * 4 + lg) * L.LDD + wb * 16 + li], sW[(ks * 4 + lg) * L.LDW + cb * 16 + li], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) sDY[(cb * 16 + li) * L.LDY + wb * 16 + lg * 4 + r] = acc[r];
    }
    __syncthreads();
    // ---- 6: dy leaves in 16-byte pieces, contiguous (N, C, T, W4).  (The next row's barriers stand between these reads and
    // the next step 5; its staging writes Y, which every wave has finished reading at the barrier above.)
    {
      T* dyb = reinterpret_cast<T*>(p.dy);
      const int ppr = W4 / VEC;
      for (int idx = tid; idx < C * ppr; idx += 256) {
        const int c = idx / ppr, w0 = (idx - c * ppr) * VEC;
        const float* src = sDY + c * L.LDY + w0;
        T* dst = dyb + ((n * C + c) * p.T + t) * W4 + w0;
        if constexpr (VEC == 4) {
          *reinterpret_cast<float4*>(dst) = make_float4(src[0], src[1], src[2], src[3]);
        } else {
          uint4 o;
          o.x = pack2<T>(src[0], src[1]); o.y = pack2<T>(src[2], src[3]);
          o.z = pack2<T>(src[4], src[5]); o.w = pack2<T>(src[6], src[7]);
          *reinterpret_cast<uint4*>(dst) = o;
        }
      }
    }
  }

  // ---- the block's parts: dW from the accumulators, d gamma / d beta summed over the four waves in wave order
  float* part = p.part + (int64_t)blockIdx.x * (H * C + 2 * T_M);
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int tile = wv + 4 * i;
    if (tile < HT * CT) {
      const int ht = tile / CT, cb = tile - ht * CT;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = ht * 16 + lg * 4 + r, c = cb * 16 + li;
        if (h < H && c < C) part[h * C + c] = accW[i][r];
      }
    }
  }
  if (act) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      sRed[(wv * 2) * TB_TMAX + lane * VEC + e] = dgam[e];
      sRed[(wv * 2 + 1) * TB_TMAX + lane * VEC + e] = dbet[e];
    }
  }
  __syncthreads();
  for (int i = tid; i < 2 * T_M; i += 256) {
    const int which = i >= T_M ? 1 : 0, j = i - which * T_M;
    float s = sRed[which * TB_TMAX + j];
#pragma unroll
    for (int w = 1; w < 4; ++w) s += sRed[(w * 2 + which) * TB_TMAX + j];
    part[H * C + i] = s;
  }
}

// out[i] = sum over the blocks of part[b][i], in block order: the same bits every run
__global__ __launch_bounds__(256) void tail_bwd_reduce(const float* part, int64_t blocks, int HC, int T_M, float* d_w, float* d_gamma,
                                                       float* d_beta) {
  const int per = HC + 2 * T_M;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  float s = 0.f;
  for (int64_t b = 0; b < blocks; ++b) s += part[b * per + i];
  if (i < HC) d_w[i] = s;
  else if (i < HC + T_M) d_gamma[i - HC] = s;
  else d_beta[i - HC - T_M] = s;
}

template <typename T, int NT>
int launch_tail_bwd_nt(const TailBwdParams& p, int64_t blocks, size_t lds, hipStream_t s) {
  static DevOnce once;
  if (once.first()) SEA_MAX_LDS((tail_bwd_kernel<T, NT>), TailBwdPlan(64, 128, 64).bytes());
  hipLaunchKernelGGL((tail_bwd_kernel<T, NT>), dim3((unsigned)blocks), dim3(256), lds, s, p);
  return SEA_OK;
}

template <typename T>
int launch_tail_bwd(const TailBwdParams& p, int64_t blocks, hipStream_t s) {
  const TailBwdPlan L(p.H, p.C, p.W4);
  const int tiles = (L.HP / 16) * (L.CP / 16);             // dW tiles, four waves: 1 .. 8 per wave
  if (tiles <= 4) return launch_tail_bwd_nt<T, 1>(p, blocks, L.bytes(), s);
  if (tiles <= 8) return launch_tail_bwd_nt<T, 2>(p, blocks, L.bytes(), s);
  if (tiles <= 16) return launch_tail_bwd_nt<T, 4>(p, blocks, L.bytes(), s);
  return launch_tail_bwd_nt<T, 8>(p, blocks, L.bytes(), s);
}

bool tail_bwd_supported(int64_t C, int64_t H, int64_t W4, int64_t up, int64_t T_m, int dtype) {
  return up == 4 && W4 > 0 && W4 * up == T_m && T_m % 32 == 0 && T_m <= TB_TMAX && H >= 1 && H <= 64 && C >= 8 && C <= 128 &&
         C % 8 == 0 && (dtype == SEA_F32 || dtype == SEA_F16 || dtype == SEA_BF16);
}

int64_t tail_bwd_blocks(int64_t rows) {
  const int64_t rb = tail_bwd_block_rows(rows);
  return (rows + rb - 1) / rb;
}

}  // namespace
}  // namespace sea

using namespace sea;

extern "C" int sea_predictor_grad_version(void) { return SEA_PREDICTOR_GRAD_ABI_VERSION; }

extern "C" int sea_predictor_tail_bwd_supported(int64_t C, int64_t H, int64_t W4, int64_t up, int64_t T_m, int dtype) {
  return tail_bwd_supported(C, H, W4, up, T_m, dtype) ? 1 : 0;
}

extern "C" int64_t sea_predictor_tail_bwd_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t T, int64_t W4, int64_t up,
                                                          int64_t T_m, int dtype) {
  if (N <= 0 || T <= 0 || N * T >= (1ll << 31) || !tail_bwd_supported(C, H, W4, up, T_m, dtype)) return 0;
  return (tail_bwd_blocks(N * T) * (H * C + 2 * T_m) * (int64_t)sizeof(float) + 15) / 16 * 16;
}

extern "C" int sea_predictor_tail_bwd(const void* y, int dtype, int64_t N, int64_t C, int64_t H, int64_t T, int64_t W4, int64_t up,
                                      int64_t T_m, const int64_t* y_strides, const float* conv_w, const void* gamma,
                                      const void* beta, float eps, const void* g_scores, const void* g_probs, void* d_y, float* d_w,
                                      float* d_gamma, float* d_beta, void* workspace, int64_t workspace_bytes, sea_stream_t stream) {
  const char* nm = "sea_predictor_tail_bwd";
#define SEA_TB_NONNULL(x) SEA_REQUIRE((x) != nullptr, SEA_EINVAL, "%s: " #x " is null", nm)
  SEA_TB_NONNULL(y); SEA_TB_NONNULL(y_strides); SEA_TB_NONNULL(conv_w); SEA_TB_NONNULL(gamma); SEA_TB_NONNULL(beta);
  SEA_TB_NONNULL(d_y); SEA_TB_NONNULL(d_w); SEA_TB_NONNULL(d_gamma); SEA_TB_NONNULL(d_beta); SEA_TB_NONNULL(workspace);
#undef SEA_TB_NONNULL
  SEA_REQUIRE(g_scores != nullptr || g_probs != nullptr, SEA_EINVAL, "%s: g_scores and g_probs are both null", nm);
  SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: unknown dtype %d", nm, dtype);
  SEA_REQUIRE(N > 0 && C > 0 && H > 0 && T > 0 && W4 > 0 && up > 0 && T_m > 0, SEA_EINVAL,
              "%s: bad shape N=%lld C=%lld H=%lld T=%lld W4=%lld up=%lld T_m=%lld", nm, (long long)N, (long long)C, (long long)H,
              (long long)T, (long long)W4, (long long)up, (long long)T_m);
  SEA_REQUIRE(up == 4 && W4 * up == T_m, SEA_EUNSUPPORTED, "%s: up=%lld, W4=%lld, T_m=%lld: needs up = 4 and W4 up = T_m", nm,
              (long long)up, (long long)W4, (long long)T_m);
  SEA_REQUIRE(T_m % 32 == 0 && T_m <= TB_TMAX, SEA_EUNSUPPORTED, "%s: T_m=%lld has no backward kernel (a multiple of 32 up to %d)", nm,
              (long long)T_m, TB_TMAX);
  SEA_REQUIRE(H <= 64, SEA_EUNSUPPORTED, "%s: H=%lld has no backward kernel (H <= 64)", nm, (long long)H);
  SEA_REQUIRE(C <= 128 && C % 8 == 0, SEA_EUNSUPPORTED, "%s: C=%lld has no backward kernel (C <= 128, C %% 8 == 0)", nm, (long long)C);
  SEA_REQUIRE(N * T < (1ll << 31), SEA_EUNSUPPORTED, "%s: N*T=%lld beyond the limit", nm, (long long)(N * T));
  const int64_t *ys = y_strides, vec = dtype == SEA_F32 ? 4 : 8;
  SEA_REQUIRE(ys[0] >= 0 && ys[1] >= 0 && ys[2] >= 0 && ys[3] >= 0, SEA_EINVAL, "%s: bad y strides {%lld, %lld, %lld, %lld}", nm,
              (long long)ys[0], (long long)ys[1], (long long)ys[2], (long long)ys[3]);
  SEA_REQUIRE(ys[3] == 1 || ys[1] == 1, SEA_EUNSUPPORTED, "%s: y must have unit stride along the width or along the channels", nm);
  {
    // no two elements at one address: the strides sorted by size, each at least the extent of the ones below it
    int64_t st[4] = {ys[0], ys[1], ys[2], ys[3]}, ex[4] = {N, C, T, W4};
    for (int i = 0; i < 4; ++i)
      for (int j = i + 1; j < 4; ++j)
        if (st[j] < st[i] || (st[j] == st[i] && ex[j] < ex[i])) { std::swap(st[i], st[j]); std::swap(ex[i], ex[j]); }
    int64_t span = 1;
    bool apart = true;
    for (int i = 0; i < 4; ++i) {
      if (ex[i] > 1 && st[i] < span) apart = false;
      span += (ex[i] - 1) * st[i];
    }
    SEA_REQUIRE(apart, SEA_EINVAL, "%s: bad y strides {%lld, %lld, %lld, %lld}: elements overlap", nm, (long long)ys[0],
                (long long)ys[1], (long long)ys[2], (long long)ys[3]);
  }
  SEA_REQUIRE(((uintptr_t)y & 15) == 0 && ys[0] % vec == 0 && ys[2] % vec == 0 && (ys[3] == 1 ? ys[1] : ys[3]) % vec == 0, SEA_EINVAL,
              "%s: y rows must be 16-byte aligned", nm);
  SEA_REQUIRE(((uintptr_t)conv_w & 15) == 0, SEA_EINVAL, "%s: conv_w rows must be 16-byte aligned", nm);
  SEA_REQUIRE((((uintptr_t)gamma | (uintptr_t)beta) & 15) == 0, SEA_EINVAL, "%s: gamma, beta rows must be 16-byte aligned", nm);
  SEA_REQUIRE((((uintptr_t)g_scores | (uintptr_t)g_probs) & 15) == 0, SEA_EINVAL, "%s: g_scores, g_probs rows must be 16-byte aligned", nm);
  SEA_REQUIRE((((uintptr_t)d_y | (uintptr_t)d_w | (uintptr_t)d_gamma | (uintptr_t)d_beta) & 15) == 0, SEA_EINVAL,
              "%s: d_y, d_w, d_gamma, d_beta rows must be 16-byte aligned", nm);
  const int64_t need = sea_predictor_tail_bwd_workspace_bytes(N, C, H, T, W4, up, T_m, dtype);
  SEA_REQUIRE(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need, SEA_EINVAL,
              "%s: workspace of %lld bytes needed (16-byte aligned), got %lld", nm, (long long)need, (long long)workspace_bytes);

  TailBwdParams p;
  p.y = y; p.gamma = gamma; p.beta = beta; p.gs = g_scores; p.gp = g_probs; p.w = conv_w; p.dy = d_y;
  p.part = reinterpret_cast<float*>(workspace);
  p.ys_n = ys[0]; p.ys_c = ys[1]; p.ys_t = ys[2]; p.ys_w = ys[3]; p.rows = N * T;
  p.eps = eps;
  p.C = (int)C; p.H = (int)H; p.T = (int)T; p.W4 = (int)W4; p.T_M = (int)T_m; p.rows_per_block = (int)tail_bwd_block_rows(N * T);
  const int64_t blocks = tail_bwd_blocks(N * T);
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == SEA_F32 ? launch_tail_bwd<float>(p, blocks, s)
               : dtype == SEA_F16 ? launch_tail_bwd<__half>(p, blocks, s) : launch_tail_bwd<__hip_bfloat16>(p, blocks, s);
  if (rc != SEA_OK) return rc;
  SEA_CHECK_LAUNCH(nm);
  const int per = (int)(H * C + 2 * T_m);
  hipLaunchKernelGGL(tail_bwd_reduce, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, s, p.part, blocks, (int)(H * C), (int)T_m,
                     d_w, d_gamma, d_beta);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}
