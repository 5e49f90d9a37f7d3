// Backward of the predictor CNN's (convolution, ReLU) pairs, gfx950, 16-bit data: include/sea_hip_predictor_cnn_grad.h, entry c1.
//
// y = relu(conv(x) + b) is sea_causal_conv_c8's 3 x 3 dilated causal layer on C8 activations (N, T, C/8, W, 8).  With d the
// dilation (= pad_w) and dp = g (.) (y > 0):
//   dx[ci,t,w]    = sum_{co,i,j} Wt[co,ci,i,j] dp[co, t+(2-i)d, w-(j-1)d]          db[co] = sum dp
//   dWt[co,ci,i,j] = sum_{n,t,w} dp[co,t,w] x[ci, t-(2-i)d, w+(j-1)d]
// Both kernels: one 256-thread workgroup walks rows_per_block consecutive rows of ONE sequence (a function of the shapes alone),
// every C8 row goes global -> registers -> LDS once per block (the mask needs g and y side by side), the next row's loads fly
// under the current row's MFMAs, and the LDS rows carry d zero pixels either side and zero channel blocks up to the operand
// tile, so that no fragment needs a mask.
//
// conv_relu_dgrad_kernel: the forward with the channel axes swapped.  M = ci, N = pixels, K = (tap, co), v_mfma_f32_16x16x32.
//   A: the transposed, tap-flipped image WT[ci][i'][j'][co] = Wt[co][ci][2-i'][2-j'] (conv_bwd_pack_kernel, per call), held in
//      REGISTERS for the whole block: wave w owns the ci tiles w and w + 4, 9 KCH fragments of 4 VGPRs each (72 at C = 64, 216 at
//      C = 80) -- the 138 KB LDS image of the forward at C = 80 would leave no room for the ring.
//   B: ds_read_b128 from a ring of 2d+1 masked dp rows (row t + i' d, pixel w + (j' - 1) d): a lane's 16 bytes are the 8
//      channels of one pixel, which is the fragment.  Tap rows >= T are skipped (wave-uniform).
//   The row leaves through an LDS image of the C8 row: 16-byte stores.
// conv_relu_wgrad_kernel: split-K GEMM, M = co, N = ci, K = pixels, one MFMA pass per tap per 32 pixels.  The C8 rows have the
//   channels innermost; the operands want 8 consecutive pixels of one channel per lane: ds_read_b64_tr_b16 turns a 4-pixel x
//   16-channel patch (lane 4q+p: pixel q, channels 4p..4p+3; lane i receives channel i), two of them per fragment, and a column
//   shift stays an address offset of whole 16-byte pixels.  x rows sit in a ring of 2d+1 slots (each loaded once per block), the
//   masked dp row in a slot of its own.  The (co tile, ci tile) pairs are dealt round the four waves; a pair's nine tap
//   accumulators stay in registers across the block's rows (144 VGPRs per wave at C = 64).  At C > 64 (25 tile pairs) the
//   grid's second dimension splits the output by kernel row i: 7 pairs x 3 taps per wave.  db: every thread sums the dp units it
//   stages, per channel, in registers; at the end of the block the pixels are added in pixel order.
// Each block writes its part (dW then db) to the workspace; conv_bwd_reduce adds the parts in block order.  No atomics.
#include "sea_common.hpp"
#include "sea_convfrag.hpp"
#include "../../include/sea_hip_predictor_cnn_grad.h"

namespace sea {
namespace {

constexpr int CB_UMAX = 3;                 // 16-byte units of a C8 row per thread: (C / 8) W <= 640 over 256 threads
constexpr int CB_MAX_LDS = 160 * 1024;

struct ConvBwdParams {
  const void *x, *y, *g;                   // (N, T, C/8, W, 8)
  const void* wt;                          // (C, 9, CP) transposed, tap-flipped weights
  void* dx;
  float* part;                             // (blocks, 9 C C + C)
  int T, W, C, CP, dil, rows_per_block, blocks_per_seq;
};

typedef short cb_s4 __attribute__((ext_vector_type(4)));

// dp = g where y > 0: a 16-bit float is positive when its pattern lies in 0x0001 .. 0x7fff
__device__ __forceinline__ uint32_t mask_pos2(uint32_t g, uint32_t y) {
  const uint32_t lo = ((y & 0xffffu) - 1u) < 0x7fffu ? 0x0000ffffu : 0u;
  const uint32_t hi = ((y >> 16) - 1u) < 0x7fffu ? 0xffff0000u : 0u;
  return g & (lo | hi);
}
__device__ __forceinline__ uint4 mask_pos(const uint4& g, const uint4& y) {
  return make_uint4(mask_pos2(g.x, y.x), mask_pos2(g.y, y.y), mask_pos2(g.z, y.z), mask_pos2(g.w, y.w));
}

// a thread's share of a C8 row: unit u = tid + 256 k <-> (channel block u / W, pixel u % W), the same for every row
struct RowUnits {
  int units, ldsoff[CB_UMAX];              // byte offset of the unit in an LDS row of `bs` bytes per block, `pad` zero pixels in front
  __device__ __forceinline__ RowUnits(int C8, int W, int bs, int pad) : units(C8 * W) {
#pragma unroll
    for (int k = 0; k < CB_UMAX; ++k) {
      const int u = (int)threadIdx.x + 256 * k, blk = u / W;
      ldsoff[k] = blk * bs + (pad + u - blk * W) * 16;
    }
  }
  template <typename T> __device__ __forceinline__ void load(const T* row, uint4 (&v)[CB_UMAX]) const {
#pragma unroll
    for (int k = 0; k < CB_UMAX; ++k) {
      const int u = (int)threadIdx.x + 256 * k;
      v[k] = make_uint4(0, 0, 0, 0);
      if (u < units) v[k] = *reinterpret_cast<const uint4*>(row + (int64_t)u * 8);
    }
  }
};

// ---- the data gradient -------------------------------------------------------------------------------------------------
// LDS: ring of R = 2d+1 rows, each 4 KCH channel blocks x (16 MT + 2d) pixels x 16 bytes, zero wherever no row is written;
// then the outgoing C8 row, (C/8) W x 16 bytes.  75 520 bytes at C = 80, W = 64, d = 2.
template <typename T, int KCH, int TPW>
__global__ __launch_bounds__(256, 1) void conv_relu_dgrad_kernel(ConvBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NST = 9 * KCH;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
  const int W = p.W, C = p.C, T_ = p.T, d = p.dil, R = 2 * d + 1;
  const int MT = (W + 15) >> 4, NT = (C + 15) >> 4;
  const int BS = (MT * 16 + 2 * d) * 16, SLOT = KCH * 4 * BS;
  char* sOut = smem + R * SLOT;
  for (int i = tid; i < R * SLOT / 16; i += 256) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);

  // this wave's A fragments: rows ci = 16 tile + li, k = co = 32 cci + 8 lg .. + 8, steps ordered (tap row, chunk, tap column)
  uint4 wreg[TPW][NST];
  {
    const T* wt = reinterpret_cast<const T*>(p.wt);
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      const int ci = (wv + 4 * k) * 16 + li;
#pragma unroll
      for (int st = 0; st < NST; ++st) {
        const int jp = st % 3, cci = (st / 3) % KCH, ip = st / (3 * KCH);
        wreg[k][st] = make_uint4(0, 0, 0, 0);
        if (ci < C) wreg[k][st] = *reinterpret_cast<const uint4*>(wt + ((int64_t)ci * 9 + ip * 3 + jp) * p.CP + cci * 32 + lg * 8);
      }
    }
  }
  const RowUnits ru(C >> 3, W, BS, d);
  const int n = (int)blockIdx.x / p.blocks_per_seq;
  const int r0 = ((int)blockIdx.x - n * p.blocks_per_seq) * p.rows_per_block, r1 = min(T_, r0 + p.rows_per_block);
  const int64_t rowlen = (int64_t)C * W;
  const T* gn = reinterpret_cast<const T*>(p.g) + (int64_t)n * T_ * rowlen;
  const T* yn = reinterpret_cast<const T*>(p.y) + (int64_t)n * T_ * rowlen;
  T* dxn = reinterpret_cast<T*>(p.dx) + (int64_t)n * T_ * rowlen;
  uint4 gv[CB_UMAX], yv[CB_UMAX];
  auto put = [&](int t) {                                    // the masked row t into its slot
    char* s = smem + (t % R) * SLOT;
#pragma unroll
    for (int k = 0; k < CB_UMAX; ++k)
      if (tid + 256 * k < ru.units) *reinterpret_cast<uint4*>(s + ru.ldsoff[k]) = mask_pos(gv[k], yv[k]);
  };
  __syncthreads();                                           // the zeros are down before any row lands on them
  for (int t = r0; t < min(T_, r0 + 2 * d); ++t) {           // rows r0 .. r0 + 2d - 1; the loop adds the halo row by row
    ru.load(gn + t * rowlen, gv); ru.load(yn + t * rowlen, yv);
    put(t);
  }
  if (r0 + 2 * d < T_) { ru.load(gn + (r0 + 2 * d) * rowlen, gv); ru.load(yn + (r0 + 2 * d) * rowlen, yv); }

  const char* lane_rd = smem + lg * BS + li * 16;            // + slot + cci 4 BS + (16 mt + j' d) 16
#pragma unroll 1
  for (int t = r0; t < r1; ++t) {
    if (t + 2 * d < T_) put(t + 2 * d);                      // into the slot of row t - 1, which nobody reads any more
    __syncthreads();
    if (t + 1 < r1 && t + 1 + 2 * d < T_) { ru.load(gn + (t + 1 + 2 * d) * rowlen, gv); ru.load(yn + (t + 1 + 2 * d) * rowlen, yv); }
    cf4 acc[TPW][4];
#pragma unroll
    for (int k = 0; k < TPW; ++k)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[k][mt] = cf4{0.f, 0.f, 0.f, 0.f};
    if (wv < NT) {
#pragma unroll
      for (int ip = 0; ip < 3; ++ip) {
        const int tr = t + ip * d;
        if (tr < T_) {                                       // (wave-uniform) rows past the sequence's end are zero
          const char* s = lane_rd + (tr % R) * SLOT;
#pragma unroll
          for (int cci = 0; cci < KCH; ++cci)
#pragma unroll
            for (int jp = 0; jp < 3; ++jp) {
              const int st = (ip * KCH + cci) * 3 + jp;
              const char* a = s + cci * 4 * BS + jp * d * 16;
#pragma unroll
              for (int mt = 0; mt < 4; ++mt)
                if (mt < MT) {
                  const cu4 b = *reinterpret_cast<const cu4*>(a + mt * 256);
#pragma unroll
                  for (int k = 0; k < TPW; ++k)
                    if (wv + 4 * k < NT) acc[k][mt] = Mfma16<T>::run(wreg[k][st], b, acc[k][mt]);
                }
            }
        }
      }
      // D: column li = pixel, rows 4 lg + r = four consecutive channels
#pragma unroll
      for (int k = 0; k < TPW; ++k)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          const int px = mt * 16 + li, c0 = (wv + 4 * k) * 16 + 4 * lg;
          if (px < W && c0 < C)
            *reinterpret_cast<uint2*>(sOut + (((c0 >> 3) * W + px) * 8 + (c0 & 7)) * 2) =
                make_uint2(pack2<T>(acc[k][mt][0], acc[k][mt][1]), pack2<T>(acc[k][mt][2], acc[k][mt][3]));
        }
    }
    __syncthreads();
    T* dst = dxn + t * rowlen;
#pragma unroll
    for (int k = 0; k < CB_UMAX; ++k) {
      const int u = tid + 256 * k;
      if (u < ru.units) *reinterpret_cast<uint4*>(dst + (int64_t)u * 8) = *reinterpret_cast<const uint4*>(sOut + u * 16);
    }
  }
}

// ---- the weight gradient -----------------------------------------------------------------------------------------------
// one fragment: channels 16 tile .. + 16 (blocks blk0, blk0 + 1) x pixels px .. px + 8 of an LDS row, lane li <-> channel
__device__ __forceinline__ uint4 tr_frag(const char* row, int BS, int blk0, int px) {
  const int i = threadIdx.x & 15, q = i >> 2, pp = i & 3;
  const char* a = row + (blk0 + (pp >> 1)) * BS + (px + q) * 16 + (pp & 1) * 8;
  const cb_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((cb_s4 __attribute__((address_space(3)))*)(a));
  const cb_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((cb_s4 __attribute__((address_space(3)))*)(a + 64));
  const uint2 l = __builtin_bit_cast(uint2, lo), h = __builtin_bit_cast(uint2, hi);
  return make_uint4(l.x, l.y, h.x, h.y);
}

// LDS: R = 2d+1 x rows and one dp row, each 2 NT channel blocks x (32 KS + 2d) pixels x 16 bytes, zero wherever no row is
// written (the pads, the pixels up to the k-step, the odd tile's second block).  65 280 bytes at C = 80, W = 64, d = 2.
// NI: kernel rows per workgroup: 3, or 1 with gridDim.y = 3.
template <typename T, int NT, int NI>
__global__ __launch_bounds__(256, 1) void conv_relu_wgrad_kernel(ConvBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TP = (NT * NT + 3) / 4;                      // (co tile, ci tile) pairs per wave
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
  const int W = p.W, C = p.C, T_ = p.T, d = p.dil, R = 2 * d + 1;
  const int KS = (W + 31) >> 5;
  const int BS = (KS * 32 + 2 * d) * 16, SLOT = 2 * NT * BS;
  char* sDP = smem + R * SLOT;
  for (int i = tid; i < (R + 1) * SLOT / 16; i += 256) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);
  const int i0 = NI == 3 ? 0 : (int)blockIdx.y;

  const RowUnits ru(C >> 3, W, BS, d);
  const int n = (int)blockIdx.x / p.blocks_per_seq;
  const int r0 = ((int)blockIdx.x - n * p.blocks_per_seq) * p.rows_per_block, r1 = min(T_, r0 + p.rows_per_block);
  const int64_t rowlen = (int64_t)C * W;
  const T* xn = reinterpret_cast<const T*>(p.x) + (int64_t)n * T_ * rowlen;
  const T* gn = reinterpret_cast<const T*>(p.g) + (int64_t)n * T_ * rowlen;
  const T* yn = reinterpret_cast<const T*>(p.y) + (int64_t)n * T_ * rowlen;
  uint4 xv[CB_UMAX], gv[CB_UMAX], yv[CB_UMAX];
  auto put_x = [&](int t) {
    char* s = smem + (t % R) * SLOT;
#pragma unroll
    for (int k = 0; k < CB_UMAX; ++k)
      if (tid + 256 * k < ru.units) *reinterpret_cast<uint4*>(s + ru.ldsoff[k]) = xv[k];
  };
  float dbacc[CB_UMAX][8];
#pragma unroll
  for (int k = 0; k < CB_UMAX; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) dbacc[k][e] = 0.f;
  cf4 acc[TP][NI * 3];
#pragma unroll
  for (int k = 0; k < TP; ++k)
#pragma unroll
    for (int a = 0; a < NI * 3; ++a) acc[k][a] = cf4{0.f, 0.f, 0.f, 0.f};

  __syncthreads();                                           // the zeros are down before any row lands on them
  for (int t = max(0, r0 - 2 * d); t < r0; ++t) {            // the 2d rows before the block (those of this sequence)
    ru.load(xn + t * rowlen, xv);
    put_x(t);
  }
  ru.load(xn + r0 * rowlen, xv); ru.load(gn + r0 * rowlen, gv); ru.load(yn + r0 * rowlen, yv);

#pragma unroll 1
  for (int t = r0; t < r1; ++t) {
    put_x(t);                                                // into the slot of row t - 2d - 1
#pragma unroll
    for (int k = 0; k < CB_UMAX; ++k)
      if (tid + 256 * k < ru.units) {
        const uint4 dp = mask_pos(gv[k], yv[k]);
        *reinterpret_cast<uint4*>(sDP + ru.ldsoff[k]) = dp;
        float f[8];
        unpack16<T>(dp, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) dbacc[k][e] += f[e];
      }
    __syncthreads();
    if (t + 1 < r1) { ru.load(xn + (t + 1) * rowlen, xv); ru.load(gn + (t + 1) * rowlen, gv); ru.load(yn + (t + 1) * rowlen, yv); }
    for (int ks = 0; ks < KS; ++ks) {
      const int px = d + ks * 32 + lg * 8;                   // this lane group's 8 pixels of the k-step (after the front pad)
#pragma unroll
      for (int k = 0; k < TP; ++k) {
        const int pr = wv + 4 * k;
        if (pr < NT * NT) {                                  // (wave-uniform)
          const int mo = pr / NT, mi = pr - mo * NT;
          const uint4 a = tr_frag(sDP, BS, 2 * mo, px);
#pragma unroll
          for (int ii = 0; ii < NI; ++ii) {
            const int tr = t - (2 - (i0 + ii)) * d;
            if (tr >= 0) {                                   // (wave-uniform) rows before the sequence are zero
              const char* s = smem + (tr % R) * SLOT;
#pragma unroll
              for (int j = 0; j < 3; ++j) {
                const uint4 b = tr_frag(s, BS, 2 * mi, px + (j - 1) * d);
                acc[k][ii * 3 + j] = Mfma16<T>::run(a, __builtin_bit_cast(cu4, b), acc[k][ii * 3 + j]);
              }
            }
          }
        }
      }
    }
    __syncthreads();
  }

  // ---- the block's part: dW[co][ci][i][j] (D: rows 4 lg + r = co, column li = ci), then db
  float* part = p.part + (int64_t)blockIdx.x * (9 * C * C + C);
#pragma unroll
  for (int k = 0; k < TP; ++k) {
    const int pr = wv + 4 * k;
    if (pr < NT * NT) {
      const int mo = pr / NT, mi = pr - mo * NT, ci = mi * 16 + li;
#pragma unroll
      for (int a = 0; a < NI * 3; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = mo * 16 + 4 * lg + r;
          if (co < C && ci < C) part[((int64_t)co * C + ci) * 9 + i0 * 3 + a] = acc[k][a][r];
        }
    }
  }
  if (i0 == 0) {                                             // (workgroup-uniform)
    float* sRed = reinterpret_cast<float*>(smem);            // (C/8) W x 8: the last barrier of the loop freed the rows
#pragma unroll
    for (int k = 0; k < CB_UMAX; ++k) {
      const int u = tid + 256 * k;
      if (u < ru.units) {
#pragma unroll
        for (int e = 0; e < 8; ++e) sRed[u * 8 + e] = dbacc[k][e];
      }
    }
    __syncthreads();
    if (tid < C) {
      float s = 0.f;
      for (int w = 0; w < W; ++w) s += sRed[((tid >> 3) * W + w) * 8 + (tid & 7)];
      part[9 * C * C + tid] = s;
    }
  }
}

// WT[ci][i'][j'][co] = Wt[co][ci][2 - i'][2 - j'] from the forward's image [co][tap][ci]; co zero-padded to CP
__global__ __launch_bounds__(256) void conv_bwd_pack_kernel(const unsigned short* w, unsigned short* wt, int C, int CP) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= C * 9 * CP) return;
  const int co = idx % CP, tp = (idx / CP) % 9, ci = idx / (CP * 9);
  wt[idx] = co < C ? w[((int64_t)co * 9 + (8 - tp)) * CP + ci] : (unsigned short)0;
}

// out[i] = sum over the blocks of part[b][i], in block order: the same bits every run
__global__ __launch_bounds__(256) void conv_bwd_reduce(const float* part, int64_t blocks, int nW, int C, float* d_w, float* d_b) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nW + C) return;
  float s = 0.f;
  for (int64_t b = 0; b < blocks; ++b) s += part[b * (nW + C) + i];
  if (i < nW) d_w[i] = s;
  else d_b[i - nW] = s;
}

// rows per workgroup: the shapes alone decide it (not the device), so the parts and their sum are the same everywhere
int64_t conv_bwd_block_rows(int64_t N, int64_t T) {
  const int64_t r = (N * T + 511) / 512;
  return r < 8 ? 8 : r > 64 ? 64 : r;
}
int64_t conv_bwd_blocks_per_seq(int64_t N, int64_t T) {
  const int64_t rb = conv_bwd_block_rows(N, T);
  return (T + rb - 1) / rb;
}

bool conv_bwd_supported(int64_t C, int64_t W, int ksize, int dilation, int pad_w, int dtype) {
  if (ksize != 3 || C < 8 || C % 8 != 0 || C > 128 || W < 8 || W % 8 != 0 || W > 64) return false;
  if (!(dilation == 1 || dilation == 2) || pad_w != dilation || !(dtype == SEA_F16 || dtype == SEA_BF16)) return false;
  // the 16-bit forward form: its LDS weight image (sea_conv.hip, launch_conv) within 160 KB
  const int64_t nt = (C + 15) / 16, cinp = (C + 31) / 32 * 32;
  return 9 * (cinp / 32) * 4 * (16 * nt) * 16 + 16 * nt * 4 <= CB_MAX_LDS;
}
int64_t conv_bwd_wt_bytes(int64_t C) { return (C * 9 * ((C + 31) / 32 * 32) * 2 + 15) / 16 * 16; }

template <typename T, int KCH, int TPW>
int launch_dgrad_k(const ConvBwdParams& p, unsigned blocks, size_t lds, hipStream_t s) {
  static DevOnce once;
  if (once.first()) SEA_MAX_LDS((conv_relu_dgrad_kernel<T, KCH, TPW>), CB_MAX_LDS);
  hipLaunchKernelGGL((conv_relu_dgrad_kernel<T, KCH, TPW>), dim3(blocks), dim3(256), lds, s, p);
  return SEA_OK;
}
template <typename T>
int launch_dgrad(const ConvBwdParams& p, unsigned blocks, hipStream_t s) {
  const int kch = p.CP / 32, mt = (p.W + 15) / 16, R = 2 * p.dil + 1;
  const size_t lds = (size_t)R * kch * 4 * (mt * 16 + 2 * p.dil) * 16 + (size_t)(p.C / 8) * p.W * 16;
  if (kch == 1) return launch_dgrad_k<T, 1, 1>(p, blocks, lds, s);
  if (kch == 2) return launch_dgrad_k<T, 2, 1>(p, blocks, lds, s);
  return launch_dgrad_k<T, 3, 2>(p, blocks, lds, s);          // 64 < C <= 80: five ci tiles, two for wave 0
}

template <typename T, int NT, int NI>
int launch_wgrad_k(const ConvBwdParams& p, unsigned blocks, size_t lds, hipStream_t s) {
  static DevOnce once;
  if (once.first()) SEA_MAX_LDS((conv_relu_wgrad_kernel<T, NT, NI>), CB_MAX_LDS);
  hipLaunchKernelGGL((conv_relu_wgrad_kernel<T, NT, NI>), dim3(blocks, NI == 3 ? 1 : 3), dim3(256), lds, s, p);
  return SEA_OK;
}
template <typename T>
int launch_wgrad(const ConvBwdParams& p, unsigned blocks, hipStream_t s) {
  const int nt = (p.C + 15) / 16, ks = (p.W + 31) / 32, R = 2 * p.dil + 1;
  const size_t lds = (size_t)(R + 1) * 2 * nt * (ks * 32 + 2 * p.dil) * 16;
  switch (nt) {
    case 1: return launch_wgrad_k<T, 1, 3>(p, blocks, lds, s);
    case 2: return launch_wgrad_k<T, 2, 3>(p, blocks, lds, s);
    case 3: return launch_wgrad_k<T, 3, 3>(p, blocks, lds, s);
    case 4: return launch_wgrad_k<T, 4, 3>(p, blocks, lds, s);
    default: return launch_wgrad_k<T, 5, 1>(p, blocks, lds, s);   // 25 tile pairs: the output split by kernel row
  }
}

}  // namespace
}  // namespace sea

using namespace sea;

extern "C" int sea_predictor_cnn_grad_version(void) { return SEA_PREDICTOR_CNN_GRAD_ABI_VERSION; }

extern "C" int sea_causal_conv_relu_bwd_supported(int64_t C, int64_t W, int ksize, int dilation, int pad_w, int dtype) {
  return conv_bwd_supported(C, W, ksize, dilation, pad_w, dtype) ? 1 : 0;
}

extern "C" int64_t sea_causal_conv_relu_bwd_workspace_bytes(int64_t N, int64_t T, int64_t W, int64_t C, int dilation, int dtype) {
  if (N <= 0 || T <= 0 || N * T >= (1ll << 30) || !conv_bwd_supported(C, W, 3, dilation, dilation, dtype)) return 0;
  return conv_bwd_wt_bytes(C) + (N * conv_bwd_blocks_per_seq(N, T) * (9 * C * C + C) * (int64_t)sizeof(float) + 15) / 16 * 16;
}

extern "C" int sea_causal_conv_relu_bwd(const void* x, const void* y, const void* g, int dtype, int64_t N, int64_t T, int64_t W,
                                        int64_t C, const void* w_packed, int64_t CinP, int dilation, int pad_w, void* d_x,
                                        float* d_w, float* d_b, void* workspace, int64_t workspace_bytes, sea_stream_t stream) {
  const char* nm = "sea_causal_conv_relu_bwd";
#define SEA_CB_NONNULL(a) SEA_REQUIRE((a) != nullptr, SEA_EINVAL, "%s: " #a " is null", nm)
  SEA_CB_NONNULL(x); SEA_CB_NONNULL(y); SEA_CB_NONNULL(g); SEA_CB_NONNULL(w_packed); SEA_CB_NONNULL(d_w); SEA_CB_NONNULL(d_b);
  SEA_CB_NONNULL(workspace);
#undef SEA_CB_NONNULL
  SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: unknown dtype %d", nm, dtype);
  SEA_REQUIRE(dtype != SEA_F32, SEA_EUNSUPPORTED, "%s: fp32 data has no backward kernel (16-bit data only)", nm);
  SEA_REQUIRE(N > 0 && T > 0 && W > 0 && C > 0 && CinP > 0 && dilation > 0 && pad_w >= 0, SEA_EINVAL,
              "%s: bad shape N=%lld T=%lld W=%lld C=%lld CinP=%lld dilation=%d pad_w=%d", nm, (long long)N, (long long)T, (long long)W,
              (long long)C, (long long)CinP, dilation, pad_w);
  SEA_REQUIRE(C % 8 == 0 && conv_bwd_supported(C, 8, 3, 1, 1, dtype), SEA_EUNSUPPORTED,
              "%s: C=%lld has no backward kernel (C %% 8 == 0, the forward's 16-bit weight image within its LDS: C <= 80)", nm, (long long)C);
  SEA_REQUIRE(CinP == (C + 31) / 32 * 32, SEA_EINVAL, "%s: CinP=%lld is not C=%lld rounded up to 32", nm, (long long)CinP, (long long)C);
  SEA_REQUIRE(dilation <= 2 && pad_w == dilation, SEA_EUNSUPPORTED, "%s: dilation=%d, pad_w=%d: needs dilation 1 or 2 and pad_w = dilation",
              nm, dilation, pad_w);
  SEA_REQUIRE(W % 8 == 0 && W <= 64, SEA_EUNSUPPORTED, "%s: W=%lld has no backward kernel (a multiple of 8 up to 64)", nm, (long long)W);
  SEA_REQUIRE(N * T < (1ll << 30), SEA_EUNSUPPORTED, "%s: N*T=%lld beyond the limit", nm, (long long)(N * T));
  SEA_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)g | (uintptr_t)w_packed) & 15) == 0, SEA_EINVAL,
              "%s: x, y, g, w_packed must be 16-byte aligned", nm);
  SEA_REQUIRE((((uintptr_t)d_x | (uintptr_t)d_w | (uintptr_t)d_b) & 15) == 0, SEA_EINVAL, "%s: d_x, d_w, d_b must be 16-byte aligned", nm);
  const int64_t need = sea_causal_conv_relu_bwd_workspace_bytes(N, T, W, C, dilation, dtype);
  SEA_REQUIRE(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need, SEA_EINVAL,
              "%s: workspace of %lld bytes needed (16-byte aligned), got %lld", nm, (long long)need, (long long)workspace_bytes);

  ConvBwdParams p;
  p.x = x; p.y = y; p.g = g; p.wt = workspace; p.dx = d_x;
  p.part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + conv_bwd_wt_bytes(C));
  p.T = (int)T; p.W = (int)W; p.C = (int)C; p.CP = (int)CinP; p.dil = dilation;
  p.rows_per_block = (int)conv_bwd_block_rows(N, T); p.blocks_per_seq = (int)conv_bwd_blocks_per_seq(N, T);
  const unsigned blocks = (unsigned)(N * p.blocks_per_seq);
  hipStream_t s = (hipStream_t)stream;
  const int nwt = (int)(C * 9 * CinP);
  hipLaunchKernelGGL(conv_bwd_pack_kernel, dim3((unsigned)((nwt + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const unsigned short*>(w_packed), reinterpret_cast<unsigned short*>(workspace), (int)C, (int)CinP);
  SEA_CHECK_LAUNCH(nm);
  int rc = SEA_OK;
  if (d_x != nullptr) {
    rc = dtype == SEA_BF16 ? launch_dgrad<__hip_bfloat16>(p, blocks, s) : launch_dgrad<__half>(p, blocks, s);
    if (rc != SEA_OK) return rc;
    SEA_CHECK_LAUNCH(nm);
  }
  rc = dtype == SEA_BF16 ? launch_wgrad<__hip_bfloat16>(p, blocks, s) : launch_wgrad<__half>(p, blocks, s);
  if (rc != SEA_OK) return rc;
  SEA_CHECK_LAUNCH(nm);
  const int nW = (int)(9 * C * C);
  hipLaunchKernelGGL(conv_bwd_reduce, dim3((unsigned)((nW + C + 255) / 256)), dim3(256), 0, s, p.part, (int64_t)blocks, nW, (int)C, d_w,
                     d_b);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}
