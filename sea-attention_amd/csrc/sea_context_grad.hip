// The sparse context branch under autograd (include/sea_hip_context_grad.h): everything around the sparse product o between
// q, k, v and the (N, T, H D) context -- the cumulative average of v, its rounding to the data type, the row scale, the mix, the
// permute and the cast -- forwards in one pass over o, v and ctx, backwards in two (one before and one after the unchanged
// sea_sparse_attention_bwd).  gfx950 only.
//
// Every scan along T is cut into CH = 64-row chunks and done on two levels: ctx_chunk_sums writes one column sum per (n, h, chunk)
// to the workspace, and each workgroup of the other kernels adds the sums of the chunks before it (after it, for the suffix scan of
// dv) in one fixed order before it scans its own 64 rows in LDS.  The grid is (N H, chunks) at every shape: nothing walks T, and
// one sequence fills the chip as a batch does.  No floating-point atomics, one summation order: the same inputs give the same bits,
// and the backward recomputes the very average the forward mixed in (avg_chunk is the one routine both call).
//
// Work split (256 threads, 4 waves): a row of D elements is D / 8 UNITS of 8 columns; a unit is one 16-byte load of 16-bit data
// (two of fp32).  Staging and the element-wise passes deal units to threads round-robin, so a wave's loads of a row are contiguous.
// The in-chunk scan runs down the rows with one lane per column (LDS reads of a row are then conflict-free).  ctx_mix_bwd gives
// each row to one DPP row of 16 lanes (D / 8 <= 16 of them hold a unit): the two D-wide dot products of a row are four DPP steps.
#include "sea_common.hpp"
#include "../../include/sea_hip_context_grad.h"

namespace sea {
namespace {

constexpr int CH = 64;          // rows per chunk
constexpr int CTX_THREADS = 256;
constexpr int CTX_GY = 32768;   // chunks per grid.y slice (grid.z takes the rest: T < 2^24 gives up to 2^18 chunks)

struct CtxParams {
  const void* v;
  int64_t v_sn, v_sh, v_st;
  const float* o;            // (N,H,T,D) fp32: the unscaled sparse product
  const void* g;             // (N,T,H D) of the output type: d ctx
  const float* row_scale;    // (N,H,T) or null
  const float* mix;          // (N,H,T)
  void* ctx;                 // (N,T,H D) of the output type
  float* d_o;                // (N,H,T,D) fp32
  float* d_rs;               // (N,H,T) or null
  float* d_mix;              // (N,H,T) or null
  const float* dv_attn;      // (N,H,T,D) fp32
  void* dv;                  // (N,H,T,D) of the data type
  float* vsum;               // workspace: (N H, chunks, D) column sums of v
  float* wsum;               // workspace: (N H, chunks, D) column sums of w
  int H, T, chunks;
};

__device__ inline int chunk_of_block() { return (int)(blockIdx.z * CTX_GY + blockIdx.y); }

// eight consecutive elements as fp32 / from fp32, 16 bytes per access
template <typename T> __device__ inline void load8(const T* p, float* f) {
  if constexpr (sizeof(T) == 4) {
    unpack16<float>(*reinterpret_cast<const uint4*>(p), f);
    unpack16<float>(*reinterpret_cast<const uint4*>(p + 4), f + 4);
  } else {
    unpack16<T>(*reinterpret_cast<const uint4*>(p), f);
  }
}
template <typename T> __device__ inline void store8(T* p, const float* f) {
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
  } else {
    uint4 r;
    r.x = pack2<T>(f[0], f[1]); r.y = pack2<T>(f[2], f[3]); r.z = pack2<T>(f[4], f[5]); r.w = pack2<T>(f[6], f[7]);
    *reinterpret_cast<uint4*>(p) = r;
  }
}
template <typename T> __device__ inline float round_to(float x) { return Elem<T>::to_f(from_f<T>(x)); }

// sum over the 16 lanes of a DPP row; every lane of the row ends with the same bits
__device__ inline float row16_sum(float v) {
  v += __uint_as_float(dpp_u32<0xB1>(__float_as_uint(v)));     // quad_perm [1,0,3,2]
  v += __uint_as_float(dpp_u32<0x4E>(__float_as_uint(v)));     // quad_perm [2,3,0,1]
  v += __uint_as_float(dpp_u32<0x141>(__float_as_uint(v)));    // row_half_mirror
  v += __uint_as_float(dpp_u32<0x140>(__float_as_uint(v)));    // row_mirror
  return v;
}

// w[t] = (1 - a_t) g_t / (t + 1): what row t's gradient sends to every row s <= t of v through the average
__device__ inline float w_of(float a, float g, int t) { return __fdiv_rn((1.0f - a) * g, (float)(t + 1)); }

// the chunk's rows of v (pair nh = n H + h, rows r0 .. r0 + nrows) as fp32 in s[r * D + col]
template <typename T, int D> __device__ inline void stage_v(const CtxParams& p, int n, int h, int r0, int nrows, float* s) {
  constexpr int UPR = D / 8;
  const T* base = static_cast<const T*>(p.v) + n * p.v_sn + h * p.v_sh;
  for (int u = threadIdx.x; u < nrows * UPR; u += CTX_THREADS) {
    const int r = u / UPR, cg = u - r * UPR;
    float f[8];
    load8<T>(base + (int64_t)(r0 + r) * p.v_st + cg * 8, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) s[r * D + cg * 8 + i] = f[i];
  }
}

// the chunk's rows of w, from g and a, in s[r * D + col]
template <typename TO, int D> __device__ inline void stage_w(const CtxParams& p, int n, int h, int r0, int nrows, float* s) {
  constexpr int UPR = D / 8;
  const TO* g = static_cast<const TO*>(p.g);
  const float* mix = p.mix + ((int64_t)n * p.H + h) * p.T;
  for (int u = threadIdx.x; u < nrows * UPR; u += CTX_THREADS) {
    const int r = u / UPR, cg = u - r * UPR, t = r0 + r;
    const float a = mix[t];
    float f[8];
    load8<TO>(g + (((int64_t)n * p.T + t) * p.H + h) * D + cg * 8, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) s[r * D + cg * 8 + i] = w_of(a, f[i], t);
  }
}

// s[r * D + col] := round_T(cumavg(v)[r0 + r][col]).  Carry = the column sums of chunks 0 .. c - 1 in ascending order, then the
// chunk's own rows in ascending order: the forward and the backward both come through here, so they see the same bits.
template <typename T, int D> __device__ inline void avg_chunk(const CtxParams& p, int n, int h, int c, int r0, int nrows, float* s) {
  stage_v<T, D>(p, n, h, r0, nrows, s);
  __syncthreads();
  if (threadIdx.x < D) {
    const int col = threadIdx.x;
    const float* vs = p.vsum + ((int64_t)n * p.H + h) * p.chunks * D + col;
    float run = 0.0f;
    for (int j = 0; j < c; ++j) run += vs[(int64_t)j * D];
    for (int r = 0; r < nrows; ++r) {
      run += s[r * D + col];
      s[r * D + col] = round_to<T>(__fdiv_rn(run, (float)(r0 + r + 1)));
    }
  }
  __syncthreads();
}

// ---- 1. per-chunk column sums: of v, and with BWD of w as well --------------------------------------------------------------
// Each wave sums a quarter of the chunk's rows per column, the four parts are added in wave order.
template <typename T, typename TO, int D, bool BWD>
__global__ __launch_bounds__(CTX_THREADS) void ctx_chunk_sums(const CtxParams p) {
  __shared__ float s[CH * D];
  __shared__ float part[4 * D];
  const int c = chunk_of_block();
  if (c >= p.chunks) return;
  const int nh = blockIdx.x, n = nh / p.H, h = nh - n * p.H;
  const int r0 = c * CH, nrows = min(CH, p.T - r0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int which = 0; which < (BWD ? 2 : 1); ++which) {
    if (which == 0) stage_v<T, D>(p, n, h, r0, nrows, s);
    else stage_w<TO, D>(p, n, h, r0, nrows, s);
    __syncthreads();
    const int ra = wave * (CH / 4), rb = min(nrows, ra + CH / 4);
    for (int col = lane; col < D; col += 64) {
      float sum = 0.0f;
      for (int r = ra; r < rb; ++r) sum += s[r * D + col];
      part[wave * D + col] = sum;
    }
    __syncthreads();
    if (threadIdx.x < D) {
      const int col = threadIdx.x;
      const float sum = ((part[col] + part[D + col]) + part[2 * D + col]) + part[3 * D + col];
      (which == 0 ? p.vsum : p.wsum)[((int64_t)nh * p.chunks + c) * D + col] = sum;
    }
    __syncthreads();                                   // s and part are free for the second pass
  }
}

// ---- 2. forward: average, rounding, scale, mix, permute and cast in one pass -----------------------------------------------
template <typename T, typename TO, int D>
__global__ __launch_bounds__(CTX_THREADS) void ctx_mix_fwd(const CtxParams p) {
  __shared__ float s[CH * D];
  constexpr int UPR = D / 8;
  const int c = chunk_of_block();
  if (c >= p.chunks) return;
  const int nh = blockIdx.x, n = nh / p.H, h = nh - n * p.H;
  const int r0 = c * CH, nrows = min(CH, p.T - r0);
  avg_chunk<T, D>(p, n, h, c, r0, nrows, s);
  const float* mix = p.mix + (int64_t)nh * p.T;
  const float* rs = p.row_scale ? p.row_scale + (int64_t)nh * p.T : nullptr;
  TO* out = static_cast<TO*>(p.ctx);
  for (int u = threadIdx.x; u < nrows * UPR; u += CTX_THREADS) {
    const int r = u / UPR, cg = u - r * UPR, t = r0 + r;
    const float a = mix[t], sc = rs ? rs[t] : 1.0f;
    float o[8], f[8];
    load8<float>(p.o + ((int64_t)nh * p.T + t) * D + cg * 8, o);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (o[i] * sc) * a + (1.0f - a) * s[r * D + cg * 8 + i];
    store8<TO>(out + (((int64_t)n * p.T + t) * p.H + h) * D + cg * 8, f);
  }
}

// ---- 3. backward of the mix: dO for the attention backward, d row_scale, d mix ----------------------------------------------
template <typename T, typename TO, int D>
__global__ __launch_bounds__(CTX_THREADS) void ctx_mix_bwd(const CtxParams p) {
  __shared__ float s[CH * D];
  constexpr int UPR = D / 8;
  static_assert(UPR <= 16, "a row's units fit one DPP row of 16 lanes");
  const int c = chunk_of_block();
  if (c >= p.chunks) return;
  const int nh = blockIdx.x, n = nh / p.H, h = nh - n * p.H;
  const int r0 = c * CH, nrows = min(CH, p.T - r0);
  avg_chunk<T, D>(p, n, h, c, r0, nrows, s);
  const float* mix = p.mix + (int64_t)nh * p.T;
  const float* rs = p.row_scale ? p.row_scale + (int64_t)nh * p.T : nullptr;
  const TO* g = static_cast<const TO*>(p.g);
  const int rg = threadIdx.x >> 4, cg = threadIdx.x & 15;
#pragma unroll 1
  for (int pass = 0; pass < CH / 16; ++pass) {          // every lane runs every pass: the DPP sums need the whole row of lanes
    const int r = pass * 16 + rg, t = r0 + r;
    const bool row = r < nrows, unit = row && cg < UPR;
    const float a = row ? mix[t] : 0.0f, sc = (row && rs) ? rs[t] : 1.0f;
    float go = 0.0f, gm = 0.0f;                         // g . o and g . (rs o - avg) over this lane's 8 columns
    if (unit) {
      float gv[8], o[8], f[8];
      load8<TO>(g + (((int64_t)n * p.T + t) * p.H + h) * D + cg * 8, gv);
      load8<float>(p.o + ((int64_t)nh * p.T + t) * D + cg * 8, o);
      const float as = a * sc;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        f[i] = as * gv[i];
        go += gv[i] * o[i];
        gm += gv[i] * (sc * o[i] - s[r * D + cg * 8 + i]);
      }
      store8<float>(p.d_o + ((int64_t)nh * p.T + t) * D + cg * 8, f);
    }
    go = row16_sum(go);
    gm = row16_sum(gm);
    if (row && cg == 0) {
      if (p.d_rs) p.d_rs[(int64_t)nh * p.T + t] = a * go;
      if (p.d_mix) p.d_mix[(int64_t)nh * p.T + t] = gm;
    }
  }
}

// ---- 5. dv = dv_attn + the suffix sum of w ------------------------------------------------------------------------------------
template <typename T, typename TO, int D>
__global__ __launch_bounds__(CTX_THREADS) void ctx_dv_finish(const CtxParams p) {
  __shared__ float s[CH * D];
  constexpr int UPR = D / 8;
  const int c = chunk_of_block();
  if (c >= p.chunks) return;
  const int nh = blockIdx.x, n = nh / p.H, h = nh - n * p.H;
  const int r0 = c * CH, nrows = min(CH, p.T - r0);
  stage_w<TO, D>(p, n, h, r0, nrows, s);
  __syncthreads();
  if (threadIdx.x < D) {
    const int col = threadIdx.x;
    const float* wsum = p.wsum + (int64_t)nh * p.chunks * D + col;
    float run = 0.0f;
    for (int j = p.chunks - 1; j > c; --j) run += wsum[(int64_t)j * D];
    for (int r = nrows - 1; r >= 0; --r) {
      run += s[r * D + col];
      s[r * D + col] = run;
    }
  }
  __syncthreads();
  T* dv = static_cast<T*>(p.dv);
  for (int u = threadIdx.x; u < nrows * UPR; u += CTX_THREADS) {
    const int r = u / UPR, cg = u - r * UPR;
    const int64_t at = ((int64_t)nh * p.T + r0 + r) * D + cg * 8;
    float f[8];
    load8<float>(p.dv_attn + at, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] += s[r * D + cg * 8 + i];
    store8<T>(dv + at, f);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
enum CtxKernel { K_SUMS_FWD, K_SUMS_BWD, K_MIX_FWD, K_MIX_BWD, K_DV };

template <typename T, typename TO, int D> void launch_one(CtxKernel which, const CtxParams& p, dim3 grid, hipStream_t st) {
  switch (which) {
    case K_SUMS_FWD: hipLaunchKernelGGL((ctx_chunk_sums<T, TO, D, false>), grid, dim3(CTX_THREADS), 0, st, p); break;
    case K_SUMS_BWD: hipLaunchKernelGGL((ctx_chunk_sums<T, TO, D, true>), grid, dim3(CTX_THREADS), 0, st, p); break;
    case K_MIX_FWD: hipLaunchKernelGGL((ctx_mix_fwd<T, TO, D>), grid, dim3(CTX_THREADS), 0, st, p); break;
    case K_MIX_BWD: hipLaunchKernelGGL((ctx_mix_bwd<T, TO, D>), grid, dim3(CTX_THREADS), 0, st, p); break;
    case K_DV: hipLaunchKernelGGL((ctx_dv_finish<T, TO, D>), grid, dim3(CTX_THREADS), 0, st, p); break;
  }
}
template <typename T, typename TO> void launch_d(CtxKernel which, int64_t D, const CtxParams& p, dim3 grid, hipStream_t st) {
  if (D == 64) launch_one<T, TO, 64>(which, p, grid, st);
  else if (D == 80) launch_one<T, TO, 80>(which, p, grid, st);
  else launch_one<T, TO, 128>(which, p, grid, st);
}
template <typename T> void launch_to(CtxKernel which, int out_dtype, int64_t D, const CtxParams& p, dim3 grid, hipStream_t st) {
  if (out_dtype == SEA_F32) launch_d<T, float>(which, D, p, grid, st);
  else if (out_dtype == SEA_F16) launch_d<T, __half>(which, D, p, grid, st);
  else launch_d<T, __hip_bfloat16>(which, D, p, grid, st);
}
int launch(const char* nm, CtxKernel which, int dtype, int out_dtype, int64_t N, int64_t D, const CtxParams& p, hipStream_t st) {
  const dim3 grid((unsigned)(N * p.H), (unsigned)min(p.chunks, CTX_GY), (unsigned)((p.chunks + CTX_GY - 1) / CTX_GY));
  if (dtype == SEA_F32) launch_to<float>(which, out_dtype, D, p, grid, st);
  else if (dtype == SEA_F16) launch_to<__half>(which, out_dtype, D, p, grid, st);
  else launch_to<__hip_bfloat16>(which, out_dtype, D, p, grid, st);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}

bool known_dtype(int d) { return d == SEA_F32 || d == SEA_F16 || d == SEA_BF16; }
int64_t chunks_of(int64_t T) { return (T + CH - 1) / CH; }

// what the three entries share: dtype codes, shape, limits, v's base and strides.  0 or the refusal's code
int check_common(const char* nm, const void* v, const int64_t* v_strides, int dtype, int out_dtype, int64_t N, int64_t H, int64_t T,
                 int64_t D) {
  SEA_REQUIRE(known_dtype(dtype), SEA_EUNSUPPORTED, "%s: unknown dtype %d", nm, dtype);
  SEA_REQUIRE(known_dtype(out_dtype), SEA_EUNSUPPORTED, "%s: unknown out_dtype %d", nm, out_dtype);
  SEA_REQUIRE(N > 0 && H > 0 && T > 0 && D > 0, SEA_EINVAL, "%s: bad shape (N=%lld, H=%lld, T=%lld, D=%lld)", nm, (long long)N,
              (long long)H, (long long)T, (long long)D);
  SEA_REQUIRE(D == 64 || D == 80 || D == 128, SEA_EUNSUPPORTED, "%s: D=%lld has no kernel (64, 80, 128)", nm, (long long)D);
  SEA_REQUIRE(T < (1ll << 24), SEA_EUNSUPPORTED, "%s: T=%lld beyond the limit (T < 2^24)", nm, (long long)T);
  SEA_REQUIRE(N * H < (1ll << 31) && H < (1ll << 31), SEA_EUNSUPPORTED, "%s: N*H=%lld beyond the limit", nm, (long long)(N * H));
  if (v != nullptr) {
    const int64_t vec = dtype == SEA_F32 ? 4 : 8;
    SEA_REQUIRE(((uintptr_t)v & 15) == 0, SEA_EINVAL, "%s: v must be 16-byte aligned", nm);
    SEA_REQUIRE(v_strides[0] >= 0 && v_strides[1] >= 0 && v_strides[2] >= D && v_strides[0] % vec == 0 && v_strides[1] % vec == 0 &&
                    v_strides[2] % vec == 0,
                SEA_EINVAL, "%s: v_strides {%lld, %lld, %lld} must be multiples of %lld elements, rows apart", nm,
                (long long)v_strides[0], (long long)v_strides[1], (long long)v_strides[2], (long long)vec);
  }
  return SEA_OK;
}

}  // namespace
}  // namespace sea

using namespace sea;

extern "C" int sea_context_grad_version(void) { return SEA_CONTEXT_GRAD_ABI_VERSION; }

extern "C" int sea_context_grad_supported(int64_t T_dst, int64_t T_src, int64_t D, int dtype, int out_dtype) {
  return T_dst == T_src && T_dst > 0 && T_dst < (1ll << 24) && (D == 64 || D == 80 || D == 128) && known_dtype(dtype) &&
                 known_dtype(out_dtype)
             ? 1
             : 0;
}

extern "C" int64_t sea_context_grad_workspace_bytes(int64_t N, int64_t H, int64_t T, int64_t D, int backward) {
  if (N <= 0 || H <= 0 || T <= 0 || T >= (1ll << 24) || !(D == 64 || D == 80 || D == 128) || N * H >= (1ll << 31)) return 0;
  return (backward ? 2 : 1) * N * H * chunks_of(T) * D * 4;
}

#define SEA_CG_NONNULL(x) SEA_REQUIRE((x) != nullptr, SEA_EINVAL, "%s: " #x " is null", nm)
#define SEA_CG_WORKSPACE(bwd)                                                                                                  \
  const int64_t need = sea_context_grad_workspace_bytes(N, H, T, D, bwd);                                                      \
  SEA_REQUIRE(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need, SEA_EINVAL,                                        \
              "%s: workspace of %lld bytes needed, 16-byte aligned (got %lld)", nm, (long long)need, (long long)workspace_bytes)

extern "C" int sea_context_mix_fwd(const void* v, const int64_t* v_strides, const float* o, const float* row_scale, const float* mix,
                                   int dtype, int out_dtype, int64_t N, int64_t H, int64_t T, int64_t D, void* ctx, void* workspace,
                                   int64_t workspace_bytes, sea_stream_t stream) {
  const char* nm = "sea_context_mix_fwd";
  SEA_CG_NONNULL(v); SEA_CG_NONNULL(v_strides); SEA_CG_NONNULL(o); SEA_CG_NONNULL(mix); SEA_CG_NONNULL(ctx); SEA_CG_NONNULL(workspace);
  if (const int rc = check_common(nm, v, v_strides, dtype, out_dtype, N, H, T, D)) return rc;
  SEA_REQUIRE((((uintptr_t)o | (uintptr_t)ctx) & 15) == 0, SEA_EINVAL, "%s: o, ctx must be 16-byte aligned", nm);
  SEA_REQUIRE((((uintptr_t)row_scale | (uintptr_t)mix) & 3) == 0, SEA_EINVAL, "%s: row_scale, mix must be 4-byte aligned", nm);
  SEA_CG_WORKSPACE(0);
  CtxParams p{};
  p.v = v; p.v_sn = v_strides[0]; p.v_sh = v_strides[1]; p.v_st = v_strides[2];
  p.o = o; p.row_scale = row_scale; p.mix = mix; p.ctx = ctx;
  p.vsum = static_cast<float*>(workspace);
  p.H = (int)H; p.T = (int)T; p.chunks = (int)chunks_of(T);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p.chunks > 1)                                     // one chunk: the carry is empty, nothing reads the sums
    if (const int rc = launch(nm, K_SUMS_FWD, dtype, out_dtype, N, D, p, st)) return rc;
  return launch(nm, K_MIX_FWD, dtype, out_dtype, N, D, p, st);
}

extern "C" int sea_context_mix_bwd(const void* v, const int64_t* v_strides, const float* o, const void* g, const float* row_scale,
                                   const float* mix, int dtype, int out_dtype, int64_t N, int64_t H, int64_t T, int64_t D, float* d_o,
                                   float* d_row_scale, float* d_mix, void* workspace, int64_t workspace_bytes, sea_stream_t stream) {
  const char* nm = "sea_context_mix_bwd";
  SEA_CG_NONNULL(v); SEA_CG_NONNULL(v_strides); SEA_CG_NONNULL(o); SEA_CG_NONNULL(g); SEA_CG_NONNULL(mix); SEA_CG_NONNULL(d_o);
  SEA_CG_NONNULL(workspace);
  if (const int rc = check_common(nm, v, v_strides, dtype, out_dtype, N, H, T, D)) return rc;
  SEA_REQUIRE((((uintptr_t)o | (uintptr_t)g | (uintptr_t)d_o) & 15) == 0, SEA_EINVAL, "%s: o, g, d_o must be 16-byte aligned", nm);
  SEA_REQUIRE((((uintptr_t)row_scale | (uintptr_t)mix | (uintptr_t)d_row_scale | (uintptr_t)d_mix) & 3) == 0, SEA_EINVAL,
              "%s: row_scale, mix, d_row_scale, d_mix must be 4-byte aligned", nm);
  SEA_CG_WORKSPACE(1);
  CtxParams p{};
  p.v = v; p.v_sn = v_strides[0]; p.v_sh = v_strides[1]; p.v_st = v_strides[2];
  p.o = o; p.g = g; p.row_scale = row_scale; p.mix = mix; p.d_o = d_o; p.d_rs = d_row_scale; p.d_mix = d_mix;
  p.H = (int)H; p.T = (int)T; p.chunks = (int)chunks_of(T);
  p.vsum = static_cast<float*>(workspace);
  p.wsum = p.vsum + N * H * p.chunks * D;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p.chunks > 1)
    if (const int rc = launch(nm, K_SUMS_BWD, dtype, out_dtype, N, D, p, st)) return rc;
  return launch(nm, K_MIX_BWD, dtype, out_dtype, N, D, p, st);
}

extern "C" int sea_context_dv_finish(const void* g, const float* mix, const float* dv_attn, int dtype, int out_dtype, int64_t N,
                                     int64_t H, int64_t T, int64_t D, void* dv, const void* workspace, int64_t workspace_bytes,
                                     sea_stream_t stream) {
  const char* nm = "sea_context_dv_finish";
  SEA_CG_NONNULL(g); SEA_CG_NONNULL(mix); SEA_CG_NONNULL(dv_attn); SEA_CG_NONNULL(dv); SEA_CG_NONNULL(workspace);
  if (const int rc = check_common(nm, nullptr, nullptr, dtype, out_dtype, N, H, T, D)) return rc;
  SEA_REQUIRE((((uintptr_t)g | (uintptr_t)dv_attn | (uintptr_t)dv) & 15) == 0, SEA_EINVAL, "%s: g, dv_attn, dv must be 16-byte aligned",
              nm);
  SEA_REQUIRE(((uintptr_t)mix & 3) == 0, SEA_EINVAL, "%s: mix must be 4-byte aligned", nm);
  SEA_CG_WORKSPACE(1);
  CtxParams p{};
  p.g = g; p.mix = mix; p.dv_attn = dv_attn; p.dv = dv;
  p.H = (int)H; p.T = (int)T; p.chunks = (int)chunks_of(T);
  p.vsum = static_cast<float*>(const_cast<void*>(workspace));
  p.wsum = p.vsum + N * H * p.chunks * D;
  return launch(nm, K_DV, dtype, out_dtype, N, D, p, static_cast<hipStream_t>(stream));
}
