// Shared declarations of the fused sparse-attention kernels (sea_attn.hip: gather kernels; sea_attn_tile.hip: MFMA tile kernel).
#pragma once
#include "sea_common.hpp"

namespace sea {

struct AttnParams {
  const void *q, *k, *v;
  int64_t qs[3], ks[3], vs[3];
  int N, H, T_dst, T_src, D;
  const int32_t* crow;
  const int32_t* col;
  int64_t col_stride_n;
  const int32_t* head_off;
  const float* row_scale;
  const void* avg;
  int64_t as[3];
  const float* mix;
  void* out;
  int64_t os[3];
  float* probs;            // optional (N, probs_stride_n): rs * softmax per entry (gather kernels only)
  int64_t probs_stride_n;
  // kernel choice by plan (sea_attention_plan): `sel` = one byte per (n, h, 16-row block), 1 where the block's entries per
  // staged 16-key tile favour the MFMA tile kernel, followed by the int32 count of such blocks.  BOTH kernels are launched
  // over the same rows and read the count: when the tile blocks' share exceeds sel_num / sel_den the tile kernel runs the
  // whole launch and the gather kernel's workgroups exit at once, otherwise the other way round (round 3: since the gather
  // kernels deal rows by length, a launch split per block between the two kernels is slower than the better of them alone)
  const uint8_t* sel;
  int sel_want, TB16;
  const int32_t* sel_count;
  int sel_total, sel_num, sel_den;
  int TB;  // row blocks per (n, h): ceil(T_dst / 4)
  // fused interpolation (sea_sparse_attention with bits): the gather kernel expands the kept pixels itself -- `col` holds no
  // columns yet, the kernel WRITES them (col_w) while it walks them.  bits (N, T_dst, W) from the selection launch.
  const uint32_t* bits;
  int32_t* col_w;
  int T_m, W, max_k, is_causal, fuse_cap;
  // fused interpolation: 0 = the expanded columns stay in LDS (blocks whose lists do not fit still go through `col`): the CSR's
  // column array is NOT an output of this launch -- the caller's handle keeps its columns pending and sea_csr_emit writes
  // them if anybody ever reads them (round 4: the copy-out was 266 MB and ~50 us of the headline launch for no reader)
  int write_cols;
  // decode form of the fused interpolation (sea_sparse_attention with t_src_dev): the row widths follow *t_src_dev (the sequence
  // length, in device memory: a graph-replayed step has static arguments) while T_src above stays the FIXED capacity the
  // column ids are encoded with (head * T_src + key) and the K / V caches are laid out for.  NULL: widths follow T_src.
  const int32_t* t_src_dev;
  int t_src_stride;   // 0: one length for the batch; else sequence n's at t_src_dev[n * t_src_stride] (per-sequence positions)
  // paged K / V (a block table; sparse_attn_decode1_kernel's PAGED form): k / v are the K / V halves of a page pool,
  // strides [page, head, row]; sequence n's key r lives in page table[n * table_stride + (r >> page_shift)] at row
  // r & (page_rows - 1).  Keys and column ids stay logical (head * T_src + key): only the K / V loads translate
  const int32_t* table;
  int table_stride, page_shift;
  // rows dealt by length over pools of `pool_rows` query rows (SEA_ATTN_ROW_POOL; the ORD forms of the fused gather kernels):
  // order (N, H, pools * pool_rows) from attn_row_order_kernel -- per pool its rows' offsets, longest row first, the slots
  // past T_dst last.  NULL: every workgroup ranks its own rows (rows_by_length)
  const uint16_t* order;
  int64_t order_stride_n;
  int pool_rows, pools;
  // the order in which the grid's workgroups take their XCD's row blocks (map_block below: SEA_GRID_*, pairs per group);
  // read by the forward prefill kernels, ascending for every other launch
  int grid_order, grid_group;
};

template <typename TO, int VEC> __device__ inline void store_frag(TO* dst, const float* f);
template <> __device__ inline void store_frag<float, 4>(float* dst, const float* f) {
  *reinterpret_cast<float4*>(dst) = make_float4(f[0], f[1], f[2], f[3]);
}
template <> __device__ inline void store_frag<float, 8>(float* dst, const float* f) {
  *reinterpret_cast<float4*>(dst) = make_float4(f[0], f[1], f[2], f[3]);
  *reinterpret_cast<float4*>(dst + 4) = make_float4(f[4], f[5], f[6], f[7]);
}
template <> __device__ inline void store_frag<__hip_bfloat16, 8>(__hip_bfloat16* dst, const float* f) {
  union { uint4 u; __hip_bfloat16 h[8]; } r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.h[i] = __float2bfloat16(f[i]);
  *reinterpret_cast<uint4*>(dst) = r.u;
}
template <> __device__ inline void store_frag<__half, 8>(__half* dst, const float* f) {
  union { uint4 u; __half h[8]; } r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.h[i] = __float2half(f[i]);
  *reinterpret_cast<uint4*>(dst) = r.u;
}
template <> __device__ inline void store_frag<__hip_bfloat16, 4>(__hip_bfloat16* dst, const float* f) {
  union { uint2 u; __hip_bfloat16 h[4]; } r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.h[i] = __float2bfloat16(f[i]);
  *reinterpret_cast<uint2*>(dst) = r.u;
}
template <> __device__ inline void store_frag<__half, 4>(__half* dst, const float* f) {
  union { uint2 u; __half h[4]; } r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.h[i] = __float2half(f[i]);
  *reinterpret_cast<uint2*>(dst) = r.u;
}

// (n, h, row-block) from the workgroup index `bid`, XCD-aware: blocks b and b+8 share an XCD (observed dispatch order; only
// affects L2 locality).  Returns false if this block has no work.  The grid is 8 * ceil(NH / 8) * TB workgroups, dispatched
// in index order, so `slot` = bid >> 3 is the position of a workgroup in ITS XCD's queue and the map decides in which order
// an XCD takes the row blocks of its NH / 8 pairs (one function for the kernels and for the host,
// sea_attention_grid_map):
//   SEA_GRID_ASCENDING    pair after pair, tb ascending -- with causal rows the lightest block of a pair first, the heaviest last;
//   SEA_GRID_HEAVY_FIRST  pair after pair, tb descending (= SEA_GRID_GROUPED with G = 1);
//   SEA_GRID_GROUPED      the XCD's pairs G at a time: the blocks of the G pairs interleaved (pair 0's block TB - 1, pair 1's
//                         block TB - 1, ..., pair 0's block TB - 2, ...), tb descending; the last group holds what is left.
enum { SEA_GRID_ASCENDING = 0, SEA_GRID_HEAVY_FIRST = 1, SEA_GRID_GROUPED = 2 };
__host__ __device__ inline bool map_block(int bid, int NH, int TB, int order, int G, int* pair, int* tb) {
  const int xcd = bid & 7, slot = bid >> 3;
  const int full = NH >> 3;                      // groups of 8 pairs: pair 8 pl + x lives on XCD x (its K / V stay in that L2)
  const bool desc = order != SEA_GRID_ASCENDING;
  if (slot < full * TB) {
    if (order != SEA_GRID_GROUPED || G == 1) {             // pair after pair (one division, as before there were orders)
      const int pl = slot / TB, rb = slot - pl * TB;
      *tb = desc ? TB - 1 - rb : rb;
      *pair = pl * 8 + xcd;
      return true;
    }
    const int grp = slot / (G * TB), w = slot - grp * (G * TB);      // group of G pairs; position inside it
    const int left = full - grp * G, cnt = left < G ? left : G;      // pairs of this group (the last one may hold fewer)
    const int rb = w / cnt;
    *tb = TB - 1 - rb;
    *pair = (grp * G + (w - rb * cnt)) * 8 + xcd;
    return true;
  }
  // the last, partial group (NH % 8 = r pairs; round 5): its r TB row blocks are dealt round-robin to ALL eight XCDs instead
  // of TB blocks to each of r XCDs while 8 - r sit idle -- 12 pairs (OPT-125m, one sequence: the long-context and grid legs)
  // were 2 + 2 + 2 + 2 + 1 + 1 + 1 + 1 pairs per XCD, i.e. the launch lasted as long as 16 pairs
  const int r = NH - full * 8;
  const int item = (slot - full * TB) * 8 + xcd;
  if (item >= r * TB) return false;              // (slot < (full + 1) * TB: the grid ends there)
  const int pr = item / TB, rb = item - pr * TB;
  *tb = desc ? TB - 1 - rb : rb;
  *pair = full * 8 + pr;
  return true;
}
// the ascending order from blockIdx: the decode forms, the key-range pair, the backward passes, the unfused CSR operators
__device__ inline bool map_block(int NH, int TB, int* pair, int* tb) {
  return map_block((int)blockIdx.x, NH, TB, SEA_GRID_ASCENDING, 1, pair, tb);
}

// ---- the gather kernels' score: q . k over a lane group (sea_attn.hip, sea_attn_keyrange.hip) -----------------------------
template <int CTRL> __device__ inline float dpp_f(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}

// sum over the LPR lanes of an aligned group; result in every lane of the group
template <int LPR> __device__ inline float group_sum(float x) {
  if (LPR >= 2) x += dpp_f<0xB1>(x);    // quad_perm [1,0,3,2]
  if (LPR >= 4) x += dpp_f<0x4E>(x);    // quad_perm [2,3,0,1]
  if (LPR >= 8) x += dpp_f<0x141>(x);   // row_half_mirror (values are quad-uniform here)
  if (LPR >= 16) x += dpp_f<0x140>(x);  // row_mirror      (values are 8-uniform here)
  if (LPR >= 32) x += __shfl_xor(x, 16);
  if (LPR >= 64) x += __shfl_xor(x, 32);
  return x;
}

// q . k over one 16-byte lane fragment.  16-bit inputs use the packed dot-product instructions
// (v_dot2c_f32_bf16 / v_dot2_f32_f16: exact products, fp32 accumulation) on the raw registers -- no unpacking.
typedef __attribute__((ext_vector_type(2))) __bf16 sea_bf2;
typedef __attribute__((ext_vector_type(2))) _Float16 sea_h2;
template <typename T> __device__ inline float frag_dot(const uint4& q, const uint4& k);
template <> __device__ inline float frag_dot<float>(const uint4& q, const uint4& k) {
  float d = __uint_as_float(q.x) * __uint_as_float(k.x);
  d = fmaf(__uint_as_float(q.y), __uint_as_float(k.y), d);
  d = fmaf(__uint_as_float(q.z), __uint_as_float(k.z), d);
  return fmaf(__uint_as_float(q.w), __uint_as_float(k.w), d);
}
template <> __device__ inline float frag_dot<__hip_bfloat16>(const uint4& q, const uint4& k) {
  float d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(sea_bf2, q.x), __builtin_bit_cast(sea_bf2, k.x), 0.f, false);
  d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(sea_bf2, q.y), __builtin_bit_cast(sea_bf2, k.y), d, false);
  d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(sea_bf2, q.z), __builtin_bit_cast(sea_bf2, k.z), d, false);
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(sea_bf2, q.w), __builtin_bit_cast(sea_bf2, k.w), d, false);
}
template <> __device__ inline float frag_dot<__half>(const uint4& q, const uint4& k) {
  float d = __builtin_amdgcn_fdot2(__builtin_bit_cast(sea_h2, q.x), __builtin_bit_cast(sea_h2, k.x), 0.f, false);
  d = __builtin_amdgcn_fdot2(__builtin_bit_cast(sea_h2, q.y), __builtin_bit_cast(sea_h2, k.y), d, false);
  d = __builtin_amdgcn_fdot2(__builtin_bit_cast(sea_h2, q.z), __builtin_bit_cast(sea_h2, k.z), d, false);
  return __builtin_amdgcn_fdot2(__builtin_bit_cast(sea_h2, q.w), __builtin_bit_cast(sea_h2, k.w), d, false);
}

// ---- d = 80 (OPT-2.7B heads), 16-bit data: 8 lanes per row, each with 8 + 2 elements -------------------------
// The power-of-two mapping gives a d = 80 row 16 lanes of which 10 carry data (4 rows per wave).  Here a row
// takes 8 lanes: lane j holds elements 8j..8j+7 (one 16-byte load) plus the pair 64+2j, 65+2j (one 4-byte load), so a
// wave advances 8 rows with every lane busy.
template <typename T> __device__ inline float tail_dot(uint32_t q, uint32_t k, float d);
template <> __device__ inline float tail_dot<__hip_bfloat16>(uint32_t q, uint32_t k, float d) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(sea_bf2, q), __builtin_bit_cast(sea_bf2, k), d, false);
}
template <> __device__ inline float tail_dot<__half>(uint32_t q, uint32_t k, float d) {
  return __builtin_amdgcn_fdot2(__builtin_bit_cast(sea_h2, q), __builtin_bit_cast(sea_h2, k), d, false);
}
template <typename T> __device__ inline void unpack2(uint32_t r, float* f);
template <> __device__ inline void unpack2<__hip_bfloat16>(uint32_t r, float* f) {
  f[0] = __uint_as_float(r << 16); f[1] = __uint_as_float(r & 0xffff0000u);
}
template <> __device__ inline void unpack2<__half>(uint32_t r, float* f) {
  const float2 t = __half22float2(__builtin_bit_cast(__half2, r));
  f[0] = t.x; f[1] = t.y;
}
template <typename TO> __device__ inline void store2(TO* dst, float a, float b) { *reinterpret_cast<uint32_t*>(dst) = pack2<TO>(a, b); }
template <> __device__ inline void store2<float>(float* dst, float a, float b) { *reinterpret_cast<float2*>(dst) = make_float2(a, b); }

// ---- what ONE LANE holds of a q / K / V / avg / out row of the gather kernels --------------------------------------------
// Lane `sub` of a row's lane group holds the 16-byte fragment `sub` (VEC elements); X80 (the d = 80 map above): also the pair
// behind the DM = 64 elements of the fragments.  NF = the lane's elements as floats.  The power-of-two form never touches `x`:
// every use of it sits under `if constexpr (X80)`, so it costs no register and no load.  Which lanes are active is the
// kernels' business (dact = sub * VEC < D, lanes beyond D re-read fragment 0; every lane is active for d = 80).
template <typename T, bool X80 = false>
struct RowFrag {
  static constexpr int VEC = Elem<T>::VEC, XT = X80 ? 2 : 0, NF = VEC + XT;
  static constexpr int DM = 8 * VEC;                       // X80: elements in the 16-byte fragments; the pairs sit behind them
  static_assert(!X80 || sizeof(T) == 2, "d = 80: 16-bit data, eight lanes per row");
  uint4 r;
  uint32_t x;

  // byte offsets of lane `sub`'s parts inside a row of T
  struct Lane { uint32_t m, x; };
  __device__ static inline Lane lane(int sub) {
    return {(uint32_t)(sub * VEC) * (uint32_t)sizeof(T), (uint32_t)(DM + sub * XT) * (uint32_t)sizeof(T)};
  }
  // (the loads and clear() fill the fragment in place: a fragment returned by value and copied into an array element cost
  // sparse_attn_decode1_kernel 22 registers)
  __device__ inline void clear() {
    r = make_uint4(0, 0, 0, 0);
    if constexpr (X80) x = 0;
  }
  // a gathered row: wave-uniform 64-bit base + 32-bit byte offset of the row + the lane's
  __device__ inline void load(const char* base, uint32_t row_off, Lane ln) {
    r = *reinterpret_cast<const uint4*>(base + (row_off + ln.m));
    if constexpr (X80) x = *reinterpret_cast<const uint32_t*>(base + (row_off + ln.x));
  }
  // a row by its pointer (q, avg; the rows staged in LDS)
  __device__ inline void load(const T* row, int sub) {
    r = *reinterpret_cast<const uint4*>(row + sub * VEC);
    if constexpr (X80) x = *reinterpret_cast<const uint32_t*>(row + DM + sub * XT);
  }
  __device__ inline void put(T* row, int sub) const {     // as loaded (staging in LDS)
    *reinterpret_cast<uint4*>(row + sub * VEC) = r;
    if constexpr (X80) *reinterpret_cast<uint32_t*>(row + DM + sub * XT) = x;
  }
  // this lane's part of q . k (exact products, fp32 accumulation; group_sum adds the lanes)
  __device__ inline float dot(const RowFrag& k) const {
    float d = frag_dot<T>(r, k.r);
    if constexpr (X80) d = tail_dot<T>(x, k.x, d);
    return d;
  }
  __device__ inline void unpack(float* f) const {
    unpack16<T>(r, f);
    if constexpr (X80) unpack2<T>(x, f + VEC);
  }
  template <typename TO> __device__ static inline void store(TO* row, int sub, const float* f) {
    store_frag<TO, VEC>(row + sub * VEC, f);
    if constexpr (X80) store2<TO>(row + DM + sub * XT, f[VEC], f[VEC + 1]);
  }
  template <typename TO> __device__ static inline void store_zero(TO* row, int sub) {
    float o[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) o[j] = 0.f;
    store<TO>(row, sub, o);
  }
};

// ---- one step of the online softmax: U scored entries into a lane group's state (m, l, acc[NF]) -------------------------
// s[u]: the group's score of entry u (group_sum of the lanes' dots), -INFINITY where the entry does not exist; mnew: the
// maximum of m and the s[u], which the caller's scoring loop tracks (found inside this function instead, the key-range
// kernel took one register more and lost a wave of occupancy); v[u]: the entry's V fragment, already loaded (a masked
// entry's is whatever the caller loaded for it: its probability is exp(-inf) = 0).  The gather kernels' walk
// (attn_rows_body) and the key-range walk take this step; sparse_attn_decode1_kernel's phases D + E repeat its operations
// in its order.
template <int U, typename F>
__device__ __forceinline__ void softmax_step(const float* s, float mnew, const F* v, float& m, float& l, float* acc) {
  const float msafe = (mnew == -INFINITY) ? 0.f : mnew;     // rows that have seen nothing yet: exp(-inf - 0) = 0
  const float alpha = __expf(m - msafe);
  l *= alpha;
#pragma unroll
  for (int j = 0; j < F::NF; ++j) acc[j] *= alpha;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float pu = __expf(s[u] - msafe);
    float vf[F::NF];
    v[u].unpack(vf);
    l += pu;
#pragma unroll
    for (int j = 0; j < F::NF; ++j) acc[j] = fmaf(pu, vf[j], acc[j]);
  }
  m = mnew;
}

// ---- the gather kernels' epilogue -------------------------------------------------------------------------------------
// what a row's sum l turns into the factor of its accumulators (and, times exp(s - m), of its per-entry probabilities)
__device__ inline float attn_row_factor(const AttnParams& p, int64_t ridx, float l) {
  float scale = (l > 0.f) ? (1.0f / l) : 0.f;
  if (p.row_scale) scale *= p.row_scale[ridx];
  return scale;
}
template <typename TO> __device__ inline TO* attn_out_row(const AttnParams& p, int n, int h, int t) {
  return reinterpret_cast<TO*>(p.out) + n * p.os[0] + h * p.os[1] + (int64_t)t * p.os[2];
}
// row (n, h, t) = ridx of the (N, H, T_dst) rows, by the lane `sub` that holds (l, acc): acc / l * row_scale, the blend with
// avg, the store in out_dtype.  The caller has picked the lanes (its row exists, the lane is active)
template <typename T, typename TO, bool X80>
__device__ __forceinline__ void attn_epilogue(const AttnParams& p, int64_t ridx, int n, int h, int t, int sub, float l, const float* acc) {
  using F = RowFrag<T, X80>;
  const float scale = attn_row_factor(p, ridx, l);
  float o[F::NF];
#pragma unroll
  for (int j = 0; j < F::NF; ++j) o[j] = (l > 0.f) ? acc[j] * scale : 0.f;   // empty row: 0 even if the clamped key's V is not finite
  if (p.mix) {
    const float a = p.mix[ridx];
    F avg;
    avg.load(reinterpret_cast<const T*>(p.avg) + n * p.as[0] + h * p.as[1] + (int64_t)t * p.as[2], sub);
    float af[F::NF];
    avg.unpack(af);
#pragma unroll
    for (int j = 0; j < F::NF; ++j) o[j] = o[j] * a + (1.0f - a) * af[j];
  }
  F::template store<TO>(attn_out_row<TO>(p, n, h, t), sub, o);
}
// the context row of a sequence that sits out a decode step (DecodeSession.pause / release): zeros
template <typename T, typename TO, bool X80>
__device__ inline void attn_zero_row(const AttnParams& p, int n, int h, int t, int sub) {
  RowFrag<T, X80>::template store_zero<TO>(attn_out_row<TO>(p, n, h, t), sub);
}

// true when the plan hands this launch to the OTHER kernel (uniform over the whole grid: every workgroup returns at once)
__device__ inline bool kernel_is_idle(const AttnParams& p) {
  if (p.sel == nullptr) return false;
  const bool tile_runs = (int64_t)p.sel_count[0] * p.sel_den > (int64_t)p.sel_total * p.sel_num;
  return tile_runs ? (p.sel_want != 1) : (p.sel_want != 0);
}

// ---- rows of a block dealt to the lane groups BY LENGTH ---------------------------------------------------------------
// The grouped top-k pools all heads of a query row, so the entries one head gets vary a lot from row to row (at the
// headline shape: mean 64, standard deviation ~32 -- four pixels of 16 keys each, Poisson-like).  A wave of the gather
// kernels walks its rows in lockstep for as long as its longest row lasts: with the rows taken in natural order only 0.64
// of the issued lane-steps carried an entry (0.73 on softmax(randn), 0.59 on the structured map).  Sorting the block's rows
// by length first (ranks 8w .. 8w+7 to wave w) puts rows of similar length into one wave: 0.83 at 32 rows per block, 0.89
// at 64, 0.93 at 128 (scripts/time_attn_variants.py).  Measured at OPT-1.3B x 8, the layer's own selection:
// 1.15 ms (natural order) -> 0.99 (32 rows) -> 0.96 (64 rows per block) -> 1.00 (128).
// `len` = entries of the row that sits at block slot `gi` in natural order (-1: no row here / not this kernel's); returns
// the slot this lane group walks; *rowok = that slot holds a row.  Two workgroup barriers: EVERY thread of the block calls.
template <int LPR> __device__ inline int lane_group_sum_i(int x) {
  static_assert(LPR == 4 || LPR == 8 || LPR == 16, "lane groups inside one DPP row");
  x += __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);                   // quad_perm [1,0,3,2]
  x += __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true);                   // quad_perm [2,3,0,1]
  if (LPR >= 8) x += __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true);    // row_half_mirror
  if (LPR >= 16) x += __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true);   // row_mirror
  return x;
}

template <int LPR, int RPB>
__device__ inline int rows_by_length(int len, int gi, int sub, bool* rowok) {
  __shared__ int s_len[RPB], s_row[RPB];
  if (sub == 0) s_len[gi] = len;
  __syncthreads();
  {
    // rank by (length descending, slot ascending): lane `sub` compares against slots sub, sub + LPR, ...
    const int mine = s_len[gi];
    int before = 0;
#pragma unroll
    for (int r = sub; r < RPB; r += LPR) {
      const int o = s_len[r];
      before += (o > mine || (o == mine && r < gi)) ? 1 : 0;
    }
    const int rank = lane_group_sum_i<LPR>(before);
    if (sub == 0) s_row[rank] = gi;
  }
  __syncthreads();
  const int slot = s_row[gi];                              // this lane group walks the row of rank gi
  *rowok = s_len[slot] >= 0;
  return slot;
}

// ---- host side, forward and backward ---------------------------------------------------------------------------------
// lanes of a row's group: 16-byte fragments of `vec` elements, a power of two, at least 4
inline int lanes_per_row(int D, int vec) {
  const int need = (D + vec - 1) / vec;
  int l = 1;
  while (l < need) l *= 2;
  return l < 4 ? 4 : l;
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool strides_ok(const int64_t* s, int vec) { return s[0] % vec == 0 && s[1] % vec == 0 && s[2] % vec == 0; }

// the tile-block counter sits behind the plan's bytes, 4-byte aligned
__host__ __device__ inline int64_t plan_count_offset(int64_t N, int64_t H, int64_t TB16) { return (N * H * TB16 + 3) & ~(int64_t)3; }

// launchers of the MFMA tile kernel (sea_attn_tile.hip); `flags`: see SEA_ATTN_* in sea_hip.h
bool attn_tile_supported(int dtype, int D, int T_src, const AttnParams& p);
int launch_attn_tile(const AttnParams& p, int dtype, int out_dtype, int flags, hipStream_t s);
int launch_attn_plan(const uint32_t* bits, int N, int H, int T_dst, int T_src, int T_m, int causal, float entries_per_tile,
                     uint8_t* sel, hipStream_t s);


// ---- key-range form (sea_attn_keyrange.hip; SEA_ATTN_KEYRANGE in sea_hip.h) ----------------------------------------------
// ws: the caller's fp32 workspace, per batch item H * n_ranges * T_dst * (D + 2) floats -- the unnormalised accumulators
// [h][range][t][D], then the pairs (m, l) [h][range][t][2]
struct KeyRangeParams {
  float* ws;
  int64_t ws_stride_n;
  int range_keys, n_ranges;
};
constexpr int SEA_KEYRANGE_LIST = 8192;          // entries of a workgroup's key lists in LDS (32 KB), shared out evenly to its rows
int launch_attn_keyrange(const AttnParams& p, const KeyRangeParams& kr, int dtype, int out_dtype, hipStream_t s);

}  // namespace sea
