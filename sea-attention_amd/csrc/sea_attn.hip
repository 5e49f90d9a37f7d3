// Row-indexed sparse attention on the flat CSR, hand-written for gfx950 (wave64).
//
// Replaces (reference, src/models/perlin_attention/ops/kernels/):
//   flat_csr_masked_bmm.py:39-125   SDDMM  (1-warp programs, scalar entry loop)
//   flat_csr_softmax.py:55-125      per-(row, head) softmax (H masked passes over the whole row)
//   flat_csr_elmul.py:42-108        row-scale multiply through a stride-0 (N,H,T,T) view
//   flat_csr_sdbmm.py:48-127,141-313  head-count pass + SpMM
// and the mix of attention.py:1236-1237.
//
// Mapping: ONE WAVEFRONT PER (n, h, t) QUERY ROW.  The 64 lanes form 64/LPR groups of LPR lanes; a
// group reads one whole K (or V) row per instruction as LPR x 16 B, so every gathered row is a
// run of full, contiguous 16-byte lane loads (a 128 B bf16 d=64 row = 8 lanes).  q stays in
// registers; the dot product is reduced inside the group with DPP; every group keeps its own
// online-softmax state (m, l, acc[VEC]) so the key loop has no cross-group traffic, and the
// groups are merged once at the end (flash-decoding style).  No LDS, no barriers.
//
// HBM / L2: K and V of one (n, h) are T_src*D*2*s bytes (1 MiB at OPT-1.3B T=4096 bf16), so the
// gathers are served by L2 when the workgroups of a head run on one XCD: blockIdx is remapped so
// that the (n, h) pair index is congruent to the XCD label blockIdx % 8 (speed only).
#include "sea_attn.hpp"

namespace sea {

// WP: also write the per-entry values rs * softmax to p.probs (`partial_attention_probs`, attention.py:1162-1171).  Pass 1
// leaves the raw score at the entry's slot, a second walk turns it into the probability once (m, l) are final; every slot
// is re-read by the lane that wrote it (a thread sees its own stores), so no fence is needed.
template <typename T, typename TO, int LPR, int U, bool WP>
__global__ __launch_bounds__(256) void sparse_attn_kernel(AttnParams p) {
  constexpr int VEC = Elem<T>::VEC;
  constexpr int KPI = 64 / LPR;  // keys per wave-instruction
  int pair, tb;
  if (!map_block((int)blockIdx.x, p.N * p.H, p.TB, p.grid_order, p.grid_group, &pair, &tb)) return;
  const int n = pair / p.H, h = pair - n * p.H;
  const int t = tb * 4 + (threadIdx.x >> 6);
  if (t >= p.T_dst) return;
  if (kernel_is_idle(p)) return;
  const int lane = threadIdx.x & 63;
  const int grp = lane / LPR, sub = lane - grp * LPR;
  const bool dact = sub * VEC < p.D;

  const T* qp = reinterpret_cast<const T*>(p.q) + n * p.qs[0] + h * p.qs[1] + t * p.qs[2] + sub * VEC;
  const T* kb = reinterpret_cast<const T*>(p.k) + n * p.ks[0] + h * p.ks[1] + sub * VEC;
  const T* vb = reinterpret_cast<const T*>(p.v) + n * p.vs[0] + h * p.vs[1] + sub * VEC;

  uint4 qraw = make_uint4(0, 0, 0, 0);
  if (dact) qraw = *reinterpret_cast<const uint4*>(qp);
  const int row_beg = p.crow[(int64_t)n * (p.T_dst + 1) + t];
  const int32_t* ho = p.head_off + ((int64_t)n * p.T_dst + t) * (p.H + 1);
  const int beg = row_beg + ho[h], end = row_beg + ho[h + 1];
  const int32_t* col = p.col + n * p.col_stride_n;
  const int hcol = h * p.T_src;

  float m = -INFINITY, l = 0.f;
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;

  for (int e0 = beg; e0 < end; e0 += KPI * U) {
    bool ok[U];
    uint4 kr[U], vr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + u * KPI + grp;
      ok[u] = e < end;
      const int key = col[ok[u] ? e : end - 1] - hcol;      // masked groups re-read the row's last entry (a finite V row)
      kr[u] = make_uint4(0, 0, 0, 0);
      vr[u] = make_uint4(0, 0, 0, 0);
      if (dact) {
        kr[u] = *reinterpret_cast<const uint4*>(kb + (int64_t)key * p.ks[2]);
        vr[u] = *reinterpret_cast<const uint4*>(vb + (int64_t)key * p.vs[2]);
      }
    }
    float s[U];
    float mnew = m;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float d = frag_dot<T>(qraw, kr[u]);
      d = group_sum<LPR>(d);
      s[u] = ok[u] ? d : -INFINITY;
      mnew = fmaxf(mnew, s[u]);
      if (WP && ok[u] && sub == 0) p.probs[n * p.probs_stride_n + e0 + u * KPI + grp] = d;
    }
    if (mnew == -INFINITY) continue;  // this group has seen no entry yet
    const float alpha = __expf(m - mnew);
    l *= alpha;
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] *= alpha;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float pu = __expf(s[u] - mnew);
      float vf[VEC];
      unpack16<T>(vr[u], vf);
      l += pu;
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[j] = fmaf(pu, vf[j], acc[j]);
    }
    m = mnew;
  }

  // merge the KPI groups (lanes with equal `sub` hold the same feature slice)
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1) {
    const float mo = __shfl_xor(m, o);
    const float lo = __shfl_xor(l, o);
    const float M = fmaxf(m, mo);
    const float a = (m == -INFINITY) ? 0.f : __expf(m - M);
    const float b = (mo == -INFINITY) ? 0.f : __expf(mo - M);
    l = l * a + lo * b;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float ao = __shfl_xor(acc[j], o);
      acc[j] = acc[j] * a + ao * b;
    }
    m = M;
  }

  const int64_t ridx = ((int64_t)n * p.H + h) * p.T_dst + t;
  if (WP && sub == 0) {                                    // every group: the entries it scored in pass 1
    const float c = attn_row_factor(p, ridx, l);
    float* pr = p.probs + n * p.probs_stride_n;
    for (int e = beg + grp; e < end; e += KPI) pr[e] = __expf(pr[e] - m) * c;
  }
  if (grp == 0 && dact) attn_epilogue<T, TO, false>(p, ridx, n, h, t, sub, l, acc);
}

// natural-order length of slot gi's row for rows_by_length (sea_attn.hpp): -1 for slots past T_dst
__device__ inline int slot_length(const AttnParams& p, int n, int h, int tn) {
  if (tn >= p.T_dst) return -1;
  const int32_t* hon = p.head_off + ((int64_t)n * p.T_dst + tn) * (p.H + 1);
  return hon[h + 1] - hon[h];
}

// ---- rows dealt by length over POOLS of rows wider than a workgroup (SEA_ATTN_ROW_POOL) ---------------------------------
// rows_by_length ranks the rows a workgroup owns, so the pool the sort draws from is tied to the workgroup size (0.89 of the
// lane-steps carry an entry at 64 rows; 128 rows gave 0.93 but a 1024-thread workgroup lost more than that won).  Here the
// ranking is a launch of its own in front of the attention launch: one workgroup counting-sorts the lengths of a pool of
// `pool` consecutive rows of one (n, h), longest first -- an LDS histogram over min(len + 1, BINS - 1), a scan of it from the
// top bin down, one LDS atomic per row for its slot; the rows of the top bin (BINS - 2 entries or more: a head that took
// most of a row's budget) are ranked among themselves by comparison, so the order is non-increasing in the true length.
// The order of rows of equal length is whatever the atomics give: one workgroup writes a pool's order and every reader reads
// that.  order[(n, h, pool), slot] = the row's offset in its pool; the slots past T_dst (length -1) come last.
constexpr int SEA_ATTN_ORDER_BINS = 512;
__global__ __launch_bounds__(1024) void attn_row_order_kernel(AttnParams p) {
  constexpr int BINS = SEA_ATTN_ORDER_BINS;
  __shared__ int s_bin[BINS];                              // the histogram, then every bin's next slot
  __shared__ int s_top[1024];                              // lengths of the rows in the top bin (by row), -1 elsewhere
  const int tid = threadIdx.x, pool = p.pool_rows;
  const int pl = (int)blockIdx.x % p.pools, pair = (int)blockIdx.x / p.pools;
  const int n = pair / p.H, h = pair - n * p.H;
  for (int b = tid; b < BINS; b += blockDim.x) s_bin[b] = 0;
  const bool mine = tid < pool;                            // (a pool of 32 rows still runs one whole wave)
  const int len = mine ? slot_length(p, n, h, pl * pool + tid) : -1;
  const int bin = len + 1 < BINS - 1 ? len + 1 : BINS - 1;
  if (mine) s_top[tid] = bin == BINS - 1 ? len : -1;
  __syncthreads();
  if (mine) atomicAdd(&s_bin[bin], 1);
  __syncthreads();
  if (tid < 64) {                                          // first slot of every bin, bins descending: lane L owns bins
    constexpr int PER = BINS / 64;                         // BINS - 1 - PER * L down to BINS - PER * (L + 1)
    int c[PER], sum = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) { c[i] = s_bin[BINS - 1 - (tid * PER + i)]; sum += c[i]; }
    int start = wave_incl_scan(sum) - sum;
#pragma unroll
    for (int i = 0; i < PER; ++i) { s_bin[BINS - 1 - (tid * PER + i)] = start; start += c[i]; }
  }
  __syncthreads();
  if (!mine) return;
  int slot;
  if (bin == BINS - 1) {                                   // the top bin starts at slot 0: rank by (length descending, row ascending)
    slot = 0;
    for (int r = 0; r < pool; ++r) {
      const int o = s_top[r];
      slot += (o > len || (o == len && r < tid)) ? 1 : 0;
    }
  } else {
    slot = atomicAdd(&s_bin[bin], 1);
  }
  uint16_t* ord = const_cast<uint16_t*>(p.order) + n * p.order_stride_n + ((int64_t)h * p.pools + pl) * pool;
  ord[slot] = (uint16_t)tid;
}

// the row this lane group walks when the rows are dealt from the pool's order: lane group (wave w, j) of the pool's block b
// (of nb = pool_rows / RPB) takes slot (w * nb + b) * RPW + j -- every wave holds RPW neighbours of the sorted order, every
// block octets spread over the whole length range (its longest rows in wave 0, its total near the mean).  Returns false for
// a block all of whose slots lie past T_dst (block-uniform; the caller returns before any barrier).
template <int LPR, int RPB>
__device__ inline bool pooled_row(const AttnParams& p, int n, int h, int tb, int grp, int* t, bool* rowok) {
  constexpr int RPW = 64 / LPR;
  const int nb = p.pool_rows / RPB;
  const int pl = tb / nb, b = tb - pl * nb;
  const int rows = min(p.pool_rows, p.T_dst - pl * p.pool_rows);   // rows of this pool: they hold the first `rows` slots
  if (b * RPW >= rows) return false;
  const int slot = (((int)threadIdx.x >> 6) * nb + b) * RPW + grp;
  const uint16_t* ord = p.order + n * p.order_stride_n + ((int64_t)h * p.pools + pl) * p.pool_rows;
  *t = pl * p.pool_rows + (int)ord[slot];
  *rowok = *t < p.T_dst;
  return true;
}

// ---- steps I + J in one launch: the interpolation of ONE (row, head) by the lane group that walks it -----------------------
// The lane group expands its row's kept pixels of head h to key columns -- the emit kernel's arithmetic, bit for bit
// (interp_scale / interp_bound, keys descending inside a pixel, the reference's fp32 stepping for a thinned pixel) -- into
// a group-private list in LDS, copies the list to `col` (the CSR's column array is an output of the layer) and then walks
// it from LDS: no separate emit launch, no column re-read from memory, and the expansion's scalar-heavy loops run in the
// shadow of a kernel that is bound by its gathers.  Lane `sub` owns mask word `sub` of the head (T_m / 32 words; more:
// rounds of LPR); a group scan orders the runs.  The list is written and read by the same wave, whose LDS operations
// execute in order: no workgroup barrier after the one that sizes the lists.  Blocks whose lists would not fit the LDS
// budget expand straight into `col` and read it back past the L1 (rare: a head that takes most of a row).
// Every thread of the block calls (one workgroup barrier inside).
template <int LPR, int RPB, bool DEC = false>
__device__ inline void fused_expand(const AttnParams& p, int n, int h, int tt, bool rowok, int gi, int sub, int beg, int end,
                                    int hcol, int t_src, int* s_keys, int* lbase_out, bool* fits_out, int* total_out) {
  __shared__ int s_glen[RPB];
  const int mylen = end - beg;
  if (sub == 0) s_glen[gi] = mylen;
  __syncthreads();
  int bef = 0, tot = 0;
#pragma unroll
  for (int r = sub; r < RPB; r += LPR) {
    const int v_ = s_glen[r];
    tot += v_;
    bef += r < gi ? v_ : 0;
  }
  const int lbase = lane_group_sum_i<LPR>(bef);
  const int total = lane_group_sum_i<LPR>(tot);
  const bool fits = total <= p.fuse_cap;                           // block-uniform
  int32_t* gcol = p.col_w + n * p.col_stride_n;
  const int WPH = p.T_m >> 5;                              // mask words per head (launcher: T_m % 32 == 0)
  const int w_t = row_width(tt, p.T_dst, t_src, p.is_causal);      // (t_src: p.T_src, or the decode form's device counter)
  const float scale = interp_scale(w_t, p.T_m);
  const uint32_t* brow = p.bits + ((int64_t)n * p.T_dst + tt) * p.W + h * WPH;
  int carry = 0;
  for (int w0 = 0; w0 < WPH; w0 += LPR) {                  // uniform
    const int wi = w0 + sub;
    const uint32_t word = (rowok && wi < WPH) ? brow[wi] : 0u;
    int nent = 0;
    for (uint32_t mm = word; mm;) {
      const int b = wi * 32 + __ffs(mm) - 1;
      mm &= mm - 1;
      const int wd = (int)interp_bound(b + 1, scale) - (int)interp_bound(b, scale);
      nent += wd < p.max_k ? wd : p.max_k;
    }
    int incl = nent;                                       // inclusive scan over the group's LPR lanes (word order)
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) {
      const int up = __shfl_up(incl, o, LPR);
      if (sub >= o) incl += up;
    }
    int off = carry + incl - nent;
    carry += __shfl(incl, LPR - 1, LPR);
    for (uint32_t mm = word; mm;) {
      const int b = wi * 32 + __ffs(mm) - 1;
      mm &= mm - 1;
      const int lo = (int)interp_bound(b, scale), hi = (int)interp_bound(b + 1, scale);
      const int wd = hi - lo;
      if (wd <= p.max_k) {
        const int c0 = hcol + hi - 1;
        if (fits) { for (int j = 0; j < wd; ++j) s_keys[lbase + off + j] = c0 - j; }
        else { for (int j = 0; j < wd; ++j) gcol[beg + off + j] = c0 - j; }
        off += wd;
      } else {                                             // thinned pixel: the reference's fp32 stepping (csr_emit_kernel)
        // DEC: hcol = h * T_cap (the cache capacity) -- stepped on the key alone, the head offset added as an integer, so that
        // the capacity cannot round a key; where h * T_cap + hi < 2^24 both forms are exact integers: the same bits
        const float fb = DEC ? 0.0f : (float)hcol;
        const int ib = DEC ? hcol : 0;
        const float rs = (float)lo + fb, re = (float)hi + fb;
        const float step = __fdiv_rn(re - rs, (float)p.max_k);
        for (int j = 0; j < p.max_k; ++j) {
          const int c = (int)((re - (float)(int)__fmul_rn((float)j, step)) - 1.0f) + ib;
          if (fits) s_keys[lbase + off + j] = c; else gcol[beg + off + j] = c;
        }
        off += p.max_k;
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  if (fits) {                                              // the CSR's columns: the list, copied out by its own lane group
    if (p.write_cols)                                      // (grid-uniform; 0: nobody reads them, the handle stays pending)
      for (int i = sub; i < mylen; i += LPR) gcol[beg + i] = s_keys[lbase + i];
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);                         // this wave's column stores have left before it reads them back
  }
  *lbase_out = lbase;
  *fits_out = fits;
  *total_out = total;
}

// Decode form (DEC kernels, T_dst of a few rows): the block's key lists are complete in LDS (or, not fitting, in `col`); before
// the one lane group per row starts its dependent walk, EVERY lane group of the block touches the K / V rows of the lists --
// what the unfused kernel's warming pass does from `col` (see there).  Every thread of the block calls (two barriers).
// one warming touch: the lane's 16-byte fragments of key_c's K and V rows; the caller sinks the returned word
__device__ inline uint32_t touch_kv(const char* kbase, const char* vbase, uint32_t key_c, uint32_t kst, uint32_t vst, uint32_t lane_off) {
  const uint4 a = *reinterpret_cast<const uint4*>(kbase + (__umul24(key_c, kst) + lane_off));
  const uint4 b = *reinterpret_cast<const uint4*>(vbase + (__umul24(key_c, vst) + lane_off));
  return a.x ^ b.x;
}

template <int LPR, int NG>
__device__ inline void fused_warm(const int* s_keys, int total, bool fits, int hcol, const char* kbase, const char* vbase,
                                  uint32_t kst, uint32_t vst, uint32_t lane_off) {
  __syncthreads();                                         // the lists of the other waves
  if (fits) {                                              // (block-uniform)
    const int g = (int)threadIdx.x / LPR;
    uint32_t sink = 0;
    for (int e = g; e < total; e += NG) sink ^= touch_kv(kbase, vbase, (uint32_t)(s_keys[e] - hcol), kst, vst, lane_off);
    asm volatile("" ::"v"(sink));                          // the loads must complete; their values are not used
  }
  __syncthreads();
}

// lane `sub`'s column of entry `ec` of its row: from the group's own list (fused, fits), from `col` past the L1 (fused, the
// block's lists did not fit: written just above by this wave), or from `col` as the emit launch left it
template <bool FUSE>
__device__ inline int entry_column(const AttnParams& p, const int32_t* col, int n, int ec, int beg, const int* s_keys, int lbase, bool fits) {
  if (FUSE && fits) return s_keys[lbase + ec - beg];
  if (FUSE) return __hip_atomic_load(p.col_w + n * p.col_stride_n + ec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return col[ec];
}

constexpr int SEA_ATTN_WARM_ROWS = 8;            // T_dst up to which the idle lane groups pre-touch the rows' K / V lines

// ---- variant B: one LPR-lane GROUP per query row (64/LPR rows per wave) -----------------------------------
// Each group walks its own row's entries, one key per instruction step, U keys in flight, with its own online
// softmax; nothing is merged across groups.  A wave therefore has 64/LPR independent
// (offsets -> col -> K/V) load chains in flight instead of one, which is what the wave-per-row mapping lacks.
// Workgroup = 4 waves = 256/LPR consecutive query rows of one (n, h).
// DEC (with FUSE): the decode form -- row widths from *p.t_src_dev, the key lists warmed by the whole block (fused_warm).
// ORD (with FUSE, without DEC / WP): the rows come from the pool's order (pooled_row) instead of rows_by_length.
// X80: the row fragment is RowFrag's d = 80 map (8 lanes of 8 + 2 elements).  ONE body, written on the fragment type, under
// two entry points: sparse_attn_rows_kernel (rows of 4 / 8 / 16 lanes) and sparse_attn_rows80_kernel, which differ in their
// launch bounds only (see there).
template <typename T, typename TO, int LPR, int U, bool WP, int NWB, bool FUSE, bool DEC, bool ORD, bool X80>
__device__ __forceinline__ void attn_rows_body(const AttnParams& p) {
  static_assert(!DEC || FUSE, "the decode form is a fused form");
  static_assert(!ORD || (FUSE && !DEC && !WP), "rows are dealt from pools in the fused inference form only");
  static_assert(!X80 || LPR == 8, "d = 80: eight lanes per row");
  using F = RowFrag<T, X80>;
  constexpr int VEC = F::VEC, NF = F::NF;
  constexpr int RPW = 64 / LPR;       // rows per wave
  constexpr int RPB = NWB * RPW;      // rows per workgroup
  int pair, tb;
  // (grid / workgroup uniform: before any barrier.)  The fused prefill forms take the launch's grid order.  The decode forms
  // keep the ascending one (their rows are one position's), and so does the unfused form -- decode steps of few rows and
  // handles whose columns are written, no prefill hot path: with the orders' code in it the compiler gave it 93 registers for
  // 78 (d = 80: 85 for 72) and a wave less per SIMD
  constexpr bool ORDERED = FUSE && !DEC;
  if (kernel_is_idle(p) ||
      !map_block((int)blockIdx.x, p.N * p.H, p.TB, ORDERED ? p.grid_order : (int)SEA_GRID_ASCENDING, ORDERED ? p.grid_group : 1, &pair, &tb))
    return;
  const int n = pair / p.H;
  // heads rotated over the XCDs per batch item: the pair index is congruent to the XCD label (map_block), so without the
  // rotation an XCD would serve the same residue class of heads for every item and a heavy head would load one XCD only
  const int h = (pair - n * p.H + n) % p.H;
  const int lane = threadIdx.x & 63;
  const int grp = lane / LPR, sub = lane - grp * LPR;
  const int gi = (int)(threadIdx.x >> 6) * RPW + grp;      // lane group index inside the block
  bool rowok;
  int t;
  if constexpr (ORD) {
    if (!pooled_row<LPR, RPB>(p, n, h, tb, grp, &t, &rowok)) return;
  } else {
    t = tb * RPB + rows_by_length<LPR, RPB>(slot_length(p, n, h, tb * RPB + gi), gi, sub, &rowok);
  }
  const bool dact = X80 || sub * VEC < p.D;
  const int tt = t < p.T_dst ? t : p.T_dst - 1;
  const int sube = dact ? sub : 0;    // lanes beyond D re-read fragment 0 (their q fragment is zero)

  // wave-uniform 64-bit bases + per-lane 32-bit byte offsets (launcher guarantees T_src*stride*sizeof(T) < 2^31)
  const char* kbase = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.k) + n * p.ks[0] + h * p.ks[1]);
  const char* vbase = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.v) + n * p.vs[0] + h * p.vs[1]);
  const uint32_t kst = (uint32_t)p.ks[2] * (uint32_t)sizeof(T), vst = (uint32_t)p.vs[2] * (uint32_t)sizeof(T);
  const typename F::Lane ln = F::lane(sube);

  F qf;
  qf.clear();
  if (dact) qf.load(reinterpret_cast<const T*>(p.q) + n * p.qs[0] + h * p.qs[1] + (int64_t)tt * p.qs[2], sub);
  const int row_beg = p.crow[(int64_t)n * (p.T_dst + 1) + tt];
  const int32_t* ho = p.head_off + ((int64_t)n * p.T_dst + tt) * (p.H + 1);
  const int beg = row_beg + ho[h];
  const int end = rowok ? row_beg + ho[h + 1] : beg;
  const int32_t* col = p.col + n * p.col_stride_n;
  const int hcol = h * p.T_src;

  // ---- FUSE: the interpolation of THIS (row, head) inside the attention launch (fused_expand below the helpers) ----------
  extern __shared__ int s_keys[];
  int lbase = 0;
  bool fits = false;
  int ltotal = 0;
  int t_src = p.T_src;
  if constexpr (DEC) {
    t_src = p.t_src_dev[n * p.t_src_stride];               // the sequence's length (block-uniform; the one load of it)
    if (t_src < 0) {                                       // the sequence sits out this step (DecodeSession.pause / release): no
      const int t0 = tb * RPB + gi;                        // K or V access (its CSR rows are empty), its context rows are zeros
      if (t0 < p.T_dst && dact) attn_zero_row<T, TO, X80>(p, n, h, t0, sub);
      return;
    }
  }
  if constexpr (FUSE) fused_expand<LPR, RPB, DEC>(p, n, h, tt, rowok, gi, sub, beg, end, hcol, t_src, s_keys, &lbase, &fits, &ltotal);
  // (d = 80: the 16-byte fragments of the lists' K / V rows: 128 of a row's 160 bytes, i.e. both of its cache lines)
  if constexpr (DEC) fused_warm<LPR, NWB * RPW>(s_keys, ltotal, fits, hcol, kbase, vbase, kst, vst, ln.m);

  // ---- a decoding step: T_dst of one or a few rows, so all but a few of the block's lane groups have no row -- and the one
  // that has walks its ~k entries down ONE dependent chain (column indices -> four K / V rows -> the next four ...: three
  // memory round trips per 8 entries, 40 us for an OPT-1.3B x 8 step whose K / V lines come cold from HBM).  The idle groups
  // first touch every K / V row the block's rows will gather, all at once: the walk below then finds them in this CU's L1 /
  // the L2.  Arithmetic untouched: the step stays bitwise the stateless forward.
  // (not for d = 80: the pass was written into the power-of-two kernel only -- DESIGN.md section 8)
  if constexpr (!FUSE && !X80) {
    if (p.T_dst <= SEA_ATTN_WARM_ROWS) {                   // (grid-uniform)
      constexpr int NG = NWB * RPW;
      const int g = (int)threadIdx.x / LPR;
      uint32_t sink = 0;
      for (int r = 0; r < p.T_dst; ++r) {
        const int rb2 = p.crow[(int64_t)n * (p.T_dst + 1) + r];
        const int32_t* ho2 = p.head_off + ((int64_t)n * p.T_dst + r) * (p.H + 1);
        const int b2 = rb2 + ho2[h], e2 = rb2 + ho2[h + 1];
        for (int e = b2 + g; e < e2; e += NG) sink ^= touch_kv(kbase, vbase, (uint32_t)(col[e] - hcol), kst, vst, ln.m);
      }
      asm volatile("" ::"v"(sink));                        // the loads must complete; their values are not used
      __syncthreads();
    }
  }

  float m = -INFINITY, l = 0.f;
  float acc[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) acc[j] = 0.f;

  // longest row of the wave bounds the loop (rows of a wave are neighbours: similar lengths)
  int zmax = end - beg;
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1) zmax = max(zmax, __shfl_xor(zmax, o));
  const int last = end - 1;

  // Column indices: lane `sub` of a group fetches entry (i0 + sub) -- one coalesced load per LPR entries -- and the
  // group reads them back one by one through the LDS crossbar (ds_bpermute), which this kernel otherwise leaves idle.
  const int grp_lane0 = (lane - sub) << 2;                 // byte address of the group's first lane for bpermute
  for (int i0 = 0; i0 < zmax; i0 += LPR) {
    int cidx;
    {
      const int e = beg + i0 + sub;
      const int ec = e < end ? e : (last >= beg ? last : 0);
      cidx = (end > beg) ? (entry_column<FUSE>(p, col, n, ec, beg, s_keys, lbase, fits) - hcol) : 0;   // rows without entries read key 0 (masked below)
    }
#pragma unroll
    for (int u0 = 0; u0 < LPR; u0 += U) {
      if (i0 + u0 < zmax) {                                // wave-uniform
        bool ok[U];
        F kr[U], vr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          ok[u] = beg + i0 + u0 + u < end;
          const uint32_t key_c = (uint32_t)__builtin_amdgcn_ds_bpermute(grp_lane0 + ((u0 + u) << 2), cidx);
          kr[u].load(kbase, __umul24(key_c, kst), ln);
          vr[u].load(vbase, __umul24(key_c, vst), ln);
        }
        float s[U];
        float mnew = m;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float d = group_sum<LPR>(qf.dot(kr[u]));
          s[u] = ok[u] ? d : -INFINITY;
          mnew = fmaxf(mnew, s[u]);
          if (WP && ok[u] && sub == u0 + u) p.probs[n * p.probs_stride_n + beg + i0 + u0 + u] = d;   // entry j by lane j % LPR
        }
        softmax_step<U>(s, mnew, vr, m, l, acc);
      }
    }
  }

  const int64_t ridx = ((int64_t)n * p.H + h) * p.T_dst + t;
  if (WP && rowok) {
    const float c = attn_row_factor(p, ridx, l);
    float* pr = p.probs + n * p.probs_stride_n;
    for (int e = beg + sub; e < end; e += LPR) pr[e] = __expf(pr[e] - m) * c;
  }
  if (rowok && dact) attn_epilogue<T, TO, X80>(p, ridx, n, h, t, sub, l, acc);
}

// -DSEA_STAMP (a diagnostic build, never the shipped library; scripts/stamp_attn_grid.py): lane 0 of wave 0 of every workgroup
// of the lane-group kernels leaves the 100 MHz clock at its entry and at its exit, and the XCC it ran on, in a buffer of its
// own -- when the workgroups of a launch are resident, per XCD.  No output depends on the stamps.
#ifdef SEA_STAMP
constexpr int SEA_ATTN_STAMP_BLOCKS = 1 << 16;             // workgroups of a launch that have a slot (the headline: 16 384)
__device__ unsigned long long sea_attn_grid_stamps[3 * SEA_ATTN_STAMP_BLOCKS];
#define ATTN_GRID_STAMP(i)                                                                                     \
  do {                                                                                                         \
    if (threadIdx.x == 0 && blockIdx.x < (unsigned)SEA_ATTN_STAMP_BLOCKS)                                      \
      sea_attn_grid_stamps[3 * blockIdx.x + (i)] = __builtin_amdgcn_s_memrealtime();                           \
  } while (0)
#define ATTN_GRID_STAMP_XCC()                                                                                  \
  do {                                                                                                         \
    if (threadIdx.x == 0 && blockIdx.x < (unsigned)SEA_ATTN_STAMP_BLOCKS)                                      \
      sea_attn_grid_stamps[3 * blockIdx.x + 2] = __builtin_amdgcn_s_getreg(20 | (3 << 11)) & 0xf; /* XCC_ID[3:0] */ \
  } while (0)
#else
#define ATTN_GRID_STAMP(i) do {} while (0)
#define ATTN_GRID_STAMP_XCC() do {} while (0)
#endif

template <typename T, typename TO, int LPR, int U, bool WP, int NWB = 4, bool FUSE = false, bool DEC = false, bool ORD = false>
// the fused 16-bit inference forms are held to 64 registers (8 waves per SIMD; 4 - 8 spilled registers): measured 0.307 ms
// against 0.328 ms at 88 registers for the 16-lane form (LLaMA-13B d = 128), and the same direction for the 8-lane form
__global__ __launch_bounds__(NWB * 64, (FUSE && !DEC && sizeof(T) == 2 && !WP) ? 8 : 1) void sparse_attn_rows_kernel(AttnParams p) {
  ATTN_GRID_STAMP(0);
  ATTN_GRID_STAMP_XCC();
  attn_rows_body<T, TO, LPR, U, WP, NWB, FUSE, DEC, ORD, false>(p);
  ATTN_GRID_STAMP(1);
}

template <typename T, typename TO, int U, bool WP, int NWB = 4, bool FUSE = false, bool DEC = false, bool ORD = false>
// (no wave floor here: capping this kernel at 80 / 64 registers for 6 / 8 waves per SIMD measured 0.427 / 0.489 ms against
// 0.418 ms as compiled, OPT-2.7B T = 8192 -- DESIGN.md section 9)
__global__ __launch_bounds__(NWB * 64) void sparse_attn_rows80_kernel(AttnParams p) {
  attn_rows_body<T, TO, 8, U, WP, NWB, FUSE, DEC, ORD, true>(p);
}

// ---- a decoding step of ONE new row per sequence (T_dst = 1): the whole workgroup serves the row (round 5) ----------------
// The lane-group kernels above give the row one lane group: its ~k entries go down one dependent chain -- column -> K, V ->
// score -> online softmax -> accumulate, four entries per memory round trip, 8 - 10 us -- while 63 of the block's 64 lane
// groups watch.  Here one 4-wave workgroup per (sequence, head):
//   B  expands the head's kept pixels with one THREAD per pixel (block scan of the widths; fused_expand's arithmetic: scale,
//      bounds, keys descending inside a pixel, the reference's fp32 stepping for a thinned pixel),
//   C  gathers K and V of all entries at once, one lane group per entry: the score q . k (the same frag_dot + group_sum, so the
//      same bits whoever computes it) goes to LDS, the V row too,
//   D  one wave turns the scores into the online softmax's per-step quantities -- the running maximum is a prefix MAX (exact in
//      any order), alpha = exp(m_before - m_after) and p = exp(s - m_after) follow per step of four entries,
//   E  one lane group runs the accumulation chain l = l * alpha + p0 + p1 + p2 + p3, acc = acc * alpha (+)= p_u * v_u from LDS in
//      the walk's order: the SAME floating-point operations in the SAME order as sparse_attn_rows_kernel (U = 4), entries past
//      the row's end included (probability exp(-inf) = 0 times the last entry's V row) -- the step stays bitwise the stateless
//      forward (tests/test_decode_session.py, test_kv_cache.py).
// Rows longer than CH entries pass through in chunks (state carried).  16-bit data, rows of 8 or 16 lanes, T_m <= 256.
// X80: d = 80 on 8 lanes per row -- lane j holds elements 8j .. 8j+7 plus the pair 64+2j, 65+2j (RowFrag's d = 80 map)
// PAGED: K / V in a page pool (AttnParams::table).  The sequence's block-table row is staged in LDS behind the V rows at kernel
// start (its first ceil(T_src / page_rows) entries; dynamic LDS sized for the capacity's), and phase C translates each key to
// (page, row) from there: the page term is a 64-bit product (page x page bytes overflows 32 bits), the row term stays 32-bit
// WP: also write the per-entry values rs * softmax to p.probs, at the slots `col` has (or would have: write_cols = 0).  Phase C's
// sub == 0 lane leaves the raw score at the slot of every real entry -- the padded slots total .. padded-1 belong to the next head
// -- and, once (m, l) are final, the same thread turns it into the probability with the expression of sparse_attn_rows_kernel's
// WP pass (a thread sees its own stores: no fence).  An empty head and a sequence that sits out write nothing.
// the kernel's chunk and its dynamic LDS (16-bit rows; PAGED: the table row comes behind these bytes)
template <int LPR, bool X80>
struct Decode1Lds {
  static constexpr int CH = LPR == 8 ? 256 : 128;          // entries per chunk: CH / 4 steps fit one wave, CH / NG = 8 per lane group
  static constexpr int DL = LPR * (8 + (X80 ? 2 : 0));     // elements of a staged V row
  static constexpr int bytes = CH * 8 + CH + CH * DL * 2;  // s_keys and s_sc [CH], s_al [CH / 4], s_v [CH][DL]
};

template <typename T, typename TO, int LPR, bool X80 = false, bool PAGED = false, bool WP = false>
__global__ __launch_bounds__(256) void sparse_attn_decode1_kernel(AttnParams p) {
  using F = RowFrag<T, X80>;
  constexpr int VEC = F::VEC, NF = F::NF, NT = 256, NG = NT / LPR;
  static_assert(!X80 || LPR == 8, "d = 80: eight lanes per row");
  constexpr int CH = Decode1Lds<LPR, X80>::CH, DL = Decode1Lds<LPR, X80>::DL;
  constexpr int EPG = CH / NG;
  static_assert(VEC == 8 && CH / 4 <= 64 && CH % NG == 0, "16-bit rows; one lane per step in phase D");
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  int* s_keys = reinterpret_cast<int*>(dsm);               // [CH]     key index (without the head offset)
  float* s_sc = reinterpret_cast<float*>(s_keys + CH);     // [CH]     scores, then probabilities
  float* s_al = s_sc + CH;                                 // [CH / 4] alpha per step
  T* s_v = reinterpret_cast<T*>(s_al + CH / 4);            // [CH][DL] V rows
  __shared__ int s_wsum[4];
  __shared__ float s_mcarry;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int grp = tid / LPR, sub = tid - grp * LPR;
  const int n = (int)blockIdx.x / p.H, h = (int)blockIdx.x - n * p.H;
  const bool dact = X80 || sub * VEC < p.D;
  const int sube = dact ? sub : 0;
  const int t_src = p.t_src_dev[n * p.t_src_stride];       // the sequence's length (block-uniform; the one load of it)
  const char* kbase = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.k) + (PAGED ? 0 : n * p.ks[0]) + h * p.ks[1]);
  const char* vbase = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.v) + (PAGED ? 0 : n * p.vs[0]) + h * p.vs[1]);
  const uint32_t kst = (uint32_t)p.ks[2] * (uint32_t)sizeof(T), vst = (uint32_t)p.vs[2] * (uint32_t)sizeof(T);
  int* s_tab = reinterpret_cast<int*>(s_v + (size_t)CH * DL);          // PAGED: [ceil(T_src / page_rows)] the table row
  if constexpr (PAGED) {
    const int npg = (t_src + (1 << p.page_shift) - 1) >> p.page_shift;   // pages holding keys
    const int32_t* trow = p.table + (int64_t)n * p.table_stride;
    for (int i = tid; i < npg; i += NT) s_tab[i] = trow[i];            // (read after phase B's barrier; none when t_src < 0)
  }
  const typename F::Lane ln = F::lane(sube);
  F qf;
  qf.clear();
  if (dact) qf.load(reinterpret_cast<const T*>(p.q) + n * p.qs[0] + h * p.qs[1], sub);
  const int beg = p.crow[(int64_t)n * 2] + p.head_off[(int64_t)n * (p.H + 1) + h];
  const int hcol = h * p.T_src;

  // the sequence sits out this step (DecodeSession.pause / release; block-uniform, at the first use of the length so that the
  // loads above do not wait for it): no table, K or V access, its context row is zeros
  if (t_src < 0) {
    if (grp == 0 && dact) attn_zero_row<T, TO, X80>(p, n, h, 0, sub);
    return;
  }

  // ---- B: one thread per pixel of the head --------------------------------------------------------------------------
  const int w_t = row_width(0, 1, t_src, p.is_causal);
  const float scale = interp_scale(w_t, p.T_m);
  const uint32_t* brow = p.bits + (int64_t)n * p.W + h * (p.T_m >> 5);
  const bool kept = tid < p.T_m && ((brow[tid >> 5] >> (tid & 31)) & 1u);
  const int lo = (int)interp_bound(tid, scale), hi = (int)interp_bound(tid + 1, scale);
  const int wd = hi - lo;
  const int cnt = kept ? (wd < p.max_k ? wd : p.max_k) : 0;
  const int incl = wave_incl_scan(cnt);
  if (lane == 63) s_wsum[wv] = incl;
  if (tid == 0) s_mcarry = -INFINITY;
  __syncthreads();
  int off = incl - cnt, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) { off += w < wv ? s_wsum[w] : 0; total += s_wsum[w]; }
  const int padded = (total + 3) & ~3;                     // the walk's steps of four: entries past the end re-read the last one
  const bool owns_last = cnt > 0 && off + cnt == total;
  int32_t* gcol = p.col_w + n * p.col_stride_n;

  float l = 0.f;
  float acc[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) acc[j] = 0.f;

  for (int c0 = 0; c0 < padded; c0 += CH) {                // (block-uniform)
    // this thread's pixel: its entries that fall into the chunk
    if (cnt > 0 && off < c0 + CH && off + cnt > c0) {
      const int j0 = max(0, c0 - off), j1 = min(cnt, c0 + CH - off);
      if (wd <= p.max_k) {
        for (int j = j0; j < j1; ++j) s_keys[off + j - c0] = hi - 1 - j;
      } else {                                             // thinned pixel: the reference's fp32 stepping (csr_emit_kernel) on
        // the key alone (fused_expand's decode form: the capacity's head offset never enters the fp32 values; where
        // h * T_cap + hi < 2^24 this is bit for bit the stepping of h * T_cap + key)
        const float rs = (float)lo, re = (float)hi;
        const float step = __fdiv_rn(re - rs, (float)p.max_k);
        for (int j = j0; j < j1; ++j) s_keys[off + j - c0] = (int)((re - (float)(int)__fmul_rn((float)j, step)) - 1.0f);
      }
      if (owns_last && j1 == cnt) {                        // the last entry's key again in the slots up to the step boundary
        const int lastkey = s_keys[total - 1 - c0];
        for (int e = total; e < padded; ++e) s_keys[e - c0] = lastkey;
      }
    }
    __syncthreads();
    const int nent = min(CH, padded - c0);                 // entries of the chunk, padding included (a multiple of 4)
    if (p.write_cols)
      for (int e = tid; e < min(nent, total - c0); e += NT) gcol[beg + c0 + e] = hcol + s_keys[e];

    // ---- C: one lane group per entry, EPG entries each, every load in flight at once ------------------------------------
    {
      F kr[EPG], vr[EPG];
#pragma unroll
      for (int i = 0; i < EPG; ++i) {
        const int e = grp + i * NG;
        const uint32_t key_c = (uint32_t)s_keys[e < nent ? e : 0];
        const char* kb = kbase;
        const char* vb = vbase;
        uint32_t ko, vo;
        if constexpr (PAGED) {
          const uint32_t pg = (uint32_t)s_tab[key_c >> p.page_shift], row = key_c & ((1u << p.page_shift) - 1u);
          kb += (uint64_t)pg * (uint32_t)p.ks[0] * sizeof(T);
          vb += (uint64_t)pg * (uint32_t)p.vs[0] * sizeof(T);
          ko = __umul24(row, kst); vo = __umul24(row, vst);
        } else {
          ko = __umul24(key_c, kst); vo = __umul24(key_c, vst);
        }
        kr[i].load(kb, ko, ln);
        vr[i].load(vb, vo, ln);
      }
      float dr[WP ? EPG : 1];                              // WP: the raw scores, for the stores below
#pragma unroll
      for (int i = 0; i < EPG; ++i) {
        const int e = grp + i * NG;
        const float d = group_sum<LPR>(qf.dot(kr[i]));
        if (e < nent) {
          if (sub == 0) s_sc[e] = c0 + e < total ? d : -INFINITY;
          if constexpr (WP) dr[i] = d;
          vr[i].put(s_v + (size_t)e * DL, sub);
        }
      }
      if constexpr (WP) {                                  // real entries only: the padded slots are the next head's
        if (sub == 0) {
          float* pr = p.probs + n * p.probs_stride_n + beg + c0;
#pragma unroll
          for (int i = 0; i < EPG; ++i)
            if (c0 + grp + i * NG < total) pr[grp + i * NG] = dr[i];
        }
      }
    }
    __syncthreads();

    // ---- D: per step of four entries (lane = step): running maximum, alpha, probabilities --------------------------------
    if (wv == 0) {
      const int nsteps = nent >> 2;
      const bool on = lane < nsteps;
      float4 sc = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      if (on) sc = *reinterpret_cast<const float4*>(s_sc + 4 * lane);
      float mx = fmaxf(fmaxf(sc.x, sc.y), fmaxf(sc.z, sc.w));
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {                   // inclusive prefix maximum over the steps
        const float t = __shfl_up(mx, o);
        if (lane >= o) mx = fmaxf(mx, t);
      }
      const float m_in = s_mcarry;
      const float m_after = fmaxf(m_in, mx);
      float m_before = __shfl_up(m_after, 1);
      if (lane == 0) m_before = m_in;
      const float msafe = (m_after == -INFINITY) ? 0.f : m_after;     // rows that have seen nothing yet: exp(-inf - 0) = 0
      if (on) {
        s_al[lane] = __expf(m_before - msafe);
        *reinterpret_cast<float4*>(s_sc + 4 * lane) = make_float4(__expf(sc.x - msafe), __expf(sc.y - msafe), __expf(sc.z - msafe), __expf(sc.w - msafe));
      }
      if (lane == nsteps - 1) s_mcarry = m_after;
    }
    __syncthreads();

    // ---- E: the accumulation chain, in the walk's order ------------------------------------------------------------------
    if (grp == 0) {
      const int nsteps = nent >> 2;
      for (int st = 0; st < nsteps; ++st) {
        const float alpha = s_al[st];
        const float4 pu4 = *reinterpret_cast<const float4*>(s_sc + 4 * st);
        const float pu[4] = {pu4.x, pu4.y, pu4.z, pu4.w};
        F vr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vr[u].load(s_v + (size_t)(4 * st + u) * DL, sub);
        l *= alpha;
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[j] *= alpha;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float vf[NF];
          vr[u].unpack(vf);
          l += pu[u];
#pragma unroll
          for (int j = 0; j < NF; ++j) acc[j] = fmaf(pu[u], vf[j], acc[j]);
        }
      }
    }
    __syncthreads();                                       // the chunk's LDS is free again
  }

  if constexpr (WP) {                                      // m: the last chunk's carry; l: group 0's, through LDS (one barrier)
    __shared__ float s_l;
    if (tid == 0) s_l = l;
    __syncthreads();
    const float m = s_mcarry;
    const float c = attn_row_factor(p, (int64_t)n * p.H + h, s_l);
    float* pr = p.probs + n * p.probs_stride_n + beg;
    if (sub == 0) {                                        // the slots this thread stored in phase C
      for (int c0 = 0; c0 < total; c0 += CH) {
#pragma unroll
        for (int i = 0; i < EPG; ++i) {
          const int e = c0 + grp + i * NG;
          if (e < total) pr[e] = __expf(pr[e] - m) * c;
        }
      }
    }
  }
  if (grp == 0 && dact) attn_epilogue<T, TO, X80>(p, (int64_t)n * p.H + h, n, h, 0, sub, l, acc);   // (t = 0, T_dst = 1)
}

// ---- unfused SDDMM: one wave per (n, t) row, all heads -----------------------------------------------
struct SddmmParams {
  const void *q, *k;
  int64_t qs[3], ks[3];
  int N, H, T_dst, T_src, D;
  const void* crow;
  const void* col;
  int64_t col_stride_n;
  float* values;
};

template <typename T, typename I, int LPR>
__global__ __launch_bounds__(256) void csr_sddmm_kernel(SddmmParams p) {
  constexpr int VEC = Elem<T>::VEC;
  constexpr int KPI = 64 / LPR;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)p.N * p.T_dst) return;
  const int n = (int)(row / p.T_dst), t = (int)(row - (int64_t)n * p.T_dst);
  const int lane = threadIdx.x & 63;
  const int grp = lane / LPR, sub = lane - grp * LPR;
  const bool dact = sub * VEC < p.D;
  const I* crow = reinterpret_cast<const I*>(p.crow) + (int64_t)n * (p.T_dst + 1);
  const I* col = reinterpret_cast<const I*>(p.col) + n * p.col_stride_n;
  float* vals = p.values + n * p.col_stride_n;
  const int64_t beg = crow[t], end = crow[t + 1];
  const T* qb = reinterpret_cast<const T*>(p.q) + n * p.qs[0] + t * p.qs[2] + sub * VEC;
  const T* kb = reinterpret_cast<const T*>(p.k) + n * p.ks[0] + sub * VEC;
  for (int64_t e0 = beg; e0 < end; e0 += KPI) {
    const int64_t e = e0 + grp;
    const bool ok = e < end;
    int64_t c = ok ? (int64_t)col[e] : 0;
    const int h = (int)(c / p.T_src);
    const int key = (int)(c - (int64_t)h * p.T_src);
    uint4 qr = make_uint4(0, 0, 0, 0), kr = make_uint4(0, 0, 0, 0);
    if (dact) {
      qr = *reinterpret_cast<const uint4*>(qb + h * p.qs[1]);
      kr = *reinterpret_cast<const uint4*>(kb + h * p.ks[1] + (int64_t)key * p.ks[2]);
    }
    float qf[VEC], kf[VEC];
    unpack16<T>(qr, qf);
    unpack16<T>(kr, kf);
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) d = fmaf(qf[j], kf[j], d);
    d = group_sum<LPR>(d);
    if (ok && sub == 0) vals[e] = d;
  }
}

// ---- unfused SpMM: one wave per (n, h, t), needs head_off --------------------------------------------
struct SpmmParams {
  const float* values;
  const void* v;
  int64_t vs[3];
  int N, H, T_dst, T_src, D;
  const void* crow;
  const void* col;
  int64_t col_stride_n;
  const int32_t* head_off;
  float* out;
  int TB;
};

template <typename T, typename I, int LPR>
__global__ __launch_bounds__(256) void csr_spmm_kernel(SpmmParams p) {
  constexpr int VEC = Elem<T>::VEC;
  constexpr int KPI = 64 / LPR;
  int pair, tb;
  if (!map_block(p.N * p.H, p.TB, &pair, &tb)) return;
  const int n = pair / p.H, h = pair - n * p.H;
  const int t = tb * 4 + (threadIdx.x >> 6);
  if (t >= p.T_dst) return;
  const int lane = threadIdx.x & 63;
  const int grp = lane / LPR, sub = lane - grp * LPR;
  const bool dact = sub * VEC < p.D;
  const I* crow = reinterpret_cast<const I*>(p.crow) + (int64_t)n * (p.T_dst + 1);
  const I* col = reinterpret_cast<const I*>(p.col) + n * p.col_stride_n;
  const float* vals = p.values + n * p.col_stride_n;
  const int32_t* ho = p.head_off + ((int64_t)n * p.T_dst + t) * (p.H + 1);
  const int64_t beg = (int64_t)crow[t] + ho[h], end = (int64_t)crow[t] + ho[h + 1];
  const T* vb = reinterpret_cast<const T*>(p.v) + n * p.vs[0] + h * p.vs[1] + sub * VEC;
  const int64_t hcol = (int64_t)h * p.T_src;
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  for (int64_t e0 = beg; e0 < end; e0 += KPI) {
    const int64_t e = e0 + grp;
    const bool ok = e < end;
    const int64_t key = ok ? ((int64_t)col[e] - hcol) : 0;
    const float pv = ok ? vals[e] : 0.f;
    uint4 vr = make_uint4(0, 0, 0, 0);
    // groups past the list's end load no V row: 0 * V[0] is NaN when row 0 is not finite, and nobody need have kept it
    if (dact && ok) vr = *reinterpret_cast<const uint4*>(vb + key * p.vs[2]);
    float vf[VEC];
    unpack16<T>(vr, vf);
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = fmaf(pv, vf[j], acc[j]);
  }
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] += __shfl_xor(acc[j], o);
  }
  if (grp == 0 && dact) {
    float* op = p.out + (((int64_t)n * p.H + h) * p.T_dst + t) * p.D + sub * VEC;
    store_frag<float, VEC>(op, acc);
  }
}

// ---- host side ---------------------------------------------------------------------------------------
// A decoding step (T_dst of a few rows per (n, h)): the fused form has nothing to win there (one row per workgroup), and the
// plain lane-group kernel warms the row's K / V lines with its idle lane groups first (below).  sea_attention_few_rows().
constexpr int64_t SEA_ATTN_FEW_ROWS = 2048;

// one new row per sequence (sparse_attn_decode1_kernel): contiguous K / V, or (p.table) the PAGED form, the table row behind the V rows
template <typename T, typename TO, int LPR, bool X80, bool WP>
static void launch_decode1(const AttnParams& p, hipStream_t s) {
  constexpr int lds = Decode1Lds<LPR, X80>::bytes;
  const dim3 grid((unsigned)(p.N * p.H)), block(256);
  if (p.table) {
    const int tab = (int)((p.T_src + (1 << p.page_shift) - 1) >> p.page_shift) * (int)sizeof(int);
    hipLaunchKernelGGL((sparse_attn_decode1_kernel<T, TO, LPR, X80, true, WP>), grid, block, lds + tab, s, p);
  } else {
    hipLaunchKernelGGL((sparse_attn_decode1_kernel<T, TO, LPR, X80, false, WP>), grid, block, lds, s, p);
  }
}

// the lane-group kernel's entry point for a row fragment: d = 80 has its own (they differ in their launch bounds)
template <typename T, typename TO, int LPR, bool WP, int NWB, bool FUSE, bool DEC, bool ORD, bool X80>
static constexpr auto rows_entry() {
  if constexpr (X80) return &sparse_attn_rows80_kernel<T, TO, 4, WP, NWB, FUSE, DEC, ORD>;
  else return &sparse_attn_rows_kernel<T, TO, LPR, 4, WP, NWB, FUSE, DEC, ORD>;
}

// the lane-group kernels over rows of LPR lanes (X80: d = 80, 8 lanes x (8 + 2) elements per row): the plain form, or with
// p.bits one of the fused forms -- decode, rows dealt from pools, fused inference
template <typename T, typename TO, int LPR, bool WP, bool X80>
static int launch_rows(AttnParams p, hipStream_t s) {
  // rows per workgroup (sorted by length inside the kernel): 64 for rows of 4 or 8 lanes, 32 for rows of 16 lanes.
  // Measured at the headline shape (layer's own selection, bf16 d = 64): 32 / 64 / 128 rows per block 0.99 / 0.96 / 1.00 ms.
  constexpr int NWB = LPR == 4 ? 4 : 8, RPB = NWB * (64 / LPR);
  const int NH = p.N * p.H;
  p.TB = (p.T_dst + RPB - 1) / RPB;
  void (*kern)(AttnParams) = rows_entry<T, TO, LPR, WP, NWB, false, false, false, X80>();
  int lds = 0;
  if (p.bits) {                                            // fused interpolation: group-private key lists in LDS
    if constexpr (LPR == 4) {
      return SEA_EUNSUPPORTED;
    } else {
      lds = p.fuse_cap * (int)sizeof(int);
      kern = rows_entry<T, TO, LPR, WP, NWB, true, false, false, X80>();
      if (p.t_src_dev) {                                   // decode form
        kern = rows_entry<T, TO, LPR, WP, NWB, true, true, false, X80>();
      } else if constexpr (!WP) {
        if (p.order) {                                     // rows dealt from pools (the entry has checked the form)
          if (p.pool_rows % RPB) return SEA_EINVAL;
          p.TB = p.pools * (p.pool_rows / RPB);
          hipLaunchKernelGGL(attn_row_order_kernel, dim3((unsigned)(NH * p.pools)), dim3(p.pool_rows < 64 ? 64 : p.pool_rows), 0, s, p);
          kern = rows_entry<T, TO, LPR, false, NWB, true, false, true, X80>();
        }
      }
    }
  }
  const dim3 grid((unsigned)((int64_t)8 * ((NH + 7) / 8) * p.TB)), block(NWB * 64);
  hipLaunchKernelGGL(kern, grid, block, lds, s, p);
  return SEA_OK;
}

template <typename T, typename TO, bool WP>
static int launch_attn_wp(AttnParams p, hipStream_t s) {
  constexpr int VEC = Elem<T>::VEC;
  const int lpr = lanes_per_row(p.D, VEC);
  const int NH = p.N * p.H;
  const int esz = (int)sizeof(T);
  const bool small = p.T_src < (1 << 24) && p.ks[2] * esz < (1 << 24) && p.vs[2] * esz < (1 << 24) &&
                     (int64_t)p.T_src * p.ks[2] * esz < (1ll << 31) && (int64_t)p.T_src * p.vs[2] * esz < (1ll << 31);
  if constexpr (sizeof(T) == 2) {
    // one new row per sequence (a DecodeSession position): the whole workgroup serves the row (sparse_attn_decode1_kernel)
    if (p.bits && p.t_src_dev && p.T_dst == 1 && p.T_m <= 256 && small && (lpr == 8 || lpr == 16 || p.D == 80)) {
      if (p.D == 80) launch_decode1<T, TO, 8, true, WP>(p, s);
      else if (lpr == 8) launch_decode1<T, TO, 8, false, WP>(p, s);
      else launch_decode1<T, TO, 16, false, WP>(p, s);
      return SEA_OK;
    }
  }
  if (p.table) return SEA_EUNSUPPORTED;                    // (only the one-row decode kernel reads a page pool)
  if constexpr (sizeof(T) == 2) {
    if (p.D == 80 && small) return launch_rows<T, TO, 8, WP, true>(p, s);
  }
  if (lpr <= 16 && small) {
    switch (lpr) {
      case 4: return launch_rows<T, TO, 4, WP, false>(p, s);
      case 8: return launch_rows<T, TO, 8, WP, false>(p, s);
      default: return launch_rows<T, TO, 16, WP, false>(p, s);
    }
  }
  if (p.bits) return SEA_EUNSUPPORTED;                      // (the wave-per-row kernel below has no fused form)
  const int64_t blocks = (int64_t)8 * ((NH + 7) / 8) * p.TB;
  dim3 grid((unsigned)blocks), block(256);
  switch (lpr) {
    case 4: hipLaunchKernelGGL((sparse_attn_kernel<T, TO, 4, 2, WP>), grid, block, 0, s, p); break;
    case 8: hipLaunchKernelGGL((sparse_attn_kernel<T, TO, 8, 4, WP>), grid, block, 0, s, p); break;
    case 16: hipLaunchKernelGGL((sparse_attn_kernel<T, TO, 16, 4, WP>), grid, block, 0, s, p); break;
    case 32: hipLaunchKernelGGL((sparse_attn_kernel<T, TO, 32, 4, WP>), grid, block, 0, s, p); break;
    case 64: hipLaunchKernelGGL((sparse_attn_kernel<T, TO, 64, 4, WP>), grid, block, 0, s, p); break;
    default: return SEA_EUNSUPPORTED;
  }
  return SEA_OK;
}

// Kernel choice (fixed, no run-time switches): 16-bit d = 80 -> rows80; rows of <= 16 lanes with 32-bit byte offsets ->
// lane-group-per-row kernel; anything else (fp32 d >= 128, huge strides) -> wave-per-row kernel.
template <typename T, typename TO>
static int launch_attn(const AttnParams& p, hipStream_t s) {
  return p.probs ? launch_attn_wp<T, TO, true>(p, s) : launch_attn_wp<T, TO, false>(p, s);
}

template <typename T, typename I>
static int launch_sddmm(const SddmmParams& p, hipStream_t s) {
  const int lpr = lanes_per_row(p.D, Elem<T>::VEC);
  const int64_t rows = (int64_t)p.N * p.T_dst;
  dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  switch (lpr) {
    case 4: hipLaunchKernelGGL((csr_sddmm_kernel<T, I, 4>), grid, block, 0, s, p); break;
    case 8: hipLaunchKernelGGL((csr_sddmm_kernel<T, I, 8>), grid, block, 0, s, p); break;
    case 16: hipLaunchKernelGGL((csr_sddmm_kernel<T, I, 16>), grid, block, 0, s, p); break;
    case 32: hipLaunchKernelGGL((csr_sddmm_kernel<T, I, 32>), grid, block, 0, s, p); break;
    case 64: hipLaunchKernelGGL((csr_sddmm_kernel<T, I, 64>), grid, block, 0, s, p); break;
    default: return SEA_EUNSUPPORTED;
  }
  return SEA_OK;
}

template <typename T, typename I>
static int launch_spmm(const SpmmParams& p, hipStream_t s) {
  const int lpr = lanes_per_row(p.D, Elem<T>::VEC);
  const int NH = p.N * p.H;
  const int64_t blocks = (int64_t)8 * ((NH + 7) / 8) * p.TB;
  dim3 grid((unsigned)blocks), block(256);
  switch (lpr) {
    case 4: hipLaunchKernelGGL((csr_spmm_kernel<T, I, 4>), grid, block, 0, s, p); break;
    case 8: hipLaunchKernelGGL((csr_spmm_kernel<T, I, 8>), grid, block, 0, s, p); break;
    case 16: hipLaunchKernelGGL((csr_spmm_kernel<T, I, 16>), grid, block, 0, s, p); break;
    case 32: hipLaunchKernelGGL((csr_spmm_kernel<T, I, 32>), grid, block, 0, s, p); break;
    case 64: hipLaunchKernelGGL((csr_spmm_kernel<T, I, 64>), grid, block, 0, s, p); break;
    default: return SEA_EUNSUPPORTED;
  }
  return SEA_OK;
}

}  // namespace sea

using namespace sea;

static int check_dtype(const char* name, int dtype) {
  SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_F16 || dtype == SEA_BF16, SEA_EINVAL, "%s: bad dtype %d", name, dtype);
  return SEA_OK;
}

// t_src_stride > 0 (the decode form only: bits and t_src_dev required): per-sequence lengths, sequence n's rows follow
// t_src_dev[n * t_src_stride].  block_table != NULL (the one-row decode form with per-sequence lengths): paged K / V -- k / v
// are the K / V halves of a page pool, strides [page, head, row]; sequence n's key r lives in page
// block_table[n * table_stride + r / page_rows] at row r % page_rows.  Column ids stay head * T_src + key.
extern "C" int sea_sparse_attention(const void* q, const void* k, const void* v, int dtype, int64_t N, int64_t H,
                                    int64_t T_dst, int64_t T_src, int64_t D, const int64_t* q_strides,
                                    const int64_t* k_strides, const int64_t* v_strides, const int32_t* crow,
                                    const int32_t* col, int64_t col_stride_n, const int32_t* head_off,
                                    const float* row_scale, const void* avg, const int64_t* avg_strides,
                                    const float* mix, void* out, int out_dtype, const int64_t* out_strides,
                                    float* probs_out, int64_t probs_stride_n, const uint8_t* block_path, int flags,
                                    const uint32_t* bits, int64_t T_m, int is_causal, int max_k, int write_cols,
                                    const int32_t* t_src_dev, int64_t t_src_stride, const int32_t* block_table,
                                    int64_t table_stride, int64_t page_rows, sea_stream_t stream) {
  const char* nm = "sea_sparse_attention";
  // SEA_ATTN_KEYRANGE: range_keys in bits 16..30 of flags, the workspace in probs_out / probs_stride_n (sea_hip.h)
  // SEA_ATTN_ROW_POOL: log2 of the pool in bits 4..7 of flags, the order workspace in block_path / probs_stride_n (sea_hip.h)
  int pool_log2 = (flags >> SEA_ATTN_ROW_POOL_SHIFT) & 0xf;
  flags &= ~(0xf << SEA_ATTN_ROW_POOL_SHIFT);
  const uint16_t* order = nullptr;
  int64_t order_stride_n = 0;
  if (pool_log2) {
    const char* rp = "the row-pool form";
    SEA_REQUIRE((flags & 0xff) != SEA_ATTN_KEYRANGE && (flags & 0xff) != SEA_ATTN_TILE, SEA_EUNSUPPORTED,
                "%s: %s deals the rows of the fused gather kernels: the key-range and tile paths have none (path %d)", nm, rp, flags & 0xff);
    SEA_REQUIRE(bits != nullptr, SEA_EUNSUPPORTED, "%s: %s is a fused form (bits is NULL)", nm, rp);
    SEA_REQUIRE(t_src_dev == nullptr && block_table == nullptr && t_src_stride == 0, SEA_EUNSUPPORTED,
                "%s: %s has no decode or paged form (t_src_dev / block_table)", nm, rp);
    SEA_REQUIRE(probs_out == nullptr, SEA_EUNSUPPORTED, "%s: %s writes no per-entry probabilities (probs_out must be NULL)", nm, rp);
    SEA_REQUIRE(N > 0 && H > 0 && T_dst > 0 && T_src > 0 && D > 0, SEA_EINVAL, "%s: bad shape", nm);
    if (N * H * T_dst <= SEA_ATTN_FEW_ROWS) {              // a launch of few rows: the field is ignored, the workspace not read
      pool_log2 = 0;
      block_path = nullptr;
      probs_stride_n = 0;
    }
  }
  if (pool_log2) {
    const char* rp = "the row-pool form";
    const int64_t pool = 1ll << pool_log2;
    SEA_REQUIRE(pool <= 1024, SEA_EUNSUPPORTED, "%s: %s takes pools of at most 1024 rows (got %lld)", nm, rp, (long long)pool);
    // rows per workgroup of the fused gather kernels (launch_attn_wp): 64 for rows of 8 lanes (d = 80 included), 32 for rows of 16
    const int64_t rpb = (dtype == SEA_F32 ? D > 32 : (D > 64 && D != 80)) ? 32 : 64;
    SEA_REQUIRE(pool % rpb == 0, SEA_EUNSUPPORTED, "%s: %s needs a pool that is a multiple of the %lld rows of a workgroup (got %lld)",
                nm, rp, (long long)rpb, (long long)pool);
    const int64_t pools = (T_dst + pool - 1) / pool, need = H * pools * pool;
    SEA_REQUIRE(block_path != nullptr && aligned16(block_path) && probs_stride_n >= need, SEA_EINVAL,
                "%s: %s needs a 16-byte aligned uint16 workspace in block_path with probs_stride_n >= %lld elements per batch "
                "item (got %lld)", nm, rp, (long long)need, (long long)probs_stride_n);
    order = reinterpret_cast<const uint16_t*>(block_path);
    order_stride_n = probs_stride_n;
    block_path = nullptr;                                  // (no plan in the fused form)
    probs_stride_n = 0;
  }
  const bool keyrange = (flags & 0xff) == SEA_ATTN_KEYRANGE;
  // bits 16..17 / 18..19 (every path but the key-range form, whose range_keys sit there): the grid order and log2 of its group
  int grid_order = SEA_GRID_ASCENDING, grid_group = 1;
  if (!keyrange) {
    grid_order = (flags >> SEA_ATTN_GRID_ORDER_SHIFT) & 3;
    grid_group = 1 << ((flags >> SEA_ATTN_GRID_GROUP_SHIFT) & 3);
    flags &= 0xffff;
    SEA_REQUIRE(grid_order <= SEA_GRID_GROUPED && grid_group <= 4, SEA_EINVAL,
                "%s: grid order %d with groups of %d pairs: orders 0 .. 2, groups of 1, 2 or 4", nm, grid_order, grid_group);
  }
  KeyRangeParams kr = {nullptr, 0, 0, 0};
  if (keyrange) {
    SEA_REQUIRE(bits != nullptr, SEA_EUNSUPPORTED, "%s: the key-range form is a fused form (bits is NULL)", nm);
    SEA_REQUIRE(t_src_dev == nullptr && block_table == nullptr && t_src_stride == 0, SEA_EUNSUPPORTED,
                "%s: the key-range form has no decode or paged form (t_src_dev / block_table)", nm);
    SEA_REQUIRE(write_cols == 0, SEA_EUNSUPPORTED, "%s: the key-range form writes no columns (write_cols must be 0)", nm);
    SEA_REQUIRE(N > 0 && H > 0 && T_dst > 0 && T_src > 0 && D > 0, SEA_EINVAL, "%s: bad shape", nm);
    SEA_REQUIRE(dtype == SEA_F32 ? (D == 32 || D == 64) : (D == 64 || D == 128), SEA_EUNSUPPORTED,
                "%s: the key-range form takes 16-bit D in {64, 128} or fp32 D in {32, 64} (dtype %d, D=%lld)", nm, dtype, (long long)D);
    const int64_t rk = (flags >> 16) & 0x7fff;
    SEA_REQUIRE(rk > 0, SEA_EINVAL, "%s: the key-range form needs range_keys (1 .. 32767) in bits 16..30 of flags", nm);
    const int64_t nr = (T_src + rk - 1) / rk;
    SEA_REQUIRE(nr <= 64, SEA_EUNSUPPORTED, "%s: the key-range form takes at most 64 ranges (%lld keys in ranges of %lld: %lld)", nm,
                (long long)T_src, (long long)rk, (long long)nr);
    SEA_REQUIRE(block_path == nullptr, SEA_EINVAL, "%s: the key-range form takes no plan (block_path must be NULL)", nm);
    const int64_t need = H * nr * T_dst * (D + 2);
    SEA_REQUIRE(probs_out != nullptr && aligned16(probs_out) && probs_stride_n >= need, SEA_EINVAL,
                "%s: the key-range form needs a 16-byte aligned fp32 workspace in probs_out with probs_stride_n >= %lld floats per "
                "batch item (got %lld)", nm, (long long)need, (long long)probs_stride_n);
    SEA_REQUIRE(N == 1 || probs_stride_n % 4 == 0, SEA_EINVAL,
                "%s: the key-range form needs every batch item of its workspace 16-byte aligned: probs_stride_n %lld is no "
                "multiple of 4", nm, (long long)probs_stride_n);
    kr.ws = probs_out; kr.ws_stride_n = probs_stride_n; kr.range_keys = (int)rk; kr.n_ranges = (int)nr;
    probs_out = nullptr;                                   // (the per-entry probabilities are not available in this form)
    probs_stride_n = 0;
  }
  if (t_src_stride || block_table) {
    SEA_REQUIRE(bits && t_src_dev && (!block_table || (k_strides && v_strides)), SEA_EINVAL, "%s: null pointer", nm);
    SEA_REQUIRE(t_src_stride > 0, SEA_EINVAL, "%s: t_src_stride must be >= 1 (got %lld)", nm, (long long)t_src_stride);
  }
  if (block_table) {
    SEA_REQUIRE(dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: 16-bit data only (dtype %d)", nm, dtype);
    if (int e = paged_layout_check(nm, dtype, D, T_src, page_rows, table_stride, N)) return e;
    SEA_REQUIRE(T_dst == 1 && T_m > 0 && T_m <= 256, SEA_EUNSUPPORTED, "%s: the one-row decode form (T_dst = 1, T_m <= 256)", nm);
    SEA_REQUIRE((T_src + page_rows - 1) / page_rows <= 4096, SEA_EUNSUPPORTED,
                "%s: a table row of %lld pages does not fit the kernel's LDS (4096 at most)", nm, (long long)((T_src + page_rows - 1) / page_rows));
    // byte offsets: the page term is 64-bit (a page index times the page stride, which must fit 32 bits), the row term 32-bit
    // (24-bit factors: __umul24 of the row and the row stride)
    const int64_t esz = 2;
    SEA_REQUIRE(k_strides[0] > 0 && v_strides[0] > 0 && k_strides[0] * esz < (1ll << 32) && v_strides[0] * esz < (1ll << 32) &&
                    k_strides[2] * esz < (1ll << 24) && v_strides[2] * esz < (1ll << 24) &&
                    page_rows * k_strides[2] * esz < (1ll << 31) && page_rows * v_strides[2] * esz < (1ll << 31),
                SEA_EUNSUPPORTED, "%s: page / row strides whose byte offsets do not fit (page stride < 4 GB, page < 2 GB)", nm);
  } else {
    SEA_REQUIRE(page_rows == 0 && table_stride == 0, SEA_EINVAL,
                "%s: null pointer: page_rows / table_stride without a block_table", nm);
  }
  // bits != NULL: the fused form -- `col` is written by the launch, not read -- which runs on the gather kernels;
  // t_src_dev != NULL: its decode form (T_src is then the capacity of the K / V caches)
  SEA_REQUIRE(bits != nullptr || t_src_dev == nullptr, SEA_EINVAL, "%s: the decode form (t_src_dev) needs bits", nm);
  if (bits && !keyrange) flags = SEA_ATTN_GATHER;
  SEA_REQUIRE(q && k && v && crow && col && head_off && out && q_strides && k_strides && v_strides && out_strides,
              SEA_EINVAL, "%s: null pointer", nm);
  if (int e = check_dtype(nm, dtype)) return e;
  SEA_REQUIRE(out_dtype == SEA_F32 || out_dtype == dtype, SEA_EUNSUPPORTED, "%s: out dtype must be fp32 or the input dtype", nm);
  SEA_REQUIRE((mix == nullptr) == (avg == nullptr), SEA_EINVAL, "%s: avg and mix go together", nm);
  SEA_REQUIRE(!avg || avg_strides, SEA_EINVAL, "%s: avg_strides is null", nm);
  SEA_REQUIRE(N > 0 && H > 0 && T_dst > 0 && T_src > 0 && D > 0, SEA_EINVAL, "%s: bad shape", nm);
  const int path = flags & 0xff;
  SEA_REQUIRE(path == SEA_ATTN_AUTO || path == SEA_ATTN_GATHER || path == SEA_ATTN_TILE || path == SEA_ATTN_KEYRANGE, SEA_EINVAL, "%s: bad path %d", nm, path);
  const int vec = dtype == SEA_F32 ? 4 : 8;
  SEA_REQUIRE(D % vec == 0 && D <= 64 * vec, SEA_EUNSUPPORTED, "%s: D=%lld must be a multiple of %d and <= %d", nm,
              (long long)D, vec, 64 * vec);
  SEA_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && (!avg || aligned16(avg)) && aligned16(out), SEA_EUNSUPPORTED,
              "%s: tensors must be 16-byte aligned", nm);
  SEA_REQUIRE(strides_ok(q_strides, vec) && strides_ok(k_strides, vec) && strides_ok(v_strides, vec) &&
                  strides_ok(out_strides, vec) && (!avg || strides_ok(avg_strides, vec)),
              SEA_EUNSUPPORTED, "%s: row strides must be multiples of %d elements", nm, vec);
  SEA_REQUIRE(N * H * ((T_dst + 3) / 4) < (1ll << 28), SEA_EUNSUPPORTED, "%s: grid too large", nm);
  AttnParams p;
  p.q = q; p.k = k; p.v = v;
  for (int i = 0; i < 3; ++i) {
    p.qs[i] = q_strides[i]; p.ks[i] = k_strides[i]; p.vs[i] = v_strides[i]; p.os[i] = out_strides[i];
    p.as[i] = avg ? avg_strides[i] : 0;
  }
  p.N = (int)N; p.H = (int)H; p.T_dst = (int)T_dst; p.T_src = (int)T_src; p.D = (int)D;
  p.crow = crow; p.col = col; p.col_stride_n = col_stride_n; p.head_off = head_off;
  p.row_scale = row_scale; p.avg = avg; p.mix = mix; p.out = out;
  p.probs = probs_out; p.probs_stride_n = probs_stride_n;
  p.sel = nullptr; p.sel_want = 0; p.TB16 = (int)((T_dst + 15) / 16);
  p.sel_count = nullptr; p.sel_total = (int)(N * H * p.TB16);
  // share of tile-favouring blocks above which the tile kernel takes the launch (scripts/sweep_plan_threshold.py, round 3:
  // with the plan's cut at 30 entries per staged tile the structured map gives 0.53 / 0.71 / 0.51 at d = 64 / 80 / 128 and
  // the tile kernel wins by 4 % / 13 % / loses by 13 %; the layer's own and independent rows give <= 0.33 and lose always)
  p.sel_num = D >= 128 ? 13 : 1; p.sel_den = D >= 128 ? 20 : 2;
  p.bits = bits; p.col_w = const_cast<int32_t*>(col); p.T_m = (int)T_m; p.W = (int)((H * T_m + 31) / 32);
  p.max_k = max_k; p.is_causal = is_causal;
  p.fuse_cap = 8192;                                        // entries of a block's key lists held in LDS (32 KB)
  p.write_cols = write_cols != 0;
  p.t_src_dev = t_src_dev;
  SEA_REQUIRE(t_src_stride >= 0 && t_src_stride * N < (1ll << 31), SEA_EINVAL, "%s: bad T_src stride %lld", nm,
              (long long)t_src_stride);
  p.t_src_stride = (int)t_src_stride;
  p.table = block_table; p.table_stride = (int)table_stride; p.page_shift = block_table ? __builtin_ctzll(page_rows) : 0;
  p.order = order; p.order_stride_n = order_stride_n;
  p.pool_rows = order ? 1 << pool_log2 : 0; p.pools = order ? (int)((T_dst + p.pool_rows - 1) / p.pool_rows) : 0;
  // the forward prefill launches take the caller's grid order; a decoding step (t_src_dev, or few rows) keeps the ascending one
  const bool prefill = t_src_dev == nullptr && N * H * T_dst > SEA_ATTN_FEW_ROWS;
  p.grid_order = prefill ? grid_order : (int)SEA_GRID_ASCENDING;
  p.grid_group = prefill ? grid_group : 1;
  if (t_src_dev) {
    SEA_REQUIRE(bits != nullptr && T_dst <= SEA_ATTN_WARM_ROWS, SEA_EUNSUPPORTED,
                "%s: the decode form takes T_dst <= %d rows per sequence", nm, SEA_ATTN_WARM_ROWS);
    // probs_out: one fp32 value per entry at the slot `col` has (or would have: write_cols = 0)
    SEA_REQUIRE(probs_out == nullptr || probs_stride_n >= col_stride_n, SEA_EINVAL,
                "%s: the decode form's probs_out needs probs_stride_n >= col_stride_n (%lld < %lld)", nm,
                (long long)probs_stride_n, (long long)col_stride_n);
  }
  if (bits) {
    SEA_REQUIRE(path != SEA_ATTN_TILE && block_path == nullptr, SEA_EUNSUPPORTED, "%s: the fused interpolation runs on the gather kernels", nm);
    SEA_REQUIRE(T_m > 0 && T_m % 32 == 0 && max_k > 0, SEA_EUNSUPPORTED, "%s: fused interpolation needs T_m %% 32 == 0", nm);
    // the stateless form steps thinned pixels on head * T_src + key in fp32 (the reference's arithmetic): sea_csr_emit's guard;
    // the decode form steps the key alone (fused_expand) and needs int32 ids and fp32-exact keys only (`small` below: T_src < 2^24)
    if (t_src_dev) SEA_REQUIRE(H * T_src < (1ll << 31), SEA_EUNSUPPORTED, "%s: the decode form needs int32 ids (H*T_cap < 2^31)", nm);
    else SEA_REQUIRE(H * T_src < (1ll << 24), SEA_EUNSUPPORTED, "%s: H*T_src must stay below 2^24 (fp32-exact ids)", nm);
  }
  p.TB = (int)((T_dst + 3) / 4);
  hipStream_t s = (hipStream_t)stream;
  if (keyrange) {                                          // two launches in stream order (sea_attn_keyrange.hip)
    const int rc = launch_attn_keyrange(p, kr, dtype, out_dtype, s);
    SEA_REQUIRE(rc == SEA_OK, rc, "%s: the key-range form needs K / V byte offsets below 2^31 and a grid below 2^31 workgroups", nm);
    SEA_CHECK_LAUNCH(nm);
    return SEA_OK;
  }
  const bool tile_ok = attn_tile_supported(dtype, (int)D, (int)T_src, p) && probs_out == nullptr;
  if (path == SEA_ATTN_TILE) {
    SEA_REQUIRE(tile_ok, SEA_EUNSUPPORTED, "%s: the tile kernel takes 16-bit data with D in {64, 80, 128} and no probs_out", nm);
  }
  int rc;
  if (path == SEA_ATTN_TILE) {
    rc = launch_attn_tile(p, dtype, out_dtype, flags, s);
    SEA_REQUIRE(rc == SEA_OK, rc, "%s: tile kernel launch parameters rejected (flags 0x%x)", nm, flags);
    SEA_CHECK_LAUNCH(nm);
    return SEA_OK;
  }
  if (path == SEA_ATTN_AUTO && block_path && tile_ok) {      // both kernels over the same rows; the plan's tile-block count
    p.sel = block_path;                                     // decides ON THE DEVICE which of them runs this launch
    p.sel_count = reinterpret_cast<const int32_t*>(block_path + plan_count_offset(N, H, p.TB16));
    p.sel_want = 1;
    rc = launch_attn_tile(p, dtype, out_dtype, flags, s);
    SEA_REQUIRE(rc == SEA_OK, rc, "%s: tile kernel launch parameters rejected (flags 0x%x)", nm, flags);
    SEA_CHECK_LAUNCH(nm);
    p.sel_want = 0;
  }
  if (dtype == SEA_F32) rc = launch_attn<float, float>(p, s);
  else if (dtype == SEA_F16) rc = out_dtype == SEA_F32 ? launch_attn<__half, float>(p, s) : launch_attn<__half, __half>(p, s);
  else rc = out_dtype == SEA_F32 ? launch_attn<__hip_bfloat16, float>(p, s) : launch_attn<__hip_bfloat16, __hip_bfloat16>(p, s);
  SEA_REQUIRE(rc == SEA_OK, rc, "%s: unsupported head size %lld", nm, (long long)D);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}

extern "C" int64_t sea_attention_few_rows(void) { return SEA_ATTN_FEW_ROWS; }

// The kernels' block map on the host (exported beside the ABI of sea_hip.h, not part of it: a test and diagnostic hook): for
// every workgroup index of a launch of NH pairs x TB row blocks, what map_block makes of it.  Returns the grid's size, or a
// negative error code.
extern "C" int64_t sea_attention_grid_map(int64_t NH, int64_t TB, int order, int group, int32_t* pair, int32_t* tb, int32_t* has_work) {
  const char* nm = "sea_attention_grid_map";
  SEA_REQUIRE(pair && tb && has_work, SEA_EINVAL, "%s: null pointer", nm);
  SEA_REQUIRE(NH > 0 && TB > 0 && 8 * ((NH + 7) / 8) * TB < (1ll << 31), SEA_EINVAL, "%s: bad grid %lld x %lld", nm, (long long)NH, (long long)TB);
  SEA_REQUIRE(order >= 0 && order <= SEA_GRID_GROUPED && (group == 1 || group == 2 || group == 4), SEA_EINVAL,
              "%s: grid order %d with groups of %d pairs: orders 0 .. 2, groups of 1, 2 or 4", nm, order, group);
  const int64_t blocks = 8 * ((NH + 7) / 8) * TB;
  for (int64_t b = 0; b < blocks; ++b) {
    int pr = -1, rb = -1;
    has_work[b] = map_block((int)b, (int)NH, (int)TB, order, group, &pr, &rb) ? 1 : 0;
    pair[b] = pr;
    tb[b] = rb;
  }
  return blocks;
}

#ifdef SEA_STAMP
// the stamps of the last lane-group launch: per workgroup (entry, exit, XCC) -- and cleared for the next one
extern "C" int sea_debug_attn_grid_stamps(unsigned long long* host, int64_t blocks) {
  if (blocks > SEA_ATTN_STAMP_BLOCKS) return SEA_EINVAL;
  const size_t bytes = sizeof(unsigned long long) * 3 * (size_t)blocks;
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(sea_attn_grid_stamps), bytes) != hipSuccess) return SEA_ELAUNCH;
  void* dev = nullptr;
  if (hipGetSymbolAddress(&dev, HIP_SYMBOL(sea_attn_grid_stamps)) != hipSuccess || hipMemset(dev, 0, bytes) != hipSuccess) return SEA_ELAUNCH;
  return SEA_OK;
}
#endif

extern "C" int sea_attention_plan(const uint32_t* bits, int64_t N, int64_t H, int64_t T_dst, int64_t T_src, int64_t T_m,
                                  int is_causal, float entries_per_tile, uint8_t* block_path, sea_stream_t stream) {
  const char* nm = "sea_attention_plan";
  SEA_REQUIRE(bits && block_path, SEA_EINVAL, "%s: null pointer", nm);
  SEA_REQUIRE(N > 0 && H > 0 && T_dst > 0 && T_src > 0 && T_m > 0, SEA_EINVAL, "%s: bad shape", nm);
  SEA_REQUIRE(hipMemsetAsync(block_path + plan_count_offset(N, H, (T_dst + 15) / 16), 0, 4, (hipStream_t)stream) == hipSuccess,
              SEA_ELAUNCH, "%s: memset failed", nm);
  const int rc = launch_attn_plan(bits, (int)N, (int)H, (int)T_dst, (int)T_src, (int)T_m, is_causal,
                                  entries_per_tile > 0.f ? entries_per_tile : 30.0f, block_path, (hipStream_t)stream);
  SEA_REQUIRE(rc == SEA_OK, rc, "%s: needs T_m %% 32 == 0, H <= 64 and H * T_m <= 32768", nm);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}

extern "C" int64_t sea_sparse_attention_bytes(int64_t Z, int64_t N, int64_t H, int64_t T_dst, int64_t D, int elem_bytes) {
  return Z * (2 * D * elem_bytes + 4) + N * H * T_dst * (2 * D * elem_bytes + 4);
}

extern "C" int sea_csr_sddmm(const void* q, const void* k, int dtype, int64_t N, int64_t H, int64_t T_dst, int64_t T_src,
                             int64_t D, const int64_t* q_strides, const int64_t* k_strides, const void* crow,
                             const void* col, int idx_bytes, int64_t col_stride_n, float* values, sea_stream_t stream) {
  const char* nm = "sea_csr_sddmm";
  SEA_REQUIRE(q && k && crow && col && values && q_strides && k_strides, SEA_EINVAL, "%s: null pointer", nm);
  if (int e = check_dtype(nm, dtype)) return e;
  SEA_REQUIRE(idx_bytes == 4 || idx_bytes == 8, SEA_EINVAL, "%s: idx_bytes must be 4 or 8", nm);
  const int vec = dtype == SEA_F32 ? 4 : 8;
  SEA_REQUIRE(D % vec == 0 && D <= 64 * vec, SEA_EUNSUPPORTED, "%s: D=%lld must be a multiple of %d", nm, (long long)D, vec);
  SEA_REQUIRE(aligned16(q) && aligned16(k) && strides_ok(q_strides, vec) && strides_ok(k_strides, vec), SEA_EUNSUPPORTED,
              "%s: q/k rows must be 16-byte aligned", nm);
  SddmmParams p;
  p.q = q; p.k = k;
  for (int i = 0; i < 3; ++i) { p.qs[i] = q_strides[i]; p.ks[i] = k_strides[i]; }
  p.N = (int)N; p.H = (int)H; p.T_dst = (int)T_dst; p.T_src = (int)T_src; p.D = (int)D;
  p.crow = crow; p.col = col; p.col_stride_n = col_stride_n; p.values = values;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (idx_bytes == 4) {
    if (dtype == SEA_F32) rc = launch_sddmm<float, int32_t>(p, s);
    else if (dtype == SEA_F16) rc = launch_sddmm<__half, int32_t>(p, s);
    else rc = launch_sddmm<__hip_bfloat16, int32_t>(p, s);
  } else {
    if (dtype == SEA_F32) rc = launch_sddmm<float, int64_t>(p, s);
    else if (dtype == SEA_F16) rc = launch_sddmm<__half, int64_t>(p, s);
    else rc = launch_sddmm<__hip_bfloat16, int64_t>(p, s);
  }
  SEA_REQUIRE(rc == SEA_OK, rc, "%s: unsupported head size", nm);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}

extern "C" int sea_csr_spmm(const float* values, const void* v, int dtype, int64_t N, int64_t H, int64_t T_dst,
                            int64_t T_src, int64_t D, const int64_t* v_strides, const void* crow, const void* col,
                            int idx_bytes, int64_t col_stride_n, const int32_t* head_off, float* out,
                            sea_stream_t stream) {
  const char* nm = "sea_csr_spmm";
  SEA_REQUIRE(values && v && crow && col && head_off && out && v_strides, SEA_EINVAL, "%s: null pointer", nm);
  if (int e = check_dtype(nm, dtype)) return e;
  SEA_REQUIRE(idx_bytes == 4 || idx_bytes == 8, SEA_EINVAL, "%s: idx_bytes must be 4 or 8", nm);
  const int vec = dtype == SEA_F32 ? 4 : 8;
  SEA_REQUIRE(D % vec == 0 && D <= 64 * vec, SEA_EUNSUPPORTED, "%s: D=%lld must be a multiple of %d", nm, (long long)D, vec);
  SEA_REQUIRE(aligned16(v) && aligned16(out) && strides_ok(v_strides, vec), SEA_EUNSUPPORTED,
              "%s: v rows must be 16-byte aligned", nm);
  SpmmParams p;
  p.values = values; p.v = v;
  for (int i = 0; i < 3; ++i) p.vs[i] = v_strides[i];
  p.N = (int)N; p.H = (int)H; p.T_dst = (int)T_dst; p.T_src = (int)T_src; p.D = (int)D;
  p.crow = crow; p.col = col; p.col_stride_n = col_stride_n; p.head_off = head_off; p.out = out;
  p.TB = (int)((T_dst + 3) / 4);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (idx_bytes == 4) {
    if (dtype == SEA_F32) rc = launch_spmm<float, int32_t>(p, s);
    else if (dtype == SEA_F16) rc = launch_spmm<__half, int32_t>(p, s);
    else rc = launch_spmm<__hip_bfloat16, int32_t>(p, s);
  } else {
    if (dtype == SEA_F32) rc = launch_spmm<float, int64_t>(p, s);
    else if (dtype == SEA_F16) rc = launch_spmm<__half, int64_t>(p, s);
    else rc = launch_spmm<__hip_bfloat16, int64_t>(p, s);
  }
  SEA_REQUIRE(rc == SEA_OK, rc, "%s: unsupported head size", nm);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}
