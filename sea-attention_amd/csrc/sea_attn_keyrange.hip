// Key-range form of the fused sparse attention (SEA_ATTN_KEYRANGE), for contexts whose K + V per head exceed an XCD's L2.
//
// The gather kernels (sea_attn.hip) walk each query row's kept keys over the whole key axis: every row block of a head drags
// the head's whole K and V through the L2 (8 MB per head at 32 768 bf16 d = 64 keys against 4 MB of L2 per XCD).  Here the key
// axis is cut into ranges of `range_keys` keys and the launch is RANGE-major per (n, h): all row blocks of one ((n, h), range)
// are dispatched next to each other on that pair's XCD, so the K / V rows in flight there are the range's.
//
//   launch 1  attn_keyrange_partial_kernel   per (n, h, t, range): the online-softmax state (m, l, acc[D]) over the kept pixels
//             whose LOWEST key lies in the range (pixels are not split) -- the gather kernel's walk on that subset: the same
//             expansion arithmetic (fused_expand), frag_dot + group_sum score, U keys in flight.  States go to the caller's
//             workspace; causal row blocks that lie entirely below the range exit before they read anything.
//   launch 2  attn_keyrange_combine_kernel   M = max m_r, L = sum l_r exp(m_r - M), A = sum acc_r exp(m_r - M) over the ranges in
//             ascending order, then the gather kernel's epilogue (A / L * row_scale, mix with avg, out_dtype, out_strides).
//
// Stream order is the only hand-off between the two: no flag, no atomics, no workgroup waits for another one.  State (n, h, t, r)
// is read by launch 2 exactly when range r starts below row t's width; launch 1 writes at least those.
#include "sea_attn.hpp"

namespace sea {

// key j of a pixel [lo, hi) wider than max_k: the reference's fp32 stepping on head * T_src + key (fused_expand / csr_emit_kernel)
__device__ inline int thinned_column(int lo, int hi, int hcol, int max_k, int j) {
  const float fb = (float)hcol;
  const float rs = (float)lo + fb, re = (float)hi + fb;
  const float step = __fdiv_rn(re - rs, (float)max_k);
  return (int)((re - (float)(int)__fmul_rn((float)j, step)) - 1.0f);
}

// The kept pixels of one (row, head) whose lowest key lies in [k0, k1), expanded as fused_expand expands them (pixels ascending,
// keys descending inside a pixel).  Returns the number of entries (every lane of the group); WRITE: entries [c0, c0 + Q) of the
// list go to slice[0 .. Q) as keys (without the head offset).  Lane `sub` owns mask word `sub` of the head, a group scan orders
// the runs.  Wave-uniform control flow around the shuffles: every lane of the wave calls.
template <int LPR, bool WRITE>
__device__ inline int keyrange_expand(const AttnParams& p, const uint32_t* brow, bool rowok, float scale, int sub, int hcol, int k0,
                                      int k1, int c0, int Q, int* slice) {
  const int WPH = p.T_m >> 5;
  int carry = 0;
  for (int w0 = 0; w0 < WPH; w0 += LPR) {                  // uniform
    const int wi = w0 + sub;
    const uint32_t word = (rowok && wi < WPH) ? brow[wi] : 0u;
    uint32_t mine = 0;                                     // the word's kept pixels that belong to this range
    int nent = 0;
    for (uint32_t mm = word; mm;) {
      const int bit = __ffs(mm) - 1;
      mm &= mm - 1;
      const int b = wi * 32 + bit;
      const int lo = (int)interp_bound(b, scale), hi = (int)interp_bound(b + 1, scale);
      const int wd = hi - lo;
      const int low = wd <= p.max_k ? lo : thinned_column(lo, hi, hcol, p.max_k, p.max_k - 1) - hcol;
      if (wd > 0 && low >= k0 && low < k1) {
        mine |= 1u << bit;
        nent += wd < p.max_k ? wd : p.max_k;
      }
    }
    int incl = nent;                                       // inclusive scan over the group's LPR lanes (word order)
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) {
      const int up = __shfl_up(incl, o, LPR);
      if (sub >= o) incl += up;
    }
    int off = carry + incl - nent - c0;                    // this lane's first entry, relative to the window
    carry += __shfl(incl, LPR - 1, LPR);
    if constexpr (WRITE) {
      for (uint32_t mm = mine; mm;) {
        const int b = wi * 32 + __ffs(mm) - 1;
        mm &= mm - 1;
        const int lo = (int)interp_bound(b, scale), hi = (int)interp_bound(b + 1, scale);
        const int wd = hi - lo;
        const int cnt = wd < p.max_k ? wd : p.max_k;
        const int j0 = off < 0 ? -off : 0, j1 = off + cnt > Q ? Q - off : cnt;     // the pixel's entries inside the window
        if (wd <= p.max_k) {
          for (int j = j0; j < j1; ++j) slice[off + j] = hi - 1 - j;
        } else {
          for (int j = j0; j < j1; ++j) slice[off + j] = thinned_column(lo, hi, hcol, p.max_k, j) - hcol;
        }
        off += cnt;
      }
    }
  }
  return carry;
}

// the range that starts at key k0 starts below row t's width: only then can a kept pixel of the row have its lowest key in it
__device__ inline bool range_reaches_row(const AttnParams& p, int t, int k0) {
  return k0 < row_width(t, p.T_dst, p.T_src, p.is_causal);
}

template <typename T, int LPR, int U, int NWB>
__global__ __launch_bounds__(NWB * 64) void attn_keyrange_partial_kernel(AttnParams p, KeyRangeParams kr) {
  using F = RowFrag<T>;
  constexpr int VEC = F::VEC;
  constexpr int RPW = 64 / LPR;       // rows per wave
  constexpr int RPB = NWB * RPW;      // rows per workgroup
  constexpr int Q = SEA_KEYRANGE_LIST / RPB;               // entries of a row's list held in LDS at a time
  static_assert(Q % LPR == 0 && Q % U == 0, "pieces keep the walk's steps of U entries aligned");
  __shared__ int s_keys[SEA_KEYRANGE_LIST];
  // workgroups numbered range-major inside a pair: map_block over TB * n_ranges "row blocks" places the pairs on the XCDs as
  // the gather kernels' launch does (the partial last group of pairs included); ranges ascend per pair
  int pair, tbr;
  if (!map_block(p.N * p.H, p.TB * kr.n_ranges, &pair, &tbr)) return;
  const int rg = tbr / p.TB, tb = tbr - rg * p.TB;
  const int k0 = rg * kr.range_keys, k1 = k0 + kr.range_keys;
  {                                                        // a causal row block entirely below the range: nothing to read,
    const int t_last = min(tb * RPB + RPB, p.T_dst) - 1;   // and launch 2 reads none of its states (block-uniform)
    if (!range_reaches_row(p, t_last, k0)) return;
  }
  const int n = pair / p.H;
  const int h = (pair - n * p.H + n) % p.H;                // heads rotated over the XCDs per item (sparse_attn_rows_kernel)
  const int lane = threadIdx.x & 63;
  const int grp = lane / LPR, sub = lane - grp * LPR;
  const int gi = (int)(threadIdx.x >> 6) * RPW + grp;      // lane group index inside the block
  const int WPH = p.T_m >> 5;
  const int hcol = h * p.T_src;

  // rows dealt to the lane groups by the length of their list IN THIS RANGE (rows_by_length): a counting pass over the natural
  // slot's row first
  int nlen = -1;
  {
    const int tn = tb * RPB + gi;
    const bool in = tn < p.T_dst;
    const int tc = in ? tn : p.T_dst - 1;
    const float sc = interp_scale(row_width(tc, p.T_dst, p.T_src, p.is_causal), p.T_m);
    const int c = keyrange_expand<LPR, false>(p, p.bits + ((int64_t)n * p.T_dst + tc) * p.W + h * WPH, in, sc, sub, hcol, k0, k1, 0,
                                              Q, nullptr);
    if (in) nlen = c;
  }
  bool rowok;
  const int t = tb * RPB + rows_by_length<LPR, RPB>(nlen, gi, sub, &rowok);
  const bool dact = sub * VEC < p.D;
  const int tt = t < p.T_dst ? t : p.T_dst - 1;
  const int sube = dact ? sub : 0;    // lanes beyond D re-read fragment 0 (their q fragment is zero)

  const char* kbase = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.k) + n * p.ks[0] + h * p.ks[1]);
  const char* vbase = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.v) + n * p.vs[0] + h * p.vs[1]);
  const uint32_t kst = (uint32_t)p.ks[2] * (uint32_t)sizeof(T), vst = (uint32_t)p.vs[2] * (uint32_t)sizeof(T);
  const typename F::Lane ln = F::lane(sube);

  F qf;
  qf.clear();
  if (dact) qf.load(reinterpret_cast<const T*>(p.q) + n * p.qs[0] + h * p.qs[1] + (int64_t)tt * p.qs[2], sub);
  const float scale = interp_scale(row_width(tt, p.T_dst, p.T_src, p.is_causal), p.T_m);
  const uint32_t* brow = p.bits + ((int64_t)n * p.T_dst + tt) * p.W + h * WPH;
  int* slice = s_keys + gi * Q;                            // written and read by this lane group alone: no workgroup barrier

  float m = -INFINITY, l = 0.f;
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;

  const int len = keyrange_expand<LPR, true>(p, brow, rowok, scale, sub, hcol, k0, k1, 0, Q, slice);
  int lenmax = len;
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1) lenmax = max(lenmax, __shfl_xor(lenmax, o));
  const int grp_lane0 = (lane - sub) << 2;                 // byte address of the group's first lane for bpermute

  // a list longer than the group's slice passes through it in pieces of Q entries, the state staying in registers
  for (int c0 = 0; c0 < lenmax; c0 += Q) {                 // wave-uniform
    if (c0 > 0) {
      __builtin_amdgcn_wave_barrier();                     // the previous piece has been read
      keyrange_expand<LPR, true>(p, brow, rowok, scale, sub, hcol, k0, k1, c0, Q, slice);
    }
    __builtin_amdgcn_wave_barrier();
    const int pn = min(max(len - c0, 0), Q);               // this group's entries in the piece
    const bool has = pn > 0;                               // a group without entries loads no K / V row at all
    int zmax = pn;
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) zmax = max(zmax, __shfl_xor(zmax, o));
    for (int i0 = 0; i0 < zmax; i0 += LPR) {
      int cidx = 0;
      if (has) {
        const int e = i0 + sub;
        cidx = slice[e < pn ? e : pn - 1];                 // past the end: the piece's last entry again (a kept key's finite row)
      }
#pragma unroll
      for (int u0 = 0; u0 < LPR; u0 += U) {
        if (i0 + u0 < zmax) {                              // wave-uniform
          bool ok[U];
          F kf[U], vr[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            ok[u] = i0 + u0 + u < pn;
            const uint32_t key_c = (uint32_t)__builtin_amdgcn_ds_bpermute(grp_lane0 + ((u0 + u) << 2), cidx);
            kf[u].clear();
            vr[u].clear();
            if (has) {
              kf[u].load(kbase, __umul24(key_c, kst), ln);
              vr[u].load(vbase, __umul24(key_c, vst), ln);
            }
          }
          float s[U];
          float mnew = m;
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const float d = group_sum<LPR>(qf.dot(kf[u]));
            s[u] = ok[u] ? d : -INFINITY;
            mnew = fmaxf(mnew, s[u]);
          }
          softmax_step<U>(s, mnew, vr, m, l, acc);
        }
      }
    }
  }

  if (rowok && dact) {
    float* wsn = kr.ws + n * kr.ws_stride_n;
    const int64_t row = ((int64_t)h * kr.n_ranges + rg) * p.T_dst + t;
    store_frag<float, VEC>(wsn + row * p.D + sub * VEC, acc);
    if (sub == 0) *reinterpret_cast<float2*>(wsn + (int64_t)p.H * kr.n_ranges * p.T_dst * p.D + row * 2) = make_float2(m, l);
  }
}

// one lane group per (n, h, t): the ranges' states merged in ascending order, then sparse_attn_rows_kernel's epilogue
template <typename T, typename TO, int LPR>
__global__ __launch_bounds__(256) void attn_keyrange_combine_kernel(AttnParams p, KeyRangeParams kr) {
  constexpr int VEC = Elem<T>::VEC;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ridx = tid / LPR;                          // ((n * H) + h) * T_dst + t
  const int sub = (int)(tid - ridx * LPR);
  if (ridx >= (int64_t)p.N * p.H * p.T_dst || sub * VEC >= p.D) return;
  const int t = (int)(ridx % p.T_dst);
  const int64_t nh = ridx / p.T_dst;
  const int n = (int)(nh / p.H), h = (int)(nh - (int64_t)n * p.H);
  // the ranges that start below the row's width (all of them for a non-causal row)
  const int w_t = row_width(t, p.T_dst, p.T_src, p.is_causal);
  const int nr = min(kr.n_ranges, (w_t + kr.range_keys - 1) / kr.range_keys);
  const float* wsn = kr.ws + n * kr.ws_stride_n;
  const int64_t rstep = p.T_dst;                           // rows between two ranges of one (h, t)
  const int64_t row0 = (int64_t)h * kr.n_ranges * p.T_dst + t;
  const float2* ml = reinterpret_cast<const float2*>(wsn + (int64_t)p.H * kr.n_ranges * p.T_dst * p.D);
  float M = -INFINITY;
  for (int r = 0; r < nr; ++r) M = fmaxf(M, ml[row0 + r * rstep].x);
  float l = 0.f;
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  for (int r = 0; r < nr; ++r) {
    const float2 s = ml[row0 + r * rstep];
    if (!(s.y > 0.f)) continue;                            // a range that held nothing for the row contributes exactly nothing
    const float w = __expf(s.x - M);
    float af[VEC];
    const float* ap = wsn + (row0 + r * rstep) * p.D + sub * VEC;
#pragma unroll
    for (int j = 0; j < VEC; j += 4) {
      const float4 a4 = *reinterpret_cast<const float4*>(ap + j);
      af[j] = a4.x; af[j + 1] = a4.y; af[j + 2] = a4.z; af[j + 3] = a4.w;
    }
    l = fmaf(s.y, w, l);
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = fmaf(af[j], w, acc[j]);
  }
  attn_epilogue<T, TO, false>(p, ridx, n, h, t, sub, l, acc);
}

template <typename T, typename TO>
static int launch_keyrange(AttnParams p, const KeyRangeParams& kr, hipStream_t s) {
  constexpr int VEC = Elem<T>::VEC;
  const int lpr = p.D / VEC;                               // 8 or 16 (the entry admits nothing else)
  const int esz = (int)sizeof(T);
  const bool small = p.T_src < (1 << 24) && p.ks[2] * esz < (1 << 24) && p.vs[2] * esz < (1 << 24) &&
                     (int64_t)p.T_src * p.ks[2] * esz < (1ll << 31) && (int64_t)p.T_src * p.vs[2] * esz < (1ll << 31);
  if (!small || (lpr != 8 && lpr != 16)) return SEA_EUNSUPPORTED;
  constexpr int NWB = 8;
  const int rpb = NWB * (64 / lpr);
  p.TB = (p.T_dst + rpb - 1) / rpb;
  const int NH = p.N * p.H;
  const int64_t blocks = (int64_t)8 * ((NH + 7) / 8) * p.TB * kr.n_ranges;
  if (blocks >= (1ll << 31)) return SEA_EUNSUPPORTED;
  const int64_t cthreads = (int64_t)NH * p.T_dst * lpr;
  dim3 grid((unsigned)blocks), block(NWB * 64), cgrid((unsigned)((cthreads + 255) / 256));
  if (lpr == 8) {
    hipLaunchKernelGGL((attn_keyrange_partial_kernel<T, 8, 4, NWB>), grid, block, 0, s, p, kr);
    hipLaunchKernelGGL((attn_keyrange_combine_kernel<T, TO, 8>), cgrid, dim3(256), 0, s, p, kr);
  } else {
    hipLaunchKernelGGL((attn_keyrange_partial_kernel<T, 16, 4, NWB>), grid, block, 0, s, p, kr);
    hipLaunchKernelGGL((attn_keyrange_combine_kernel<T, TO, 16>), cgrid, dim3(256), 0, s, p, kr);
  }
  return SEA_OK;
}

int launch_attn_keyrange(const AttnParams& p, const KeyRangeParams& kr, int dtype, int out_dtype, hipStream_t s) {
  if (dtype == SEA_F32) return launch_keyrange<float, float>(p, kr, s);
  if (dtype == SEA_F16) return out_dtype == SEA_F32 ? launch_keyrange<__half, float>(p, kr, s) : launch_keyrange<__half, __half>(p, kr, s);
  return out_dtype == SEA_F32 ? launch_keyrange<__hip_bfloat16, float>(p, kr, s) : launch_keyrange<__hip_bfloat16, __hip_bfloat16>(p, kr, s);
}

}  // namespace sea
