// Causal Performer (generalized ReLU feature map + causal linear attention) as ONE fused kernel, gfx950.  Three forms:
// performer_kernel (fp32 data, described here), performer_bf16_kernel and performer_bf16w_kernel (16-bit data, D = 64 and
// D = 80 / 128); perf_form at the end of the file picks one per (dtype, D, nb).
//
// Replaces step B of SEA's estimator (reference: src/models/perlin_attention/attention.py:497-514,556-590 ->
// performer_pytorch.FastAttention, causal=True, generalized_attention=True; not vendored, see
// perlin_attention/performer.py for the restated algorithm) together with the two concatenations around it:
//     v_for_atten = cat([v_eye_learned_causal[:T], v])          (attention.py:506-510)
//     ctx         = FastAttention(q, k, v_for_atten)            (fp32)
//     performer_value = cat([ctx, v])                           (attention.py:577-590)
// Output: performer_value (N,H,T,3D) = [ctx_pos | ctx_v | v] written directly; nothing else touches HBM.
//
//   phi(x) = relu(D^-1/4 * x W^T) + 1e-3                        W: (nb, D) projection
//   ctx_t  = sum_{s<=t} (phi(q_t).phi(k_s)) V_s / (phi(q_t).(sum_{s<=t} phi(k_s) + 1e-6))
//
// One 512-thread workgroup (8 waves) per (n, h) walks the sequence in chunks of C rows.  The running state
// S = sum phi(k)^T V (NBP x 2D) never leaves the accumulator registers of the wave that owns its columns:
// it is both the C operand of the update S += phi(K_c)^T V_c and -- register r of a 16x16 tile being row
// 4g+r of lane group g -- the B operand of the carry term phi(Q_c) S, with the k index of that product
// permuted accordingly on the A side.  All products run on v_mfma_f32_16x16x4_f32 (exact fp32).
#include "sea_performer16.hpp"
#include <cstdlib>

#ifdef SEA_STAMP
__device__ unsigned long long sea_dbg_perf[16];
__device__ unsigned long long sea_dbg_wg[2048];   // [start, end] (s_memrealtime, 100 MHz) of every workgroup of the wide kernel's output pass
#define PSTAMP(i) do { if (threadIdx.x == 0) { unsigned long long _t = __builtin_amdgcn_s_memtime(); atomicAdd(&sea_dbg_perf[i], _t - _tprev); _tprev = _t; } } while (0)
// (the wide kernel keeps its deltas in registers and adds them once at the end: an atomic per phase sits in front of every vmcnt wait)
#define WSTAMP(i) do { if (threadIdx.x == 0 && (STATE_ONLY || blockIdx.y == 0 || blockIdx.y == gridDim.y - 1)) { unsigned long long _t = __builtin_amdgcn_s_memtime(); _tacc[i] += _t - _tprev; _tprev = _t; } } while (0)
#define WSTAMP_FLUSH() do { if (!STATE_ONLY && threadIdx.x == 0 && (blockIdx.y == 0 || blockIdx.y == gridDim.y - 1)) for (int _i = 0; _i < 4; ++_i) atomicAdd(&sea_dbg_perf[_i + (blockIdx.y ? 0 : 4)], _tacc[_i]); \
    if (STATE_ONLY && threadIdx.x == 0) for (int _i = 0; _i < 4; ++_i) atomicAdd(&sea_dbg_perf[10 + _i], _tacc[_i]); \
    if (threadIdx.x == 0) atomicAdd(&sea_dbg_perf[STATE_ONLY ? 8 : 9], __builtin_amdgcn_s_memtime() - _tstart); \
    if (!STATE_ONLY && threadIdx.x == 0) { const int _w = blockIdx.y * gridDim.x + blockIdx.x; if (_w < 1024) { sea_dbg_wg[2 * _w] = _rstart; sea_dbg_wg[2 * _w + 1] = __builtin_amdgcn_s_memrealtime(); } } } while (0)
#else
#define PSTAMP(i) do {} while (0)
#define WSTAMP(i) do {} while (0)
#define WSTAMP_FLUSH() do {} while (0)
#endif

namespace sea {

#define SEA_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)


// fp32 data.  NW = 8 waves per workgroup: two per SIMD, so one wave's LDS/MFMA latency hides behind the other's issue
template <int D, int NBT, int C, bool STATE_ONLY>
__global__ __launch_bounds__(512) void performer_kernel(PerfParams p) {
  using P = PerfF32Plan<D, NBT, C>;          // the constants, the LDS images and the carry size (sea_performer16.hpp)
  constexpr int NW = P::NW, NTH = P::NTH, NBP = P::NBP, RB = P::RB, EB = P::EB, JB = P::JB;
  constexpr int LDQ = P::LDQ, LDV = P::LDV, LDP = P::LDP, LDA = P::LDA, LDW = P::LDW, DSL = P::DSL;
  constexpr int VEC = Elem<float>::VEC;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *sW = smem + P::oW, *sQ = smem + P::oQ, *sK = smem + P::oK, *sV = smem + P::oV, *sQp = smem + P::oQp, *sKp = smem + P::oKp;
  float *sKsum = smem + P::oKsum, *sDen = smem + P::oDen, *sDenP = smem + P::oDenP;
  float* sA = sQ;                 // the masked A tile overlays the Q chunk

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;   // MFMA lane coordinates
  const int nh = blockIdx.x;
  const int n = nh / p.H, h = nh - n * p.H;
  const int seg = blockIdx.y;
  const int t_begin = seg * p.seg_len, t_end = min(p.T, t_begin + p.seg_len);
  const float* qb = reinterpret_cast<const float*>(p.q) + n * p.qs[0] + h * p.qs[1];
  const float* kb = reinterpret_cast<const float*>(p.k) + n * p.ks[0] + h * p.ks[1];
  const float* vb = reinterpret_cast<const float*>(p.v) + n * p.vs[0] + h * p.vs[1];
  const int tb = p.t_base_dev ? *p.t_base_dev : p.t_base;       // rows the state has already seen (block-uniform)
  const float* pb = reinterpret_cast<const float*>(p.pos) + (p.t_base_dev ? (int64_t)tb * p.pos_stride : 0);
  float* ob = reinterpret_cast<float*>(p.out) + (int64_t)nh * p.T * (3 * D);
  const float cnorm = powf((float)D, -0.25f);

  for (int i = tid; i < NBP * LDW; i += NTH) {
    const int r = i / LDW, c = i - r * LDW;
    sW[i] = (r < p.nb && c < D) ? p.W[r * D + c] : 0.f;
  }

  // state = sum of the increments of the segments before this one (fixed order); raw per-thread register images
  constexpr int CARRY = (int)P::carry_floats;
  f4 S[JB][NBT];
#pragma unroll
  for (int a = 0; a < JB; ++a)
#pragma unroll
    for (int b = 0; b < NBT; ++b) S[a][b] = f4{0.f, 0.f, 0.f, 0.f};
  {
    float ks0 = 0.f;
    if (!STATE_ONLY && p.state_in) {                       // increments of pass 1 do not include the incoming state
      const float* cr = p.state_in + (int64_t)nh * CARRY;
#pragma unroll
      for (int a = 0; a < JB; ++a)
#pragma unroll
        for (int b = 0; b < NBT; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) S[a][b][r] = cr[((a * NBT + b) * 4 + r) * NTH + tid];
      if (tid < NBP) ks0 = cr[P::ksum_at + tid];
    }
    if (!STATE_ONLY) {
      for (int s2 = 0; s2 < seg; ++s2) {
        const float* cr = p.carry + ((int64_t)nh * (p.nseg - 1) + s2) * CARRY;
#pragma unroll
        for (int a = 0; a < JB; ++a)
#pragma unroll
          for (int b = 0; b < NBT; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) S[a][b][r] += cr[((a * NBT + b) * 4 + r) * NTH + tid];
        if (tid < NBP) ks0 += cr[P::ksum_at + tid];
      }
    }
    if (tid < NBP) sKsum[tid] = ks0;
  }

#ifdef SEA_STAMP
  unsigned long long _tprev = __builtin_amdgcn_s_memtime();
#endif
  // chunk staging is software-pipelined: the global loads of chunk c+1 are issued before the MFMA phases of
  // chunk c and only written to LDS after them (the loads stay in flight across the barriers)
  constexpr int NCH = (C * (D / VEC) + NTH - 1) / NTH;     // 16-byte pieces per thread and tensor
  uint4 pq[NCH], pk[NCH], pv[NCH], pp[NCH];
  auto issue_loads = [&](int t0n) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = tid + i * NTH;
      const int r = ch / (D / VEC), c = (ch - r * (D / VEC)) * VEC;
      pq[i] = pk[i] = pv[i] = pp[i] = make_uint4(0, 0, 0, 0);
      if (ch < C * (D / VEC) && t0n + r < t_end) {
        const int64_t t = t0n + r;
        if (!STATE_ONLY) pq[i] = *reinterpret_cast<const uint4*>(qb + t * p.qs[2] + c);
        pk[i] = *reinterpret_cast<const uint4*>(kb + t * p.ks[2] + c);
        pv[i] = *reinterpret_cast<const uint4*>(vb + t * p.vs[2] + c);
        pp[i] = *reinterpret_cast<const uint4*>(pb + t * p.pos_stride + c);
      }
    }
  };
  issue_loads(t_begin);

  for (int t0 = t_begin; t0 < t_end; t0 += C) {
    const int rows = min(C, t_end - t0);
    // ---- (a) registers -> LDS as fp32: Q, K (C x D), V = [pos | v] (C x 2D); copy v into out[..., 2D:3D] ------
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = tid + i * NTH;
      if (ch < C * (D / VEC)) {
        const int r = ch / (D / VEC), c = (ch - r * (D / VEC)) * VEC;
        float fq[VEC], fk[VEC], fv[VEC], fp[VEC];
        if (!STATE_ONLY && r < rows) *reinterpret_cast<uint4*>(ob + (int64_t)(t0 + r) * (3 * D) + 2 * D + c) = pv[i];
        unpack16<float>(pv[i], fv); unpack16<float>(pp[i], fp);
        unpack16<float>(pq[i], fq); unpack16<float>(pk[i], fk);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          sQ[r * LDQ + c + j] = fq[j];
          sK[r * LDQ + c + j] = fk[j];
          sV[r * LDV + c + j] = fp[j];
          sV[r * LDV + D + c + j] = fv[j];
        }
      }
    }
    if (t0 + C < t_end) issue_loads(t0 + C);               // next chunk: in flight during phases (b)..(e)
    if (!STATE_ONLY) for (int i = tid; i < C * DSL; i += NTH) sDenP[i] = 0.f;
    __syncthreads();
    PSTAMP(0);   // (a) staging

    // ---- (b) feature maps phi(Q), phi(K): (C x D) @ W^T -> (C x NBP) -------------------------------------
    // a wave takes (matrix, row block) pairs: one A fragment feeds NBT independent accumulators
    for (int grp = (STATE_ONLY ? RB : 0) + wv; grp < 2 * RB; grp += NW) {   // the state-only pass needs phi(K) alone
      const int which = grp / RB, ib = grp - which * RB;        // 0: Q, 1: K
      const float* src = which ? sK : sQ;
      f4 acc[NBT];
#pragma unroll
      for (int jb = 0; jb < NBT; ++jb) acc[jb] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int ks = 0; ks < D / 4; ++ks) {
        const float a = src[(ib * 16 + li) * LDQ + ks * 4 + lg];       // A[i][k]
#pragma unroll
        for (int jb = 0; jb < NBT; ++jb) {
          const float b = sW[(jb * 16 + li) * LDW + ks * 4 + lg];      // B[k][j] = W[j][k]
          acc[jb] = SEA_MFMA(a, b, acc[jb]);
        }
      }
      float* dst = which ? sKp : sQp;
#pragma unroll
      for (int jb = 0; jb < NBT; ++jb) {
        const int col = jb * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = ib * 16 + lg * 4 + r;
          float val = fmaxf(cnorm * acc[jb][r], 0.f) + 1e-3f;
          if (col >= p.nb || row >= rows) val = 0.f;       // padded features / rows beyond T contribute nothing
          dst[row * LDP + col] = val;
        }
      }
    }
    __syncthreads();
    PSTAMP(1);   // (b) feature maps

    // ---- (c) A = tril(phi(Q) phi(K)^T) (C x C, lower-triangular blocks), row sums into sDen -------------------
    if constexpr (!STATE_ONLY) {
    for (int tile = wv; tile < RB * (RB + 1) / 2; tile += NW) {
      int ib = 0, rem = tile;
      while (rem > ib) { rem -= ib + 1; ++ib; }          // tile -> (ib, jb) with jb <= ib
      const int jb = rem;
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NBP / 4; ++ks) {
        const float a = sQp[(ib * 16 + li) * LDP + ks * 4 + lg];   // A[i][r]
        const float b = sKp[(jb * 16 + li) * LDP + ks * 4 + lg];   // B[r][j] = Kp[j][r]
        acc = SEA_MFMA(a, b, acc);
      }
      const int col = jb * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ib * 16 + lg * 4 + r;
        const float val = (col <= row) ? acc[r] : 0.f;
        sA[row * LDA + col] = val;                       // NOTE: overlays sQ, which step (b) no longer needs
        float s = val;                                   // sum over the 16 columns held by lanes li = 0..15
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
        if (li == 0) sDenP[row * DSL + jb] = s;            // one writer per (row, key block)
      }
    }
    // denominators' carry part: phi(q_i) . (ksum + eps)   (ksum = state BEFORE this chunk)
    {
      constexpr int PARTS = NTH / C;                       // threads per row
      const int row = tid % C, part = tid / C;
      const int per = (NBP + PARTS - 1) / PARTS;
      float s = 0.f;
      for (int r = part * per; r < min(p.nb, (part + 1) * per); ++r) s = fmaf(sQp[row * LDP + r], sKsum[r] + 1e-6f, s);
      sDenP[row * DSL + RB + part] = s;
    }
    __syncthreads();
    if (tid < C) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < DSL; ++i) s += sDenP[tid * DSL + i];
      sDen[tid] = s;
    }
    __syncthreads();
    }
    PSTAMP(2);   // (c) A + denominators
    // the diagonal part of the denominator also carries eps: sum_r phi(q)_r * eps is already in the carry term;
    // the intra-chunk part needs none (eps is added once to the k-sum, not per key).

    // ---- (d) O = A V + phi(Q) S, divided by the denominators; (e) S += phi(K)^T V -----------------------------
    // per owned column block: all RB row blocks of O are accumulated together (one V / S fragment feeds RB MFMAs)
#pragma unroll
    for (int a_ = 0; a_ < JB; ++a_) {
      const int jb = wv + NW * a_;
      if (jb < EB) {
        if constexpr (!STATE_ONLY) {
        f4 o[RB];
#pragma unroll
        for (int ib = 0; ib < RB; ++ib) o[ib] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb2 = 0; kb2 < RB; ++kb2) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const float b = sV[(kb2 * 16 + ks * 4 + lg) * LDV + jb * 16 + li];
#pragma unroll
            for (int ib = 0; ib < RB; ++ib) {
              if (ib >= kb2) {                                   // causal: key blocks above the diagonal are zero
                const float a = sA[(ib * 16 + li) * LDA + kb2 * 16 + ks * 4 + lg];
                o[ib] = SEA_MFMA(a, b, o[ib]);
              }
            }
          }
        }
#pragma unroll
        for (int rb = 0; rb < NBT; ++rb) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            // k-step `ks` of this product sums over state rows {rb*16 + 4g + ks}: register ks of the S tile
            const float b = S[a_][rb][ks];
#pragma unroll
            for (int ib = 0; ib < RB; ++ib) {
              const float a = sQp[(ib * 16 + li) * LDP + rb * 16 + 4 * lg + ks];
              o[ib] = SEA_MFMA(a, b, o[ib]);
            }
          }
        }
        const int col = jb * 16 + li;
#pragma unroll
        for (int ib = 0; ib < RB; ++ib) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = ib * 16 + lg * 4 + r;
            if (row < rows) ob[(int64_t)(t0 + row) * (3 * D) + col] = o[ib][r] / sDen[row];
          }
        }
        }
        // (e) state update: one V fragment feeds the NBT state tiles of this column block
#pragma unroll 4
        for (int ks = 0; ks < C / 4; ++ks) {
          const float b = sV[(ks * 4 + lg) * LDV + jb * 16 + li];           // B[k][j]
#pragma unroll
          for (int rb = 0; rb < NBT; ++rb) {
            const float a = sKp[(ks * 4 + lg) * LDP + rb * 16 + li];        // A[r][k] = Kp[k][r]
            S[a_][rb] = SEA_MFMA(a, b, S[a_][rb]);
          }
        }
      }
    }
    __syncthreads();
    PSTAMP(3);   // (d)+(e)
    // running sum of phi(k) (after every wave has used the old value in step (c))
    if (tid < NBP) {
      float s = sKsum[tid];
      for (int r = 0; r < C; ++r) s += sKp[r * LDP + tid];
      sKsum[tid] = s;
    }
    __syncthreads();
    PSTAMP(4);   // ksum
  }
  if constexpr (STATE_ONLY) {
    float* cw = p.carry + ((int64_t)nh * (p.nseg - 1) + seg) * CARRY;
#pragma unroll
    for (int a = 0; a < JB; ++a)
#pragma unroll
      for (int b = 0; b < NBT; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) cw[((a * NBT + b) * 4 + r) * NTH + tid] = S[a][b][r];
    if (tid < NBP) cw[P::ksum_at + tid] = sKsum[tid];
  } else if (p.state_out && seg == p.nseg - 1) {           // the block that walked the last rows holds the final state
    float* cw = p.state_out + (int64_t)nh * CARRY;
#pragma unroll
    for (int a = 0; a < JB; ++a)
#pragma unroll
      for (int b = 0; b < NBT; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) cw[((a * NBT + b) * 4 + r) * NTH + tid] = S[a][b][r];
    if (tid < NBP) cw[P::ksum_at + tid] = sKsum[tid];
  }
}


// ======================================================================================================
// bf16 variant (D = 64): the same algorithm on v_mfma_f32_16x16x32_bf16 -- 16x the fp32 MFMA rate.
//
// What keeps it accurate: q, k, v, pos and the projection ARE bf16 values, so the feature-map product is exact
// in the products and fp32 in the sums, as before.  Everything that is genuinely fp32 afterwards -- phi(q),
// phi(k), the masked tile A, the running state S -- enters the matrix cores SPLIT in two bf16 terms
// (x = hi + lo, hi = bf16(x), lo = bf16(x - hi): 16 significand bits), and a product of two split operands
// takes three MFMAs (hi.hi + hi.lo + lo.hi), one split against an exact bf16 operand takes two.  Relative
// error 2^-17 per term, accumulated in fp32, in front of a result that is rounded to bf16 (2^-9).
// The state S itself stays fp32 in the accumulators for the whole sequence.
//
// Layout notes (16x16x32 operand maps: A lane l = row l%16, k = 8(l/16)+j; B lane l = col l%16, same k):
//   * X^T = W . Q^T is computed transposed, so a lane holds 4 consecutive FEATURES of one row: the split
//     values leave as 8-byte row-major pieces, which is what the later A-operand reads want.
//   * the tile A is computed transposed too (A^T = phi(K) . phi(Q)^T): same reason, and its row sums (the
//     denominators) become an in-lane sum plus two cross-lane adds.
//   * products that contract over the chunk rows (A.V, phi(K)^T.V) need V and phi(K) "k-major"; both stay
//     row-major in LDS and are fetched with the transposing read ds_read_b64_tr_b16.
//   * S is, as in the fp32 kernel, the B operand of phi(Q).S straight from the accumulator registers; element j
//     of lane group g is feature 16*(2kk + j/4) + 4g + j%4, and the phi(Q) fragment is gathered in that order.
//
// The plan (Perf16Plan), the workgroup prologue, the carry image and the phases of a chunk are in sea_performer16.hpp, shared
// with the wide-head kernel below; here: the staging and the chunk walk.
// ======================================================================================================
template <typename T, int NBT, bool STATE_ONLY, bool SEQ = false, bool PAGED = false>
__global__ __launch_bounds__(512) void performer_bf16_kernel(PerfParams p) {
  using P = Perf16Plan<64, 64, NBT>;
  constexpr int D = P::D, C = P::C, E = P::E, NSET = P::NSET;
  static_assert(P::EB == P::NW, "one 16-column block of [pos | v] per wave");
  extern __shared__ __attribute__((aligned(16))) char smem_b[];
  const Perf16Lds<P> L(smem_b);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const Perf16Wg<T, D, C, SEQ, PAGED> wg(p);
  const float cnorm = powf((float)D, -0.25f);

  perf16_lds_init<T, P>(L, p.W, p.nb, tid);
  f4 S[1][NBT];
  float csum[1][4];
  perf16_state_init<P, STATE_ONLY>(p, wg.nh, wg.seg, tid, S, csum, L.sKsum);

  // a sequence that sits out this step (DecodeSession.pause / release: its counter row is negative, tb < 0) does nothing: no
  // K / V / q read, state image and output rows untouched (a paged one has read entry 0 of its table row and uses it for
  // nothing).  Block-uniform; here, at the position's first use, so that the staging above does not wait for the counter
  if constexpr (SEQ) { if (wg.tb < 0) return; }
  const Perf16Bufs B = wg.buffers(p);
  const int t_begin = wg.t_begin, t_end = wg.t_end, lead = wg.lead;
  // one 16-byte piece of each tensor per thread and chunk; prefetched one chunk ahead
  const int sr = tid >> 3, sc = tid & 7;        // staging row, 8-element column chunk
  bu4 pq, pk, pv, pp;
  auto issue_qk = [&](int t0n) {
    const int t = t0n + sr;
    const bool ok = t < t_end;
    pq = __builtin_amdgcn_raw_buffer_load_b128(B.rq, (ok && !STATE_ONLY && t >= lead) ? (int)((t * p.qs[2] + sc * 8) * 2) : PERF16_OOB, 0, 0);
    pk = __builtin_amdgcn_raw_buffer_load_b128(B.rk, ok ? (int)((t * p.ks[2] + sc * 8) * 2) : PERF16_OOB, 0, 0);
  };
  auto issue_v = [&](int t0n) {
    const int t = t0n + sr;
    const bool ok = t < t_end;
    pv = __builtin_amdgcn_raw_buffer_load_b128(B.rv, ok ? (int)((t * p.vs[2] + sc * 8) * 2) : PERF16_OOB, 0, 0);
    pp = __builtin_amdgcn_raw_buffer_load_b128(B.rp, ok ? (int)((t * p.pos_stride + sc * 8) * 2) : PERF16_OOB, 0, 0);
  };
#ifdef SEA_STAMP
  unsigned long long _tprev = __builtin_amdgcn_s_memtime();
  const unsigned long long _rstart64 = __builtin_amdgcn_s_memrealtime();
#endif
  issue_qk(t_begin);
  issue_v(t_begin);
  uint4 tril[P::RB][C / 32];
  perf16_tril_table<T, P>(tril, li, lg);

  // ---- the chunk walk, software-pipelined over THREE barriers per chunk (the first version ran a chunk's five phases one after
  // the other behind five barriers; at two waves per SIMD every phase is a dependent chain -- LDS read -> MFMA -> vector ->
  // LDS write -- that nothing else covers: ablation builds put (b) at 28 %, (c) 12 %, (d) 31 %, (e) 14 %, the flush 8 % of the
  // kernel, adding up).  Iteration j:
  //   P1  (d_j)(e_j): output products and the state update of chunk j   +   (b_{j+1}): feature maps of the NEXT chunk, into the
  //       other phi image;
  //   P2  (c_{j+1}): A tiles and partials of chunk j+1;  [pos | v] of chunk j+1 and q, k of chunk j+2 go from the prefetch
  //       registers to LDS (their old images were last read in P1), the loads of chunks j+2 / j+3 are issued;
  //   (until round 4 a third phase P3 -- denominators, 1 / row index and the k-sum of chunk j+1 on a few threads, behind its own
  //   barrier; now the first lines of (d), see perf16_denoms: TWO barriers per chunk).
  auto stage_qk = [&]() {
    *reinterpret_cast<bu4*>(L.sQ + (sc * C + P::qk_slot(sr, sc)) * 8) = pq;
    *reinterpret_cast<bu4*>(L.sK + (sc * C + P::qk_slot(sr, sc)) * 8) = pk;
  };
  auto stage_v = [&](int t0) {                               // chunk t0's [pos | v] rows; v also is the third block of the output
    const int rows = wg.rows_of(t0);
    if (!STATE_ONLY) __builtin_amdgcn_raw_buffer_store_b128(pv, B.ro, (sr < rows && t0 + sr >= lead) ? ((t0 + sr) * (3 * D) + 2 * D + sc * 8) * 2 : PERF16_OOB, 0, 0);
    *reinterpret_cast<bu4*>(L.sV + sr * E + P::vchunk(sr, sc) * 8) = pp;
    *reinterpret_cast<bu4*>(L.sV + sr * E + P::vchunk(sr, D / 8 + sc) * 8) = pv;
  };
  auto run_b = [&](int t0, int buf) { perf16_phase_b<T, P, STATE_ONLY>(L, L.set(buf), wg.rows_of(t0), p.nb, cnorm, wv, li, lg); };
  auto run_c = [&](int buf) { perf16_phase_c<T, P, STATE_ONLY>(L, L.set(buf), tid, wv, lane, li, lg); };
  auto run_de = [&](int t0, int buf) {
    perf16_phase_de<T, P, STATE_ONLY>(L, L.set(buf), B, t0, wg.rows_of(t0), wg.row_base, lead, wg.upd_of(t0), wg.want_avg, S, csum, tril,
                                      tid, wv, lane, li, lg);
  };
  if (t_begin < t_end) {
    // prologue: chunk 0 through (b), (c); chunk 1's q, k staged; loads of chunk 1 ([pos | v]) and chunk 2 (q, k) in flight
    stage_qk();
    stage_v(t_begin);
    issue_qk(t_begin + C);
    issue_v(t_begin + C);
    __syncthreads();
    run_b(t_begin, 0);
    __syncthreads();
    run_c(0);
    stage_qk();
    issue_qk(t_begin + 2 * C);
    __syncthreads();
    int buf = 0;
    for (int t0 = t_begin; t0 < t_end; t0 += C, buf ^= (NSET - 1)) {
      const bool has_next = t0 + C < t_end;                  // block-uniform
      // (measured and not taken: the two waves of a SIMD running P1's two parts in opposite order, 328 vs 306 us; (b) cut in two
      // and placed between the parts of (d), 320 vs 306 us -- DESIGN.md section 9)
      run_de(t0, buf);
      if constexpr (NSET == 1) __syncthreads();              // one image set: chunk j's must have been read
      if (has_next) run_b(t0 + C, buf ^ (NSET - 1));
      __syncthreads();
      PSTAMP(0);
      if (has_next) {
        run_c(buf ^ (NSET - 1));
        stage_v(t0 + C);
        issue_v(t0 + 2 * C);
        stage_qk();
        issue_qk(t0 + 3 * C);
      }
      __syncthreads();
      PSTAMP(1);
    }
  }
  perf16_state_finish<P, STATE_ONLY>(p, wg.nh, wg.seg, tid, li, t_end - t_begin <= C && !wg.upd_of(t_begin), S, csum, L.sKsum);
#ifdef SEA_STAMP
  if (!STATE_ONLY && threadIdx.x == 0) { const int _w = blockIdx.y * gridDim.x + blockIdx.x; if (_w < 1024) { sea_dbg_wg[2 * _w] = _rstart64; sea_dbg_wg[2 * _w + 1] = __builtin_amdgcn_s_memrealtime(); } }
#endif
}

// ---- wide heads (D = 80, 128): the same algorithm with the chunk cut to C = 32 rows so that the LDS images fit (the
// D = 64 plan scaled up is 208 KB), up to two 16-column blocks of [pos | v] per wave (E / 16 = 16 or 10 blocks over 8
// waves: a wave keeps two state tiles S; at D = 80 only waves 0 and 1 own a second block), D / 8 staging chunks per row
// on the first C * D / 8 threads, the head dimension zero-padded to whole 32-wide k-steps (D = 80: 96) in the operand
// images of the feature-map product, and a V image of 512-byte rows whose chunk swizzle spreads the eight rows of a
// transposing read over the eight 8-bank groups.  Everything else -- split operands, transposed products, transposing
// reads, the cumulative average on the matrix cores, segments, state images, and (round 4) the chunk walk pipelined over
// three barriers with two sets of phi images and results stored straight from the accumulators -- is the D = 64 kernel's.
// The 25 KB of result tiles the first version flushed one chunk later paid for the second image set (d = 128: 120 KB).
template <typename T, int D, int C, int NBT, bool STATE_ONLY, bool SEQ = false, bool PAGED = false>
__global__ __launch_bounds__(512) void performer_bf16w_kernel(PerfParams p) {
  using P = Perf16Plan<D, C, NBT>;
  constexpr int NW = P::NW, NTH = P::NTH, CPR = P::CPR, KC = P::KC, EL = P::EL, NBP = P::NBP, KF = P::KF, FP = P::FP;
  constexpr int RB = P::RB, EB = P::EB, JB = P::JB;
  constexpr int LDQ2 = P::LDQ2, LDK2 = P::LDK2, LDA = P::LDA, DSL = P::DSL, PHI = P::PHI;
  constexpr int STG = C * CPR;                           // threads that stage one 16-byte piece of each tensor
  static_assert(P::WIDE && P::NSET == 2 && C <= 32, "two phi image sets, two chunks per state-pass iteration");
  extern __shared__ __attribute__((aligned(16))) char smem_b[];
  const Perf16Lds<P> L(smem_b);                          // for the shared phases (b), (c)
  // This kernel keeps its own pointer chain, its (d)(e) and tril / vchunk lambdas: taken from the shared header (Perf16Lds,
  // perf16_phase_de, perf16_state_update) the same source compiles to another register allocation and schedule -- D = 80 output
  // forms 217 -> 170 VGPRs, D = 128 254 -> 236 -- and measured 1.5 - 4.5 % slower.  The chain is the plan's:
  static_assert(KC * NBP * 8 == P::oQ && KC * C * 8 == P::oK - P::oQ && KC * C * 8 == P::oV - P::oK && C * EL == P::oPhi - P::oV &&
                    2 * PHI == P::oA - P::oPhi && P::n16 == P::oA + 2 * C * LDA && FP == P::oDenP && C * DSL == P::oKsP - P::oDenP &&
                    NW * FP == P::oKsP2 - P::oKsP && P::oV2_bytes == 2 * (size_t)P::n16 + sizeof(float) * (P::oKsP2 + NW * FP) &&
                    P::lds_bytes == P::oV2_bytes + 2 * C * EL,
                "the pointer chain below and the plan's offsets are one layout");
  unsigned short* sW = reinterpret_cast<unsigned short*>(smem_b);   // [KC][NBP][8]  projection, k-chunked (zero padded)
  unsigned short* sQ = sW + KC * NBP * 8;                           // [KC][C][8]    (chunks >= D / 8: zero)
  unsigned short* sK = sQ + KC * C * 8;                             // [KC][C][8]
  unsigned short* sV = sK + KC * C * 8;                             // [C][EL] 512-byte rows, chunk-swizzled
  unsigned short* sPhi = sV + C * EL;                               // [2][ [C][LDQ2] x 2, [C][LDK2] x 2 ]: two chunks in flight
  unsigned short* sAh = sPhi + 2 * PHI;                             // [C][LDA]
  unsigned short* sAl = sAh + C * LDA;
  float* sKsum = reinterpret_cast<float*>(sAl + C * LDA);           // [FP]
  float* sDenP = sKsum + FP;                                        // [C][DSL]
  float* sKsP = sDenP + C * DSL;                                    // [NW][FP]   per-wave k-sum increments
  float* sKsP2 = sKsP + NW * FP;                                    // [NW][FP]   (state pass: the second chunk of an iteration)
  unsigned short* sV2 = reinterpret_cast<unsigned short*>(sKsP2 + NW * FP);   // [C][EL] (state pass: the second chunk's [pos | v])

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const Perf16Wg<T, D, C, SEQ, PAGED> wg(p);
  const int nh = wg.nh, seg = wg.seg, tb = wg.tb, lead = wg.lead, row_base = wg.row_base, t_begin = wg.t_begin, t_end = wg.t_end;
  const float cnorm = powf((float)D, -0.25f);

  // projection (its values are bf16-exact: the reference casts the buffer to the data dtype), zero padded rows
  for (int i = tid; i < KC * NBP * 8; i += NTH) {
    const int j = i & 7, f = (i >> 3) % NBP, kc = (i >> 3) / NBP;
    sW[i] = (f < p.nb && kc < CPR) ? S16<T>::bits(p.W[f * D + kc * 8 + j]) : (unsigned short)0;
  }
  if constexpr (KC > CPR)                                  // padded k-chunks of the q / k images: zero, never written again
    for (int i = tid; i < (KC - CPR) * C * 8; i += NTH) sQ[CPR * C * 8 + i] = sK[CPR * C * 8 + i] = 0;
  // phi and A images: padded features / upper-triangular tiles are written once (zero) and never again
  for (int i = tid; i < 2 * PHI + 2 * C * LDA; i += NTH) sPhi[i] = 0;
  for (int i = tid; i < C * DSL; i += NTH) sDenP[i] = 0.f;   // slots of key blocks above the diagonal stay zero

  constexpr int CARRY = (int)P::carry_floats;
  f4 S[JB][NBT];
  float csum[JB][4];
  perf16_state_init<P, STATE_ONLY>(p, nh, seg, tid, S, csum, sKsum);

  // a sequence that sits out this step (DecodeSession.pause / release: its counter row is negative, tb < 0) does nothing: no
  // K / V / q read, state image and output rows untouched (a paged one has read entry 0 of its table row and uses it for
  // nothing).  Block-uniform; here, at the position's first use, so that the staging above does not wait for the counter
  if constexpr (SEQ) { if (tb < 0) return; }
  // one 16-byte piece of each tensor per thread and chunk; q, k prefetched two chunks ahead, [pos | v] one
  // (D = 80: the LAST C * D / 8 = 320 threads stage -- waves 0 and 1 carry a second column block in (d)(e))
  const bool stager = tid >= NTH - STG;
  const int stid = stager ? tid - (NTH - STG) : 0;
  const int sr = stid / CPR, sc = stid - sr * CPR;   // staging row, 8-element column chunk
  // All global traffic goes through buffer instructions with hardware range checking: a row beyond T reads zeros /
  // drops its store WITHOUT a branch.  (Branches around loads and stores make the compiler's vmcnt bookkeeping
  // pessimistic: the wait for the prefetched chunk then also waits for every output store of the previous one.)
  constexpr unsigned OOB = 0x7FFFFF00u;
  const Perf16Bufs B = wg.buffers(p);
  const __amdgpu_buffer_rsrc_t rq = B.rq, rk = B.rk, rv = B.rv, rp = B.rp, ro = B.ro, rg = B.rg;
  const bool want_avg = wg.want_avg;
  // two sets of prefetch registers: every load has two chunk times between issue and use (d = 128: 202.7 -> 199.9 us; halves the lag
  // of the last segment's workgroups in the pipelined walk)
  struct Pre { bu4 q, k, v, p; };
  Pre pa, pn;
  auto issue_qk = [&](int t0n, Pre& r) {
    const int t = t0n + sr;
    const bool ok = t < t_end && stager;
    r.q = __builtin_amdgcn_raw_buffer_load_b128(rq, (ok && !STATE_ONLY && t >= lead) ? (int)((t * p.qs[2] + sc * 8) * 2) : (int)OOB, 0, 0);
    r.k = __builtin_amdgcn_raw_buffer_load_b128(rk, ok ? (int)((t * p.ks[2] + sc * 8) * 2) : (int)OOB, 0, 0);
  };
  auto issue_v = [&](int t0n, Pre& r) {
    const int t = t0n + sr;
    const bool ok = t < t_end && stager;
    r.v = __builtin_amdgcn_raw_buffer_load_b128(rv, ok ? (int)((t * p.vs[2] + sc * 8) * 2) : (int)OOB, 0, 0);
    r.p = __builtin_amdgcn_raw_buffer_load_b128(rp, ok ? (int)((t * p.pos_stride + sc * 8) * 2) : (int)OOB, 0, 0);
  };
  issue_qk(t_begin, pa);
  issue_v(t_begin, pa);
  // swizzled chunk position inside a row of the V image (conflict-free transposing reads):
  // 512-byte rows (32 chunks): rows {r..r+3, r+8..r+11} of one transposing read get the eight values of
  // (row & 3) | (bit 3 of row) << 2 XOR-ed into bits 1..3 of the chunk index -> eight disjoint 8-bank groups
  auto vchunk = [](int row, int ch) { return ch ^ ((((row & 3) | (((row >> 3) & 1) << 2))) << 1); };

  // cumulative average of v (step K's input) on the waves that own the v columns: prefix sum over the chunk rows =
  // tril(ones) . V on the matrix cores (1.0 and v are exact in bf16, fp32 accumulation) + the running column sum
  auto tril_frag = [&](int ib, int ks) {
    unsigned short o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (ks * 32 + lg * 8 + j <= ib * 16 + li) ? S16<T>::ONE : (unsigned short)0;
    const unsigned short (&o0)[4] = *reinterpret_cast<const unsigned short (*)[4]>(&o[0]);
    const unsigned short (&o1)[4] = *reinterpret_cast<const unsigned short (*)[4]>(&o[4]);
    return cat8(pack4(o0), pack4(o1));
  };

  uint4 tril[RB][C / 32];                                  // loop-invariant operands of the prefix-sum product
#pragma unroll
  for (int ib = 0; ib < RB; ++ib)
#pragma unroll
    for (int ks = 0; ks < C / 32; ++ks) tril[ib][ks] = tril_frag(ib, ks);

  auto write_image = [&](float* cw) { perf16_carry_write<P>(cw, tid, li, S, csum, sKsum); };

  // ---- the chunk walk: the D = 64 kernel's three-barrier pipeline (P1 = (d)(e) of chunk j + (b) of chunk j+1 into the other
  // image set; P2 = (c) of chunk j+1, staging of [pos | v] of chunk j+1 and q, k of chunk j+2, loads issued; P3 = denominators
  // and k-sum of chunk j+1) ----------------------------------------------------------------------------------------------------
  auto rows_of = [&](int t0) { return min(C, t_end - t0); };
  auto upd_of = [&](int t0) { return !(p.aligned && rows_of(t0) < C); };   // an open last chunk leaves the state at the boundary
  auto stage_qk = [&](const Pre& r) {
    // row slot XOR chunk: the 16 lanes of a b128 store (one row x 16 chunks at D = 128; chunk images are 512 B = 0 mod 64
    // banks apart) land in 16 different 4-bank groups instead of one; the reads of (b) permute inside their 16-row runs
    if (stager) {
      *reinterpret_cast<bu4*>(sQ + (sc * C + (sr ^ sc)) * 8) = r.q;
      *reinterpret_cast<bu4*>(sK + (sc * C + (sr ^ sc)) * 8) = r.k;
    }
  };
  auto stage_v = [&](int t0, const Pre& r) {                 // chunk t0's [pos | v] rows; v also is the third block of the output
    const int rows = rows_of(t0);
    if (!STATE_ONLY) __builtin_amdgcn_raw_buffer_store_b128(r.v, ro, (stager && sr < rows && t0 + sr >= lead) ? ((t0 + sr) * (3 * D) + 2 * D + sc * 8) * 2 : (int)OOB, 0, 0);
    if (stager) {
      *reinterpret_cast<bu4*>(sV + sr * EL + vchunk(sr, sc) * 8) = r.p;
      *reinterpret_cast<bu4*>(sV + sr * EL + vchunk(sr, CPR + sc) * 8) = r.v;
    }
  };
  // ---- (b) feature maps, transposed: X^T[f][t] = sum_d W[f][d] x[t][d]; wave = (Q | K, row block, part of the feature blocks) ----
  auto phase_b = [&](int rows, unsigned short* set) { perf16_phase_b<T, P, STATE_ONLY>(L, set, rows, p.nb, cnorm, wv, li, lg); };
  // ---- (c) A^T tiles (lower triangle), denominator and k-sum partials ------------------------------------
  auto phase_c = [&](const unsigned short* set) { perf16_phase_c<T, P, STATE_ONLY>(L, set, tid, wv, lane, li, lg); };
  // ---- (d) O = A V + phi(Q) S over this wave's column blocks; (e) S += phi(K)^T V ------------------------------
  auto phase_de = [&](int t0, int rows, bool upd, const unsigned short* set) {
    const unsigned short* sQh = set;
    const unsigned short* sQl = sQh + C * LDQ2;
    const unsigned short* sKh = sQl + C * LDQ2;
    const unsigned short* sKl = sKh + C * LDK2;
    // what a phase of its own (and its barrier) did in the first version: the k-sum takes this chunk's increments (the partials
    // of (c) read it before, the next chunk's (c) runs behind the next barrier), and every lane sums the denominator partials of
    // ITS rows -- the same additions in the same order in every lane that holds the row
    if (tid < FP) {
      float s = sKsum[tid];
#pragma unroll
      for (int i = 0; i < NW; ++i) s += sKsP[i * FP + tid];       // fixed order: bitwise reproducible
      if (upd) sKsum[tid] = s;
    }
    // (a lane sums ONE row -- lane group g the rows of block g % RB -- and the reciprocals travel by lane permutes: four rows and
    // eight divisions per lane made the phase VALU-bound, 2.5 % slower than the barrier it replaces at 256 workgroups)
    float dn[RB], ri1 = 0.f;
    if constexpr (!STATE_ONLY) {
      const int myrow = (lg % RB) * 16 + li;
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < DSL; ++i) s += sDenP[myrow * DSL + i];
      const float d1 = 1.0f / s;
      ri1 = 1.0f / (float)(row_base + t0 + myrow + 1);
#pragma unroll
      for (int ib = 0; ib < RB; ++ib) dn[ib] = __shfl(d1, ib * 16 + li);
    }
#pragma unroll
    for (int jq = 0; jq < JB; ++jq) {
      const int jb = wv + jq * NW, e0 = jb * 16;
      if (EB % NW != 0 && jb >= EB) break;                 // wave-uniform: no such column block
      // V fragments (k = chunk row): rows 32ks + 8lg + {0..3 | 4..7}, columns e0 .. e0+15
      uint4 vf[C / 32];
      {
        const int q = li >> 2, pp_ = li & 3;
#pragma unroll
        for (int ks = 0; ks < C / 32; ++ks) {
          const int r0 = ks * 32 + lg * 8;
          const uint2 a = lds_tr(sV + (r0 + q) * EL + vchunk(r0 + q, 2 * jb + (pp_ >> 1)) * 8 + 4 * (pp_ & 1));
          const uint2 b = lds_tr(sV + (r0 + 4 + q) * EL + vchunk(r0 + 4 + q, 2 * jb + (pp_ >> 1)) * 8 + 4 * (pp_ & 1));
          vf[ks] = cat8(a, b);
        }
      }
      if constexpr (STATE_ONLY) {
        if (want_avg && jb >= EB / 2) {                    // column total of the chunk = the last row's prefix
          f4 cum = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks <= (RB - 1) / 2; ++ks) cum = S16<T>::mfma(vf[ks], tril[RB - 1][ks], cum);
#pragma unroll
          for (int r = 0; r < 4; ++r) csum[jq][r] += __shfl(cum[r], (lane & 48) | 15);
        }
      } else {
      f4 o[RB];
#pragma unroll
      for (int ib = 0; ib < RB; ++ib) o[ib] = f4{0.f, 0.f, 0.f, 0.f};
      // Operands SWAPPED as in the D = 64 kernel (O^T = V^T A^T + S^T phi(Q)^T; the A and B fragment layouts mirror each other):
      // the accumulator of query block ib holds, per lane, row ib*16 + li and the four consecutive columns e0 + 4 lg + r.
      // A V: key k-step ks covers key blocks 2ks, 2ks+1; query block ib needs k-steps <= ib/2
#pragma unroll
      for (int ib = 0; ib < RB; ++ib) {
#pragma unroll
        for (int ks = 0; ks <= ib / 2; ++ks) {
          const uint4 ah = *reinterpret_cast<const uint4*>(sAh + (ib * 16 + li) * LDA + ks * 32 + lg * 8);
          const uint4 al = *reinterpret_cast<const uint4*>(sAl + (ib * 16 + li) * LDA + ks * 32 + lg * 8);
          o[ib] = S16<T>::mfma(vf[ks], ah, o[ib]);
          o[ib] = S16<T>::mfma(vf[ks], al, o[ib]);
        }
      }
      // phi(Q) S: the state tiles, split; k-step kk pairs feature blocks 2kk and 2kk+1
#pragma unroll
      for (int kk = 0; kk < KF; ++kk) {
        unsigned short h0[4], h1[4], l0[4], l1[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          split16<T>(S[jq][2 * kk][r], h0[r], l0[r]);
          if (2 * kk + 1 < NBT) split16<T>(S[jq][(2 * kk + 1 < NBT) ? 2 * kk + 1 : 0][r], h1[r], l1[r]);
          else h1[r] = l1[r] = 0;
        }
        const uint4 bh = cat8(pack4(h0), pack4(h1)), bl = cat8(pack4(l0), pack4(l1));
#pragma unroll
        for (int ib = 0; ib < RB; ++ib) {
          const uint4 ah = *reinterpret_cast<const uint4*>(sQh + (ib * 16 + li) * LDQ2 + kk * 32 + lg * 8);
          const uint4 al = *reinterpret_cast<const uint4*>(sQl + (ib * 16 + li) * LDQ2 + kk * 32 + lg * 8);
          o[ib] = S16<T>::mfma(bh, ah, o[ib]);
          o[ib] = S16<T>::mfma(bl, ah, o[ib]);
          o[ib] = S16<T>::mfma(bh, al, o[ib]);
        }
      }
      const int col = e0 + 4 * lg;
#pragma unroll
      for (int ib = 0; ib < RB; ++ib) {
        const int row = ib * 16 + li;
        unsigned short o4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) o4[r] = S16<T>::bits(o[ib][r] * dn[ib]);
        const uint2 w2 = pack4(o4);
        __builtin_amdgcn_raw_buffer_store_b64(bu2{w2.x, w2.y}, ro, (row < rows && t0 + row >= lead) ? ((t0 + row) * (3 * D) + col) * 2 : (int)OOB, 0, 0);
      }
      if (want_avg && jb >= EB / 2) {                      // wave-uniform: this wave's 16 columns are v features
        f4 cum[RB];
#pragma unroll
        for (int ib = 0; ib < RB; ++ib) {
          cum[ib] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks <= ib / 2; ++ks) cum[ib] = S16<T>::mfma(vf[ks], tril[ib][ks], cum[ib]);
        }
        const int gcol = col - D;
#pragma unroll
        for (int ib = 0; ib < RB; ++ib) {
          const int row = ib * 16 + li;
          const float ri = __shfl(ri1, ib * 16 + li);
          unsigned short g4[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) g4[r] = S16<T>::bits((cum[ib][r] + csum[jq][r]) * ri);
          const uint2 w2 = pack4(g4);
          __builtin_amdgcn_raw_buffer_store_b64(bu2{w2.x, w2.y}, rg, (row < rows && t0 + row >= lead) ? ((t0 + row) * D + gcol) * 2 : (int)OOB, 0, 0);
        }
        if (upd) {                                         // column totals of the chunk = its last row's prefix (lane li = 15)
#pragma unroll
          for (int r = 0; r < 4; ++r) csum[jq][r] += __shfl(cum[RB - 1][r], (lane & 48) | 15);
        }
      }
      }
      // (e) S[f][e] += sum_s phi(k_s)[f] V[s][e]: A operand = phi(K)^T by transposing reads of the row-major images
      if (upd) {
        const int q = li >> 2, pp_ = li & 3;
#pragma unroll
        for (int rb = 0; rb < NBT; ++rb) {
#pragma unroll
          for (int ks = 0; ks < C / 32; ++ks) {
            const int r0 = ks * 32 + lg * 8;
            const int co = (rb >> 1) * 32 + 8 * pp_ + (rb & 1) * 4;      // positions of features 16rb + 4p .. +3
            const uint4 kh = cat8(lds_tr(sKh + (r0 + q) * LDK2 + co), lds_tr(sKh + (r0 + 4 + q) * LDK2 + co));
            const uint4 kl = cat8(lds_tr(sKl + (r0 + q) * LDK2 + co), lds_tr(sKl + (r0 + 4 + q) * LDK2 + co));
            S[jq][rb] = S16<T>::mfma(kh, vf[ks], S[jq][rb]);
            S[jq][rb] = S16<T>::mfma(kl, vf[ks], S[jq][rb]);
          }
        }
      }
    }
  };
  // ---- pass 1 (STATE_ONLY) walks TWO chunks per iteration on three barriers (round 5, late) --------------------------------------
  // The state pass needs phi(K) and S += phi(K)^T [pos | v] only: no causal structure, nothing to store per row.  Walked like
  // the output pass it spent its time between barriers with half the waves idle ((b): the four "K" waves; stamps: 1.65 us per
  // 32-row chunk at d = 80 on four barriers, 2.7 us at d = 128 on two).  Here the four "Q" waves of (b) take the NEXT chunk's k
  // rows (staged where q goes, phi images into the second image set), the k-sum partials are produced beside the state
  // update and folded in one barrier later, and (e) runs for both chunks back to back.  Same operand placement and k order per
  // chunk as before: the state tiles S are bit for bit the output pass's; the k-sum's partials are summed per chunk in the
  // same fixed order.
  if constexpr (STATE_ONLY) {
    auto stage_k_to = [&](unsigned short* dst, const bu4& r) {
      if (stager) *reinterpret_cast<bu4*>(dst + (sc * C + (sr ^ sc)) * 8) = r;
    };
    auto stage_v_to = [&](unsigned short* dst, const bu4& rp_, const bu4& rv_) {
      if (stager) {
        *reinterpret_cast<bu4*>(dst + sr * EL + vchunk(sr, sc) * 8) = rp_;
        *reinterpret_cast<bu4*>(dst + sr * EL + vchunk(sr, CPR + sc) * 8) = rv_;
      }
    };
    auto load_k = [&](int t0n) {
      const int t = t0n + sr;
      return __builtin_amdgcn_raw_buffer_load_b128(rk, (t < t_end && stager) ? (int)((t * p.ks[2] + sc * 8) * 2) : (int)OOB, 0, 0);
    };
    // phi(K) of one chunk by HALF the workgroup (the waves whose `which` selects it): src = staged k rows, dh = hi image
    auto phase_bk = [&](int rows, const unsigned short* src, unsigned short* dh) { perf16_feature_map<T, P>(src, L.sW, dh, P::LDK2, rows, p.nb, cnorm, wv, li, lg); };
    // per-wave k-sum increments of one chunk (phase (c)'s code) into `dst` [NW][FP]
    auto ksum_partial = [&](const unsigned short* sKh, float* dst) { perf16_ksum_partial<T, P>(sKh, dst, wv, lane); };
    auto ksum_fold = [&](const float* src) { perf16_ksum_fold<P>(sKsum, src, tid, true); };
    // column totals of v and S += phi(K)^T [pos | v] for one chunk: phase (d)(e)'s STATE_ONLY code
    auto phase_e = [&](const unsigned short* sVi, const unsigned short* sKh) {
      const unsigned short* sKl = sKh + C * LDK2;
      const int q = li >> 2, pp_ = li & 3;
      // V fragments of BOTH column blocks of the wave first: a phi(K) fragment, which depends on (feature block, k-step) only, is
      // then read ONCE and feeds both blocks' state tiles (the output pass's loop reads it per block: 40 transposing reads per
      // chunk and wave at d = 128, all eight waves reading the same 12 KB of images -- the phase is bound by the LDS array)
      uint4 vf[JB][C / 32];
      bool has[JB];
#pragma unroll
      for (int jq = 0; jq < JB; ++jq) {
        const int jb = wv + jq * NW;
        has[jq] = !(EB % NW != 0 && jb >= EB);               // (wave-uniform) no such column block
        const int jbc = has[jq] ? jb : wv;
#pragma unroll
        for (int ks = 0; ks < C / 32; ++ks) {
          const int r0 = ks * 32 + lg * 8;
          const uint2 a = lds_tr(sVi + (r0 + q) * EL + vchunk(r0 + q, 2 * jbc + (pp_ >> 1)) * 8 + 4 * (pp_ & 1));
          const uint2 b = lds_tr(sVi + (r0 + 4 + q) * EL + vchunk(r0 + 4 + q, 2 * jbc + (pp_ >> 1)) * 8 + 4 * (pp_ & 1));
          vf[jq][ks] = cat8(a, b);
        }
        if (has[jq] && want_avg && jb >= EB / 2) {
          f4 cum = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks <= (RB - 1) / 2; ++ks) cum = S16<T>::mfma(vf[jq][ks], tril[RB - 1][ks], cum);
#pragma unroll
          for (int r = 0; r < 4; ++r) csum[jq][r] += __shfl(cum[r], (lane & 48) | 15);
        }
      }
#pragma unroll
      for (int rb = 0; rb < NBT; ++rb) {
#pragma unroll
        for (int ks = 0; ks < C / 32; ++ks) {
          const int r0 = ks * 32 + lg * 8;
          const int co = (rb >> 1) * 32 + 8 * pp_ + (rb & 1) * 4;
          const uint4 kh = cat8(lds_tr(sKh + (r0 + q) * LDK2 + co), lds_tr(sKh + (r0 + 4 + q) * LDK2 + co));
          const uint4 kl = cat8(lds_tr(sKl + (r0 + q) * LDK2 + co), lds_tr(sKl + (r0 + 4 + q) * LDK2 + co));
#pragma unroll
          for (int jq = 0; jq < JB; ++jq) {
            if (has[jq]) {                                   // per tile: hi then lo, k-steps ascending -- the output pass's order
              S[jq][rb] = S16<T>::mfma(kh, vf[jq][ks], S[jq][rb]);
              S[jq][rb] = S16<T>::mfma(kl, vf[jq][ks], S[jq][rb]);
            }
          }
        }
      }
    };
    unsigned short* kA = sPhi + 2 * C * LDQ2;                // K images of the two sets
    unsigned short* kB = sPhi + PHI + 2 * C * LDQ2;
    // prefetch registers: pa = chunk A (k in .k, [pos | v] in .p / .v), pn = chunk B; the loads of the next iteration leave
    // right after this iteration's registers went to LDS
    pa.k = load_k(t_begin);  issue_v(t_begin, pa);            // (issue_qk / issue_v of the prologue above already asked for
    pn.k = load_k(t_begin + C);  issue_v(t_begin + C, pn);    //  chunk A: the duplicates are dropped by the compiler or hit L1)
    bool pending = false;                                    // k-sum partials of the previous iteration not folded yet
    for (int t0 = t_begin; t0 < t_end; t0 += 2 * C) {
      const bool two = t0 + C < t_end;                       // (block-uniform) the last iteration may hold one chunk
      stage_k_to(sK, pa.k);  stage_v_to(sV, pa.p, pa.v);
      stage_k_to(sQ, pn.k);  stage_v_to(sV2, pn.p, pn.v);
      pa.k = load_k(t0 + 2 * C);  issue_v(t0 + 2 * C, pa);
      pn.k = load_k(t0 + 3 * C);  issue_v(t0 + 3 * C, pn);
      if (pending) { ksum_fold(sKsP); }
      __syncthreads();                                       // staged rows visible; the fold above has read sKsP
      if (pending) { ksum_fold(sKsP2); }                     // (second chunk of the previous iteration: after the first, same order)
      if (wv >= NW / 2) phase_bk(rows_of(t0), sK, kA);
      else if (two) phase_bk(rows_of(t0 + C), sQ, kB);
      __syncthreads();                                       // phi(K) images visible
      ksum_partial(kA, sKsP);
      if (two) ksum_partial(kB, sKsP2);
      else if (lane < FP / 4) *reinterpret_cast<float4*>(sKsP2 + wv * FP + lane * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
      phase_e(sV, kA);
      if (two) phase_e(sV2, kB);
      pending = true;
      __syncthreads();                                       // images, staging buffers and partials are free / complete
    }
    if (pending) { ksum_fold(sKsP); }
    __syncthreads();
    if (pending) { ksum_fold(sKsP2); }
    __syncthreads();
    write_image(p.carry + ((int64_t)nh * (p.nseg - 1) + seg) * CARRY);
    return;
  }
  // D = 80 keeps the phases one after the other (four barriers): pipelined, the median workgroup is 7 % faster (105 vs 113.6 us on
  // 1 x 32 x 8192) but the workgroups of the LAST segment run 10 us behind (every chunk's P2 is longer; not a cold-cache effect: a
  // warming walk changes nothing), and the launch ends later (128.5 vs 121.9 us; two-chunk prefetch: 5 us behind) -- DESIGN.md section 9
  constexpr bool PIPE = D != 80;
#ifdef SEA_STAMP
  unsigned long long _tacc[4] = {0, 0, 0, 0};
  unsigned long long _tprev = __builtin_amdgcn_s_memtime();
  const unsigned long long _tstart = _tprev, _rstart = __builtin_amdgcn_s_memrealtime();
#endif
  if constexpr (!PIPE) {
    for (int t0 = t_begin; t0 < t_end; t0 += C) {
      stage_qk(pa);
      stage_v(t0, pa);
      issue_qk(t0 + C, pa);
      issue_v(t0 + C, pa);
      __syncthreads();
      WSTAMP(0);
      phase_b(rows_of(t0), sPhi);
      __syncthreads();
      WSTAMP(1);
      phase_c(sPhi);
      __syncthreads();
      WSTAMP(2);
      phase_de(t0, rows_of(t0), upd_of(t0), sPhi);
      __syncthreads();
      WSTAMP(3);
    }
  } else
  if (t_begin < t_end) {
    // prologue: chunk 0 through (b), (c); chunk 1's q, k staged; in flight: [pos | v] of chunks 1 (set A) and 2 (set B), q, k of
    // chunks 2 (B) and 3 (A)
    stage_qk(pa);
    stage_v(t_begin, pa);
    issue_qk(t_begin + C, pa);
    issue_v(t_begin + C, pa);
    issue_qk(t_begin + 2 * C, pn);
    issue_v(t_begin + 2 * C, pn);
    __syncthreads();
    phase_b(rows_of(t_begin), sPhi);
    __syncthreads();
    phase_c(sPhi);
    stage_qk(pa);
    issue_qk(t_begin + 3 * C, pa);
    __syncthreads();
    // iteration j: [pos | v] of chunk j+1 leaves set `rv_` (refilled with chunk j+3), q, k of chunk j+2 leave set `rqk_` (refilled
    // with chunk j+4); the sets swap roles every iteration, so the walk is unrolled by two
    auto iter = [&](int t0, int buf, Pre& rv_, Pre& rqk_) {
      const bool has_next = t0 + C < t_end;                  // block-uniform
      phase_de(t0, rows_of(t0), upd_of(t0), sPhi + buf * PHI);
      WSTAMP(0);
      if (has_next) phase_b(rows_of(t0 + C), sPhi + (buf ^ 1) * PHI);
      __syncthreads();
      WSTAMP(1);
      if (has_next) {
        phase_c(sPhi + (buf ^ 1) * PHI);
        stage_v(t0 + C, rv_);
        issue_v(t0 + 3 * C, rv_);
        stage_qk(rqk_);
        issue_qk(t0 + 4 * C, rqk_);
      }
      __syncthreads();
      WSTAMP(2);
    };
    for (int t0 = t_begin; t0 < t_end; t0 += 2 * C) {
      iter(t0, 0, pa, pn);
      if (t0 + C < t_end) iter(t0 + C, 1, pn, pa);
    }
  }
  WSTAMP_FLUSH();
  if constexpr (STATE_ONLY) {
    write_image(p.carry + ((int64_t)nh * (p.nseg - 1) + seg) * CARRY);
  } else {
    // the block that walked the last rows holds the final state (aligned step: the state at the last chunk boundary); a step that
    // closed no chunk and updates the image in place has nothing to write (see the D = 64 kernel)
    const bool unchanged = p.aligned && p.state_in == p.state_out && t_end - t_begin <= C && !upd_of(t_begin);
    if (p.state_out && seg == p.nseg - 1 && !unchanged) write_image(p.state_out + (int64_t)nh * CARRY);
  }
}

}  // namespace sea

using namespace sea;

// Both passes of one kernel form: pass 1 (STATE_ONLY) on the first nseg-1 segments, pass 2 on all nseg (see PerfParams).
// Every form runs 512-thread workgroups.  SEQ_PASS: OUT_PASS with a position per sequence (t_base_stride > 0, one segment);
// PAGED_PASS: SEQ_PASS over a page pool (p.table; null: the form has none).
template <void (*STATE_PASS)(PerfParams), void (*OUT_PASS)(PerfParams), void (*SEQ_PASS)(PerfParams),
          void (*PAGED_PASS)(PerfParams), int C, size_t LDS>
static int launch_perf(const PerfParams& p, hipStream_t s) {
  static_assert(LDS <= 160 * 1024, "LDS budget");
  static DevOnce once;              // one per template instantiation and device; the attribute call is a slow driver round trip
  if (LDS > 64 * 1024 && once.first()) {
    SEA_MAX_LDS(STATE_PASS, LDS);
    SEA_MAX_LDS(OUT_PASS, LDS);
    SEA_MAX_LDS(SEQ_PASS, LDS);
    if constexpr (PAGED_PASS != nullptr) SEA_MAX_LDS(PAGED_PASS, LDS);
  }
  if (p.seg_len % C != 0) return SEA_EINVAL;
  if (p.table) {
    if constexpr (PAGED_PASS == nullptr) return SEA_EUNSUPPORTED;
    else {
      if (p.nseg != 1 || p.t_base_stride <= 0) return SEA_EINVAL;
      hipLaunchKernelGGL(PAGED_PASS, dim3((unsigned)(p.N * p.H)), dim3(512), LDS, s, p);
      return SEA_OK;
    }
  }
  if (p.t_base_stride > 0) {
    if (p.nseg != 1) return SEA_EINVAL;
    hipLaunchKernelGGL(SEQ_PASS, dim3((unsigned)(p.N * p.H)), dim3(512), LDS, s, p);
    return SEA_OK;
  }
  if (p.nseg > 1)
    hipLaunchKernelGGL(STATE_PASS, dim3((unsigned)(p.N * p.H), (unsigned)(p.nseg - 1)), dim3(512), LDS, s, p);
  hipLaunchKernelGGL(OUT_PASS, dim3((unsigned)(p.N * p.H), (unsigned)p.nseg), dim3(512), LDS, s, p);
  return SEA_OK;
}

// A kernel form: the launch, its chunk rows, the size of its carry / state image, and whether it is one of the 16-bit
// MFMA kernels, which alone have the chunk-aligned step and the cumulative average (avg_out).
struct PerfForm {
  int (*launch)(const PerfParams&, hipStream_t) = nullptr;   // null: no form for this shape
  int C = 0;
  int64_t carry_floats = 0;       // per (n, h, segment)
  bool mfma16 = false;
};

// Every form's LDS bytes and carry floats come from its plan (PerfF32Plan / Perf16Plan), which the kernel carves its images from.
template <int D, int NBT, int C>
static PerfForm perf_f32_form() {
  using P = PerfF32Plan<D, NBT, C>;
  return {launch_perf<performer_kernel<D, NBT, C, true>, performer_kernel<D, NBT, C, false>, performer_kernel<D, NBT, C, false>,
                      nullptr, C, P::lds_bytes>, C, P::carry_floats, false};
}

// 16-bit kernel, D = 64
template <typename T, int NBT>
static PerfForm perf_bf16_form() {
  using P = Perf16Plan<64, 64, NBT>;
  static_assert(P::lds_bytes > 64 * 1024, "the attribute is set above 64 KB");
  return {launch_perf<performer_bf16_kernel<T, NBT, true>, performer_bf16_kernel<T, NBT, false>,
                      performer_bf16_kernel<T, NBT, false, true>, performer_bf16_kernel<T, NBT, false, true, true>, P::C,
                      P::lds_bytes>, P::C, P::carry_floats, true};
}

// the wide-head form of the 16-bit kernel (d = 80 / 128: 32-row chunks, up to two column blocks per wave)
template <typename T, int D, int NBT>
static PerfForm perf_bf16w_form() {
  using P = Perf16Plan<D, 32, NBT>;
  static_assert(P::lds_bytes > 64 * 1024, "the attribute is set above 64 KB");
  return {launch_perf<performer_bf16w_kernel<T, D, 32, NBT, true>, performer_bf16w_kernel<T, D, 32, NBT, false>,
                      performer_bf16w_kernel<T, D, 32, NBT, false, true>, performer_bf16w_kernel<T, D, 32, NBT, false, true, true>,
                      P::C, P::lds_bytes>, P::C, P::carry_floats, true};
}

template <typename T>
static PerfForm perf_form16(int64_t D, int64_t nbt) {
  if (D == 64 && nbt <= 3) return perf_bf16_form<T, 3>();
  if (D == 64 && nbt <= 5) return perf_bf16_form<T, 5>();
  if (D == 80 && nbt <= 3) return perf_bf16w_form<T, 80, 3>();
  if (D == 80 && nbt <= 5) return perf_bf16w_form<T, 80, 5>();
  if (D == 128 && nbt <= 5) return perf_bf16w_form<T, 128, 5>();
  return {};
}

// The one table of kernel forms: 16-bit data takes the split-operand 16-bit MFMA kernels, fp32 data the fp32-MFMA kernel.
static PerfForm perf_form(int dtype, int64_t D, int64_t nb) {
  if (D <= 0 || nb <= 0) return {};
  const int64_t nbt = (nb + 15) / 16;
  if (dtype == SEA_F16) return perf_form16<__half>(D, nbt);
  if (dtype == SEA_BF16) return perf_form16<__hip_bfloat16>(D, nbt);
  if (dtype != SEA_F32) return {};
  if (D == 64 && nbt <= 3) return perf_f32_form<64, 3, 64>();
  if (D == 64 && nbt <= 5) return perf_f32_form<64, 5, 64>();
  if (D == 80 && nbt <= 3) return perf_f32_form<80, 3, 64>();
  if (D == 80 && nbt <= 5) return perf_f32_form<80, 5, 32>();
  if (D == 128 && nbt <= 5) return perf_f32_form<128, 5, 32>();
  return {};
}

#ifdef SEA_STAMP
extern "C" int sea_debug_perf_wg(unsigned long long* host2048) {
  (void)hipMemcpyFromSymbol(host2048, HIP_SYMBOL(sea_dbg_wg), sizeof(unsigned long long) * 2048);
  return 0;
}
extern "C" int sea_debug_perf_stamps(unsigned long long* host8) {
  (void)hipMemcpyFromSymbol(host8, HIP_SYMBOL(sea_dbg_perf), sizeof(unsigned long long) * 16);
  unsigned long long z[16] = {0};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(sea_dbg_perf), z, sizeof(z));
  return 0;
}
#endif

extern "C" int64_t sea_performer_chunk_rows(int64_t D, int64_t nb, int dtype) {
  const PerfForm f = perf_form(dtype, D, nb);
  return f.mfma16 ? f.C : 0;
}

// rows per segment: whole 64-row chunks (a multiple of every kernel's chunk size), segments as even as possible
static int64_t perf_seg_len(int64_t T, int64_t nseg) {
  const int64_t chunks = (T + 63) / 64;
  return ((chunks + nseg - 1) / nseg) * 64;
}

// avg_out comes from the 16-bit MFMA kernels only (16-bit data, d = 64, 80 or 128, up to 80 features)
extern "C" int sea_performer_avg_supported(int64_t D, int64_t nb, int dtype) { return perf_form(dtype, D, nb).mfma16; }

extern "C" int sea_performer_plan(int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb, int dtype,
                                  int64_t* n_segments, int64_t* workspace_bytes) {
  const char* nm = "sea_performer_plan";
  SEA_REQUIRE(n_segments && workspace_bytes, SEA_EINVAL, "%s: null pointer", nm);
  SEA_REQUIRE(N > 0 && H > 0 && T > 0 && D > 0 && nb > 0, SEA_EINVAL, "%s: bad shape", nm);
  const int64_t cf = perf_form(dtype, D, nb).carry_floats;
  SEA_REQUIRE(cf > 0, SEA_EUNSUPPORTED, "%s: unsupported head size D=%lld / feature count nb=%lld", nm, (long long)D, (long long)nb);
  // One workgroup walks one (n, h) pair's rows in order; with fewer pairs than compute units the rows are cut into
  // segments (pass 1 re-does the phi(K) / state part of all but the last: ~1/3 extra work for nseg x the parallelism).
  const int64_t pairs = N * H, chunks = (T + 63) / 64;
  int64_t nseg = 1;
  if (pairs <= 128 && chunks >= 8) {
    nseg = 256 / pairs;                                      // all workgroups of a pass resident at once (1 per CU: LDS)
    if (nseg > chunks / 4) nseg = chunks / 4;
    if (nseg > 16) nseg = 16;
    const int64_t len = perf_seg_len(T, nseg);
    nseg = (T + len - 1) / len;                              // no empty segment
  }
  *n_segments = nseg;
  *workspace_bytes = pairs * (nseg - 1) * cf * (int64_t)sizeof(float);
  return SEA_OK;
}

static int perf_entry(const char* nm, const void* q, const void* k, const void* v, const void* pos, int dtype,
                      const float* proj, int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb,
                      const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                      int64_t pos_stride, void* out, void* avg_out, int64_t n_segments, void* workspace,
                      int64_t workspace_bytes, const void* state_in, void* state_out, int64_t state_bytes, int64_t t_base,
                      const int32_t* t_base_dev, int64_t t_base_stride, int aligned,
                      const int32_t* table, int64_t table_stride, int page_shift, sea_stream_t stream) {
  SEA_REQUIRE(q && k && v && pos && proj && out && q_strides && k_strides && v_strides, SEA_EINVAL, "%s: null pointer", nm);
  SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_F16 || dtype == SEA_BF16, SEA_EINVAL, "%s: bad dtype %d", nm, dtype);
  SEA_REQUIRE(N > 0 && H > 0 && T > 0 && D > 0 && nb > 0, SEA_EINVAL, "%s: bad shape", nm);
  const int vec = dtype == SEA_F32 ? 4 : 8;
  auto ok3 = [&](const int64_t* s) { return s[0] % vec == 0 && s[1] % vec == 0 && s[2] % vec == 0; };
  SEA_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)pos | (uintptr_t)out) & 15) == 0 && ok3(q_strides) &&
                  ok3(k_strides) && ok3(v_strides) && pos_stride % vec == 0,
              SEA_EUNSUPPORTED, "%s: rows must be 16-byte aligned", nm);
  PerfParams p;
  p.q = q; p.k = k; p.v = v; p.pos = pos; p.W = proj; p.out = out; p.avg = avg_out;
  const PerfForm form = perf_form(dtype, D, nb);
  SEA_REQUIRE(avg_out == nullptr || (form.mfma16 && ((uintptr_t)avg_out & 15) == 0),
              SEA_EUNSUPPORTED, "%s: avg_out needs the 16-bit MFMA kernels (bf16 / fp16 data, D = 64, 80, 128)", nm);
  for (int i = 0; i < 3; ++i) { p.qs[i] = q_strides[i]; p.ks[i] = k_strides[i]; p.vs[i] = v_strides[i]; }
  p.pos_stride = pos_stride;
  p.N = (int)N; p.H = (int)H; p.T = (int)T; p.nb = (int)nb;
  SEA_REQUIRE(n_segments >= 1 && n_segments <= 64, SEA_EINVAL, "%s: n_segments %lld outside 1..64", nm, (long long)n_segments);
  p.nseg = (int)n_segments;
  // local rows of the call: the new rows plus, for a chunk-aligned step, the open chunk's old rows in front of them (with the
  // position in device memory the host cannot know how many: up to a chunk -- one segment, any length covers it)
  int64_t TL = T;
  p.aligned = aligned;
  if (aligned) {
    SEA_REQUIRE(form.mfma16, SEA_EUNSUPPORTED, "%s: the chunk-aligned step runs on the 16-bit MFMA kernels (bf16 / fp16 data, D = 64, 80, 128)", nm);
    TL = T + (t_base_dev ? form.C - 1 : t_base % form.C);
  }
  p.seg_len = (int)perf_seg_len(TL, n_segments);
  p.carry = reinterpret_cast<float*>(workspace);
  p.state_in = reinterpret_cast<const float*>(state_in);
  p.state_out = reinterpret_cast<float*>(state_out);
  p.t_base = (int)t_base;
  p.t_base_dev = t_base_dev;
  SEA_REQUIRE(t_base_stride >= 0 && t_base_stride * N < (1ll << 31), SEA_EINVAL, "%s: bad position stride %lld", nm,
              (long long)t_base_stride);
  p.t_base_stride = (int)t_base_stride;
  p.table = table; p.table_stride = (int)table_stride; p.page_shift = page_shift;
  if (state_in || state_out) {
    const int64_t need = N * H * form.carry_floats * (int64_t)sizeof(float);
    SEA_REQUIRE(need > 0 && state_bytes >= need && ((((uintptr_t)state_in) | ((uintptr_t)state_out)) & 15) == 0 && t_base >= 0,
                SEA_EINVAL, "%s: state images of %lld bytes needed (16-byte aligned), got %lld", nm, (long long)need, (long long)state_bytes);
    SEA_REQUIRE(state_in != nullptr || t_base == 0, SEA_EINVAL, "%s: t_base %lld without state_in", nm, (long long)t_base);
    SEA_REQUIRE(n_segments == 1 || state_in != state_out, SEA_EINVAL, "%s: state_in and state_out may alias only with one segment", nm);
  }
  if (n_segments > 1) {
    SEA_REQUIRE((n_segments - 1) * (int64_t)p.seg_len < TL, SEA_EINVAL, "%s: %lld segments leave one empty at T=%lld (use sea_performer_plan)",
                nm, (long long)n_segments, (long long)TL);
    const int64_t need = N * H * (n_segments - 1) * form.carry_floats * (int64_t)sizeof(float);
    SEA_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need, SEA_EINVAL,
                "%s: workspace of %lld bytes needed (16-byte aligned), got %lld", nm, (long long)need, (long long)workspace_bytes);
  }
  const int rc = form.launch ? form.launch(p, (hipStream_t)stream) : SEA_EUNSUPPORTED;
  SEA_REQUIRE(rc == SEA_OK, rc, "%s: unsupported head size D=%lld / feature count nb=%lld", nm, (long long)D, (long long)nb);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}

// n_segments = 1, workspace = NULL: one pass over the rows; more segments run in parallel (sea_performer_plan picks them)
extern "C" int sea_performer_causal(const void* q, const void* k, const void* v, const void* pos, int dtype,
                                    const float* proj, int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb,
                                    const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                    int64_t pos_stride, void* out, void* avg_out, int64_t n_segments,
                                    void* workspace, int64_t workspace_bytes, sea_stream_t stream) {
  return perf_entry("sea_performer_causal", q, k, v, pos, dtype, proj, N, H, T, D, nb, q_strides, k_strides,
                    v_strides, pos_stride, out, avg_out, n_segments, workspace, workspace_bytes, nullptr, nullptr, 0, 0, nullptr, 0, 0,
                    nullptr, 0, 0, stream);
}

extern "C" int64_t sea_performer_state_bytes(int64_t N, int64_t H, int64_t D, int64_t nb, int dtype) {
  if (N <= 0 || H <= 0 || D <= 0 || nb <= 0) return 0;
  return N * H * perf_form(dtype, D, nb).carry_floats * (int64_t)sizeof(float);
}

// Stateful step, CHUNK ALIGNED (kv-cache decoding that reproduces the stateless pass bit for bit, attention_state.py:43-140 /
// test_perlin_opt_cache.py:7-32): the sequences have seen `t_base` rows, the image is the state at the last chunk boundary
// c0 = floor(t_base / C) * C (C = sea_performer_chunk_rows), and the call walks the open chunk again from c0.
//   k, v, pos  point at ROW c0 (the caller's kv-cache / embedding table hold those rows), T + t_base % C rows are read;
//   q, out, avg_out point at the first NEW row, T rows.
// state_out = the image at the last chunk boundary at or below t_base + T.  16-bit data, D in {64, 80, 128}.
// t_base_dev != NULL: the position lives in DEVICE memory (SURVEY 8f-3 / opt_generate.py:131: the decode loop captured once as
// a HIP graph and replayed per token -- nothing position-dependent may live in kernel arguments).  *t_base_dev = rows the
// state has seen, `t_base` is not read; k / v are the BASES (row 0) of the kv-caches, which already hold the new rows, pos
// the BASE of the value-embedding table: the kernel finds the chunk boundary itself.  state_in and state_out may be the
// same image (updated in place); one segment.
// t_base_stride > 0 (device-position form): a position PER SEQUENCE, sequence n has seen t_base_dev[n * t_base_stride] rows.
// block_table != NULL (with per-sequence positions, one new row each): paged K / V -- k / v are the K / V halves of a page
// pool (strides [page, head, row]); sequence n's open chunk c0 .. seen and its new row lie in page
// block_table[n * table_stride + c0 / page_rows], from row c0 % page_rows on.
extern "C" int sea_performer_causal_step(const void* q, const void* k, const void* v, const void* pos, int dtype,
                                         const float* proj, int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb,
                                         const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                         int64_t pos_stride, void* out, void* avg_out, const void* state_in,
                                         void* state_out, int64_t state_bytes, int64_t t_base, const int32_t* t_base_dev,
                                         int64_t t_base_stride, int64_t n_segments, void* workspace, int64_t workspace_bytes,
                                         const int32_t* block_table, int64_t table_stride, int64_t page_rows, int64_t capacity,
                                         sea_stream_t stream) {
  const char* nm = "sea_performer_causal_step";
  if (t_base_stride || block_table) {
    SEA_REQUIRE(t_base_dev, SEA_EINVAL, "%s: null pointer", nm);
    SEA_REQUIRE(t_base_stride > 0, SEA_EINVAL, "%s: t_base_stride must be >= 1 (got %lld)", nm, (long long)t_base_stride);
  }
  if (block_table) {
    SEA_REQUIRE(T == 1, SEA_EINVAL, "%s: one new row per sequence (T=%lld)", nm, (long long)T);
    const PerfForm form = perf_form(dtype, D, nb);
    SEA_REQUIRE(form.mfma16, SEA_EUNSUPPORTED, "%s: the chunk-aligned step runs on the 16-bit MFMA kernels (bf16 / fp16 data, D = 64, 80, 128)", nm);
    if (int e = paged_layout_check(nm, dtype, D, capacity, page_rows, table_stride, N)) return e;
    SEA_REQUIRE(page_rows % form.C == 0, SEA_EINVAL, "%s: page_rows %lld is not a multiple of the chunk (%d rows)", nm,
                (long long)page_rows, form.C);
  } else {
    SEA_REQUIRE(page_rows == 0 && table_stride == 0 && capacity == 0, SEA_EINVAL,
                "%s: null pointer: page_rows / table_stride / capacity without a block_table", nm);
  }
  if (t_base_dev) {
    SEA_REQUIRE(state_in && state_out, SEA_EINVAL, "%s: null pointer", nm);
    SEA_REQUIRE(n_segments == 1, SEA_EUNSUPPORTED, "%s: the device-position step runs one segment", nm);
    t_base = 0; workspace = nullptr; workspace_bytes = 0;
  }
  return perf_entry(nm, q, k, v, pos, dtype, proj, N, H, T, D, nb, q_strides, k_strides, v_strides, pos_stride, out, avg_out,
                    n_segments, workspace, workspace_bytes, state_in, state_out, state_bytes, t_base, t_base_dev, t_base_stride, 1,
                    block_table, table_stride, block_table ? __builtin_ctzll(page_rows) : 0, stream);
}
