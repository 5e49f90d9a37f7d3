// What the Performer kernels of sea_performer.hip share: the parameter block, one constexpr plan per kernel form (every derived
// constant, the LDS carving, the size of the carry / state image -- read by the kernel AND by the host's form table, so the
// launch's dynamic LDS and the ABI-visible image size cannot drift from what the kernel addresses), and for the two 16-bit
// kernels (performer_bf16_kernel, D = 64, C = 64; performer_bf16w_kernel, D = 80 / 128, C = 32) the workgroup prologue, the
// carry image and the phases of a chunk.  What differs between the two -- the V-image row length, the staging and V-image
// swizzles, one or two phi image sets -- enters through the plan; the chunk walks (barriers, prefetch sets, PIPE, the wide
// kernel's two-chunk state pass) stay with the kernels.  Both kernels take the prologue, the carry image, the feature map, phase
// (c) and the k-sum pieces from here; Perf16Lds, the tril table, the V fragments and (d)(e) serve the D = 64 kernel alone: the wide
// kernel compiles to a slower schedule with them and keeps its own.  See sea_performer.hip for the algorithm.
#pragma once
#include "sea_common.hpp"

namespace sea {

using f4 = __attribute__((ext_vector_type(4))) float;

struct PerfParams {
  const void *q, *k, *v;   // (N,H,T,D)
  const void* pos;         // (>=T, D) learned causal value embedding
  const float* W;          // (nb, D) fp32
  void* out;               // (N,H,T,3D)
  void* avg;               // optional (N,H,T,D): cumulative average of v (bf16 kernel only)
  int64_t qs[3], ks[3], vs[3];
  int64_t pos_stride;
  int N, H, T, nb;
  // sequence-parallel form (few (n,h) pairs): the T rows are cut into nseg segments of seg_len rows (a multiple of the
  // chunk size).  Pass 1 (STATE_ONLY kernels, grid.y = nseg-1) leaves every segment's state increment in `carry`,
  // pass 2 (grid.y = nseg) starts each segment from the sum of the increments before it.  nseg = 1: one pass.
  float* carry;
  int nseg, seg_len;
  // stateful form (kv-cache decoding): the rows handed in continue a sequence.  state_in / state_out are per-(n,h)
  // images in the carry format (state registers, k-sum, column sum of v); t_base = rows the state has already seen
  // (only the cumulative average needs the absolute row index).  Either may be null.
  const float* state_in;
  float* state_out;
  int t_base;
  // device-resident form of t_base (a captured decode step replayed as a HIP graph: the position lives in memory).  When
  // set, `pos` is the BASE of the embedding table and the kernel reads its rows from row *t_base_dev on.
  const int32_t* t_base_dev;
  // per-sequence positions (t_base_stride > 0, the SEQ instantiations of the 16-bit kernels): sequence n has seen
  // t_base_dev[n * t_base_stride] rows.  0: the one position above
  int t_base_stride;
  // chunk-aligned step (the 16-bit MFMA kernels): the state image is the state at the last CHUNK BOUNDARY c0 =
  // floor(t_base / C) * C, and the open chunk's rows c0 .. t_base-1 are walked again (k, v, pos from the caller's kv-cache,
  // no q, no output), so that every new row is computed by the very instruction sequence the stateless pass runs for it --
  // bitwise the stateless result for any split of the sequence into calls.  k / v / pos then point at row c0 (with
  // t_base_dev: at row 0 of the caches / the table, the kernel adds c0); q / out / avg at the first new row.
  int aligned;
  // paged K / V (a block table, the PAGED instantiations of the SEQ forms): k / v are the K / V halves of a page pool,
  // strides [page, head, row]; sequence n's chunk c0 lives in page table[n * table_stride + c0 / page_rows] at row
  // c0 % page_rows (page_rows = 1 << page_shift, a multiple of C: the open chunk and the new row lie in that one page)
  const int32_t* table;
  int table_stride, page_shift;
};

// ---- fp32 kernel (performer_kernel): LDS images in floats, carry = the per-thread state registers + the k-sum -------------
template <int D_, int NBT_, int C_>
struct PerfF32Plan {
  static constexpr int D = D_, NBT = NBT_, C = C_, NW = 8, NTH = NW * 64;
  static constexpr int E = 2 * D, NBP = NBT * 16;
  static constexpr int RB = C / 16;                  // row blocks per chunk
  static constexpr int EB = E / 16;                  // column blocks of V / S / O
  static constexpr int JB = (EB + NW - 1) / NW;      // column blocks owned by one wave
  static constexpr int LDQ = D + 2, LDV = E + 16, LDP = NBP + 2, LDA = C + 2, LDW = D + 2;
  static constexpr int DSL = RB + NTH / C;           // partial-denominator slots per row: RB key blocks + carry parts
  static_assert(LDA <= LDQ, "the A tile is overlaid on the Q tile");
  // float offsets of the images
  static constexpr int oW = 0;                       // NBP x LDW   W (rows >= nb are zero)
  static constexpr int oQ = oW + NBP * LDW;          // C x LDQ     Q chunk, later the masked A tile (C x LDA)
  static constexpr int oK = oQ + C * LDQ;            // C x LDQ
  static constexpr int oV = oK + C * LDQ;            // C x LDV     [pos | v]
  static constexpr int oQp = oV + C * LDV;           // C x LDP     phi(Q)
  static constexpr int oKp = oQp + C * LDP;          // C x LDP     phi(K)
  static constexpr int oKsum = oKp + C * LDP;        // NBP         running sum of phi(k)
  static constexpr int oDen = oKsum + NBP;           // C           denominators of the current chunk
  static constexpr int oDenP = oDen + C;             // C x DSL     partials, summed in a fixed order (bitwise reproducible)
  static constexpr size_t lds_bytes = sizeof(float) * (oDenP + C * DSL);
  static constexpr int ksum_at = JB * NBT * 4 * NTH; // raw per-thread register images first, then the k-sum
  static constexpr int64_t carry_floats = ksum_at + NBP;
};
static_assert(PerfF32Plan<64, 3, 64>::lds_bytes == 112448 && PerfF32Plan<64, 3, 64>::carry_floats == 6192, "fp32, D = 64, NBT = 3");
static_assert(PerfF32Plan<64, 5, 64>::lds_bytes == 137408 && PerfF32Plan<64, 5, 64>::carry_floats == 10320, "fp32, D = 64, NBT = 5");
static_assert(PerfF32Plan<80, 3, 64>::lds_bytes == 131904 && PerfF32Plan<80, 3, 64>::carry_floats == 12336, "fp32, D = 80, NBT = 3");
static_assert(PerfF32Plan<80, 5, 32>::lds_bytes == 93504 && PerfF32Plan<80, 5, 32>::carry_floats == 20560, "fp32, D = 80, NBT = 5");
static_assert(PerfF32Plan<128, 5, 32>::lds_bytes == 133440 && PerfF32Plan<128, 5, 32>::carry_floats == 20560, "fp32, D = 128, NBT = 5");

// ======================================================================================================
// 16-bit kernels
// ======================================================================================================
typedef __attribute__((ext_vector_type(8))) __bf16 pbf8;
typedef __attribute__((ext_vector_type(8))) _Float16 ph8;
typedef __attribute__((ext_vector_type(4))) short ps4;
typedef __attribute__((ext_vector_type(4))) unsigned int bu4;
typedef __attribute__((ext_vector_type(2))) unsigned int bu2;

// 16-bit storage type of the split operands: bf16 data splits into bf16 terms (2 x 8 significand bits), fp16 data into
// fp16 terms (2 x 11 bits; the state S and the products stay well inside fp16's range for T up to tens of thousands)
template <typename T> struct S16;
template <> struct S16<__hip_bfloat16> {
  static constexpr unsigned short ONE = 0x3F80;
  __device__ static inline unsigned short bits(float x) { return __builtin_bit_cast(unsigned short, __float2bfloat16(x)); }
  __device__ static inline float val(unsigned short b) { return __uint_as_float((uint32_t)b << 16); }
  __device__ static inline f4 mfma(const uint4& a, const uint4& b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pbf8, a), __builtin_bit_cast(pbf8, b), c, 0, 0, 0);
  }
};
template <> struct S16<__half> {
  static constexpr unsigned short ONE = 0x3C00;
  __device__ static inline unsigned short bits(float x) { return __builtin_bit_cast(unsigned short, __float2half(x)); }
  __device__ static inline float val(unsigned short b) { return __half2float(__builtin_bit_cast(__half, b)); }
  __device__ static inline f4 mfma(const uint4& a, const uint4& b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(ph8, a), __builtin_bit_cast(ph8, b), c, 0, 0, 0);
  }
};

// x -> (hi, lo) 16-bit patterns with hi + lo ~ x to twice the type's significand bits
template <typename T> __device__ inline void split16(float x, unsigned short& hi, unsigned short& lo) {
  hi = S16<T>::bits(x);
  lo = S16<T>::bits(x - S16<T>::val(hi));
}
__device__ inline uint2 pack4(const unsigned short (&v)[4]) {
  return make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16));
}
__device__ inline uint4 cat8(uint2 a, uint2 b) { return make_uint4(a.x, a.y, b.x, b.y); }
__device__ inline uint2 lds_tr(const unsigned short* p) {      // ds_read_b64_tr_b16
  const ps4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ps4 __attribute__((address_space(3)))*)(p));
  return __builtin_bit_cast(uint2, v);
}

// ---- the plan of one 16-bit form.  D = 64 walks chunks of C = 64 rows, one 16-column block of [pos | v] per wave; the wide
// heads (D = 80, 128) cut the chunk to C = 32 so that the images fit (the D = 64 plan scaled up is 208 KB), keep up to two
// column blocks per wave (E / 16 = 16 or 10 blocks over 8 waves; at D = 80 only waves 0 and 1 own a second one), pad the head
// dimension to whole 32-wide k-steps (D = 80: 96) in the operand images of the feature-map product, and give the V image
// 512-byte rows whose chunk swizzle spreads the eight rows of a transposing read over the eight 8-bank groups.
template <int D_, int C_, int NBT_>
struct Perf16Plan {
  static constexpr int D = D_, C = C_, NBT = NBT_, NW = 8, NTH = 512, E = 2 * D;
  static constexpr bool WIDE = D != 64;
  static constexpr int CPR = D / 8;                  // 8-element (16-byte) staging chunks per row
  static constexpr int DP = (D + 31) / 32 * 32, KC = DP / 8;   // head dimension padded to whole k-steps, its 8-element chunks
  static constexpr int NBP = NBT * 16;
  static constexpr int KF = (NBT + 1) / 2;           // 32-wide k-steps over the (padded) features
  static constexpr int FP = KF * 32;                 // padded feature count
  static constexpr int RB = C / 16, EB = E / 16, JB = (EB + NW - 1) / NW;
  // (b) runs on all eight waves: a (Q | K, row block) pair is shared by BW waves, each taking FBP of the feature blocks
  static constexpr int BW = NW / (2 * RB), FBP = (NBT + BW - 1) / BW;
  static_assert(2 * RB * BW == NW, "feature-map product: whole waves per (tensor, row block)");
  static_assert(D % 16 == 0 && C % 16 == 0 && C * CPR <= NTH, "whole column blocks; staging pieces fit the block");
  // LDS row strides picked with a bank model of the two access patterns (64 banks x 4 B; b128 row reads are served in
  // 4 lane groups of 16, transposing b64 reads in 2 of 32): 160 / 224 B rows make the operand row reads conflict-free
  // (4 cycles per wave instruction; the first version's 144 B rows: 8), 192 B rows halve the conflicts of the
  // transposing reads of phi(K) (4 cycles; 144 B: 8; the conflict-free 2 needs a swizzle); rows stay 16-byte multiples
  static constexpr int LDQ2 = FP + 16;               // phi(Q) rows (elements): row reads only
  static constexpr int LDK2 = (FP == 64) ? 96 : FP + 8;   // phi(K) rows (16-byte multiples): transposing reads + a few row reads
  static constexpr int LDA = C + 16;                 // A rows: row reads only
  static constexpr int NPART = 8;                    // threads per row of the denominators' carry part
  static_assert(NTH / C >= NPART && (FP / NPART) % 4 == 0, "four positions per step");
  static constexpr int DSL = RB + NPART;             // denominator partial slots per row
  static constexpr int EL = WIDE ? 256 : E;          // elements per row of the V image (wide: 512 bytes, room for the swizzle)
  static_assert(E <= EL, "a [pos | v] row fits its image row");
  static constexpr int PHI = 2 * C * LDQ2 + 2 * C * LDK2;   // elements of one phi image set: Qh, Ql [C][LDQ2], Kh, Kl [C][LDK2]
  static constexpr int oQl = C * LDQ2, oKh = 2 * C * LDQ2, oKl = oKh + C * LDK2;   // ... and the images' offsets in it
  // two sets (two chunks in flight) where they fit (D = 64, FP = 64: 152 KB in all); with FP = 96 one set, and (b) of the next
  // chunk waits for a fourth barrier.  The 25 KB of result tiles the wide kernel's first version flushed one chunk later paid
  // for its second set (d = 128: 120 KB)
  static constexpr int NSET = (WIDE || FP == 64) ? 2 : 1;
  static constexpr bool TWO = WIDE;                  // the state pass walks two chunks per iteration: second partials, second V image
  // element offsets of the 16-bit images
  static constexpr int oW = 0;                       // [KC][NBP][8]  projection, k-chunked (zero padded)
  static constexpr int oQ = oW + KC * NBP * 8;       // [KC][C][8]    (chunks >= D / 8: zero)
  static constexpr int oK = oQ + KC * C * 8;         // [KC][C][8]
  static constexpr int oV = oK + KC * C * 8;         // [C][EL]       [pos | v], chunk-swizzled
  static constexpr int oPhi = oV + C * EL;           // [NSET][PHI]
  static constexpr int oA = oPhi + NSET * PHI;       // [2][C][LDA]   A hi, lo (behind the last set)
  static constexpr int n16 = oA + 2 * C * LDA;
  // float offsets of what follows them
  static constexpr int oKsum = 0;                    // [FP]
  static constexpr int oDenP = oKsum + FP;           // [C][DSL]
  static constexpr int oKsP = oDenP + C * DSL;       // [NW][FP]      per-wave k-sum increments
  static constexpr int oKsP2 = oKsP + NW * FP;       // [NW][FP]      (TWO: the second chunk of an iteration)
  static constexpr int n32 = oKsP2 + (TWO ? NW * FP : 0);
  static constexpr size_t oV2_bytes = 2 * (size_t)n16 + sizeof(float) * n32;   // [C][EL] (TWO: the second chunk's [pos | v])
  static constexpr size_t lds_bytes = oV2_bytes + (TWO ? 2 * C * EL : 0);
  // carry image of one (n, h[, segment]): per-thread state registers S[JB][NBT] (f4), the k-sum, the column sums of v.
  // Running column sums (cumulative-average output): in the transposed accumulator layout of (d) a lane owns the four columns
  // e0 + 4 lg + r of each of its wave's blocks; the 16 lanes of a lane group carry the same four.  Image slot of column r of
  // block jq: lane (lg, li = r) of the wave, i.e. csum_at(jq) + (tid & ~15) + r.
  static __host__ __device__ constexpr int s_at(int jq, int b, int r) { return ((jq * NBT + b) * 4 + r) * NTH; }   // + tid
  static constexpr int ksum_at = JB * NBT * 4 * NTH;
  static __host__ __device__ constexpr int csum_at(int jq) { return ksum_at + FP + jq * NTH; }
  static constexpr int64_t carry_floats = ksum_at + FP + JB * NTH;
  // slot of staged row `row` in k-chunk `ch` of the q / k images.  D = 64: row slot XOR 2 * chunk -- the 16 lanes of a b128
  // store (2 rows x 8 chunks; chunk images are 1 KB = 0 mod 64 banks apart) land in 16 different 4-bank groups instead of 2
  // (8-way conflicts).  Wide: row slot XOR chunk (one row x 16 chunks at D = 128; chunk images 512 B apart): 16 groups
  // instead of one.  The reads of (b) permute inside their 16-row runs
  static __host__ __device__ constexpr int qk_slot(int row, int ch) { return WIDE ? row ^ ch : row ^ (2 * ch); }
  // swizzled chunk position inside a row of the V image (conflict-free transposing reads).  256-byte rows (D = 64): see the
  // bank model above.  512-byte rows (32 chunks): rows {r..r+3, r+8..r+11} of one transposing read get the eight values of
  // (row & 3) | (bit 3 of row) << 2 XOR-ed into bits 1..3 of the chunk index -> eight disjoint 8-bank groups
  static __host__ __device__ constexpr int vchunk(int row, int ch) {
    return WIDE ? ch ^ ((((row & 3) | (((row >> 3) & 1) << 2))) << 1) : ch ^ (((row & 3) << 2) | ((row >> 2) & 3));
  }
};
static_assert(Perf16Plan<64, 64, 3>::lds_bytes == 154880 && Perf16Plan<64, 64, 3>::carry_floats == 6720, "D = 64, NBT = 3");
static_assert(Perf16Plan<64, 64, 5>::lds_bytes == 125312 && Perf16Plan<64, 64, 5>::carry_floats == 10848, "D = 64, NBT = 5");
static_assert(Perf16Plan<80, 32, 3>::lds_bytes == 111104 && Perf16Plan<80, 32, 3>::carry_floats == 13376, "D = 80, NBT = 3");
static_assert(Perf16Plan<80, 32, 5>::lds_bytes == 129664 && Perf16Plan<80, 32, 5>::carry_floats == 21600, "D = 80, NBT = 5");
static_assert(Perf16Plan<128, 32, 5>::lds_bytes == 138880 && Perf16Plan<128, 32, 5>::carry_floats == 21600, "D = 128, NBT = 5");
static_assert(Perf16Plan<64, 64, 3>::JB == 1 && Perf16Plan<64, 64, 3>::BW == 1 && Perf16Plan<64, 64, 3>::KC == Perf16Plan<64, 64, 3>::CPR,
              "D = 64: one column block per wave, a whole (tensor, row block) per wave, no padded k-chunks");

// the kernel's pointers, carved from the plan
template <class P>
struct Perf16Lds {
  unsigned short *sW, *sQ, *sK, *sV, *sPhi, *sAh, *sAl;
  float *sKsum, *sDenP, *sKsP;                 // (the wide kernel, which alone has the plan's second partials and V image, carves its own chain)
  __device__ __forceinline__ explicit Perf16Lds(char* b)
      : sW(reinterpret_cast<unsigned short*>(b) + P::oW), sQ(sW + P::oQ), sK(sW + P::oK), sV(sW + P::oV), sPhi(sW + P::oPhi),
        sAh(sW + P::oA), sAl(sAh + P::C * P::LDA), sKsum(reinterpret_cast<float*>(sW + P::n16) + P::oKsum),
        sDenP(sKsum + P::oDenP), sKsP(sKsum + P::oKsP) {}
  __device__ __forceinline__ unsigned short* set(int buf) const { return sPhi + buf * P::PHI; }
};

// ---- workgroup prologue: where this workgroup's rows are.  Built in two steps around the SEQ forms' early return: the
// positions and base pointers first (the counter load leaves before the LDS staging), the buffer resources behind the return.
constexpr int PERF16_OOB = (int)0x7FFFFF00u;     // offset of a load that reads zeros / a store that is dropped
struct Perf16Bufs {
  __amdgpu_buffer_rsrc_t rq, rk, rv, rp, ro, rg;
};
template <typename T, int D, int C, bool SEQ, bool PAGED>
struct Perf16Wg {
  int nh, n, h, seg;
  int tb;                  // rows seen (block-uniform)
  int lead, row_base, TL, t_begin, t_end, aligned;
  const T *qb, *kb, *vb, *pb;
  T *ob, *gb;
  bool want_avg;           // block-uniform
  __device__ __forceinline__ explicit Perf16Wg(const PerfParams& p) {
    nh = blockIdx.x;
    n = nh / p.H, h = nh - n * p.H;
    seg = blockIdx.y;                                        // sequence-parallel form, see PerfParams
    tb = SEQ ? p.t_base_dev[n * p.t_base_stride] : p.t_base_dev ? *p.t_base_dev : p.t_base;
    // (SEQ: per-sequence positions; a form of its own, so that the shared-position step's counter load does not wait for n)
    // chunk-aligned step: local row 0 is the chunk boundary at or below tb; the `lead` rows up to tb are the open chunk's old
    // rows (k, v, pos only).  Otherwise lead = 0 and local row 0 is row tb.
    aligned = p.aligned;
    lead = p.aligned ? tb % C : 0;
    row_base = tb - lead;                                    // absolute index of local row 0
    TL = p.T + lead;                                         // local rows of this call
    t_begin = seg * p.seg_len, t_end = min(TL, t_begin + p.seg_len);
    qb = reinterpret_cast<const T*>(p.q) + n * p.qs[0] + h * p.qs[1] - (int64_t)lead * p.qs[2];   // rows < lead are never read
    int64_t cache_row = (p.aligned && p.t_base_dev) ? row_base : 0;            // k / v given as cache bases: start at the boundary
    int64_t kv_n = n;
    if constexpr (PAGED) {                                   // one table lookup per workgroup: the chunk's page
      static_assert(SEQ, "the paged step has a position per sequence");
      kv_n = p.table[(int64_t)n * p.table_stride + (max(row_base, 0) >> p.page_shift)];   // (tb < 0, a sequence sitting out: entry 0, unused)
      cache_row = row_base & ((1 << p.page_shift) - 1);
    }
    kb = reinterpret_cast<const T*>(p.k) + kv_n * p.ks[0] + h * p.ks[1] + cache_row * p.ks[2];
    vb = reinterpret_cast<const T*>(p.v) + kv_n * p.vs[0] + h * p.vs[1] + cache_row * p.vs[2];
    pb = reinterpret_cast<const T*>(p.pos) + (p.t_base_dev ? (int64_t)row_base * p.pos_stride : 0);
    ob = reinterpret_cast<T*>(p.out) + (int64_t)nh * p.T * (3 * D) - (int64_t)lead * (3 * D);           // rows < lead are never stored
    want_avg = p.avg != nullptr;
    gb = reinterpret_cast<T*>(p.avg) + (want_avg ? (int64_t)nh * p.T * D - (int64_t)lead * D : 0);
  }
  // All global traffic goes through buffer instructions with hardware range checking: a row beyond T reads zeros /
  // drops its store WITHOUT a branch.  (Branches around loads and stores make the compiler's vmcnt bookkeeping
  // pessimistic: the wait for the prefetched chunk then also waits for every output store of the previous one.)
  __device__ __forceinline__ Perf16Bufs buffers(const PerfParams& p) const {
    auto mk = [&](const T* base, int64_t bytes) {
      return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base), 0, (int)bytes, 0x00020000);
    };
    auto rows = [&](int64_t row_stride) { return ((int64_t)(TL - 1) * row_stride + D) * 2; };
    return {mk(qb, rows(p.qs[2])), mk(kb, rows(p.ks[2])), mk(vb, rows(p.vs[2])), mk(pb, rows(p.pos_stride)),
            mk(ob, (int64_t)TL * 3 * D * 2), mk(gb, want_avg ? (int64_t)TL * D * 2 : 0)};
  }
  __device__ __forceinline__ int rows_of(int t0) const { return min(C, t_end - t0); }
  // aligned step, open chunk (always the call's last): its rows produce output but do NOT enter the state -- S, the k-sum
  // and the column sums stay the state AT THE BOUNDARY, which is the image the next call continues from (it walks this
  // chunk's rows again).  Block-uniform.
  __device__ __forceinline__ bool upd_of(int t0) const { return !(aligned && rows_of(t0) < C); }
};

// ---- LDS images that are written once: the projection (its values are 16-bit exact: the reference casts the buffer to the data
// dtype; padded rows and k-chunks zero), the padded k-chunks of the q / k images, the phi and A images (padded features /
// upper-triangular tiles stay zero), the denominator partials (slots of key blocks above the diagonal stay zero)
template <typename T, class P>
__device__ __forceinline__ void perf16_lds_init(const Perf16Lds<P>& L, const float* W, int nb, int tid) {
  for (int i = tid; i < P::KC * P::NBP * 8; i += P::NTH) {
    const int j = i & 7, f = (i >> 3) % P::NBP, kc = (i >> 3) / P::NBP;
    L.sW[i] = (f < nb && kc < P::CPR) ? S16<T>::bits(W[f * P::D + kc * 8 + j]) : (unsigned short)0;
  }
  if constexpr (P::KC > P::CPR)
    for (int i = tid; i < (P::KC - P::CPR) * P::C * 8; i += P::NTH) L.sQ[P::CPR * P::C * 8 + i] = L.sK[P::CPR * P::C * 8 + i] = 0;
  for (int i = tid; i < P::NSET * P::PHI + 2 * P::C * P::LDA; i += P::NTH) L.sPhi[i] = 0;
  for (int i = tid; i < P::C * P::DSL; i += P::NTH) L.sDenP[i] = 0.f;
}

// ---- carry / state image: load, add-in of the earlier segments, write -- one byte layout (Perf16Plan::s_at / ksum_at / csum_at)
template <class P, bool ADD>
__device__ __forceinline__ void perf16_carry_take(const float* cr, int tid, f4 (&S)[P::JB][P::NBT], float (&csum)[P::JB][4], float& ks0) {
  const int cslot = tid & ~15;
#pragma unroll
  for (int jq = 0; jq < P::JB; ++jq) {
#pragma unroll
    for (int b = 0; b < P::NBT; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float x = cr[P::s_at(jq, b, r) + tid];
        S[jq][b][r] = ADD ? S[jq][b][r] + x : x;
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float x = cr[P::csum_at(jq) + cslot + r];
      csum[jq][r] = ADD ? csum[jq][r] + x : x;
    }
  }
  if (tid < P::FP) ks0 = ADD ? ks0 + cr[P::ksum_at + tid] : cr[P::ksum_at + tid];
}
template <class P>
__device__ __forceinline__ void perf16_carry_load(const float* state_in, int64_t nh, int tid, f4 (&S)[P::JB][P::NBT], float (&csum)[P::JB][4],
                                                  float& ks0) {
  perf16_carry_take<P, false>(state_in + nh * P::carry_floats, tid, S, csum, ks0);
}
template <class P>
__device__ __forceinline__ void perf16_carry_add_segments(const float* carry, int64_t nh, int nseg, int seg, int tid, f4 (&S)[P::JB][P::NBT],
                                                          float (&csum)[P::JB][4], float& ks0) {
  for (int s2 = 0; s2 < seg; ++s2)                           // fixed order: bitwise reproducible
    perf16_carry_take<P, true>(carry + (nh * (nseg - 1) + s2) * P::carry_floats, tid, S, csum, ks0);
}
template <class P>
__device__ __forceinline__ void perf16_carry_write(float* cw, int tid, int li, const f4 (&S)[P::JB][P::NBT], const float (&csum)[P::JB][4],
                                                   const float* sKsum) {
#pragma unroll
  for (int jq = 0; jq < P::JB; ++jq) {
#pragma unroll
    for (int b = 0; b < P::NBT; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) cw[P::s_at(jq, b, r) + tid] = S[jq][b][r];
    // the 16 slots of a lane group: its four sums, then zeros.  The same bytes in two forms, each the one its kernel always had:
    // JB = 1, one store per thread (lanes li = 0..3 select their sum).  With more blocks that select chain becomes an index into
    // csum, which then lives in scratch (48 bytes per lane, written back every chunk): lane li = 0 stores the four, lanes >= 4 a zero
    if constexpr (P::JB == 1) {
      cw[P::csum_at(jq) + tid] = li == 0 ? csum[jq][0] : li == 1 ? csum[jq][1] : li == 2 ? csum[jq][2] : li == 3 ? csum[jq][3] : 0.f;
    } else {
      float* cs = cw + P::csum_at(jq) + tid;
      if (li == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) cs[r] = csum[jq][r];
      } else if (li >= 4) cs[0] = 0.f;
    }
  }
  if (tid < P::FP) cw[P::ksum_at + tid] = sKsum[tid];
}
// state at the start of this workgroup's rows = the incoming image + the increments of the segments before this one
template <class P, bool STATE_ONLY>
__device__ __forceinline__ void perf16_state_init(const PerfParams& p, int nh, int seg, int tid, f4 (&S)[P::JB][P::NBT], float (&csum)[P::JB][4],
                                                  float* sKsum) {
#pragma unroll
  for (int jq = 0; jq < P::JB; ++jq) {
#pragma unroll
    for (int r = 0; r < 4; ++r) csum[jq][r] = 0.f;
#pragma unroll
    for (int b = 0; b < P::NBT; ++b) S[jq][b] = f4{0.f, 0.f, 0.f, 0.f};
  }
  float ks0 = 0.f;
  if (!STATE_ONLY && p.state_in) perf16_carry_load<P>(p.state_in, nh, tid, S, csum, ks0);   // increments of pass 1 do not include the incoming state
  if (!STATE_ONLY) perf16_carry_add_segments<P>(p.carry, nh, p.nseg, seg, tid, S, csum, ks0);
  if (tid < P::FP) sKsum[tid] = ks0;
}
// ... and at their end: pass 1 leaves the segment's increment; in pass 2 the block that walked the last rows holds the final
// state (aligned step: the state at the last chunk boundary).  A step that closed no chunk (`closed_none`: one chunk walked,
// not entered into the state) leaves the image as it found it: updated in place (a DecodeSession) there is nothing to write --
// 25 KB of stores per (n, h) whose drain was the end of the launch on 63 of 64 positions
template <class P, bool STATE_ONLY>
__device__ __forceinline__ void perf16_state_finish(const PerfParams& p, int nh, int seg, int tid, int li, bool closed_none,
                                                    const f4 (&S)[P::JB][P::NBT], const float (&csum)[P::JB][4], const float* sKsum) {
  if constexpr (STATE_ONLY) {
    perf16_carry_write<P>(p.carry + ((int64_t)nh * (p.nseg - 1) + seg) * P::carry_floats, tid, li, S, csum, sKsum);
  } else {
    const bool unchanged = p.aligned && p.state_in == p.state_out && closed_none;
    if (p.state_out && seg == p.nseg - 1 && !unchanged) perf16_carry_write<P>(p.state_out + (int64_t)nh * P::carry_floats, tid, li, S, csum, sKsum);
  }
}

// ---- cumulative average of v (step K's input) on the waves that own the v columns: prefix sum over the chunk rows =
// tril(ones) . V on the matrix cores (1.0 and v are exact in 16 bits, fp32 accumulation) + the running column sum.
// The loop-invariant A operands of that product:
template <typename T>
__device__ __forceinline__ uint4 perf16_tril_frag(int ib, int ks, int li, int lg) {
  unsigned short o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (ks * 32 + lg * 8 + j <= ib * 16 + li) ? S16<T>::ONE : (unsigned short)0;
  const unsigned short (&o0)[4] = *reinterpret_cast<const unsigned short (*)[4]>(&o[0]);
  const unsigned short (&o1)[4] = *reinterpret_cast<const unsigned short (*)[4]>(&o[4]);
  return cat8(pack4(o0), pack4(o1));
}
template <typename T, class P>
__device__ __forceinline__ void perf16_tril_table(uint4 (&tril)[P::RB][P::C / 32], int li, int lg) {
#pragma unroll
  for (int ib = 0; ib < P::RB; ++ib)
#pragma unroll
    for (int ks = 0; ks < P::C / 32; ++ks) tril[ib][ks] = perf16_tril_frag<T>(ib, ks, li, lg);
}

// ---- (b) feature maps, transposed: X^T[f][t] = sum_d W[f][d] x[t][d]; wave = (Q | K, row block, part of the feature blocks) ----
// epilogue of one 16-feature block: a lane holds 4 consecutive features of row `row`
template <typename T>
__device__ __forceinline__ void perf16_phi_store(const f4& acc, int fbg, int row, int rows, int nb, float cnorm, int lg, unsigned short* dh,
                                                 unsigned short* dl, int ldx) {
  unsigned short hh[4], ll[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int f = fbg * 16 + lg * 4 + r;
    float val = fmaxf(cnorm * acc[r], 0.f) + 1e-3f;
    if (f >= nb || row >= rows) val = 0.f;                   // padded features / rows beyond T contribute nothing
    split16<T>(val, hh[r], ll[r]);
  }
  // feature 32kk + 16a + 4g + j is stored at position 32kk + 8g + 4a + j: the 8 features lane group g needs of
  // a 32-wide k-step in (d) (4 of tile 2kk, 4 of tile 2kk+1) are then one 16-byte piece
  const int pos = (fbg >> 1) * 32 + lg * 8 + (fbg & 1) * 4;
  *reinterpret_cast<uint2*>(dh + row * ldx + pos) = pack4(hh);
  *reinterpret_cast<uint2*>(dl + row * ldx + pos) = pack4(ll);
}
// the product of one staged image (q or k rows of a chunk) by this wave: its row block, its share of the feature blocks; the
// hi image at dh ([C][ldx]), the lo image behind it
template <typename T, class P>
__device__ __forceinline__ void perf16_feature_map(const unsigned short* src, const unsigned short* sW, unsigned short* dh, int ldx, int rows,
                                                   int nb, float cnorm, int wv, int li, int lg) {
  constexpr int C = P::C, NBT = P::NBT, NBP = P::NBP, FBP = P::FBP;
  // D = 80: waves 0 and 1 (SIMDs 0, 1) own a second column block in (d)(e), so the larger share of the feature blocks goes
  // to the waves of SIMDs 2 and 3
  const int rb = wv & (P::RB - 1), part = (P::BW - 1) - ((wv % (P::NW / 2)) / P::RB);
  f4 acc[FBP];
#pragma unroll
  for (int fb = 0; fb < FBP; ++fb) acc[fb] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < P::DP / 32; ++ks) {
    const uint4 bx = *reinterpret_cast<const uint4*>(src + ((4 * ks + lg) * C + P::qk_slot(rb * 16 + li, 4 * ks + lg)) * 8);
#pragma unroll
    for (int fb = 0; fb < FBP; ++fb) {
      const int fbg = part * FBP + fb;                       // (wave-uniform)
      if (fbg < NBT) {
        const uint4 aw = *reinterpret_cast<const uint4*>(sW + ((4 * ks + lg) * NBP + fbg * 16 + li) * 8);
        acc[fb] = S16<T>::mfma(aw, bx, acc[fb]);
      }
    }
  }
  unsigned short* dl = dh + C * ldx;
#pragma unroll
  for (int fb = 0; fb < FBP; ++fb) {
    const int fbg = part * FBP + fb;
    if (fbg < NBT) perf16_phi_store<T>(acc[fb], fbg, rb * 16 + li, rows, nb, cnorm, lg, dh, dl, ldx);
  }
}
// phase (b) of the output walks: the first four waves take q, the last four k
template <typename T, class P, bool STATE_ONLY>
__device__ __forceinline__ void perf16_phase_b(const Perf16Lds<P> L, unsigned short* set, int rows, int nb, float cnorm, int wv, int li, int lg) {
  const int which = wv / (P::NW / 2);                        // 0: Q, 1: K
  if (!STATE_ONLY || which == 1)                             // the state-only pass needs phi(K) alone (wave-uniform)
    perf16_feature_map<T, P>(which ? L.sK : L.sQ, L.sW, set + (which ? P::oKh : 0), which ? P::LDK2 : P::LDQ2, rows, nb, cnorm, wv, li, lg);
}

// ---- k-sum increment of one chunk: per-wave partials into dst [NW][FP] (wave w owns rows (C / NW) w ..; lane = (4-position
// group fc, row lane rr)), folded into the k-sum one barrier later
template <typename T, class P>
__device__ __forceinline__ void perf16_ksum_partial(const unsigned short* sKh, float* dst, int wv, int lane) {
  constexpr int C = P::C, NW = P::NW, FP = P::FP, LDK2 = P::LDK2;
  const unsigned short* sKl = sKh + C * LDK2;
  constexpr int FG = FP / 4, RRN = 64 / FG, RPL = (C / NW) / RRN;
  const int fc = lane % FG, rr = lane / FG;
  float k4[4] = {0.f, 0.f, 0.f, 0.f};
  if (rr < RRN) {
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
      const int r2 = wv * (C / NW) + rr * RPL + j;
      const uint2 kh = *reinterpret_cast<const uint2*>(sKh + r2 * LDK2 + fc * 4);
      const uint2 kl = *reinterpret_cast<const uint2*>(sKl + r2 * LDK2 + fc * 4);
      k4[0] += S16<T>::val((unsigned short)(kh.x & 0xffff)) + S16<T>::val((unsigned short)(kl.x & 0xffff));
      k4[1] += S16<T>::val((unsigned short)(kh.x >> 16)) + S16<T>::val((unsigned short)(kl.x >> 16));
      k4[2] += S16<T>::val((unsigned short)(kh.y & 0xffff)) + S16<T>::val((unsigned short)(kl.y & 0xffff));
      k4[3] += S16<T>::val((unsigned short)(kh.y >> 16)) + S16<T>::val((unsigned short)(kl.y >> 16));
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if constexpr (FG == 16) {
      k4[j] = xor16_sum(xor32_sum(k4[j]));                   // (l, l+32) then (+16): same association as the shuffle form
    } else {
#pragma unroll
      for (int o = FG * (RRN / 2); o >= FG; o >>= 1) k4[j] += __shfl_down(k4[j], o);   // fixed order
    }
  }
  if (lane < FG) *reinterpret_cast<float4*>(dst + wv * FP + fc * 4) = make_float4(k4[0], k4[1], k4[2], k4[3]);
}
template <class P>
__device__ __forceinline__ void perf16_ksum_fold(float* sKsum, const float* src, int tid, bool upd) {
  if (tid < P::FP) {
    float s = sKsum[tid];
#pragma unroll
    for (int i = 0; i < P::NW; ++i) s += src[i * P::FP + tid];     // fixed order: bitwise reproducible
    if (upd) sKsum[tid] = s;
  }
}

// ---- (c) A^T tiles (lower triangle), denominator and k-sum partials ------------------------------------
template <typename T, class P, bool STATE_ONLY>
__device__ __forceinline__ void perf16_phase_c(const Perf16Lds<P> L, const unsigned short* set, int tid, int wv, int lane, int li, int lg) {
  constexpr int C = P::C, NW = P::NW, RB = P::RB, KF = P::KF, LDQ2 = P::LDQ2, LDK2 = P::LDK2, LDA = P::LDA, DSL = P::DSL, NPART = P::NPART;
  const unsigned short* sQh = set;
  const unsigned short* sQl = set + P::oQl;
  const unsigned short* sKh = set + P::oKh;
  const unsigned short* sKl = set + P::oKl;
  if constexpr (!STATE_ONLY)
  for (int tile = wv; tile < RB * (RB + 1) / 2; tile += NW) {   // (wide: the first waves -- they stage nothing at D = 80)
    int ib = 0, rem = tile;
    while (rem > ib) { rem -= ib + 1; ++ib; }              // tile -> (query block ib, key block jb <= ib)
    const int jb = rem;
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KF; ++ks) {
      const int ko = ks * 32 + lg * 8;
      const uint4 kh = *reinterpret_cast<const uint4*>(sKh + (jb * 16 + li) * LDK2 + ko);
      const uint4 kl = *reinterpret_cast<const uint4*>(sKl + (jb * 16 + li) * LDK2 + ko);
      const uint4 qh = *reinterpret_cast<const uint4*>(sQh + (ib * 16 + li) * LDQ2 + ko);
      const uint4 ql = *reinterpret_cast<const uint4*>(sQl + (ib * 16 + li) * LDQ2 + ko);
      acc = S16<T>::mfma(kh, qh, acc);
      acc = S16<T>::mfma(kh, ql, acc);
      acc = S16<T>::mfma(kl, qh, acc);
    }
    const int trow = ib * 16 + li;                         // lane: A[trow][s0 .. s0+3]
    const int s0 = jb * 16 + lg * 4;
    unsigned short hh[4], ll[4];
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float val = (s0 + r <= trow) ? acc[r] : 0.f;   // causal mask inside the diagonal tiles
      rs += val;
      split16<T>(val, hh[r], ll[r]);
    }
    *reinterpret_cast<uint2*>(L.sAh + trow * LDA + s0) = pack4(hh);
    *reinterpret_cast<uint2*>(L.sAl + trow * LDA + s0) = pack4(ll);
    rs = xor32_sum(xor16_sum(rs));
    if (lg == 0) L.sDenP[trow * DSL + jb] = rs;            // one writer per (row, key block)
  }
  {
    // carry part of the denominators: phi(q_t) . (ksum + eps) over the (permuted) feature positions
    const int row = tid & (C - 1), part = tid / C;         // NPART parts x (FP / NPART) positions
    constexpr int PER = P::FP / NPART;
    const bool live = P::NTH / C == NPART || part < NPART;
    float s = 0.f;
    if constexpr (!STATE_ONLY)
    if (live)
#pragma unroll
    for (int g4 = 0; g4 < PER / 4; ++g4) {
      const int f = part * PER + g4 * 4;
      const uint2 qh = *reinterpret_cast<const uint2*>(sQh + row * LDQ2 + f);
      const uint2 ql = *reinterpret_cast<const uint2*>(sQl + row * LDQ2 + f);
      const float4 ks = *reinterpret_cast<const float4*>(L.sKsum + f);
      s = fmaf(S16<T>::val((unsigned short)(qh.x & 0xffff)) + S16<T>::val((unsigned short)(ql.x & 0xffff)), ks.x + 1e-6f, s);
      s = fmaf(S16<T>::val((unsigned short)(qh.x >> 16)) + S16<T>::val((unsigned short)(ql.x >> 16)), ks.y + 1e-6f, s);
      s = fmaf(S16<T>::val((unsigned short)(qh.y & 0xffff)) + S16<T>::val((unsigned short)(ql.y & 0xffff)), ks.z + 1e-6f, s);
      s = fmaf(S16<T>::val((unsigned short)(qh.y >> 16)) + S16<T>::val((unsigned short)(ql.y >> 16)), ks.w + 1e-6f, s);
    }
    if (live) L.sDenP[row * DSL + RB + part] = s;
    perf16_ksum_partial<T, P>(sKh, L.sKsP, wv, lane);
  }
}

// ---- first lines of (d): what a phase of its own (and its barrier) did in the first versions.  The k-sum takes this chunk's
// increments (perf16_ksum_fold: the partials of (c) read it before, the next chunk's (c) runs behind the next barrier), and
// every lane sums the denominator partials of ITS rows -- the same additions in the same order in every lane that holds the
// row, so nothing changes in the results.  (A lane sums ONE row -- lane group g the rows of block g % RB -- and the
// reciprocals travel by lane permutes: four rows and eight divisions per lane made the phase VALU-bound, 2.5 % slower than
// the barrier it replaces at 256 workgroups.)  dn[ib] = 1 / denominator of row ib*16 + li; ri1 = 1 / (absolute index + 1) of
// this lane's row; row0 = absolute index of the chunk's first row
template <class P>
__device__ __forceinline__ void perf16_denoms(const float* sDenP, int row0, int li, int lg, float (&dn)[P::RB], float& ri1) {
  const int myrow = (lg % P::RB) * 16 + li;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < P::DSL; ++i) s += sDenP[myrow * P::DSL + i];
  const float d1 = 1.0f / s;
  ri1 = 1.0f / (float)(row0 + myrow + 1);
#pragma unroll
  for (int ib = 0; ib < P::RB; ++ib) dn[ib] = __shfl(d1, ib * 16 + li);
}

// V fragments of column block jb (B operand, k = chunk row): rows 32ks + 8lg + {0..3 | 4..7}, columns 16 jb .. 16 jb + 15
template <class P>
__device__ __forceinline__ void perf16_v_frags(const unsigned short* sV, int jb, int li, int lg, uint4 (&vf)[P::C / 32]) {
  const int q = li >> 2, pp_ = li & 3;
#pragma unroll
  for (int ks = 0; ks < P::C / 32; ++ks) {
    const int r0 = ks * 32 + lg * 8;
    const uint2 a = lds_tr(sV + (r0 + q) * P::EL + P::vchunk(r0 + q, 2 * jb + (pp_ >> 1)) * 8 + 4 * (pp_ & 1));
    const uint2 b = lds_tr(sV + (r0 + 4 + q) * P::EL + P::vchunk(r0 + 4 + q, 2 * jb + (pp_ >> 1)) * 8 + 4 * (pp_ & 1));
    vf[ks] = cat8(a, b);
  }
}
// state pass: column total of a chunk of v = the last row's prefix
template <typename T, class P>
__device__ __forceinline__ void perf16_col_total(const uint4 (&vf)[P::C / 32], const uint4 (&tril)[P::RB][P::C / 32], float (&csum)[4], int lane) {
  f4 cum = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks <= (P::RB - 1) / 2; ++ks) cum = S16<T>::mfma(vf[ks], tril[P::RB - 1][ks], cum);
#pragma unroll
  for (int r = 0; r < 4; ++r) csum[r] += __shfl(cum[r], (lane & 48) | 15);
}

// ---- (d) O = A V + phi(Q) S over one 16-column block (e0 = its first column), divided by the denominators and stored; on the v
// columns (`avg`, wave-uniform) the cumulative average and, when the chunk enters the state (`upd`), its column totals.
// Every product has its operands SWAPPED (O^T = V^T A^T + S^T phi(Q)^T; the A and B fragment layouts are mirror images, so the
// same registers serve): the accumulator of query block ib then holds, per lane, row ib*16 + li and the FOUR CONSECUTIVE COLUMNS
// e0 + 4 lg + r -- results leave straight from the accumulators in 8-byte pieces, one denominator per block.
template <typename T, class P>
__device__ __forceinline__ void perf16_out_block(const uint4 (&vf)[P::C / 32], const f4 (&S)[P::NBT], float (&csum)[4], const float (&dn)[P::RB],
                                                 float ri1, const uint4 (&tril)[P::RB][P::C / 32], const unsigned short* set,
                                                 const unsigned short* sAh, __amdgpu_buffer_rsrc_t ro, __amdgpu_buffer_rsrc_t rg, int t0, int rows,
                                                 int lead, bool upd, bool avg, int e0, int lane, int li, int lg) {
  constexpr int D = P::D, C = P::C, NBT = P::NBT, RB = P::RB, KF = P::KF, LDQ2 = P::LDQ2, LDA = P::LDA;
  const unsigned short* sQh = set;
  const unsigned short* sQl = set + P::oQl;
  const unsigned short* sAl = sAh + C * LDA;
  f4 o[RB];
#pragma unroll
  for (int ib = 0; ib < RB; ++ib) o[ib] = f4{0.f, 0.f, 0.f, 0.f};
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
  // phi(Q) S: the state tiles, split, are the B operand; k-step kk pairs feature blocks 2kk and 2kk+1
#pragma unroll
  for (int kk = 0; kk < KF; ++kk) {
    unsigned short h0[4], h1[4], l0[4], l1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      split16<T>(S[2 * kk][r], h0[r], l0[r]);
      if (2 * kk + 1 < NBT) split16<T>(S[(2 * kk + 1 < NBT) ? 2 * kk + 1 : 0][r], h1[r], l1[r]);
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
    __builtin_amdgcn_raw_buffer_store_b64(bu2{w2.x, w2.y}, ro, (row < rows && t0 + row >= lead) ? ((t0 + row) * (3 * D) + col) * 2 : PERF16_OOB, 0, 0);
  }
  if (avg) {                                                 // wave-uniform: this wave's 16 columns are v features
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
      for (int r = 0; r < 4; ++r) g4[r] = S16<T>::bits((cum[ib][r] + csum[r]) * ri);
      const uint2 w2 = pack4(g4);
      __builtin_amdgcn_raw_buffer_store_b64(bu2{w2.x, w2.y}, rg, (row < rows && t0 + row >= lead) ? ((t0 + row) * D + gcol) * 2 : PERF16_OOB, 0, 0);
    }
    if (upd) {                                               // column totals of the chunk = its last row's prefix (lane li = 15)
#pragma unroll
      for (int r = 0; r < 4; ++r) csum[r] += __shfl(cum[RB - 1][r], (lane & 48) | 15);
    }
  }
}

// ---- (e) S[f][e] += sum_s phi(k_s)[f] V[s][e] for one column block: A operand = phi(K)^T by transposing reads of the row-major
// images.  Per tile: hi then lo, k-steps ascending.
template <class P>
__device__ __forceinline__ void perf16_phik_frag(const unsigned short* sKh, int rb, int ks, int li, int lg, uint4& kh, uint4& kl) {
  const unsigned short* sKl = sKh + P::C * P::LDK2;
  const int q = li >> 2, pp_ = li & 3;
  const int r0 = ks * 32 + lg * 8;
  const int co = (rb >> 1) * 32 + 8 * pp_ + (rb & 1) * 4;    // positions of features 16rb + 4p .. +3
  kh = cat8(lds_tr(sKh + (r0 + q) * P::LDK2 + co), lds_tr(sKh + (r0 + 4 + q) * P::LDK2 + co));
  kl = cat8(lds_tr(sKl + (r0 + q) * P::LDK2 + co), lds_tr(sKl + (r0 + 4 + q) * P::LDK2 + co));
}
template <typename T, class P>
__device__ __forceinline__ void perf16_state_update(const unsigned short* sKh, const uint4 (&vf)[P::C / 32], f4 (&S)[P::NBT], int li, int lg) {
#pragma unroll
  for (int rb = 0; rb < P::NBT; ++rb) {
#pragma unroll
    for (int ks = 0; ks < P::C / 32; ++ks) {
      uint4 kh, kl;
      perf16_phik_frag<P>(sKh, rb, ks, li, lg, kh, kl);
      S[rb] = S16<T>::mfma(kh, vf[ks], S[rb]);
      S[rb] = S16<T>::mfma(kl, vf[ks], S[rb]);
    }
  }
}

// ---- (d)(e) of one chunk in the output walks (and in the D = 64 state pass, which walks like them): every column block of the
// wave in turn
template <typename T, class P, bool STATE_ONLY>
__device__ __forceinline__ void perf16_phase_de(const Perf16Lds<P> L, const unsigned short* set, const Perf16Bufs B, int t0, int rows, int row_base,
                                                int lead, bool upd, bool want_avg, f4 (&S)[P::JB][P::NBT], float (&csum)[P::JB][4],
                                                const uint4 (&tril)[P::RB][P::C / 32], int tid, int wv, int lane, int li, int lg) {
  constexpr int C = P::C, NW = P::NW, EB = P::EB, JB = P::JB, RB = P::RB;
  perf16_ksum_fold<P>(L.sKsum, L.sKsP, tid, upd);
  float dn[RB], ri1 = 0.f;
  if constexpr (!STATE_ONLY) perf16_denoms<P>(L.sDenP, row_base + t0, li, lg, dn, ri1);
#pragma unroll
  for (int jq = 0; jq < JB; ++jq) {
    const int jb = wv + jq * NW;
    if (EB % NW != 0 && jb >= EB) break;                     // wave-uniform: no such column block
    uint4 vf[C / 32];
    perf16_v_frags<P>(L.sV, jb, li, lg, vf);
    const bool avg = want_avg && jb >= EB / 2;               // wave-uniform: this wave's 16 columns are v features
    if constexpr (STATE_ONLY) {
      if (avg) perf16_col_total<T, P>(vf, tril, csum[jq], lane);
    } else {
      perf16_out_block<T, P>(vf, S[jq], csum[jq], dn, ri1, tril, set, L.sAh, B.ro, B.rg, t0, rows, lead, upd, avg, jb * 16, lane, li, lg);
    }
    if (upd) perf16_state_update<T, P>(set + P::oKh, vf, S[jq], li, lg);
  }
}

}  // namespace sea
