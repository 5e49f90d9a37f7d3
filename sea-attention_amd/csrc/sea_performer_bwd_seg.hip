// Row-segmented backward of the causal Performer, gfx950: include/sea_hip_estimator_grad_seg.h, entry s1; DESIGN 5.10a.
//
// sea_performer_bwd.hip runs one workgroup per (n, h) in each sweep: with one sequence per GPU that is 12 .. 32 workgroups on 256
// CUs.  Here the rows of a pair are cut into Sg segments of whole chunks and both sweeps (the kernels of sea_performer_bwd.hpp,
// SEG = true) run on the grid (N H, Sg).  What a segment's sweep starts from is a sum over the segments before it (S, z) or after
// it (R, r).  performer_bwd_seg_state computes each segment's own part of that sum ahead of the sweep, the sweep's prologue adds
// the parts in one order (load_carry):
//   1  seg_state<REV = false>  (N H, Sg - 1)   dS_j = sum b^T V, dz_j = sum b           segments 0 .. Sg-2
//   2  fwd_sweep<SEG>          (N H, Sg)       from S = sum_{j' < j} dS_j', ascending; writes dq and the row scalars
//   3  seg_state<REV = true>   (N H, Sg - 1)   dR_j = sum a^T G, dr_j = sum a^T e        segments 1 .. Sg-1, from the row scalars
//   4  rev_sweep<SEG>          (N H, Sg)       from R = sum_{j' > j} dR_j', descending; writes dk, dv, the dpos parts
//   5  performer_bwd_dpos
// No atomics, no waiting between workgroups: every dependency is a launch boundary.  The state kernel has a plan of its own: it
// needs phi of ONE of q / k and one product per chunk, none of the A / B tiles, so the NBP x E sum stays in accumulators (wave wv
// owns column block wv: NBT f4 registers) and the LDS holds W, the feature map and one 64 x 132 tile -- 77568 / 60672 bytes at
// NBT = 5 / 3, at most 68 VGPRs: two workgroups per CU.  Compiled without packed fp32 arithmetic (_build.FILE_FLAGS).
#include "sea_performer_bwd.hpp"

namespace sea {
namespace {

// ---- a segment's own part of the state: no A / B / G tiles, the sum in accumulators -------------------------------------
// LDS (fp32; bytes at NBT = 5 / 3): W NBP x 68 (21760 / 13056) resident; F 64 x (NBP + 4) (21504 / 13312) the feature map;
// Y 64 x 132 (33792) the staged rows of q or k (64 x 66), then V or G; 1 / den and e.  77568 / 60672 bytes: two workgroups per CU.
template <int NBT>
struct PerfBwdStatePlan {
  using P = PerfBwdPlan<NBT>;
  static constexpr int oW = 0, oF = oW + P::NBP * P::LDW, oY = oF + P::C * P::LDP, oInv = oY + P::C * P::LDV, oE = oInv + P::C;
  static constexpr int lds_bytes = (oE + P::C) * 4;
  static_assert(P::C * P::LDX <= P::C * P::LDV, "the staged rows lie in the Y region");
  static_assert(2 * lds_bytes <= 160 * 1024, "two workgroups per CU");
};

// phi of ONE staged matrix (64 x LDX) -> dst (64 x LDP): wave wv owns row block wv & 3 and the feature blocks of its parity.
// Element for element the sums of feature_maps, so a and b here are bitwise those of the sweeps.
template <int NBT>
__device__ inline void feature_map_one(const float* src, const float* sW, float* dst, int rows, int nb, float cnorm) {
  using P = PerfBwdPlan<NBT>;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  const int ib = wv & 3, half = wv >> 2;
  constexpr int NJ = (NBT + 1) / 2;
  f4 acc[NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) acc[i] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int ks = 0; ks < P::D / 4; ++ks) {
    const float a = src[(ib * 16 + li) * P::LDX + ks * 4 + lg];
#pragma unroll
    for (int i = 0; i < NJ; ++i)
      if (half + 2 * i < NBT) acc[i] = SEA_BWD_MFMA(a, sW[((half + 2 * i) * 16 + li) * P::LDW + ks * 4 + lg], acc[i]);
  }
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    const int col = (half + 2 * i) * 16 + li;
    if (half + 2 * i < NBT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ib * 16 + lg * 4 + r;
        dst[row * P::LDP + col] = (col < nb && row < rows) ? fmaxf(cnorm * acc[i][r], 0.f) + 1e-3f : 0.f;
      }
    }
  }
}

// REV = false: dS = sum b^T V, dz = sum b over segment blockIdx.y (0 .. Sg-2).  REV = true: dR = sum a^T G, dr = sum a^T e over
// segment blockIdx.y + 1, chunks downwards as the reverse sweep takes them.  Wave wv keeps column block wv of the NBP x E sum in
// NBT accumulators (20 registers at NBT = 5) for the whole walk; thread f < NBP keeps element f of the vector.
template <typename T, int NBT, bool REV>
__global__ __launch_bounds__(512) void performer_bwd_seg_state(PerfBwdParams p, PerfBwdSeg sg) {
  using P = PerfBwdPlan<NBT>;
  using L = PerfBwdStatePlan<NBT>;
  constexpr int D = P::D, E = P::E, C = P::C, NBP = P::NBP, LDP = P::LDP, LDV = P::LDV;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *sW = smem + L::oW, *sF = smem + L::oF, *sY = smem + L::oY, *sInv = smem + L::oInv, *sE = smem + L::oE;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int nh = blockIdx.x, n = nh / p.H, h = nh - n * p.H, T_ = p.T, j = (int)blockIdx.y + (REV ? 1 : 0);
  const int64_t* xs = REV ? p.qs : p.ks;
  const T* xb = reinterpret_cast<const T*>(REV ? p.q : p.k) + n * xs[0] + h * xs[1];
  const T* vb = reinterpret_cast<const T*>(p.v) + n * p.vs[0] + h * p.vs[1];
  const T* pb = reinterpret_cast<const T*>(p.pos);
  const T* gb = reinterpret_cast<const T*>(p.g) + (int64_t)nh * T_ * (3 * D);
  const float* rs = p.rowstat + (int64_t)nh * T_ * 2;
  const float cnorm = powf((float)D, -0.25f);
  auto one = [](int) { return 1.f; };
  const int t_lo = j * sg.cps * C, t_hi = min(T_, t_lo + sg.cps * C);

  f4 acc[NBT];
#pragma unroll
  for (int fb = 0; fb < NBT; ++fb) acc[fb] = f4{0.f, 0.f, 0.f, 0.f};
  float vec = 0.f;
  stage_w<NBT>(sW, p.W, p.nb);                                       // the first barrier of the walk stands behind it
  for (int c = 0; c < (t_hi - t_lo + C - 1) / C; ++c) {
    const int t0 = REV ? ((t_hi - 1) / C - c) * C : t_lo + c * C;
    const int rows = min(C, T_ - t0);
    stage_rows<T>(sY, P::LDX, xb, xs[2], t0, rows, D, one);
    if (REV && tid < C) {
      sInv[tid] = (tid < rows) ? rs[(int64_t)(t0 + tid) * 2] : 0.f;
      sE[tid] = (tid < rows) ? -rs[(int64_t)(t0 + tid) * 2 + 1] : 0.f;
    }
    __syncthreads();
    feature_map_one<NBT>(sY, sW, sF, rows, p.nb, cnorm);
    __syncthreads();
    if (REV) {
      stage_rows<T>(sY, LDV, gb, 3 * D, t0, rows, E, [&](int r) { return sInv[r]; });
    } else {
      stage_rows<T>(sY, LDV, pb, p.pos_stride, t0, rows, D, one);
      stage_rows<T>(sY + D, LDV, vb, p.vs[2], t0, rows, D, one);
    }
    __syncthreads();
#pragma unroll 4
    for (int ks = 0; ks < C / 4; ++ks) {
      const float y = sY[(ks * 4 + lg) * LDV + wv * 16 + li];
#pragma unroll
      for (int fb = 0; fb < NBT; ++fb) acc[fb] = SEA_BWD_MFMA(sF[(ks * 4 + lg) * LDP + fb * 16 + li], y, acc[fb]);
    }
    if (tid < NBP)
      for (int r = 0; r < C; ++r) vec = REV ? fmaf(sF[r * LDP + tid], sE[r], vec) : vec + sF[r * LDP + tid];
    __syncthreads();                                                 // the next chunk's rows go where V or G is read
  }
  float* out = (REV ? sg.rev : sg.fwd) + ((int64_t)nh * sg.Sg + j) * P::CARRY;
#pragma unroll
  for (int fb = 0; fb < NBT; ++fb)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(fb * 16 + lg * 4 + r) * E + wv * 16 + li] = acc[fb][r];
  if (tid < NBP) out[NBP * E + tid] = vec;
}

// the four launches, each behind the one it reads from on the stream
template <typename T, int NBT>
int launch_bwd_seg(const PerfBwdParams& p, const PerfBwdSeg& sg, int64_t pairs, hipStream_t s) {
  using P = PerfBwdPlan<NBT>;
  using L = PerfBwdStatePlan<NBT>;
  static DevOnce once;
  if (once.first()) {
    SEA_MAX_LDS((performer_bwd_seg_state<T, NBT, false>), L::lds_bytes);
    SEA_MAX_LDS((performer_bwd_seg_state<T, NBT, true>), L::lds_bytes);
    SEA_MAX_LDS((performer_bwd_fwd_sweep<T, NBT, true>), P::lds_bytes);
    SEA_MAX_LDS((performer_bwd_rev_sweep<T, NBT, true>), P::lds_bytes);
  }
  const dim3 all((unsigned)pairs, (unsigned)sg.Sg), but_one((unsigned)pairs, (unsigned)(sg.Sg - 1));
  hipLaunchKernelGGL((performer_bwd_seg_state<T, NBT, false>), but_one, dim3(512), L::lds_bytes, s, p, sg);
  hipLaunchKernelGGL((performer_bwd_fwd_sweep<T, NBT, true>), all, dim3(512), P::lds_bytes, s, p, sg);
  hipLaunchKernelGGL((performer_bwd_seg_state<T, NBT, true>), but_one, dim3(512), L::lds_bytes, s, p, sg);
  hipLaunchKernelGGL((performer_bwd_rev_sweep<T, NBT, true>), all, dim3(512), P::lds_bytes, s, p, sg);
  return SEA_OK;
}

template <typename T>
int launch_bwd_seg_nbt(const PerfBwdParams& p, const PerfBwdSeg& sg, int64_t pairs, hipStream_t s) {
  return p.nb <= 48 ? launch_bwd_seg<T, 3>(p, sg, pairs, s) : launch_bwd_seg<T, 5>(p, sg, pairs, s);
}

// the rule of the header: chunks per segment for a request, and the count that leaves no segment empty
int64_t seg_chunks(int64_t T, int64_t requested) {
  const int64_t nc = (T + 63) / 64, r = std::max<int64_t>(1, std::min(requested, nc));
  return (nc + r - 1) / r;
}
int64_t seg_count(int64_t T, int64_t requested) {
  const int64_t nc = (T + 63) / 64, cps = seg_chunks(T, requested);
  return (nc + cps - 1) / cps;
}
int64_t carry_floats(int64_t nb) { return nb <= 48 ? PerfBwdPlan<3>::CARRY : PerfBwdPlan<5>::CARRY; }

}  // namespace
}  // namespace sea

using namespace sea;

extern "C" int sea_estimator_grad_seg_version(void) { return SEA_ESTIMATOR_GRAD_SEG_ABI_VERSION; }

extern "C" int64_t sea_performer_causal_bwd_seg_count(int64_t T, int64_t requested) {
  return T < 1 || requested < 1 ? 0 : seg_count(T, requested);
}

extern "C" int64_t sea_performer_causal_bwd_seg_workspace_bytes(int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb, int dtype,
                                                                int64_t segments) {
  const int64_t base = sea_performer_causal_bwd_workspace_bytes(N, H, T, D, nb, dtype);
  if (base == 0 || segments < 1) return 0;
  return base + align16(2 * N * H * seg_count(T, segments) * carry_floats(nb) * (int64_t)sizeof(float));
}

extern "C" int sea_performer_causal_bwd_seg(const void* q, const void* k, const void* v, const void* pos, int dtype, const float* proj,
                                            int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb,
                                            const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                            int64_t pos_stride, const void* grad_out, void* d_q, void* d_k, void* d_v, float* d_pos,
                                            int64_t segments, void* workspace, int64_t workspace_bytes, sea_stream_t stream) {
  const char* nm = "sea_performer_causal_bwd_seg";
  SEA_REQUIRE(segments >= 1, SEA_EINVAL, "%s: segments=%lld must be at least 1", nm, (long long)segments);
  PerfBwdParams p;
  const int ok = bwd_prepare(nm, sea_performer_causal_bwd_seg_workspace_bytes(N, H, T, D, nb, dtype, segments), q, k, v, pos, dtype,
                             proj, N, H, T, D, nb, q_strides, k_strides, v_strides, pos_stride, grad_out, d_q, d_k, d_v, d_pos,
                             workspace, workspace_bytes, p);
  if (ok != SEA_OK) return ok;
  const int64_t Sg = seg_count(T, segments);
  SEA_REQUIRE(Sg <= 65535, SEA_EUNSUPPORTED, "%s: %lld segments are beyond the grid (65535)", nm, (long long)Sg);
  if (Sg == 1)                                                       // exactly the launches of entry g1, from its own code
    return sea_performer_causal_bwd(q, k, v, pos, dtype, proj, N, H, T, D, nb, q_strides, k_strides, v_strides, pos_stride, grad_out,
                                    d_q, d_k, d_v, d_pos, workspace, workspace_bytes, stream);
  PerfBwdSeg sg;
  sg.fwd = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + sea_performer_causal_bwd_workspace_bytes(N, H, T, D, nb, dtype));
  sg.rev = sg.fwd + N * H * Sg * carry_floats(nb);
  sg.cps = (int)seg_chunks(T, segments); sg.Sg = (int)Sg;
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == SEA_F32 ? launch_bwd_seg_nbt<float>(p, sg, N * H, s)
               : dtype == SEA_F16 ? launch_bwd_seg_nbt<__half>(p, sg, N * H, s) : launch_bwd_seg_nbt<__hip_bfloat16>(p, sg, N * H, s);
  if (rc != SEA_OK) return rc;
  SEA_CHECK_LAUNCH(nm);
  const int64_t TD = T * D;
  hipLaunchKernelGGL(performer_bwd_dpos, dim3((unsigned)((TD + 255) / 256)), dim3(256), 0, s, p.dpos_part, d_pos, N * H, TD);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}
