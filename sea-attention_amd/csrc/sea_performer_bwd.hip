// Backward of the causal Performer (sea_performer_causal), gfx950: include/sea_hip_estimator_grad.h, entry g1.
//
// Nothing of the forward is saved.  With a = phi(q), b = phi(k), V = [pos | v] (E = 2D wide), S / z the running state and k-sum
// BEFORE a chunk, G = g[:E] / den, e = -(g[:E] . num) / den^2 (the gradient of the column of ones that carries the denominator):
//   per chunk of C rows        A = tril(a b^T)                 B = tril(G V^T + e 1^T)
//   forward sweep   (S, z)     da = B b + G S^T + e (z + 1e-6)^T          then  S += b^T V,  z += sum b
//   reverse sweep   (R, r)     dV = A^T G + b R,   db = B^T a + V R^T + 1 r^T      then  R += a^T G,  r += a^T e
//   dq = s (da (.) [q W^T > 0]) W,  dk likewise,  dv = dV[:, D:] + g[:, E:],  dpos = sum over (n, h) of dV[:, :D]
// Two launches of one 512-thread workgroup (8 waves) per (n, h): performer_bwd_fwd_sweep walks the chunks upwards, computes den
// and num again, writes dq and the two row scalars 1 / den and g . ctx / den to the workspace; performer_bwd_rev_sweep walks them
// downwards from the partial chunk, reads the scalars, writes dk, dv and this pair's part of dpos.  performer_bwd_dpos adds the
// parts in the order of (n, h).  No atomics.  Every product is fp32 on v_mfma_f32_16x16x4_f32; 16-bit data is widened on load.
//
// LDS plan (D = 64, C = 64, NBP = 16 NBT features, fp32; bytes at NBT = 5 / 3), DESIGN 5.10:
//   state   NBP x 132   42240 / 25344    S (forward sweep) or R (reverse sweep), resident for the whole walk
//   P       64 x max(NBP + 4, 68)  21504 / 17408    a; then the B tile (forward) ; then the masked da
//   Kf      same                                      b; then the B tile (reverse)
//   V       64 x 132    33792            Q and K staging (2 x 64 x 66); V; the A tile and then the masked db (reverse)
//   G       64 x 132    33792            W (NBP x 68) across the chunk boundary; the A tile (forward); G
//   small   z or r, 1 / den, e, two 64 x 8 partial-sum tables, the ReLU masks (one 64-bit ballot per tile register)
// 158400 bytes at NBT = 5, 130752 at NBT = 3: one workgroup per CU either way.  A padded feature and a padded row of the last
// chunk are ZERO in a and b (their phi would be 1e-3), G, e and V of a padded row are zero, and the masks are clear there.
//
// The kernels and the refusals are in sea_performer_bwd.hpp, shared with the row-segmented form of sea_performer_bwd_seg.hip
// (entry s1); this file instantiates the one-segment sweeps and launches them.
#include "sea_performer_bwd.hpp"

namespace sea {
namespace {

template <typename T, int NBT>
int launch_bwd(const PerfBwdParams& p, int64_t pairs, hipStream_t s) {
  using P = PerfBwdPlan<NBT>;
  static DevOnce once;
  if (once.first()) {
    SEA_MAX_LDS((performer_bwd_fwd_sweep<T, NBT>), P::lds_bytes);
    SEA_MAX_LDS((performer_bwd_rev_sweep<T, NBT>), P::lds_bytes);
  }
  hipLaunchKernelGGL((performer_bwd_fwd_sweep<T, NBT>), dim3((unsigned)pairs), dim3(512), P::lds_bytes, s, p, PerfBwdSeg{});
  hipLaunchKernelGGL((performer_bwd_rev_sweep<T, NBT>), dim3((unsigned)pairs), dim3(512), P::lds_bytes, s, p, PerfBwdSeg{});
  return SEA_OK;
}

template <typename T>
int launch_bwd_nbt(const PerfBwdParams& p, int64_t pairs, hipStream_t s) {
  return p.nb <= 48 ? launch_bwd<T, 3>(p, pairs, s) : launch_bwd<T, 5>(p, pairs, s);
}

}  // namespace
}  // namespace sea

using namespace sea;

extern "C" int sea_estimator_grad_version(void) { return SEA_ESTIMATOR_GRAD_ABI_VERSION; }

extern "C" int sea_performer_causal_bwd_supported(int64_t D, int64_t nb, int dtype) { return bwd_supported(D, nb, dtype) ? 1 : 0; }

extern "C" int64_t sea_performer_causal_bwd_workspace_bytes(int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb, int dtype) {
  if (N <= 0 || H <= 0 || T <= 0 || !bwd_supported(D, nb, dtype)) return 0;
  return rowstat_bytes(N, H, T) + align16(N * H * T * D * (int64_t)sizeof(float));
}

extern "C" int sea_performer_causal_bwd(const void* q, const void* k, const void* v, const void* pos, int dtype, const float* proj,
                                        int64_t N, int64_t H, int64_t T, int64_t D, int64_t nb,
                                        const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                        int64_t pos_stride, const void* grad_out, void* d_q, void* d_k, void* d_v, float* d_pos,
                                        void* workspace, int64_t workspace_bytes, sea_stream_t stream) {
  const char* nm = "sea_performer_causal_bwd";
  PerfBwdParams p;
  const int ok = bwd_prepare(nm, sea_performer_causal_bwd_workspace_bytes(N, H, T, D, nb, dtype), q, k, v, pos, dtype, proj, N, H, T, D,
                             nb, q_strides, k_strides, v_strides, pos_stride, grad_out, d_q, d_k, d_v, d_pos, workspace,
                             workspace_bytes, p);
  if (ok != SEA_OK) return ok;
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == SEA_F32 ? launch_bwd_nbt<float>(p, N * H, s)
               : dtype == SEA_F16 ? launch_bwd_nbt<__half>(p, N * H, s) : launch_bwd_nbt<__hip_bfloat16>(p, N * H, s);
  if (rc != SEA_OK) return rc;
  SEA_CHECK_LAUNCH(nm);
  const int64_t TD = T * D;
  hipLaunchKernelGGL(performer_bwd_dpos, dim3((unsigned)((TD + 255) / 256)), dim3(256), 0, s, p.dpos_part, d_pos, N * H, TD);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}
