// The pixel map of the estimator's distillation loss (include/sea_hip_train.h t1): which of the T_M pixels key s of a causal row
// reads, and where a pixel's keys begin.  Shared by the row kernels (sea_kd_loss.hip) and the tile kernel with the factored
// teacher (sea_kd_score_loss.hip), so that both place every key in the same pixel.
#pragma once
#include "sea_common.hpp"

namespace sea {

constexpr int KD_MAX_TM = 512;
constexpr int KD_MAX_T = 16384;

// pixel of key s in a row of `len` = t + 1 keys: ops/resize_dense.py, fp32 with IEEE operations (rank = s + 1, no padding)
__device__ inline int kd_pix(int s, float len, float tm, int T_M) {
  const float v = __fsub_rn(__fmul_rn(__fdiv_rn(__fsub_rn((float)(s + 1), 0.5f), len), tm), 1e-4f);
  const int p = (int)floorf(v);
  return p < 0 ? 0 : (p > T_M ? T_M : p);
}
// first key of pixel b: the least s in 0 .. t + 1 with s == t + 1 or pix(s) >= b.  pix is non-decreasing in s (every operation
// in it is), so pixel b holds the keys first(b) .. first(b + 1) - 1.  The guess inverts the formula in real numbers; the two
// loops settle it against the fp32 formula itself (a step or two).
__device__ inline int kd_first(int b, int t, float len, float tm, int T_M) {
  if (b >= T_M) return t + 1;
  const float g = ceilf(((float)b + 1e-4f) * len / tm - 0.5f);
  int s = g < 0.f ? 0 : (g > len ? t + 1 : (int)g);
  while (s > 0 && kd_pix(s - 1, len, tm, T_M) >= b) --s;
  while (s <= t && kd_pix(s, len, tm, T_M) < b) ++s;
  return s;
}

}  // namespace sea
