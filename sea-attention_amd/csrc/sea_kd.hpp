// What the two sources of the distillation losses (include/sea_hip_train.h) share: sea_kd_loss.hip, the estimator's row
// kernels, and sea_kd_score_loss.hip, the tile kernels.
//   device  the pixel map of the estimator's loss: which of the T_M pixels key s of a causal row reads, and where a pixel's keys
//           begin, so that the row kernels and the tile kernel with the factored teacher place every key in the same pixel
//   host    the argument checks of the four entries, each written once, under the header's one rule: SEA_EINVAL for null
//           pointers, shapes that are not positive, bad strides, misalignment and a teacher given twice; SEA_EUNSUPPORTED for
//           what the kernels have no form for
#pragma once
#include "sea_common.hpp"

namespace sea {

constexpr int KD_MAX_TM = 512;
constexpr int KD_MAX_T = 16384;
constexpr int KS_TILE = 64;             // the tile kernels: swept indices per tile; also own indices per workgroup (4 waves x 16)

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

// ---- host: argument checks ------------------------------------------------------------------------------------------------------
struct KdArg { const char* name; const void* ptr; };
template <int K> inline int kd_check_nulls(const char* nm, const KdArg (&a)[K]) {
  for (const KdArg& t : a) SEA_REQUIRE(t.ptr, SEA_EINVAL, "%s: %s is null", nm, t.name);
  return SEA_OK;
}

// a dtype code (argument `arg`, holding `what`); `f32`: the kernels take fp32 there
inline int kd_check_dtype(const char* nm, const char* arg, const char* what, int code, bool f32) {
  SEA_REQUIRE(f32 || code != SEA_F32, SEA_EUNSUPPORTED, "%s: fp32 %s (%s) is outside the kernels: 16-bit data only", nm, what, arg);
  SEA_REQUIRE(code == SEA_F32 || code == SEA_F16 || code == SEA_BF16, SEA_EUNSUPPORTED, "%s: unknown %s %d", nm, arg, code);
  return SEA_OK;
}

// N, H, T and the grid of a kernel whose workgroups take `block_rows` rows each
inline int kd_check_shape(const char* nm, int64_t N, int64_t H, int64_t T, int block_rows) {
  SEA_REQUIRE(N > 0 && H > 0 && T > 0, SEA_EINVAL, "%s: bad shape N=%lld H=%lld T=%lld", nm, (long long)N, (long long)H,
              (long long)T);
  SEA_REQUIRE(T <= KD_MAX_T, SEA_EUNSUPPORTED, "%s: T=%lld (needs T <= %d)", nm, (long long)T, KD_MAX_T);
  SEA_REQUIRE(N * H * ((T + block_rows - 1) / block_rows) < (1ll << 31), SEA_EUNSUPPORTED, "%s: grid too large", nm);
  return SEA_OK;
}
inline int kd_check_tm(const char* nm, int64_t T_m) {
  SEA_REQUIRE(T_m > 0, SEA_EINVAL, "%s: bad shape T_m=%lld", nm, (long long)T_m);
  SEA_REQUIRE(T_m % 4 == 0 && T_m <= KD_MAX_TM, SEA_EUNSUPPORTED, "%s: T_m=%lld (needs T_m %% 4 == 0 and T_m <= %d)", nm,
              (long long)T_m, KD_MAX_TM);
  return SEA_OK;
}
inline int kd_check_head(const char* nm, int64_t D) {
  SEA_REQUIRE(D > 0, SEA_EINVAL, "%s: bad shape D=%lld", nm, (long long)D);
  SEA_REQUIRE(D == 64 || D == 80 || D == 128, SEA_EUNSUPPORTED, "%s: D=%lld (needs D in {64, 80, 128})", nm, (long long)D);
  return SEA_OK;
}

// A tensor read in rows of `row` elements of `dtype` through strides {n, h, t}: est, truth, q, k, teacher_q, teacher_k alike.
// The kernels load 16-byte chunks, so the base pointer and every stride are 16-byte aligned; the innermost stride is 1, so rows
// cannot be closer than `row`
struct KdRows { const char* name; const void* ptr; const int64_t* s; int64_t row; int dtype; };
template <int K> inline int kd_check_rows(const char* nm, const KdRows (&a)[K]) {
  for (const KdRows& t : a) {
    const int vec = t.dtype == SEA_F32 ? 4 : 8;
    SEA_REQUIRE(t.s[0] >= 0 && t.s[1] >= 0 && t.s[2] >= t.row, SEA_EINVAL, "%s: bad %s strides {%lld, %lld, %lld} for rows of %lld",
                nm, t.name, (long long)t.s[0], (long long)t.s[1], (long long)t.s[2], (long long)t.row);
    SEA_REQUIRE(((uintptr_t)t.ptr & 15) == 0 && t.s[0] % vec == 0 && t.s[1] % vec == 0 && t.s[2] % vec == 0, SEA_EINVAL,
                "%s: %s rows must be 16-byte aligned (base pointer and every stride)", nm, t.name);
  }
  return SEA_OK;
}

// The teacher of t1, t3 and t4, given exactly one way: truth (N,H,T,T), or -- truth == NULL -- teacher_q, teacher_k (N,H,T,D).
// Arguments of the form that is not given are not looked at.  `student_dtype`: what a factored teacher must agree with, < 0
// for none (t1).  Call it after the shape checks: it ends with the rows of T or D elements
inline int kd_check_teacher(const char* nm, const void* truth, int truth_dtype, const int64_t* truth_strides, const void* tq,
                            const void* tk, int teacher_dtype, const int64_t* tq_strides, const int64_t* tk_strides,
                            int student_dtype, int64_t T, int64_t D) {
  if (truth) {
    SEA_REQUIRE(!tq && !tk && !tq_strides && !tk_strides, SEA_EINVAL,
                "%s: the teacher is given twice: with truth, teacher_q, teacher_k and their strides must be null", nm);
    SEA_REQUIRE(truth_strides, SEA_EINVAL, "%s: truth_strides is null", nm);
    const int rc = kd_check_dtype(nm, "truth_dtype", "truth", truth_dtype, true);
    if (rc != SEA_OK) return rc;
    return kd_check_rows(nm, {KdRows{"truth", truth, truth_strides, T, truth_dtype}});
  }
  SEA_REQUIRE(tq, SEA_EINVAL, "%s: teacher_q is null, and truth is null too: give the teacher as truth or as teacher_q, teacher_k",
              nm);
  int rc = kd_check_nulls(nm, {KdArg{"teacher_k", tk}, {"teacher_q_strides", tq_strides}, {"teacher_k_strides", tk_strides}});
  if (rc != SEA_OK) return rc;
  rc = kd_check_dtype(nm, "teacher_dtype", "teacher q / k", teacher_dtype, false);
  if (rc != SEA_OK) return rc;
  SEA_REQUIRE(student_dtype < 0 || teacher_dtype == student_dtype, SEA_EUNSUPPORTED,
              "%s: teacher_dtype %d is not qk_dtype %d (the teacher's q / k must have the student's type)", nm, teacher_dtype,
              student_dtype);
  return kd_check_rows(nm,
                       {KdRows{"teacher_q", tq, tq_strides, D, teacher_dtype}, {"teacher_k", tk, tk_strides, D, teacher_dtype}});
}

// t1 with the factored teacher, arguments checked: clears pix_tgt on `s` and launches the tile kernel (sea_kd_score_loss.hip)
int kdq_launch_fwd(const char* nm, const void* est, int est_dtype, const int64_t* est_strides, const void* tq, const void* tk,
                   int teacher_dtype, const int64_t* tq_strides, const int64_t* tk_strides, int64_t N, int64_t H, int64_t T,
                   int64_t T_m, int64_t D, float* row_kl, float* row_mse, float* pix_tgt, float* row_stats, hipStream_t s);

}  // namespace sea
