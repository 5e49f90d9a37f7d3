// Glue of a graph-replayed decoding step (perlin_attention/decode.py; reference loop: src/main/opt_generate.py:131 ->
// the `use_cache` branches of perlin_attention/attention.py + attention_state.py:142-203).
//
// A position of the session is ~10 kernels of 4 - 25 us; the framework's own glue around them was eleven more launches
// of ~4.5 us each (three input copies, an index_copy_ into the caches, a cat + a copy for the CNN window, two counter
// adds, ...: 50 of a step's 130 us; after: profiles/r04b_decode_kernel_stats.csv).  Two kernels replace most of it:
//
//   decode_stage_kernel   copies the new q row into the static input buffer and writes the new k / v rows straight into the
//                         caches at the row the session's device-side counter names.  The only launch of a step whose
//                         arguments change (the caller's q / k / v): it runs eagerly in front of the replay.
//   c8_window_shift_kernel  the CNN window (N, rows, row) moved up by one row in place; a thread owns a 16-byte column of
//                         all rows and walks them top to bottom, so no thread reads what another one writes.  It is the
//                         LAST launch of a step and also advances the two counters (rows the state has seen, keys the next
//                         row sees): every reader of this step has finished (stream order), the next step's have not begun.
#include "sea_common.hpp"

namespace sea {

struct StageParams {
  const void *q, *k, *v;
  int64_t qs[2], ks[2], vs[2];       // element strides [n, h] of the (N, H, 1, D) inputs (feature stride 1)
  void* q_in;                        // (N, H, D) dense
  void* kv_cache;                    // (2, N, H, cap, D) dense
  const int32_t* ctr;                // [seen, tsrc] of THIS step: the new token's cache row is ctr[0]
  int N, H, D, cap;
};
// PAGED (sea_decode_stage_paged): kv_cache is a pool (2, pool_pages, H, page_rows, D); sequence n's logical row r lives in
// page table[n * table_stride + r / page_rows] at row r % page_rows (page_rows = 1 << page_shift).  A type of its own, so that
// the other forms' kernel arguments -- and code -- stay what they were
struct StagePagedParams : StageParams {
  const int32_t* table;
  int table_stride, page_shift, pool_pages;
};

// RAGGED: a counter pair per sequence, sequence n's at ctr + n * ctr_stride (read per item: the items of a workgroup span
// sequences); a sequence whose row lies outside the caches writes nothing.  PAGED (with RAGGED): the row goes to the page the
// sequence's block table names; a row without a page (an entry outside 0 .. pool_pages-1) writes nothing either
template <typename T, bool RAGGED, bool PAGED = false>
__global__ __launch_bounds__(256) void decode_stage_kernel(std::conditional_t<PAGED, StagePagedParams, StageParams> p, int ctr_stride) {
  static_assert(RAGGED || !PAGED, "the paged stage has a position per sequence");
  const int pos0 = p.ctr[0];
  if (!RAGGED && (pos0 < 0 || pos0 >= p.cap)) return;       // (the host mirrors the length and refuses before this can happen)
  const int rows = p.N * p.H;
  const int per = p.D / 8;                                   // 16-byte chunks per row (launcher: D % 8 == 0)
  const T* srcs[3] = {reinterpret_cast<const T*>(p.q), reinterpret_cast<const T*>(p.k), reinterpret_cast<const T*>(p.v)};
  const int64_t* strs[3] = {p.qs, p.ks, p.vs};
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < 3 * rows * per; c += gridDim.x * blockDim.x) {
    const int which = c / (rows * per);
    const int r = (c - which * rows * per) / per, j = c % per;
    const int n = r / p.H, h = r - n * p.H;
    const int pos = RAGGED ? p.ctr[n * ctr_stride] : pos0;
    if (RAGGED && which != 0 && (pos < 0 || pos >= p.cap)) continue;
    const uint4 val = *reinterpret_cast<const uint4*>(srcs[which] + n * strs[which][0] + h * strs[which][1] + j * 8);
    T* dst;
    if (which == 0) dst = reinterpret_cast<T*>(p.q_in) + (int64_t)r * p.D;
    else if constexpr (PAGED) {
      const int pg = p.table[(int64_t)n * p.table_stride + (pos >> p.page_shift)];
      if (pg < 0 || pg >= p.pool_pages) continue;
      const int prow = pos & ((1 << p.page_shift) - 1);
      dst = reinterpret_cast<T*>(p.kv_cache) + ((((int64_t)(which - 1) * p.pool_pages + pg) * p.H + h) * ((int64_t)1 << p.page_shift) + prow) * p.D;
    }
    else dst = reinterpret_cast<T*>(p.kv_cache) + (((int64_t)(which - 1) * rows + r) * p.cap + pos) * p.D;
    *reinterpret_cast<uint4*>(dst + j * 8) = val;
  }
}

__global__ __launch_bounds__(256) void c8_window_shift_kernel(uint4* xs, int rows, int64_t chunks_per_row, int64_t items_chunks,
                                                              int32_t* counters) {
  // xs (N, rows, chunks_per_row) in 16-byte chunks: xs[n, r] = xs[n, r + 1] for r < rows - 1
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid == 0 && counters != nullptr) { counters[0] += 1; counters[1] += 1; }
  if (gid >= items_chunks) return;
  const int64_t n = gid / chunks_per_row, c = gid - n * chunks_per_row;
  if (rows < 2) return;
  uint4* base = xs + n * rows * chunks_per_row + c;
  uint4 nxt = base[chunks_per_row];
  for (int r = 0; r + 1 < rows; ++r) {
    const uint4 cur = nxt;
    if (r + 2 < rows) nxt = base[(int64_t)(r + 2) * chunks_per_row];
    base[(int64_t)r * chunks_per_row] = cur;
  }
}

}  // namespace sea

using namespace sea;

static int decode_stage_entry(const char* nm, const void* q, const void* k, const void* v, int dtype, int64_t N, int64_t H,
                              int64_t D, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                              void* q_in, void* kv_cache, int64_t capacity, const int32_t* counters, int64_t counter_stride,
                              const int32_t* table, int64_t table_stride, int page_shift, int64_t pool_pages,
                              sea_stream_t stream) {
  SEA_REQUIRE(q && k && v && q_strides && k_strides && v_strides && q_in && kv_cache && counters, SEA_EINVAL, "%s: null pointer", nm);
  SEA_REQUIRE(dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: 16-bit data only (dtype %d)", nm, dtype);
  SEA_REQUIRE(N > 0 && H > 0 && D > 0 && capacity > 0 && N * H * D < (1ll << 24), SEA_EINVAL, "%s: bad shape", nm);
  SEA_REQUIRE(counter_stride >= 0 && counter_stride * N < (1ll << 31), SEA_EINVAL, "%s: bad counter stride %lld", nm,
              (long long)counter_stride);
  SEA_REQUIRE(D % 8 == 0, SEA_EUNSUPPORTED, "%s: D must be a multiple of 8 (16-byte rows)", nm);
  bool al = (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)q_in | (uintptr_t)kv_cache) & 15) == 0;
  for (int i = 0; i < 2; ++i) al = al && q_strides[i] % 8 == 0 && k_strides[i] % 8 == 0 && v_strides[i] % 8 == 0;
  SEA_REQUIRE(al, SEA_EUNSUPPORTED, "%s: rows must be 16-byte aligned", nm);
  StagePagedParams p;
  p.q = q; p.k = k; p.v = v; p.q_in = q_in; p.kv_cache = kv_cache; p.ctr = counters;
  for (int i = 0; i < 2; ++i) { p.qs[i] = q_strides[i]; p.ks[i] = k_strides[i]; p.vs[i] = v_strides[i]; }
  p.N = (int)N; p.H = (int)H; p.D = (int)D; p.cap = (int)capacity;
  p.table = table; p.table_stride = (int)table_stride; p.page_shift = page_shift; p.pool_pages = (int)pool_pages;
  hipStream_t s = (hipStream_t)stream;
  const int64_t chunks = 3 * N * H * (D / 8);
  const unsigned blocks = (unsigned)((chunks + 255) / 256 > 1024 ? 1024 : (chunks + 255) / 256);
  const int cs = (int)counter_stride;
  const StageParams b = p;                                   // (the unpaged forms' arguments)
  if (table) {
    if (dtype == SEA_F16) hipLaunchKernelGGL((decode_stage_kernel<__half, true, true>), dim3(blocks), dim3(256), 0, s, p, cs);
    else hipLaunchKernelGGL((decode_stage_kernel<__hip_bfloat16, true, true>), dim3(blocks), dim3(256), 0, s, p, cs);
  } else if (dtype == SEA_F16) {
    if (cs) hipLaunchKernelGGL((decode_stage_kernel<__half, true>), dim3(blocks), dim3(256), 0, s, b, cs);
    else hipLaunchKernelGGL((decode_stage_kernel<__half, false>), dim3(blocks), dim3(256), 0, s, b, 0);
  } else {
    if (cs) hipLaunchKernelGGL((decode_stage_kernel<__hip_bfloat16, true>), dim3(blocks), dim3(256), 0, s, b, cs);
    else hipLaunchKernelGGL((decode_stage_kernel<__hip_bfloat16, false>), dim3(blocks), dim3(256), 0, s, b, 0);
  }
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}

extern "C" int sea_decode_stage(const void* q, const void* k, const void* v, int dtype, int64_t N, int64_t H, int64_t D,
                                const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                void* q_in, void* kv_cache, int64_t capacity, const int32_t* counters, sea_stream_t stream) {
  return decode_stage_entry("sea_decode_stage", q, k, v, dtype, N, H, D, q_strides, k_strides, v_strides, q_in, kv_cache, capacity,
                            counters, 0, nullptr, 0, 0, 0, stream);
}

// per-sequence positions: sequence n's new row goes to cache row counters[n * counter_stride] (counter_stride >= 1)
extern "C" int sea_decode_stage_ragged(const void* q, const void* k, const void* v, int dtype, int64_t N, int64_t H, int64_t D,
                                       const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                       void* q_in, void* kv_cache, int64_t capacity, const int32_t* counters,
                                       int64_t counter_stride, sea_stream_t stream) {
  const char* nm = "sea_decode_stage_ragged";
  SEA_REQUIRE(counter_stride > 0, SEA_EINVAL, "%s: counter_stride must be >= 1 (got %lld)", nm, (long long)counter_stride);
  return decode_stage_entry(nm, q, k, v, dtype, N, H, D, q_strides, k_strides, v_strides, q_in, kv_cache, capacity, counters,
                            counter_stride, nullptr, 0, 0, 0, stream);
}

// paged K / V: sequence n's new rows go to page block_table[n * table_stride + ctr / page_rows] of the pool
// (2, pool_pages, H, page_rows, D), row ctr % page_rows
extern "C" int sea_decode_stage_paged(const void* q, const void* k, const void* v, int dtype, int64_t N, int64_t H, int64_t D,
                                      const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                      void* q_in, void* kv_pool, int64_t capacity, const int32_t* counters,
                                      int64_t counter_stride, const int32_t* block_table, int64_t table_stride,
                                      int64_t page_rows, int64_t pool_pages, sea_stream_t stream) {
  const char* nm = "sea_decode_stage_paged";
  SEA_REQUIRE(counter_stride > 0, SEA_EINVAL, "%s: counter_stride must be >= 1 (got %lld)", nm, (long long)counter_stride);
  SEA_REQUIRE(block_table, SEA_EINVAL, "%s: null pointer", nm);
  SEA_REQUIRE(dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: 16-bit data only (dtype %d)", nm, dtype);
  if (int e = paged_layout_check(nm, dtype, D, capacity, page_rows, table_stride, N)) return e;
  SEA_REQUIRE(pool_pages > 0 && 2 * pool_pages * H * page_rows * D < (1ll << 62) && pool_pages < (1ll << 31), SEA_EINVAL,
              "%s: bad pool of %lld pages", nm, (long long)pool_pages);
  return decode_stage_entry(nm, q, k, v, dtype, N, H, D, q_strides, k_strides, v_strides, q_in, kv_pool, capacity, counters,
                            counter_stride, block_table, table_stride, __builtin_ctzll(page_rows), pool_pages, stream);
}

extern "C" int sea_c8_window_shift(void* xs, int64_t N, int64_t rows, int64_t row_bytes, int32_t* counters, sea_stream_t stream) {
  const char* nm = "sea_c8_window_shift";
  SEA_REQUIRE(xs, SEA_EINVAL, "%s: null pointer", nm);
  SEA_REQUIRE(N > 0 && rows > 0 && row_bytes > 0, SEA_EINVAL, "%s: bad shape", nm);
  SEA_REQUIRE(row_bytes % 16 == 0 && ((uintptr_t)xs & 15) == 0, SEA_EUNSUPPORTED, "%s: rows are whole 16-byte chunks", nm);
  const int64_t cpr = row_bytes / 16, total = N * cpr;
  SEA_REQUIRE(total < (1ll << 31), SEA_EUNSUPPORTED, "%s: window too large", nm);
  hipLaunchKernelGGL(c8_window_shift_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<uint4*>(xs), (int)rows, cpr, total, counters);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}
