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
//   decode_fork_kernel    between two steps, slots of a paged session continue as copies of other slots (fork / beam
//                         reorder): a slot's small state and its open page are copied, its closed pages are shared.
//   decode_gather_rows_kernel / decode_append_rows_kernel  between two steps, one slot takes MANY new rows at once
//                         (DecodeSession.extend): the module's cached forward reads contiguous K / V, so the slot's rows are
//                         gathered from its pages into a contiguous scratch, and the result -- the new K / V rows, the CNN
//                         rings, the Performer image and the counter row -- is filed into the slot by one launch.
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
// PAGED (a block table): kv_cache is a pool (2, pool_pages, H, page_rows, D); sequence n's logical row r lives in
// page table[n * table_stride + r / page_rows] at row r % page_rows (page_rows = 1 << page_shift).  A type of its own, so that
// the other forms' kernel arguments -- and code -- stay what they were
struct StagePagedParams : StageParams {
  const int32_t* table;
  int table_stride, page_shift, pool_pages;
};

// RAGGED: a counter pair per sequence, sequence n's at ctr + n * ctr_stride (read per item: the items of a workgroup span
// sequences); a sequence whose row lies outside the caches writes nothing -- which is also how a sequence that sits out a step
// (DecodeSession.pause / release: its counters are negative, ~seen) keeps its K / V; its q row is handed over and never read.
// PAGED (with RAGGED): the row goes to the page the
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

// ROWS (sea_decode_stage with rows in 2 .. 8): `rows` new rows per sequence, (N, H, rows, D) with [n, h, t] strides; q_in (N, H,
// rows, D) dense; row j of sequence n goes to cache row ctr[n * ctr_stride] + j, nothing for a row at or beyond the capacity and nothing
// for a sequence whose counter is negative (it sits out the step).  A kernel of its own, so that the one-row form's code stays
// what it was
struct StageRowsParams {
  const void *q, *k, *v;
  int64_t qs[3], ks[3], vs[3];       // element strides [n, h, t] (feature stride 1)
  void* q_in;                        // (N, H, rows, D) dense
  void* kv_cache;                    // (2, N, H, cap, D) dense
  const int32_t* ctr;
  int N, H, rows, D, cap, ctr_stride;
};

template <typename T>
__global__ __launch_bounds__(256) void decode_stage_rows_kernel(StageRowsParams p) {
  const int items = p.N * p.H * p.rows;                      // (n, h, j), j fastest: q_in's row order
  const int per = p.D / 8;
  const T* srcs[3] = {reinterpret_cast<const T*>(p.q), reinterpret_cast<const T*>(p.k), reinterpret_cast<const T*>(p.v)};
  const int64_t* strs[3] = {p.qs, p.ks, p.vs};
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < 3 * items * per; c += gridDim.x * blockDim.x) {
    const int which = c / (items * per);
    const int r = (c - which * items * per) / per, i = c % per;
    const int nh = r / p.rows, j = r - nh * p.rows;
    const int n = nh / p.H, h = nh - n * p.H;
    const int seen = p.ctr[n * p.ctr_stride];                // (negative: the sequence sits out this step, no K / V row of it)
    const int pos = seen + j;
    if (which != 0 && (seen < 0 || pos >= p.cap)) continue;
    const uint4 val = *reinterpret_cast<const uint4*>(srcs[which] + n * strs[which][0] + h * strs[which][1] + j * strs[which][2] + i * 8);
    T* dst = which == 0 ? reinterpret_cast<T*>(p.q_in) + (int64_t)r * p.D
                        : reinterpret_cast<T*>(p.kv_cache) + (((int64_t)(which - 1) * p.N * p.H + nh) * p.cap + pos) * p.D;
    *reinterpret_cast<uint4*>(dst + i * 8) = val;
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

// sea_decode_fork: M moves (src, dst, src_open, dst_open, stage) between slots of a paged session.  A move's work is a row of
// items: the slot's 16-byte chunks of the Performer image, x ring and y1 ring, then its three counters and its block-table
// entries (int32 items), then -- second launch only -- both halves of the open page in 16-byte chunks.  One grid-stride loop
// walks (move, item): the open-page copy (the bulk of the bytes) is spread over the whole grid.
// STAGE (first launch): the small state of every move with a staging slot (stage >= 0: its source is also a destination)
// goes to that slot.  Second launch: every destination is written, from the staging slot when the move has one, else from
// the source's own rows -- which no move of the call writes (host precondition) -- so each destination gets its source's
// state as it was before the call.  The pages copied from are no destination's open page (they are the sources' open pages,
// held by their slots), and the destination pages are held by no other slot: no item reads what another item writes.
struct ForkParams {
  const int32_t* moves;                 // (M, 5)
  uint4 *image, *x_ring, *y1_ring;      // slot n's slices at n * img16 / x16 / y16 chunks
  int32_t *ctr, *table;                 // slot n's counters at n * ctr_stride, table row at n * table_stride
  uint4* pool;                          // (2, pool_pages, page16) chunks: K pages, then V pages
  uint4* staging;                       // n_staged slots of slot16 chunks: image | x | y1 | counters (1 chunk) | table entries
  int M, n_staged, N, img16, x16, y16, ctr_stride, table_stride, n_entries, page_shift, pool_pages, page16, slot16;
};

template <bool STAGE>
__global__ __launch_bounds__(256) void decode_fork_kernel(ForkParams p) {
  const int vec = p.img16 + p.x16 + p.y16;
  const int small = vec + 3 + p.n_entries;
  const int per = small + (STAGE ? 0 : 2 * p.page16);
  const int total = per * p.M;                               // (host: < 2^31)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int m = i / per, c = i - m * per;
    const int32_t* mv = p.moves + 5 * m;
    const int src = mv[0], dst = mv[1], stage = mv[4];
    if (src < 0 || src >= p.N || dst < 0 || dst >= p.N) continue;
    const bool staged = stage >= 0 && stage < p.n_staged;
    if (STAGE && !staged) continue;
    uint4* slot = staged ? p.staging + (int64_t)stage * p.slot16 : nullptr;
    int32_t* slot_ctr = staged ? reinterpret_cast<int32_t*>(slot + vec) : nullptr;
    int32_t* slot_tab = staged ? slot_ctr + 4 : nullptr;
    if (c < vec) {                                           // image / rings: 16-byte chunks
      uint4* base;
      int per_slot, j;
      if (c < p.img16) { base = p.image; per_slot = p.img16; j = c; }
      else if (c < p.img16 + p.x16) { base = p.x_ring; per_slot = p.x16; j = c - p.img16; }
      else { base = p.y1_ring; per_slot = p.y16; j = c - p.img16 - p.x16; }
      if (STAGE) slot[c] = base[(int64_t)src * per_slot + j];
      else base[(int64_t)dst * per_slot + j] = staged ? slot[c] : base[(int64_t)src * per_slot + j];
    } else if (c < vec + 3) {                                // counters [seen, tsrc, tsrc of the step just closed]
      const int k = c - vec;
      if (STAGE) slot_ctr[k] = p.ctr[(int64_t)src * p.ctr_stride + k];
      else p.ctr[(int64_t)dst * p.ctr_stride + k] = staged ? slot_ctr[k] : p.ctr[(int64_t)src * p.ctr_stride + k];
    } else if (c < small) {                                  // block-table entry j
      const int j = c - vec - 3;
      if (STAGE) { slot_tab[j] = p.table[(int64_t)src * p.table_stride + j]; continue; }
      // below the source's open page index (the page row `seen` lies in): the shared closed pages; at it: the destination's
      // own open page (or -1: the source has none); behind it: no page
      // (a paused source holds ~seen, negative: the copy takes the counters as they are -- it is paused too -- and the open
      // page index comes from the decoded value)
      const int enc = staged ? slot_ctr[0] : p.ctr[(int64_t)src * p.ctr_stride];
      const int seen = enc < 0 ? ~enc : enc;
      const int open = seen >> p.page_shift;
      int32_t e = -1;
      if (j < open) e = staged ? slot_tab[j] : p.table[(int64_t)src * p.table_stride + j];
      else if (j == open) e = mv[3];
      p.table[(int64_t)dst * p.table_stride + j] = e;
    } else if (!STAGE) {                                     // the open page: K half, then V half
      const int src_pg = mv[2], dst_pg = mv[3];
      if (src_pg < 0 || src_pg >= p.pool_pages || dst_pg < 0 || dst_pg >= p.pool_pages) continue;
      const int k = c - small, half = k >= p.page16 ? 1 : 0, j = k - half * p.page16;
      const int64_t h0 = (int64_t)half * p.pool_pages;
      p.pool[(h0 + dst_pg) * p.page16 + j] = p.pool[(h0 + src_pg) * p.page16 + j];
    }
  }
}

// sea_decode_gather_rows: rows [r0, r1) of ONE sequence, K and V, from the page pool (2, pool_pages, H, page_rows, D) into a
// contiguous (2, H, out_rows, D) buffer (row r at out row r - r0), through the sequence's block-table row on the device.  A
// grid-stride loop over (half, head, row, 16-byte chunk), chunk fastest: a wave reads whole rows of a page and writes whole
// rows of the buffer.  A row at or beyond the capacity, or whose table entry is outside the pool, is skipped.
struct GatherRowsParams {
  const uint4* pool;
  uint4* out;
  const int32_t* table;                 // the sequence's table row
  int H, per, r0, rows, cap, out_rows, page_shift, pool_pages;       // per = D / 8 chunks per row; rows = r1 - r0
};

__global__ __launch_bounds__(256) void decode_gather_rows_kernel(GatherRowsParams p) {
  const int64_t total = (int64_t)2 * p.H * p.rows * p.per;
  const int64_t page16 = ((int64_t)p.H << p.page_shift) * p.per;     // chunks of one half of a page
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(c % p.per);
    const int64_t t = c / p.per;
    const int i = (int)(t % p.rows);
    const int hh = (int)(t / p.rows);                                 // half * H + head
    const int half = hh / p.H, h = hh - half * p.H;
    const int r = p.r0 + i;
    if (r >= p.cap) continue;
    const int pg = p.table[r >> p.page_shift];
    if (pg < 0 || pg >= p.pool_pages) continue;
    const int prow = r & ((1 << p.page_shift) - 1);
    p.out[((int64_t)hh * p.out_rows + i) * p.per + j] =
        p.pool[((int64_t)half * p.pool_pages + pg) * page16 + (((int64_t)h << p.page_shift) + prow) * p.per + j];
  }
}

// sea_decode_append_rows: slot `slot` of a ragged session, which stood at `seen` rows, takes the result of an extend by `rows`
// rows (it stands at t = seen + rows afterwards).  One grid-stride loop over the items of five parts, each 16-byte chunks but
// the last:
//   K / V   rows seen .. t-1 from contiguous buffers ([h, row] strides) into the slot's pages through its table row (paged
//           sessions only: a contiguous session's rows are staged where the forward reads them);
//   x ring  the window's `win_rows` rows (positions t - win_rows .. t-1) at position % ring; the other ring rows stay;
//   y1 ring conv1's last `keep_rows` rows over that window (positions t - keep_rows .. t-1) at position % ring, zeros in
//           every other ring row (keep_rows < ring rows: a ring row takes one position at most, so every chunk of the ring
//           is written by exactly one item -- no item reads or writes what another one writes);
//   image   the slot's Performer image slice;
//   counters the slot's three int32, as given by the host (plain or complement).
struct AppendRowsParams {
  const uint4 *k_rows, *v_rows;         // row seen + i of head h at h * src_h16 + i * src_t16 chunks
  uint4* pool;                          // nullptr: no K / V part
  const int32_t* table;                 // the slot's table row
  const uint4 *window, *conv1, *image_src;
  uint4 *x_ring, *y1_ring, *image;      // the slot's slices
  int32_t* ctr;                         // the slot's counter row
  int64_t src_h16[2], src_t16[2];
  int H, per, seen, rows, cap, page_shift, pool_pages;
  int row16, win_rows, keep_rows, x_rows, y_rows, img16;
  int32_t c0, c1, c2;
};

__global__ __launch_bounds__(256) void decode_append_rows_kernel(AppendRowsParams p) {
  const int64_t n_kv = p.pool ? (int64_t)2 * p.H * p.rows * p.per : 0;
  const int64_t n_x = (int64_t)p.win_rows * p.row16, n_y = (int64_t)p.y_rows * p.row16;
  const int64_t total = n_kv + n_x + n_y + p.img16 + 3;               // (host: < 2^31 each)
  const int t = p.seen + p.rows;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += (int64_t)gridDim.x * blockDim.x) {
    if (c < n_kv) {
      const int j = (int)(c % p.per);
      const int64_t u = c / p.per;
      const int i = (int)(u % p.rows);
      const int hh = (int)(u / p.rows);
      const int half = hh / p.H, h = hh - half * p.H;
      const int r = p.seen + i;
      if (r >= p.cap) continue;
      const int pg = p.table[r >> p.page_shift];
      if (pg < 0 || pg >= p.pool_pages) continue;
      const int prow = r & ((1 << p.page_shift) - 1);
      const uint4* src = half ? p.v_rows : p.k_rows;
      p.pool[(((int64_t)half * p.pool_pages + pg) * p.H + h) * (((int64_t)1 << p.page_shift) * p.per) + (int64_t)prow * p.per + j] =
          src[h * p.src_h16[half] + i * p.src_t16[half] + j];
      continue;
    }
    int64_t k = c - n_kv;
    if (k < n_x) {                                           // window row i is position t - win_rows + i
      const int i = (int)(k / p.row16), j = (int)(k - (int64_t)i * p.row16);
      const int pos = t - p.win_rows + i;
      p.x_ring[(int64_t)(pos % p.x_rows) * p.row16 + j] = p.window[k];
      continue;
    }
    k -= n_x;
    if (k < n_y) {                                           // ring row q: the one position of t - keep_rows .. t-1 it holds, else 0
      const int q = (int)(k / p.row16), j = (int)(k - (int64_t)q * p.row16);
      const int back = ((t - 1) % p.y_rows - q + p.y_rows) % p.y_rows;        // position t - 1 - back sits in ring row q
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (back < p.keep_rows) val = p.conv1[(int64_t)(p.win_rows - 1 - back) * p.row16 + j];
      p.y1_ring[k] = val;
      continue;
    }
    k -= n_y;
    if (k < p.img16) { p.image[k] = p.image_src[k]; continue; }
    k -= p.img16;
    p.ctr[k] = k == 0 ? p.c0 : k == 1 ? p.c1 : p.c2;
  }
}

}  // namespace sea

using namespace sea;

// counter_stride > 0: a counter PER SEQUENCE, sequence n's new row goes to cache row counters[n * counter_stride];
// block_table != NULL (with a counter per sequence): paged K / V, the rows go to page block_table[n * table_stride + ctr /
// page_rows] of the pool (2, pool_pages, H, page_rows, D), row ctr % page_rows;
// rows in 2 .. 8 (contiguous caches): row j of sequence n goes to cache row counters[n * counter_stride] + j (include/sea_hip.h)
extern "C" int sea_decode_stage(const void* q, const void* k, const void* v, int dtype, int64_t N, int64_t H, int64_t rows,
                                int64_t D, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                void* q_in, void* kv_cache, int64_t capacity, const int32_t* counters, int64_t counter_stride,
                                const int32_t* block_table, int64_t table_stride, int64_t page_rows, int64_t pool_pages,
                                sea_stream_t stream) {
  const char* nm = "sea_decode_stage";
  if (counter_stride || block_table)
    SEA_REQUIRE(counter_stride > 0, SEA_EINVAL, "%s: bad counter stride: counter_stride must be >= 1 (got %lld)", nm,
                (long long)counter_stride);
  if (block_table) {
    SEA_REQUIRE(rows <= 1, SEA_EUNSUPPORTED, "%s: paged K / V takes one row per step (rows %lld)", nm, (long long)rows);
    SEA_REQUIRE(dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: 16-bit data only (dtype %d)", nm, dtype);
    if (int e = paged_layout_check(nm, dtype, D, capacity, page_rows, table_stride, N)) return e;
    SEA_REQUIRE(pool_pages > 0 && 2 * pool_pages * H * page_rows * D < (1ll << 62) && pool_pages < (1ll << 31), SEA_EINVAL,
                "%s: bad pool of %lld pages", nm, (long long)pool_pages);
  } else {
    SEA_REQUIRE(page_rows == 0 && table_stride == 0 && pool_pages == 0, SEA_EINVAL,
                "%s: null pointer: page_rows / table_stride / pool_pages without a block_table", nm);
  }
  SEA_REQUIRE(q && k && v && q_strides && k_strides && v_strides && q_in && kv_cache && counters, SEA_EINVAL, "%s: null pointer", nm);
  SEA_REQUIRE(rows >= 1 && rows <= 8, SEA_EINVAL, "%s: rows %lld outside 1 .. 8", nm, (long long)rows);
  SEA_REQUIRE(dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: 16-bit data only (dtype %d)", nm, dtype);
  SEA_REQUIRE(N > 0 && H > 0 && D > 0 && capacity > 0 && capacity < (1ll << 31) && N * H * rows * D < (1ll << 24), SEA_EINVAL,
              "%s: bad shape", nm);
  SEA_REQUIRE(counter_stride >= 0 && counter_stride * N < (1ll << 31), SEA_EINVAL, "%s: bad counter stride %lld", nm,
              (long long)counter_stride);
  SEA_REQUIRE(D % 8 == 0, SEA_EUNSUPPORTED, "%s: D must be a multiple of 8 (16-byte rows)", nm);
  const int ns = rows > 1 ? 3 : 2;                           // (one row: the t stride is not read)
  bool al = (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)q_in | (uintptr_t)kv_cache) & 15) == 0;
  for (int i = 0; i < ns; ++i) al = al && q_strides[i] % 8 == 0 && k_strides[i] % 8 == 0 && v_strides[i] % 8 == 0;
  SEA_REQUIRE(al, SEA_EUNSUPPORTED, "%s: rows must be 16-byte aligned", nm);
  hipStream_t s = (hipStream_t)stream;
  const int64_t chunks = 3 * N * H * rows * (D / 8);
  const unsigned blocks = (unsigned)((chunks + 255) / 256 > 1024 ? 1024 : (chunks + 255) / 256);
  if (rows == 1) {
    StagePagedParams p;
    p.q = q; p.k = k; p.v = v; p.q_in = q_in; p.kv_cache = kv_cache; p.ctr = counters;
    for (int i = 0; i < 2; ++i) { p.qs[i] = q_strides[i]; p.ks[i] = k_strides[i]; p.vs[i] = v_strides[i]; }
    p.N = (int)N; p.H = (int)H; p.D = (int)D; p.cap = (int)capacity;
    p.table = block_table; p.table_stride = (int)table_stride; p.page_shift = block_table ? __builtin_ctzll(page_rows) : 0;
    p.pool_pages = (int)pool_pages;
    const int cs = (int)counter_stride;
    const StageParams b = p;                                   // (the unpaged forms' arguments)
    if (block_table) {
      if (dtype == SEA_F16) hipLaunchKernelGGL((decode_stage_kernel<__half, true, true>), dim3(blocks), dim3(256), 0, s, p, cs);
      else hipLaunchKernelGGL((decode_stage_kernel<__hip_bfloat16, true, true>), dim3(blocks), dim3(256), 0, s, p, cs);
    } else if (dtype == SEA_F16) {
      if (cs) hipLaunchKernelGGL((decode_stage_kernel<__half, true>), dim3(blocks), dim3(256), 0, s, b, cs);
      else hipLaunchKernelGGL((decode_stage_kernel<__half, false>), dim3(blocks), dim3(256), 0, s, b, 0);
    } else {
      if (cs) hipLaunchKernelGGL((decode_stage_kernel<__hip_bfloat16, true>), dim3(blocks), dim3(256), 0, s, b, cs);
      else hipLaunchKernelGGL((decode_stage_kernel<__hip_bfloat16, false>), dim3(blocks), dim3(256), 0, s, b, 0);
    }
  } else {
    StageRowsParams r;
    r.q = q; r.k = k; r.v = v; r.q_in = q_in; r.kv_cache = kv_cache; r.ctr = counters;
    for (int i = 0; i < 3; ++i) { r.qs[i] = q_strides[i]; r.ks[i] = k_strides[i]; r.vs[i] = v_strides[i]; }
    r.N = (int)N; r.H = (int)H; r.rows = (int)rows; r.D = (int)D; r.cap = (int)capacity; r.ctr_stride = (int)counter_stride;
    if (dtype == SEA_F16) hipLaunchKernelGGL(decode_stage_rows_kernel<__half>, dim3(blocks), dim3(256), 0, s, r);
    else hipLaunchKernelGGL(decode_stage_rows_kernel<__hip_bfloat16>, dim3(blocks), dim3(256), 0, s, r);
  }
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
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

// fork / reorder of a paged session's slots (decode.py: DecodeSession.fork / reorder); include/sea_hip.h states the layout
// and the preconditions the caller guarantees
extern "C" int sea_decode_fork(const int32_t* moves, int64_t M, int64_t n_staged, int dtype, int64_t N, int64_t H, int64_t D,
                               int64_t nb, void* image, void* x_ring, int64_t x_ring_bytes, void* y1_ring, int64_t y1_ring_bytes,
                               int32_t* counters, int64_t counter_stride, int32_t* block_table, int64_t table_stride,
                               int64_t capacity, void* kv_pool, int64_t page_rows, int64_t pool_pages, void* staging,
                               int64_t staging_bytes, sea_stream_t stream) {
  const char* nm = "sea_decode_fork";
  SEA_REQUIRE(moves && image && x_ring && y1_ring && counters && block_table && kv_pool, SEA_EINVAL, "%s: null pointer", nm);
  SEA_REQUIRE(dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: 16-bit data only (dtype %d)", nm, dtype);
  SEA_REQUIRE(N > 0 && H > 0 && D > 0 && nb > 0 && N < (1ll << 24), SEA_EINVAL, "%s: bad shape", nm);
  SEA_REQUIRE(M >= 1 && M <= N, SEA_EINVAL, "%s: %lld moves for %lld slots (1 .. N, distinct destinations)", nm, (long long)M,
              (long long)N);
  SEA_REQUIRE(n_staged >= 0 && n_staged <= M, SEA_EINVAL, "%s: n_staged %lld outside 0 .. M = %lld", nm, (long long)n_staged,
              (long long)M);
  SEA_REQUIRE(counter_stride >= 3 && counter_stride * N < (1ll << 31), SEA_EINVAL, "%s: counter_stride %lld (3 counters per slot)",
              nm, (long long)counter_stride);
  if (int e = paged_layout_check(nm, dtype, D, capacity, page_rows, table_stride, N)) return e;
  SEA_REQUIRE(pool_pages > 0 && pool_pages < (1ll << 31), SEA_EINVAL, "%s: bad pool of %lld pages", nm, (long long)pool_pages);
  const int64_t img_bytes = sea_performer_state_bytes(1, H, D, nb, dtype);
  SEA_REQUIRE(img_bytes > 0 && img_bytes % 16 == 0 && x_ring_bytes > 0 && x_ring_bytes % 16 == 0 && y1_ring_bytes > 0 &&
              y1_ring_bytes % 16 == 0, SEA_EUNSUPPORTED, "%s: per-slot image / ring bytes (%lld, %lld, %lld) must be whole 16-byte chunks",
              nm, (long long)img_bytes, (long long)x_ring_bytes, (long long)y1_ring_bytes);
  const int64_t page_bytes = H * page_rows * D * 2;          // one half (K or V) of a page
  const int64_t n_entries = (capacity + page_rows - 1) / page_rows;
  const int64_t vec = (img_bytes + x_ring_bytes + y1_ring_bytes) / 16;
  const int64_t slot16 = vec + 1 + (n_entries + 3) / 4;
  const int64_t per = vec + 3 + n_entries + 2 * page_bytes / 16;
  SEA_REQUIRE(per * M < (1ll << 31) && pool_pages * page_bytes * 2 < (1ll << 62) && N * vec < (1ll << 31), SEA_EUNSUPPORTED,
              "%s: slot state or pages too large", nm);
  SEA_REQUIRE(n_staged == 0 || (staging && staging_bytes >= n_staged * slot16 * 16), SEA_EINVAL,
              "%s: staging buffer of %lld bytes, %lld needed (%lld slots of %lld)", nm, (long long)(staging ? staging_bytes : 0),
              (long long)(n_staged * slot16 * 16), (long long)n_staged, (long long)(slot16 * 16));
  const uintptr_t al = (uintptr_t)image | (uintptr_t)x_ring | (uintptr_t)y1_ring | (uintptr_t)kv_pool | (uintptr_t)staging;
  SEA_REQUIRE((al & 15) == 0, SEA_EUNSUPPORTED, "%s: image, rings, pool and staging must be 16-byte aligned", nm);
  ForkParams p;
  p.moves = moves; p.image = (uint4*)image; p.x_ring = (uint4*)x_ring; p.y1_ring = (uint4*)y1_ring;
  p.ctr = counters; p.table = block_table; p.pool = (uint4*)kv_pool; p.staging = (uint4*)staging;
  p.M = (int)M; p.n_staged = (int)n_staged; p.N = (int)N;
  p.img16 = (int)(img_bytes / 16); p.x16 = (int)(x_ring_bytes / 16); p.y16 = (int)(y1_ring_bytes / 16);
  p.ctr_stride = (int)counter_stride; p.table_stride = (int)table_stride; p.n_entries = (int)n_entries;
  p.page_shift = __builtin_ctzll(page_rows); p.pool_pages = (int)pool_pages; p.page16 = (int)(page_bytes / 16);
  p.slot16 = (int)slot16;
  hipStream_t s = (hipStream_t)stream;
  auto grid = [](int64_t items) { return (unsigned)((items + 255) / 256 < 2048 ? (items + 255) / 256 : 2048); };
  if (n_staged > 0) {
    hipLaunchKernelGGL(decode_fork_kernel<true>, dim3(grid((vec + 3 + n_entries) * M)), dim3(256), 0, s, p);
    SEA_CHECK_LAUNCH(nm);
  }
  hipLaunchKernelGGL(decode_fork_kernel<false>, dim3(grid(per * M)), dim3(256), 0, s, p);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}

// DecodeSession.extend: rows [r0, r1) of sequence `slot` from the page pool into a contiguous (2, H, out_rows, D) buffer
// (include/sea_hip.h)
extern "C" int sea_decode_gather_rows(const void* kv_pool, int dtype, int64_t N, int64_t H, int64_t D, int64_t capacity,
                                      const int32_t* block_table, int64_t table_stride, int64_t page_rows, int64_t pool_pages,
                                      int64_t slot, int64_t r0, int64_t r1, void* out, int64_t out_rows, sea_stream_t stream) {
  const char* nm = "sea_decode_gather_rows";
  SEA_REQUIRE(kv_pool && block_table && out, SEA_EINVAL, "%s: null pointer", nm);
  SEA_REQUIRE(dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: 16-bit data only (dtype %d)", nm, dtype);
  SEA_REQUIRE(N > 0 && H > 0 && D > 0 && H < (1ll << 16), SEA_EINVAL, "%s: bad shape", nm);
  if (int e = paged_layout_check(nm, dtype, D, capacity, page_rows, table_stride, N)) return e;
  SEA_REQUIRE(pool_pages > 0 && pool_pages < (1ll << 31) && 2 * pool_pages * H * page_rows * D < (1ll << 62), SEA_EINVAL,
              "%s: bad pool of %lld pages", nm, (long long)pool_pages);
  SEA_REQUIRE(slot >= 0 && slot < N, SEA_EINVAL, "%s: slot %lld outside 0 .. %lld", nm, (long long)slot, (long long)(N - 1));
  SEA_REQUIRE(r0 >= 0 && r0 <= r1 && r1 <= capacity, SEA_EINVAL, "%s: rows [%lld, %lld) outside 0 <= r0 <= r1 <= capacity = %lld",
              nm, (long long)r0, (long long)r1, (long long)capacity);
  SEA_REQUIRE(out_rows >= r1 - r0 && out_rows < (1ll << 24), SEA_EINVAL, "%s: a buffer of %lld rows for %lld", nm,
              (long long)out_rows, (long long)(r1 - r0));
  SEA_REQUIRE((((uintptr_t)kv_pool | (uintptr_t)out) & 15) == 0, SEA_EUNSUPPORTED, "%s: rows must be 16-byte aligned", nm);
  if (r0 == r1) return SEA_OK;
  GatherRowsParams p;
  p.pool = (const uint4*)kv_pool; p.out = (uint4*)out; p.table = block_table + slot * table_stride;
  p.H = (int)H; p.per = (int)(D / 8); p.r0 = (int)r0; p.rows = (int)(r1 - r0); p.cap = (int)capacity; p.out_rows = (int)out_rows;
  p.page_shift = __builtin_ctzll(page_rows); p.pool_pages = (int)pool_pages;
  const int64_t chunks = 2 * H * (r1 - r0) * (D / 8);
  const unsigned blocks = (unsigned)((chunks + 255) / 256 < 2048 ? (chunks + 255) / 256 : 2048);
  hipLaunchKernelGGL(decode_gather_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}

// DecodeSession.extend: the result of an extend by `rows` rows, filed into slot `slot` by one launch (include/sea_hip.h)
extern "C" int sea_decode_append_rows(int dtype, int64_t slot, int64_t N, int64_t H, int64_t D, int64_t nb, int64_t seen,
                                      int64_t rows, int64_t capacity, const void* k_rows, const void* v_rows,
                                      const int64_t* k_strides, const int64_t* v_strides, void* kv_pool,
                                      const int32_t* block_table, int64_t table_stride, int64_t page_rows, int64_t pool_pages,
                                      const void* window, int64_t window_rows, const void* conv1_rows, int64_t keep_rows,
                                      int64_t row_bytes, void* x_ring, int64_t x_ring_rows, void* y1_ring, int64_t y1_ring_rows,
                                      const void* image_src, void* image, int32_t* counters, int64_t counter_stride,
                                      int32_t ctr_seen, int32_t ctr_tsrc, int32_t ctr_done, sea_stream_t stream) {
  const char* nm = "sea_decode_append_rows";
  SEA_REQUIRE(window && conv1_rows && x_ring && y1_ring && image_src && image && counters, SEA_EINVAL,
              "%s: null pointer", nm);
  SEA_REQUIRE(dtype == SEA_F16 || dtype == SEA_BF16, SEA_EUNSUPPORTED, "%s: 16-bit data only (dtype %d)", nm, dtype);
  SEA_REQUIRE(N > 0 && H > 0 && D > 0 && nb > 0 && N < (1ll << 24) && H < (1ll << 16), SEA_EINVAL, "%s: bad shape", nm);
  SEA_REQUIRE(slot >= 0 && slot < N, SEA_EINVAL, "%s: slot %lld outside 0 .. %lld", nm, (long long)slot, (long long)(N - 1));
  SEA_REQUIRE(counter_stride >= 3 && counter_stride * N < (1ll << 31), SEA_EINVAL, "%s: counter_stride %lld (3 counters per slot)",
              nm, (long long)counter_stride);
  SEA_REQUIRE(capacity > 0 && capacity < (1ll << 24) && seen >= 0 && rows >= 1 && seen + rows <= capacity, SEA_EINVAL,
              "%s: rows [%lld, %lld) outside 0 <= r0 < r1 <= capacity = %lld", nm, (long long)seen, (long long)(seen + rows),
              (long long)capacity);
  SEA_REQUIRE(window_rows >= 1 && window_rows <= x_ring_rows && window_rows <= seen + rows && keep_rows >= 0 &&
              keep_rows <= window_rows && keep_rows < y1_ring_rows && x_ring_rows < (1ll << 16) && y1_ring_rows < (1ll << 16),
              SEA_EINVAL, "%s: a window of %lld rows (%lld of conv1 kept) does not fit rings of %lld and %lld rows", nm,
              (long long)window_rows, (long long)keep_rows, (long long)x_ring_rows, (long long)y1_ring_rows);
  const int64_t img_bytes = sea_performer_state_bytes(1, H, D, nb, dtype);
  SEA_REQUIRE(img_bytes > 0 && img_bytes % 16 == 0 && row_bytes > 0 && row_bytes % 16 == 0 && D % 8 == 0, SEA_EUNSUPPORTED,
              "%s: image bytes %lld, ring row bytes %lld and K / V rows (D = %lld) must be whole 16-byte chunks", nm,
              (long long)img_bytes, (long long)row_bytes, (long long)D);
  SEA_REQUIRE((x_ring_rows + y1_ring_rows) * row_bytes * N < (1ll << 34) && img_bytes * N < (1ll << 34), SEA_EUNSUPPORTED,
              "%s: slot state too large", nm);
  uintptr_t al = (uintptr_t)window | (uintptr_t)conv1_rows | (uintptr_t)x_ring | (uintptr_t)y1_ring | (uintptr_t)image_src |
                 (uintptr_t)image;
  AppendRowsParams p;
  p.pool = nullptr; p.table = nullptr; p.k_rows = p.v_rows = nullptr;
  p.page_shift = 0; p.pool_pages = 0;
  for (int i = 0; i < 2; ++i) p.src_h16[i] = p.src_t16[i] = 0;
  if (kv_pool) {
    SEA_REQUIRE(k_rows && v_rows && k_strides && v_strides && block_table, SEA_EINVAL, "%s: null pointer", nm);
    if (int e = paged_layout_check(nm, dtype, D, capacity, page_rows, table_stride, N)) return e;
    SEA_REQUIRE(pool_pages > 0 && pool_pages < (1ll << 31) && 2 * pool_pages * H * page_rows * D < (1ll << 62), SEA_EINVAL,
                "%s: bad pool of %lld pages", nm, (long long)pool_pages);
    bool ok = true;
    for (int i = 0; i < 2; ++i) ok = ok && k_strides[i] % 8 == 0 && v_strides[i] % 8 == 0;
    al |= (uintptr_t)kv_pool | (uintptr_t)k_rows | (uintptr_t)v_rows;
    SEA_REQUIRE(ok && (al & 15) == 0, SEA_EUNSUPPORTED, "%s: rows must be 16-byte aligned", nm);
    p.pool = (uint4*)kv_pool; p.table = block_table + slot * table_stride;
    p.k_rows = (const uint4*)k_rows; p.v_rows = (const uint4*)v_rows;
    p.src_h16[0] = k_strides[0] / 8; p.src_t16[0] = k_strides[1] / 8; p.src_h16[1] = v_strides[0] / 8; p.src_t16[1] = v_strides[1] / 8;
    p.page_shift = __builtin_ctzll(page_rows); p.pool_pages = (int)pool_pages;
  } else {
    SEA_REQUIRE(!block_table && page_rows == 0 && table_stride == 0 && pool_pages == 0, SEA_EINVAL,
                "%s: null pointer: a block_table / page_rows / table_stride / pool_pages without a kv_pool", nm);
  }
  SEA_REQUIRE((al & 15) == 0, SEA_EUNSUPPORTED, "%s: rows must be 16-byte aligned", nm);
  p.H = (int)H; p.per = (int)(D / 8); p.seen = (int)seen; p.rows = (int)rows; p.cap = (int)capacity;
  p.row16 = (int)(row_bytes / 16); p.win_rows = (int)window_rows; p.keep_rows = (int)keep_rows;
  p.x_rows = (int)x_ring_rows; p.y_rows = (int)y1_ring_rows; p.img16 = (int)(img_bytes / 16);
  p.window = (const uint4*)window; p.conv1 = (const uint4*)conv1_rows; p.image_src = (const uint4*)image_src;
  p.x_ring = (uint4*)x_ring + slot * x_ring_rows * p.row16;
  p.y1_ring = (uint4*)y1_ring + slot * y1_ring_rows * p.row16;
  p.image = (uint4*)image + slot * p.img16;
  p.ctr = counters + slot * counter_stride;
  p.c0 = ctr_seen; p.c1 = ctr_tsrc; p.c2 = ctr_done;
  const int64_t items = (kv_pool ? 2 * H * rows * (D / 8) : 0) + (window_rows + y1_ring_rows) * p.row16 + p.img16 + 3;
  const unsigned blocks = (unsigned)((items + 255) / 256 < 2048 ? (items + 255) / 256 : 2048);
  hipLaunchKernelGGL(decode_append_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
  SEA_CHECK_LAUNCH(nm);
  return SEA_OK;
}
