// The sort join's order of efl.psi.strsort on the device: efl_strings_sort, efl_strings_search,
// efl_strings_run_heads and their host twins efl_strings_*_host (include/efl_hip.h). The per-row steps
// are strsort.h; this file gives them one lane each and the launch boundaries that order them.
//
// As in idset.hip and bucket.hip no kernel waits for another lane, wave or workgroup: no spin loop, no
// lock, no look-back. The sort is entries | tile sort | ceil(log2(tiles)) rank merges that ping-pong
// two entry buffers in the caller's scratch; the only synchronisation inside a kernel is the workgroup
// barrier between the steps of a tile's bitonic network, which every lane reaches. Every place is
// computed from a total order, not claimed, so a call's output is the same bytes on every run.
#include <algorithm>
#include <initializer_list>
#include <vector>

#include "common.h"
#include "strsort.h"

namespace efl {
namespace {

using namespace strsort;

constexpr int kPerLane = kTile / kBlock;       // 8

static_assert(kTile == kBlock * kPerLane, "a tile is kPerLane rows per lane");
static_assert(sizeof(Entry) == 16, "an entry is 16 bytes");

// one lane per row: the field extents (record mode), then the row's entry
__global__ __launch_bounds__(kBlock) void k_entries(const uint8_t* __restrict__ chars, const long long* __restrict__ offsets,
                                                    const int32_t* __restrict__ segment, long long n, int mode,
                                                    long long* __restrict__ ext, Entry* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t* off = reinterpret_cast<const int64_t*>(offsets);
  int64_t* x = reinterpret_cast<int64_t*>(ext);
  if (mode == kSortRecord) write_extents(chars, off, i, x);    // this lane reads back only what it wrote
  const Rows R{chars, off, x, mode};
  out[i] = make_entry(R, segment, i);
}

// one workgroup per tile: the tile's entries sorted in LDS (32 KiB), written back in place, or their
// rows to `order` when the tile is the whole input
__global__ __launch_bounds__(kBlock) void k_tile_sort(const uint8_t* __restrict__ chars, const long long* __restrict__ offsets,
                                                      const long long* __restrict__ ext, int mode, long long n,
                                                      Entry* entries, long long* __restrict__ order) {
  __shared__ Entry tile[kTile];
  const Rows R{chars, reinterpret_cast<const int64_t*>(offsets), reinterpret_cast<const int64_t*>(ext), mode};
  const long long base = (long long)blockIdx.x * kTile;
  const long long left = n - base;
  const int count = left < kTile ? (int)left : kTile;
  const int span = tile_span(count);
  for (int x = threadIdx.x; x < span; x += kBlock) tile[x] = x < count ? entries[base + x] : no_entry();
  __syncthreads();
  for (int k = 2; k <= span; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < span / 2; t += kBlock) bitonic_exchange(R, tile, k, j, t);
      __syncthreads();
    }
  for (int x = threadIdx.x; x < count; x += kBlock) {
    if (order) order[base + x] = (long long)tile[x].row;
    else entries[base + x] = tile[x];
  }
}

// one lane per entry: its place after the pairwise merge of runs of `run` entries; the last pass
// writes the rows to `order`
__global__ __launch_bounds__(kBlock) void k_merge(const uint8_t* __restrict__ chars, const long long* __restrict__ offsets,
                                                  const long long* __restrict__ ext, int mode, long long n, long long run,
                                                  const Entry* __restrict__ src, Entry* __restrict__ dst,
                                                  long long* __restrict__ order) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const Rows R{chars, reinterpret_cast<const int64_t*>(offsets), reinterpret_cast<const int64_t*>(ext), mode};
  const long long at = merge_place(R, src, n, run, i);
  if (at < 0 || at >= n) return;                   // never, unless the buffers changed between the launches
  if (order) order[at] = (long long)src[i].row;
  else dst[at] = src[i];
}

// one lane per query
__global__ __launch_bounds__(kBlock) void k_search(const uint8_t* __restrict__ t_chars, const long long* __restrict__ t_offsets,
                                                   const long long* __restrict__ t_order, long long m,
                                                   const uint8_t* __restrict__ q_chars, const long long* __restrict__ q_offsets,
                                                   long long nq, long long* __restrict__ out) {
  const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (j >= nq) return;
  if (m == 0) {
    out[j] = -1;
    return;
  }
  const int64_t* qo = reinterpret_cast<const int64_t*>(q_offsets);
  out[j] = search_one(t_chars, reinterpret_cast<const int64_t*>(t_offsets), reinterpret_cast<const int64_t*>(t_order), m,
                      q_chars + qo[j], row_len(qo, j));
}

// one lane per place of `order`
__global__ __launch_bounds__(kBlock) void k_run_heads(const uint8_t* __restrict__ chars, const long long* __restrict__ offsets,
                                                      const long long* __restrict__ order, long long n,
                                                      uint8_t* __restrict__ heads) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  heads[k] = run_head(chars, reinterpret_cast<const int64_t*>(offsets), reinterpret_cast<const int64_t*>(order), n, k);
}

long long blocks_of(long long n) { return (n + kBlock - 1) / kBlock; }

long long tiles_of(long long n) { return (n + kTile - 1) / kTile; }

// two entry buffers (16 n bytes each), then the field extents (two int64 per row)
size_t sort_scratch(long long n) { return (size_t)n * 48; }

int invalid(const char* text) {
  set_error("%s", text);
  return EFL_E_INVALID_ARGUMENT;
}

// the checks the entry points share; > 0: nothing to do
int check_rows(int64_t n, std::initializer_list<const void*> bufs) {
  if (n < 0) return invalid("negative count");
  if (n == 0) return 1;
  for (const void* p : bufs)
    if (!p) return invalid("null buffer");
  return EFL_OK;
}

int too_many(int64_t n) {
  set_error("%lld rows: a call takes at most 2^31 - 2", (long long)n);
  return EFL_E_RESOURCE_EXHAUSTED;
}

bool mode_ok(int mode) { return mode == kSortBytes || mode == kSortRecord; }

int bad_mode(int mode) {
  set_error("mode %d: EFL_SORT_BYTES (0) or EFL_SORT_RECORD (1)", mode);
  return EFL_E_INVALID_ARGUMENT;
}

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API int efl_strings_sort_host(const char* chars, const int64_t* offsets, const int32_t* segment, int64_t n, int mode,
                                  int64_t* order) {
  const int rc = check_rows(n, {chars, offsets, order});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (!mode_ok(mode)) return bad_mode(mode);
  if (n > kMaxRows) return too_many(n);
  const uint8_t* c = reinterpret_cast<const uint8_t*>(chars);
  std::vector<int64_t> ext;
  if (mode == kSortRecord) {
    ext.resize((size_t)n * 2);
    for (int64_t r = 0; r < n; ++r) write_extents(c, offsets, r, ext.data());
  }
  const Rows R{c, offsets, mode == kSortRecord ? ext.data() : nullptr, mode};
  for (int64_t r = 0; r < n; ++r) order[r] = r;
  // stable: rows that compare equal keep their order, the row index of the total order
  std::stable_sort(order, order + n, [&](int64_t a, int64_t b) {
    if (segment && segment[a] != segment[b]) return segment[a] < segment[b];
    return compare_rows(R, a, b) < 0;
  });
  return EFL_OK;
}

EFL_API int efl_strings_search_host(const char* t_chars, const int64_t* t_offsets, const int64_t* t_order, int64_t m,
                                    const char* q_chars, const int64_t* q_offsets, int64_t nq, int64_t* out) {
  const int rc = check_rows(nq, {q_chars, q_offsets, out});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (m < 0) return invalid("negative table size");
  if (m > 0 && (!t_chars || !t_offsets || !t_order)) return invalid("null buffer");
  if (nq > kMaxRows) return too_many(nq);
  if (m > kMaxRows) return too_many(m);
  const uint8_t* q = reinterpret_cast<const uint8_t*>(q_chars);
  for (int64_t j = 0; j < nq; ++j)
    out[j] = m == 0 ? -1
                    : search_one(reinterpret_cast<const uint8_t*>(t_chars), t_offsets, t_order, m, q + q_offsets[j],
                                 row_len(q_offsets, j));
  return EFL_OK;
}

EFL_API int efl_strings_run_heads_host(const char* chars, const int64_t* offsets, const int64_t* order, int64_t n,
                                       uint8_t* heads) {
  const int rc = check_rows(n, {chars, offsets, order, heads});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (n > kMaxRows) return too_many(n);
  for (int64_t k = 0; k < n; ++k) heads[k] = run_head(reinterpret_cast<const uint8_t*>(chars), offsets, order, n, k);
  return EFL_OK;
}

EFL_API int64_t efl_strings_sort_scratch_bytes(int64_t n) { return n <= 0 || n > kMaxRows ? 0 : (int64_t)sort_scratch(n); }

EFL_API int efl_strings_sort(const char* chars, const int64_t* offsets, const int32_t* segment, int64_t n, int mode,
                             int64_t* order, void* scratch, int64_t scratch_len, void* stream) {
  const int rc = check_rows(n, {chars, offsets, order, scratch});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (!mode_ok(mode)) return bad_mode(mode);
  if (!aligned(offsets, 8) || !aligned(order, 8) || !aligned(segment, 4) || !aligned(scratch, 16))
    return invalid("offsets, order, segment or scratch is misaligned");
  if (n > kMaxRows) return too_many(n);
  if (scratch_len < (int64_t)sort_scratch(n)) {
    set_error("scratch of %lld bytes, efl_strings_sort_scratch_bytes(n) = %lld", (long long)scratch_len,
              (long long)sort_scratch(n));
    return EFL_E_INVALID_ARGUMENT;
  }
  hipStream_t st = (hipStream_t)stream;
  const long long N = n, tiles = tiles_of(N);
  const uint8_t* c = reinterpret_cast<const uint8_t*>(chars);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  long long* ord = reinterpret_cast<long long*>(order);
  Entry* a = static_cast<Entry*>(scratch);
  Entry* b = a + N;
  long long* ext = reinterpret_cast<long long*>(b + N);
  hipLaunchKernelGGL(k_entries, dim3((unsigned)blocks_of(N)), dim3(kBlock), 0, st, c, off, segment, N, mode, ext, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_status(e, "efl_strings_sort");
  hipLaunchKernelGGL(k_tile_sort, dim3((unsigned)tiles), dim3(kBlock), 0, st, c, off, (const long long*)ext, mode, N, a,
                     tiles == 1 ? ord : nullptr);
  e = hipGetLastError();
  for (long long run = kTile; e == hipSuccess && run < N; run *= 2) {
    const bool last = run * 2 >= N;
    hipLaunchKernelGGL(k_merge, dim3((unsigned)blocks_of(N)), dim3(kBlock), 0, st, c, off, (const long long*)ext, mode, N,
                       run, (const Entry*)a, b, last ? ord : nullptr);
    e = hipGetLastError();
    std::swap(a, b);
  }
  return hip_status(e, "efl_strings_sort");
}

EFL_API int efl_strings_search(const char* t_chars, const int64_t* t_offsets, const int64_t* t_order, int64_t m,
                               const char* q_chars, const int64_t* q_offsets, int64_t nq, int64_t* out, void* stream) {
  const int rc = check_rows(nq, {q_chars, q_offsets, out});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (m < 0) return invalid("negative table size");
  if (m > 0 && (!t_chars || !t_offsets || !t_order)) return invalid("null buffer");
  if (!aligned(t_offsets, 8) || !aligned(t_order, 8) || !aligned(q_offsets, 8) || !aligned(out, 8))
    return invalid("t_offsets, t_order, q_offsets or out is misaligned");
  if (nq > kMaxRows) return too_many(nq);
  if (m > kMaxRows) return too_many(m);
  hipLaunchKernelGGL(k_search, dim3((unsigned)blocks_of(nq)), dim3(kBlock), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint8_t*>(t_chars), reinterpret_cast<const long long*>(t_offsets),
                     reinterpret_cast<const long long*>(t_order), (long long)m, reinterpret_cast<const uint8_t*>(q_chars),
                     reinterpret_cast<const long long*>(q_offsets), (long long)nq, reinterpret_cast<long long*>(out));
  return hip_status(hipGetLastError(), "efl_strings_search");
}

EFL_API int efl_strings_run_heads(const char* chars, const int64_t* offsets, const int64_t* order, int64_t n, uint8_t* heads,
                                  void* stream) {
  const int rc = check_rows(n, {chars, offsets, order, heads});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (!aligned(offsets, 8) || !aligned(order, 8)) return invalid("offsets or order is misaligned");
  if (n > kMaxRows) return too_many(n);
  hipLaunchKernelGGL(k_run_heads, dim3((unsigned)blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint8_t*>(chars), reinterpret_cast<const long long*>(offsets),
                     reinterpret_cast<const long long*>(order), (long long)n, heads);
  return hip_status(hipGetLastError(), "efl_strings_run_heads");
}
