// The signed-ID store of efl.psi.IdStore on the device: efl_idset_insert / efl_idset_find /
// efl_idset_rehash and the host-only efl_idset_hash (include/efl_hip.h). The per-row steps are
// idset.h; this file gives them one lane each and the launch boundaries that order them.
//
// No kernel here waits for another lane, wave or workgroup: there is no spin loop, no lock and no
// look-back. The winners' ranks come from three passes (per-block counts in k_settle, k_scan over the
// counts in one workgroup, block-local ranks in k_append); the only synchronisation inside a kernel
// is the workgroup barrier of those block scans, which every lane reaches. Every slot access of
// k_claim and k_place is an agent-scope atomic (the XCDs' L2s are separate); everything another lane
// wrote is read in a later launch.
#include "common.h"
#include "idset.h"

namespace efl {
namespace {

using namespace idset;

constexpr int kScanBlock = 1024;

struct AgentAtomics {
  static __device__ uint32_t load(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) {
    __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;      // the value found: `expect` itself when the exchange happened
  }
  static __device__ void min(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// exclusive scan of one flag per lane over the workgroup (kBlock lanes); *total <- the block's sum
__device__ uint32_t block_rank(bool flag, uint32_t* total) {
  __shared__ uint32_t wave_sum[kBlock / 64];
  const unsigned long long ballot = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t below = (uint32_t)__popcll(ballot & ((1ull << lane) - 1));
  if (lane == 0) wave_sum[wave] = (uint32_t)__popcll(ballot);
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int w = 0; w < kBlock / 64; ++w) {
    before += w < wave ? wave_sum[w] : 0;
    all += wave_sum[w];
  }
  *total = all;
  return before + below;
}

// scratch: settled [n] | rank [n] | counts [blocks] | total | size0
struct Scratch {
  uint32_t *settled, *rank, *counts;
  long long blocks;
};

template <int WORDS>
__global__ __launch_bounds__(kBlock) void k_claim(uint32_t* slots, uint64_t capacity, uint64_t seed,
                                                  const uint8_t* keys, const uint8_t* rows, long long n,
                                                  long long* slot_of) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  slot_of[i] = claim<AgentAtomics, WORDS>(slots, capacity, seed, keys, rows, i);
}

__global__ __launch_bounds__(kBlock) void k_settle(const uint32_t* slots, const long long* slot_of, long long n,
                                                   Scratch s) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  uint32_t e = kEmpty;
  if (i < n) {
    e = settle(slots, slot_of[i]);
    s.settled[i] = e;
  }
  uint32_t total;
  block_rank(i < n && won(e, i), &total);
  if (threadIdx.x == 0) s.counts[blockIdx.x] = total;
}

// one workgroup: counts <- their exclusive scan, counts[blocks] <- the sum, counts[blocks + 1] <-
// size0, and the store's size counter advanced (the later kernels read size0 from the scratch)
__global__ __launch_bounds__(kScanBlock) void k_scan(Scratch s, long long* size, long long key_capacity) {
  __shared__ uint32_t part[kScanBlock];
  const long long per = (s.blocks + kScanBlock - 1) / kScanBlock;
  const long long lo = (long long)threadIdx.x * per, hi = lo + per < s.blocks ? lo + per : s.blocks;
  uint32_t sum = 0;
  for (long long b = lo; b < hi; ++b) sum += s.counts[b];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < kScanBlock; d <<= 1) {       // Hillis-Steele over the per-lane sums
    const uint32_t v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = part[threadIdx.x] - sum;
  for (long long b = lo; b < hi; ++b) {
    const uint32_t c = s.counts[b];
    s.counts[b] = run;
    run += c;
  }
  if (threadIdx.x == kScanBlock - 1) {
    const long long size0 = *size, total = part[kScanBlock - 1];
    s.counts[s.blocks] = (uint32_t)total;
    s.counts[s.blocks + 1] = (uint32_t)size0;
    // a caller whose size_bound was below *size cannot push the appends past the key array
    *size = size0 + total <= key_capacity ? size0 + total : key_capacity;
  }
}

template <int WORDS>
__global__ __launch_bounds__(kBlock) void k_append(const uint8_t* rows, long long n, Scratch s, uint8_t* keys,
                                                   long long key_capacity) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool win = i < n && won(s.settled[i], i);
  uint32_t total;
  const uint32_t r = s.counts[blockIdx.x] + block_rank(win, &total);
  if (i >= n) return;
  s.rank[i] = r;
  const long long at = (long long)s.counts[s.blocks + 1] + r;
  if (win && at < key_capacity) store_row<WORDS>(keys, at, load_row<WORDS>(rows, i));
}

// pos_out holds each row's slot on entry and its position on return
__global__ __launch_bounds__(kBlock) void k_finish(uint32_t* slots, long long n, Scratch s, long long* pos) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const long long size0 = s.counts[s.blocks + 1];
  const uint32_t e = s.settled[i];
  if (won(e, i)) slots[pos[i]] = (uint32_t)(size0 + s.rank[i]);
  pos[i] = position(e, size0, s.rank);
}

template <int WORDS>
__global__ __launch_bounds__(kBlock) void k_find(const uint32_t* slots, uint64_t capacity, uint64_t seed,
                                                 const uint8_t* keys, const uint8_t* rows, long long n,
                                                 long long* pos) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  pos[i] = find<WORDS>(slots, capacity, seed, keys, load_row<WORDS>(rows, i));
}

template <int WORDS>
__global__ __launch_bounds__(kBlock) void k_place(uint32_t* slots, uint64_t capacity, uint64_t seed,
                                                  const uint8_t* keys, const long long* size, long long bound) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= bound || e >= *size) return;
  place<AgentAtomics, WORDS>(slots, capacity, seed, keys, e);
}

long long blocks_of(long long n) { return (n + kBlock - 1) / kBlock; }

size_t scratch_bytes(long long n) { return ((size_t)2 * n + blocks_of(n) + 2) * 4; }

int invalid(const char* text) {
  set_error("%s", text);
  return EFL_E_INVALID_ARGUMENT;
}

// the checks the three entry points share; > 0: nothing to do
int check_table(int64_t n, int width, int64_t capacity, std::initializer_list<const void*> bufs,
                std::initializer_list<const void*> rows) {
  if (n < 0) return invalid("negative count");
  if (n == 0) return 1;
  if (width != 8 && width != 32) {
    set_error("width %d: rows are 8 or 32 bytes", width);
    return EFL_E_INVALID_ARGUMENT;
  }
  for (const void* p : bufs)
    if (!p) return invalid("null buffer");
  for (const void* p : rows)
    if (!aligned(p, width == 32 ? 16 : 8)) {
      set_error("rows of %d bytes must be %d-byte aligned", width, width == 32 ? 16 : 8);
      return EFL_E_INVALID_ARGUMENT;
    }
  if (capacity < 2 || capacity > kMaxCapacity || (capacity & (capacity - 1))) {
    set_error("capacity %lld is not a power of two in 2 .. 2^32", (long long)capacity);
    return EFL_E_INVALID_ARGUMENT;
  }
  return EFL_OK;
}

int too_small(int64_t capacity, int64_t entries) {
  set_error("capacity %lld is below twice the %lld entries it may hold", (long long)capacity, (long long)entries);
  return EFL_E_INVALID_ARGUMENT;
}

int too_many(int64_t entries) {
  set_error("%lld entries: a store holds at most 2^31 - 2", (long long)entries);
  return EFL_E_RESOURCE_EXHAUSTED;
}

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API uint64_t efl_idset_hash(uint64_t seed, const uint8_t* row, int width) {
  if (!row || (width != 8 && width != 32)) return 0;
  return idset::hash_bytes(seed, row, width);
}

EFL_API int64_t efl_idset_scratch_bytes(int64_t n) {
  return n <= 0 || n > idset::kMaxEntries ? 0 : (int64_t)scratch_bytes(n);
}

EFL_API int efl_idset_insert(const uint8_t* rows, int64_t n, int width, uint8_t* keys, int64_t key_capacity,
                             int64_t* size, int64_t size_bound, uint32_t* slots, int64_t capacity, uint64_t seed,
                             int64_t* pos_out, void* scratch, int64_t scratch_len, void* stream) {
  const int rc = check_table(n, width, capacity, {rows, keys, size, slots, pos_out, scratch}, {rows, keys});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (size_bound < 0) return invalid("negative size_bound");
  if (!aligned(size, 8) || !aligned(pos_out, 8) || !aligned(slots, 4) || !aligned(scratch, 4))
    return invalid("size, pos_out, slots or scratch is misaligned");
  if (n > kMaxEntries) return too_many(n);
  if (size_bound > kMaxEntries - n) return too_many(size_bound > kMaxEntries ? size_bound : size_bound + n);
  if (capacity < 2 * (size_bound + n)) return too_small(capacity, size_bound + n);
  if (key_capacity < size_bound + n) {
    set_error("key_capacity %lld is below size_bound + n = %lld", (long long)key_capacity, (long long)(size_bound + n));
    return EFL_E_INVALID_ARGUMENT;
  }
  if (scratch_len < (int64_t)scratch_bytes(n)) {
    set_error("scratch of %lld bytes, efl_idset_scratch_bytes(%lld) = %lld", (long long)scratch_len, (long long)n,
              (long long)scratch_bytes(n));
    return EFL_E_INVALID_ARGUMENT;
  }
  hipStream_t st = (hipStream_t)stream;
  const long long N = n, nb = blocks_of(N);
  uint32_t* w = static_cast<uint32_t*>(scratch);
  const Scratch s{w, w + N, w + 2 * N, nb};
  long long* pos = reinterpret_cast<long long*>(pos_out);
  long long* sz = reinterpret_cast<long long*>(size);
  const dim3 grid((unsigned)nb), block(kBlock);
  const uint64_t cap = (uint64_t)capacity;
#define EFL_IDSET_LAUNCHED()                                    \
  do {                                                          \
    const hipError_t e = hipGetLastError();                     \
    if (e != hipSuccess) return hip_status(e, "efl_idset_insert"); \
  } while (0)
  if (width == 8)
    hipLaunchKernelGGL(k_claim<1>, grid, block, 0, st, slots, cap, seed, keys, rows, N, pos);
  else
    hipLaunchKernelGGL(k_claim<4>, grid, block, 0, st, slots, cap, seed, keys, rows, N, pos);
  EFL_IDSET_LAUNCHED();
  hipLaunchKernelGGL(k_settle, grid, block, 0, st, slots, pos, N, s);
  EFL_IDSET_LAUNCHED();
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanBlock), 0, st, s, sz, (long long)key_capacity);
  EFL_IDSET_LAUNCHED();
  if (width == 8)
    hipLaunchKernelGGL(k_append<1>, grid, block, 0, st, rows, N, s, keys, (long long)key_capacity);
  else
    hipLaunchKernelGGL(k_append<4>, grid, block, 0, st, rows, N, s, keys, (long long)key_capacity);
  EFL_IDSET_LAUNCHED();
  hipLaunchKernelGGL(k_finish, grid, block, 0, st, slots, N, s, pos);
  EFL_IDSET_LAUNCHED();
#undef EFL_IDSET_LAUNCHED
  return EFL_OK;
}

EFL_API int efl_idset_find(const uint8_t* rows, int64_t n, int width, const uint8_t* keys, const uint32_t* slots,
                           int64_t capacity, uint64_t seed, int64_t* pos_out, void* stream) {
  const int rc = check_table(n, width, capacity, {rows, keys, slots, pos_out}, {rows, keys});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (!aligned(pos_out, 8) || !aligned(slots, 4)) return invalid("pos_out or slots is misaligned");
  if (n > kMaxEntries) return too_many(n);
  const long long N = n;
  long long* pos = reinterpret_cast<long long*>(pos_out);
  const dim3 grid((unsigned)blocks_of(N)), block(kBlock);
  if (width == 8)
    hipLaunchKernelGGL(k_find<1>, grid, block, 0, (hipStream_t)stream, slots, (uint64_t)capacity, seed, keys, rows, N,
                       pos);
  else
    hipLaunchKernelGGL(k_find<4>, grid, block, 0, (hipStream_t)stream, slots, (uint64_t)capacity, seed, keys, rows, N,
                       pos);
  return hip_status(hipGetLastError(), "efl_idset_find");
}

EFL_API int efl_idset_rehash(const uint8_t* keys, int width, const int64_t* size, int64_t size_bound, uint32_t* slots,
                             int64_t capacity, uint64_t seed, void* stream) {
  // an empty store still gets its slots cleared: the count that decides "nothing to do" is 1 here
  if (size_bound < 0) return invalid("negative count");
  const int rc = check_table(1, width, capacity, {keys, size, slots}, {keys});
  if (rc) return rc;
  if (!aligned(size, 8) || !aligned(slots, 4)) return invalid("size or slots is misaligned");
  if (size_bound > kMaxEntries) return too_many(size_bound);
  if (capacity < 2 * size_bound) return too_small(capacity, size_bound);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(slots, 0xFF, (size_t)capacity * 4, st);
  if (e != hipSuccess || size_bound == 0) return hip_status(e, "efl_idset_rehash");
  const dim3 grid((unsigned)blocks_of(size_bound)), block(kBlock);
  const long long* sz = reinterpret_cast<const long long*>(size);
  if (width == 8)
    hipLaunchKernelGGL(k_place<1>, grid, block, 0, st, slots, (uint64_t)capacity, seed, keys, sz, (long long)size_bound);
  else
    hipLaunchKernelGGL(k_place<4>, grid, block, 0, st, slots, (uint64_t)capacity, seed, keys, sz, (long long)size_bound);
  return hip_status(hipGetLastError(), "efl_idset_rehash");
}
