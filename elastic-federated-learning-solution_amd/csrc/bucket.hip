// The bucket hash and partition of efl.psi.bucket on the device: efl_mmh3_hash, efl_bucket_ids,
// efl_bucket_partition, efl_strings_gather and the host-only efl_mmh3_*_host (include/efl_hip.h). The
// per-row steps are mmh3.h; this file gives them one lane each and the launch boundaries that order
// them.
//
// As in idset.hip no kernel waits for another lane, wave or workgroup: no spin loop, no lock, no
// look-back. The partition is histogram | scan | scatter and the gather is scan | copy, the scan three
// launches of its own (per-block sums, one workgroup over those sums, per-block exclusive scans); the
// only synchronisation inside a kernel is the workgroup barrier, which every lane reaches. Nothing
// here depends on the order in which lanes, waves or workgroups run: the histogram's LDS adds are
// integer sums, and every place in `order` is computed, not claimed, so a call's output is the same
// bytes on every run.
#include "common.h"
#include "mmh3.h"

namespace efl {
namespace {

using namespace mmh3;

constexpr int kWaves = kBlock / 64;
constexpr int kChunk = kTile / kWaves;         // rows of a tile one wave ranks: 512
constexpr int kRounds = kChunk / 64;           // 8
constexpr int kPerLane = 8;                    // elements of a scan one lane sums
constexpr int kScanTile = kBlock * kPerLane;   // 2048 elements per workgroup of the scan
constexpr int kTopBlock = 1024;

static_assert(kTile == kBlock * kRounds, "a tile is kRounds rows per lane");

__global__ __launch_bounds__(kBlock) void k_mmh3(const uint8_t* __restrict__ chars, const long long* __restrict__ offsets,
                                                 long long n, uint32_t seed, int32_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const long long lo = offsets[i], hi = offsets[i + 1];
  out[i] = (int32_t)murmur3_x86_32(chars + lo, hi > lo ? hi - lo : 0, seed);
}

__global__ __launch_bounds__(kBlock) void k_bucket_ids(const int32_t* __restrict__ hash, long long n, long long modulus,
                                                       int32_t divisor, int32_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = bucket_id(hash[i], modulus, divisor);
}

// ---- the multi-block exclusive scan -----------------------------------------------------------------
// element j of the scanned sequence is load(j); lane l of workgroup b takes the kPerLane consecutive
// elements from b * kScanTile + l * kPerLane

struct LoadCounts {
  const uint32_t* v;
  __device__ uint64_t operator()(long long j) const { return v[j]; }
};

// the length of string order[j]; element n (the one past the last string) and a row index outside
// [0, n) are empty strings
struct LoadLengths {
  const long long *offsets, *order;
  long long n;
  __device__ uint64_t operator()(long long j) const {
    if (j >= n) return 0;
    const long long r = order[j];
    if (r < 0 || r >= n) return 0;
    const long long d = offsets[r + 1] - offsets[r];
    return d > 0 ? (uint64_t)d : 0;
  }
};

// exclusive scan of one value per lane over the workgroup; *total <- the workgroup's sum
__device__ uint64_t block_scan(uint64_t v, uint64_t* total) {
  __shared__ uint64_t part[kBlock];
  part[threadIdx.x] = v;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {       // Hillis-Steele
    const uint64_t below = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += below;
    __syncthreads();
  }
  *total = part[kBlock - 1];
  return part[threadIdx.x] - v;
}

template <class Load>
__global__ __launch_bounds__(kBlock) void k_scan_sums(Load load, long long count, uint64_t* __restrict__ sums) {
  const long long lo = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kPerLane;
  uint64_t sum = 0;
  for (int e = 0; e < kPerLane; ++e)
    if (lo + e < count) sum += load(lo + e);
  uint64_t total;
  block_scan(sum, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums <- their exclusive scan
__global__ __launch_bounds__(kTopBlock) void k_scan_top(uint64_t* sums, long long blocks) {
  __shared__ uint64_t part[kTopBlock];
  const long long per = (blocks + kTopBlock - 1) / kTopBlock;
  const long long lo = (long long)threadIdx.x * per < blocks ? (long long)threadIdx.x * per : blocks;
  const long long hi = lo + per < blocks ? lo + per : blocks;
  uint64_t sum = 0;
  for (long long b = lo; b < hi; ++b) sum += sums[b];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < kTopBlock; d <<= 1) {
    const uint64_t below = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += below;
    __syncthreads();
  }
  uint64_t run = part[threadIdx.x] - sum;
  for (long long b = lo; b < hi; ++b) {
    const uint64_t c = sums[b];
    sums[b] = run;
    run += c;
  }
}

// out may be the array `load` reads: a lane has read its kPerLane elements before it writes them,
// and no other lane reads them
template <class Load, class Out>
__global__ __launch_bounds__(kBlock) void k_scan_apply(Load load, long long count, const uint64_t* __restrict__ sums,
                                                       Out* out) {
  const long long lo = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kPerLane;
  uint64_t v[kPerLane], sum = 0;
  for (int e = 0; e < kPerLane; ++e) {
    v[e] = lo + e < count ? load(lo + e) : 0;
    sum += v[e];
  }
  uint64_t total;
  uint64_t run = sums[blockIdx.x] + block_scan(sum, &total);
  for (int e = 0; e < kPerLane; ++e) {
    if (lo + e < count) out[lo + e] = (Out)run;
    run += v[e];
  }
}

long long scan_blocks(long long count) { return (count + kScanTile - 1) / kScanTile; }

template <class Load, class Out>
hipError_t run_scan(Load load, long long count, uint64_t* sums, Out* out, hipStream_t st) {
  const long long nb = scan_blocks(count);
  hipLaunchKernelGGL(k_scan_sums<Load>, dim3((unsigned)nb), dim3(kBlock), 0, st, load, count, sums);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kTopBlock), 0, st, sums, nb);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_scan_apply<Load, Out>), dim3((unsigned)nb), dim3(kBlock), 0, st, load, count,
                     (const uint64_t*)sums, out);
  return hipGetLastError();
}

// ---- the partition ----------------------------------------------------------------------------------

struct LdsAtomics {
  static __device__ void add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
};

// LDS: one word per slot. Integer adds: the sums do not depend on the order of the lanes.
__global__ __launch_bounds__(kBlock) void k_histogram(const int32_t* __restrict__ bucket, long long n, int buckets,
                                                      long long tiles, uint32_t* __restrict__ counts) {
  extern __shared__ uint32_t hist[];
  const int S = buckets + 1;
  for (int s = threadIdx.x; s < S; s += kBlock) hist[s] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * kTile;
  for (int r = 0; r < kRounds; ++r) {
    const long long i = base + r * kBlock + threadIdx.x;
    if (i < n) count_row<LdsAtomics>(hist, bucket[i], buckets);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < S; s += kBlock) counts[counts_index(s, blockIdx.x, tiles)] = hist[s];
}

// the lanes of the wave whose row is in slot s, by one 64-bit ballot per bit of the slot number; every
// lane of the wave calls it (nbits is uniform), a lane without a row gets 0
__device__ unsigned long long peers_of(int s, bool valid, int nbits) {
  unsigned long long m = __ballot(valid);
  for (int b = 0; b < nbits; ++b) {
    const bool bit = (s >> b) & 1;
    const unsigned long long set = __ballot(valid && bit);
    m &= bit ? set : ~set;
  }
  return valid ? m : 0ull;
}

// LDS: base [S] uint32, then rel [kWaves][S] uint16. Wave w ranks the rows base + w * kChunk ..: its
// counter of a slot runs through the places, relative to the tile's first row of the slot, of its own
// rows of that slot (at most kTile, which a uint16 holds). Only the lowest lane among equal slots
// touches a counter, so the lanes of a wave never meet on a word, and no wave touches another's.
__global__ __launch_bounds__(kBlock) void k_scatter(const int32_t* __restrict__ bucket, long long n, int buckets, int nbits,
                                                    long long tiles, const uint32_t* __restrict__ counts,
                                                    long long* __restrict__ order, long long* __restrict__ starts) {
  extern __shared__ uint32_t lds[];
  const int S = buckets + 1;
  uint32_t* base = lds;
  uint16_t* rel = reinterpret_cast<uint16_t*>(lds + S);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint16_t* mine = rel + wave * S;
  for (int s = threadIdx.x; s < kWaves * S; s += kBlock) rel[s] = 0;
  __syncthreads();
  const long long first = (long long)blockIdx.x * kTile + wave * kChunk;
  const unsigned long long below = (1ull << lane) - 1;
  int slot[kRounds];
  for (int r = 0; r < kRounds; ++r) {
    const long long i = first + r * 64 + lane;
    const bool valid = i < n;
    slot[r] = valid ? slot_of(bucket[i], buckets) : -1;
    const unsigned long long peers = peers_of(slot[r], valid, nbits);
    if (valid && !(peers & below)) mine[slot[r]] = (uint16_t)(mine[slot[r]] + __popcll(peers));
  }
  __syncthreads();
  for (int s = threadIdx.x; s < S; s += kBlock) {
    uint32_t run = 0;
    for (int w = 0; w < kWaves; ++w) {
      const uint32_t c = rel[w * S + s];
      rel[w * S + s] = (uint16_t)run;
      run += c;
    }
    base[s] = counts[counts_index(s, blockIdx.x, tiles)];
    if (blockIdx.x == 0) starts[s] = (long long)base[s];
  }
  __syncthreads();
  for (int r = 0; r < kRounds; ++r) {
    const long long i = first + r * 64 + lane;
    const bool valid = slot[r] >= 0;
    const unsigned long long peers = peers_of(slot[r], valid, nbits);
    const uint32_t rank = (uint32_t)__popcll(peers & below);
    uint32_t old = 0;
    if (valid && rank == 0) {
      old = mine[slot[r]];
      mine[slot[r]] = (uint16_t)(old + __popcll(peers));
    }
    old = __shfl(old, valid ? __ffsll((long long)peers) - 1 : lane);
    if (valid) {
      const long long at = (long long)base[slot[r]] + old + rank;
      if (at < n) order[at] = i;        // always, unless `bucket` changed between the launches
    }
  }
}

// one lane per string
__global__ __launch_bounds__(kBlock) void k_gather(const uint8_t* __restrict__ chars, const long long* __restrict__ offsets,
                                                   const long long* __restrict__ order, long long n,
                                                   uint8_t* __restrict__ out_chars,
                                                   const long long* __restrict__ out_offsets) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const long long r = order[i];
  if (r < 0 || r >= n) return;
  const uint8_t* src = chars + offsets[r];
  const long long len = offsets[r + 1] - offsets[r];
  uint8_t* dst = out_chars + out_offsets[i];
  for (long long j = 0; j < len; ++j) dst[j] = src[j];
}

long long blocks_of(long long n) { return (n + kBlock - 1) / kBlock; }

long long slots_total(long long n, int buckets) { return (long long)(buckets + 1) * tiles_of(n); }

size_t partition_scratch(long long n, int buckets) {
  const long long M = slots_total(n, buckets);
  return (size_t)scan_blocks(M) * 8 + (size_t)M * 4;
}

size_t gather_scratch(long long n) { return (size_t)scan_blocks(n + 1) * 8; }

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

bool buckets_ok(int buckets) { return buckets >= 1 && buckets <= kMaxBuckets; }

int bad_buckets(int buckets) {
  set_error("%d buckets: 1 <= buckets <= %d", buckets, kMaxBuckets);
  return EFL_E_INVALID_ARGUMENT;
}

int bad_scratch(const char* fn, int64_t have, size_t need) {
  set_error("scratch of %lld bytes, %s = %lld", (long long)have, fn, (long long)need);
  return EFL_E_INVALID_ARGUMENT;
}

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API int32_t efl_mmh3_hash_host(const void* data, int64_t len, uint32_t seed) {
  if (len < 0 || (!data && len > 0)) return 0;
  return (int32_t)murmur3_x86_32(static_cast<const uint8_t*>(data), len, seed);
}

EFL_API int efl_mmh3_hash_rows_host(const char* chars, const int64_t* offsets, int64_t n, uint32_t seed, int32_t* out) {
  const int rc = check_rows(n, {chars, offsets, out});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (n > kMaxRows) return too_many(n);
  const uint8_t* c = reinterpret_cast<const uint8_t*>(chars);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t len = offsets[i + 1] - offsets[i];
    out[i] = (int32_t)murmur3_x86_32(c + offsets[i], len > 0 ? len : 0, seed);
  }
  return EFL_OK;
}

EFL_API int32_t efl_mmh3_checksum_host(int32_t cur, const char* chars, const int64_t* offsets, int64_t n) {
  if (n <= 0 || !chars || !offsets) return cur;
  const uint8_t* c = reinterpret_cast<const uint8_t*>(chars);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t len = offsets[i + 1] - offsets[i];
    cur = checksum_add(cur, c + offsets[i], len > 0 ? len : 0);
  }
  return cur;
}

EFL_API int efl_mmh3_hash(const char* chars, const int64_t* offsets, int64_t n, uint32_t seed, int32_t* out,
                          void* stream) {
  const int rc = check_rows(n, {chars, offsets, out});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (!aligned(offsets, 8) || !aligned(out, 4)) return invalid("offsets or out is misaligned");
  if (n > kMaxRows) return too_many(n);
  hipLaunchKernelGGL(k_mmh3, dim3((unsigned)blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint8_t*>(chars), reinterpret_cast<const long long*>(offsets), (long long)n,
                     seed, out);
  return hip_status(hipGetLastError(), "efl_mmh3_hash");
}

EFL_API int efl_bucket_ids(const int32_t* hash, int64_t n, int64_t modulus, int32_t divisor, int32_t* out, void* stream) {
  const int rc = check_rows(n, {hash, out});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (divisor < 1 || modulus < divisor || modulus > 0x7FFFFFFF) {
    set_error("modulus %lld, divisor %d: 1 <= divisor <= modulus <= 2^31 - 1", (long long)modulus, (int)divisor);
    return EFL_E_INVALID_ARGUMENT;
  }
  if (!aligned(hash, 4) || !aligned(out, 4)) return invalid("hash or out is misaligned");
  if (n > kMaxRows) return too_many(n);
  hipLaunchKernelGGL(k_bucket_ids, dim3((unsigned)blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, hash,
                     (long long)n, (long long)modulus, divisor, out);
  return hip_status(hipGetLastError(), "efl_bucket_ids");
}

EFL_API int64_t efl_bucket_scratch_bytes(int64_t n, int buckets) {
  return n <= 0 || n > kMaxRows || !buckets_ok(buckets) ? 0 : (int64_t)partition_scratch(n, buckets);
}

EFL_API int efl_bucket_partition(const int32_t* bucket, int64_t n, int buckets, int64_t* order, int64_t* starts,
                                 void* scratch, int64_t scratch_len, void* stream) {
  const int rc = check_rows(n, {bucket, order, starts, scratch});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (!buckets_ok(buckets)) return bad_buckets(buckets);
  if (!aligned(bucket, 4) || !aligned(order, 8) || !aligned(starts, 8) || !aligned(scratch, 8))
    return invalid("bucket, order, starts or scratch is misaligned");
  if (n > kMaxRows) return too_many(n);
  if (scratch_len < (int64_t)partition_scratch(n, buckets))
    return bad_scratch("efl_bucket_scratch_bytes(n, buckets)", scratch_len, partition_scratch(n, buckets));
  hipStream_t st = (hipStream_t)stream;
  const long long N = n, tiles = tiles_of(N), M = slots_total(N, buckets);
  const int S = buckets + 1;
  int nbits = 0;
  while ((1 << nbits) <= buckets) ++nbits;       // slot numbers run to `buckets` itself
  uint64_t* sums = static_cast<uint64_t*>(scratch);
  uint32_t* counts = reinterpret_cast<uint32_t*>(sums + scan_blocks(M));
  hipLaunchKernelGGL(k_histogram, dim3((unsigned)tiles), dim3(kBlock), (size_t)S * 4, st, bucket, N, buckets, tiles, counts);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = run_scan(LoadCounts{counts}, M, sums, counts, st);
  if (e != hipSuccess) return hip_status(e, "efl_bucket_partition");
  hipLaunchKernelGGL(k_scatter, dim3((unsigned)tiles), dim3(kBlock), (size_t)S * 4 + (size_t)kWaves * S * 2, st, bucket, N,
                     buckets, nbits, tiles, (const uint32_t*)counts, reinterpret_cast<long long*>(order),
                     reinterpret_cast<long long*>(starts));
  return hip_status(hipGetLastError(), "efl_bucket_partition");
}

EFL_API int64_t efl_strings_gather_scratch_bytes(int64_t n) {
  return n <= 0 || n > kMaxRows ? 0 : (int64_t)gather_scratch(n);
}

EFL_API int efl_strings_gather(const char* chars, const int64_t* offsets, const int64_t* order, int64_t n,
                               char* out_chars, int64_t* out_offsets, void* scratch, int64_t scratch_len, void* stream) {
  const int rc = check_rows(n, {chars, offsets, order, out_chars, out_offsets, scratch});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (!aligned(offsets, 8) || !aligned(order, 8) || !aligned(out_offsets, 8) || !aligned(scratch, 8))
    return invalid("offsets, order, out_offsets or scratch is misaligned");
  if (n > kMaxRows) return too_many(n);
  if (scratch_len < (int64_t)gather_scratch(n))
    return bad_scratch("efl_strings_gather_scratch_bytes(n)", scratch_len, gather_scratch(n));
  hipStream_t st = (hipStream_t)stream;
  const long long N = n;
  const long long* off = reinterpret_cast<const long long*>(offsets);
  const long long* ord = reinterpret_cast<const long long*>(order);
  long long* out_off = reinterpret_cast<long long*>(out_offsets);
  const hipError_t e = run_scan(LoadLengths{off, ord, N}, N + 1, static_cast<uint64_t*>(scratch), out_off, st);
  if (e != hipSuccess) return hip_status(e, "efl_strings_gather");
  hipLaunchKernelGGL(k_gather, dim3((unsigned)blocks_of(N)), dim3(kBlock), 0, st, reinterpret_cast<const uint8_t*>(chars),
                     off, ord, N, reinterpret_cast<uint8_t*>(out_chars), (const long long*)out_off);
  return hip_status(hipGetLastError(), "efl_strings_gather");
}
