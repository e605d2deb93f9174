// The bucket hash of efl.psi (efl.psi.bucket): MurmurHash3_x86_32 as the reference's `mmh3.hash`
// gives it (efls-data/xfl/data/functions.py:37-46, xfl/data/check_sum.py), Python's `%` of the signed
// result, and the per-row steps of the bucket partition. Plain C++: the kernels of bucket.hip, the
// host entry points (efl_mmh3_hash_host, efl_mmh3_checksum_host) and the host program of
// tests/test_mmh3_host.py are all compiled from this header.
//
// The hash is Austin Appleby's public-domain MurmurHash3_x86_32 (SMHasher verification value
// 0xB0F57EE3): 4-byte blocks read little-endian, the 1 to 3 tail bytes as unsigned bytes, fmix32 of
// the state xor the length.
//
// The partition is a stable counting sort of n rows by bucket, tile by tile (kTile rows each). Row
// i's slot is its bucket, or `buckets` (one slot past the last bucket) when bucket[i] is outside
// [0, buckets). With S = buckets + 1 slots and T tiles the steps are
//   histogram  counts[s * T + t] <- the rows of tile t in slot s       (slot-major, tile-minor)
//   scan       counts <- its exclusive scan in that order: entry (s, t) becomes the place in `order`
//              of tile t's first row of slot s, and entry (s, 0) is starts[s]
//   scatter    the rows of tile t in ascending order: order[counts[s * T + t] + (rows of the tile
//              before this one in the same slot)] <- i
// each a launch of its own on the device, so the only order between them is the launch boundary.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define EFL_MMH3_FN __host__ __device__ inline
#else
#define EFL_MMH3_FN inline
#endif

namespace efl {
namespace mmh3 {

EFL_MMH3_FN uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

EFL_MMH3_FN uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

EFL_MMH3_FN uint32_t mix_k(uint32_t k) { return rotl32(k * 0xCC9E2D51u, 15) * 0x1B873593u; }

// one 4-byte block into the state
EFL_MMH3_FN uint32_t mix_block(uint32_t h, uint32_t k) { return rotl32(h ^ mix_k(k), 13) * 5u + 0xE6546B64u; }

// MurmurHash3_x86_32 of p[0 .. len): any length, any alignment; every byte is read as unsigned and
// once. The length enters the final mix modulo 2^32, as in the original.
EFL_MMH3_FN uint32_t murmur3_x86_32(const uint8_t* p, int64_t len, uint32_t seed) {
  uint32_t h = seed;
  const int64_t blocks = len >> 2;
  for (int64_t b = 0; b < blocks; ++b, p += 4)
    h = mix_block(h, (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
  uint32_t k = 0;
  switch (len & 3) {
    case 3: k |= (uint32_t)p[2] << 16; [[fallthrough]];
    case 2: k |= (uint32_t)p[1] << 8; [[fallthrough]];
    case 1: k |= (uint32_t)p[0]; h ^= mix_k(k);
  }
  return fmix32(h ^ (uint32_t)len);
}

// Python's h % m for m > 0: in [0, m) for negative h too
EFL_MMH3_FN int64_t floor_mod(int32_t h, int64_t m) {
  const int64_t r = (int64_t)h % m;
  return r < 0 ? r + m : r;
}

// DefaultKeySelector.get_key is bucket_id(h, bucket_num * c, c), get_local_bucket_id is bucket_id(h, c, 1)
EFL_MMH3_FN int32_t bucket_id(int32_t h, int64_t modulus, int32_t divisor) {
  return (int32_t)(floor_mod(h, modulus) / divisor);
}

// ---- the partition --------------------------------------------------------------------------------

constexpr int kMaxBuckets = 4096;
constexpr int kTile = 2048;                          // rows per tile: 256 lanes x 8
constexpr int64_t kMaxRows = 0x7FFFFFFE;             // 2^31 - 2, as the ID store's batches

EFL_MMH3_FN int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }

// a row's slot: its bucket, or the overflow slot `buckets`
EFL_MMH3_FN int slot_of(int32_t bucket, int buckets) { return bucket >= 0 && bucket < buckets ? (int)bucket : buckets; }

EFL_MMH3_FN int64_t counts_index(int slot, int64_t tile, int64_t tiles) { return (int64_t)slot * tiles + tile; }

// histogram, one row: A::add(p, 1) is the only operation two rows of a tile may apply to one word
template <class A>
EFL_MMH3_FN void count_row(uint32_t* tile_hist, int32_t bucket, int buckets) {
  A::add(tile_hist + slot_of(bucket, buckets), 1u);
}

// the serial form of the scan: v <- its exclusive scan, the total returned
template <class T>
inline uint64_t exclusive_scan(T* v, int64_t count) {
  uint64_t run = 0;
  for (int64_t j = 0; j < count; ++j) {
    const uint64_t c = (uint64_t)v[j];
    v[j] = (T)run;
    run += c;
  }
  return run;
}

// scatter, one row, the rows of a tile taken in ascending order: `cursor` (one word per slot) starts
// as the tile's scanned counts
inline void scatter_row(uint32_t* cursor, int32_t bucket, int buckets, int64_t i, int64_t* order) {
  order[cursor[slot_of(bucket, buckets)]++] = i;
}

// ---- CheckSum ---------------------------------------------------------------------------------------

// str(cur).encode() into out (at most 11 bytes: a '-' and ten digits); the length
EFL_MMH3_FN int decimal_of(int32_t cur, uint8_t out[11]) {
  uint8_t rev[10];
  uint32_t m = cur < 0 ? 0u - (uint32_t)cur : (uint32_t)cur;      // |INT32_MIN| fits the unsigned form
  int d = 0;
  do {
    rev[d++] = (uint8_t)('0' + m % 10u);
    m /= 10u;
  } while (m);
  int len = 0;
  if (cur < 0) out[len++] = '-';
  while (d) out[len++] = rev[--d];
  return len;
}

// CheckSum.add: mmh3.hash(str(cur).encode() + value), seed 0, without building the concatenation:
// the blocks are taken from the two pieces through one index
inline int32_t checksum_add(int32_t cur, const uint8_t* value, int64_t len) {
  uint8_t head[11];
  const int hl = decimal_of(cur, head);
  const int64_t total = hl + len;
  auto at = [&](int64_t j) -> uint32_t { return j < hl ? head[j] : value[j - hl]; };
  uint32_t h = 0;
  const int64_t blocks = total >> 2;
  for (int64_t b = 0; b < blocks; ++b)
    h = mix_block(h, at(4 * b) | at(4 * b + 1) << 8 | at(4 * b + 2) << 16 | at(4 * b + 3) << 24);
  uint32_t k = 0;
  const int64_t t = 4 * blocks;
  switch (total & 3) {
    case 3: k |= at(t + 2) << 16; [[fallthrough]];
    case 2: k |= at(t + 1) << 8; [[fallthrough]];
    case 1: k |= at(t); h ^= mix_k(k);
  }
  return (int32_t)fmix32(h ^ (uint32_t)total);
}

}  // namespace mmh3
}  // namespace efl
