// The signed-ID store of efl.psi (efl.psi.IdStore): what the reference keeps in a Python dict
// (efls-data/xfl/data/store/sample_kv_store.py, DictSampleKvStore) as an open-addressing hash table
// over fixed-width byte rows. Plain C++: the kernels of idset.hip, efl_idset_hash and the host
// program of tests/test_idset_host.py are all compiled from this header.
//
// Layout. `slots` is uint32 [capacity], capacity a power of two, linear probing. A slot holds
// kEmpty or an entry index e: the key of e is row e of the dense `keys` array (uint8 [.., W] in
// insertion order). While a batch is being inserted a slot may also hold kBatch | i, "claimed by row
// i of the batch", whose key is row i of the batch; the last insert kernel replaces each by the
// entry index it was given, so between calls a slot is kEmpty or an index below 2^31 - 1.
//
// One batch goes through five per-row steps, each a launch of its own (idset.hip), so the only
// order between them is the launch boundary and no step waits for another lane:
//   claim   every row walks its probe chain to a slot that holds its key, or claims the first empty
//           one with CAS(kEmpty -> kBatch | i); on a slot claimed by an equal row of the batch it
//           lowers the slot with min(kBatch | i), so the lowest row index among equal keys owns it
//   settle  row i reads its slot once more: it is the batch's winner for its key iff the slot holds
//           kBatch | i; winners are counted
//   (scan of the counts)
//   append  winners, ranked in row order, copy their row to keys[size0 + rank]
//   finish  every row's position; winners write the final entry index into their slot
// Every slot access of `claim` goes through the Atomics policy (agent-scope atomics on the device):
// it is the only step in which two lanes touch the same word. With at most capacity / 2 entries a
// probe chain ends at an empty slot; every loop is bounded by `capacity` all the same.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define EFL_IDSET_FN __host__ __device__ inline
#else
#define EFL_IDSET_FN inline
#endif

namespace efl {
namespace idset {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kBatch = 0x80000000u;
constexpr int64_t kMaxEntries = 0x7FFFFFFE;        // entries and batch rows: 2^31 - 2
constexpr int64_t kMaxCapacity = (int64_t)1 << 32;

// a row of W = 8 * WORDS bytes as little-endian 64-bit words
template <int WORDS>
struct Row {
  uint64_t w[WORDS];
};

// rows are 8-byte aligned for W = 8 and 16-byte aligned for W = 32
template <int WORDS>
EFL_IDSET_FN Row<WORDS> load_row(const uint8_t* base, int64_t i) {
  const uint64_t* p = static_cast<const uint64_t*>(
      __builtin_assume_aligned(base + i * (8 * WORDS), WORDS >= 2 ? 16 : 8));
  Row<WORDS> r;
  for (int j = 0; j < WORDS; ++j) r.w[j] = p[j];
  return r;
}

template <int WORDS>
EFL_IDSET_FN void store_row(uint8_t* base, int64_t i, const Row<WORDS>& r) {
  uint64_t* p = static_cast<uint64_t*>(__builtin_assume_aligned(base + i * (8 * WORDS), WORDS >= 2 ? 16 : 8));
  for (int j = 0; j < WORDS; ++j) p[j] = r.w[j];
}

template <int WORDS>
EFL_IDSET_FN bool equal(const Row<WORDS>& a, const Row<WORDS>& b) {
  uint64_t d = 0;
  for (int j = 0; j < WORDS; ++j) d |= a.w[j] ^ b.w[j];
  return d == 0;
}

// Seeded 64-bit mix of every word. Each step is a bijection of the state for a fixed word (xor, an
// odd multiplier, xor-shift), so two rows that differ in one word, or two seeds, never hash alike;
// rows that share a prefix share nothing of their probe chains unless the seed is known.
EFL_IDSET_FN uint64_t fmix(uint64_t h) {
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33;
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  return h;
}

template <int WORDS>
EFL_IDSET_FN uint64_t hash(uint64_t seed, const Row<WORDS>& r) {
  uint64_t h = fmix(seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)WORDS));
  for (int j = 0; j < WORDS; ++j) h = fmix((h ^ r.w[j]) * 0x9E3779B97F4A7C15ull + (uint64_t)j);
  return h;
}

// the key a slot value stands for during a batch
template <int WORDS>
EFL_IDSET_FN Row<WORDS> key_of(uint32_t e, const uint8_t* keys, const uint8_t* rows) {
  return (e & kBatch) ? load_row<WORDS>(rows, (int64_t)(e & ~kBatch)) : load_row<WORDS>(keys, (int64_t)e);
}

// claim: the slot of row i's key, or -1 if `capacity` probes found neither the key nor an empty
// slot (impossible at a load factor of 1/2). A: load / cas / min on one slot word.
template <class A, int WORDS>
EFL_IDSET_FN int64_t claim(uint32_t* slots, uint64_t capacity, uint64_t seed, const uint8_t* keys,
                           const uint8_t* rows, int64_t i) {
  const Row<WORDS> mine = load_row<WORDS>(rows, i);
  const uint32_t me = kBatch | (uint32_t)i;
  uint64_t h = hash<WORDS>(seed, mine) & (capacity - 1);
  for (uint64_t probes = 0; probes < capacity; ++probes, h = (h + 1) & (capacity - 1)) {
    uint32_t e = A::load(slots + h);
    if (e == kEmpty) {
      e = A::cas(slots + h, kEmpty, me);
      if (e == kEmpty) return (int64_t)h;
    }
    if (equal(mine, key_of<WORDS>(e, keys, rows))) {
      if (e & kBatch) A::min(slots + h, me);
      return (int64_t)h;
    }
  }
  return -1;
}

// settle (a later launch: plain loads): what row i's slot holds now; the row won iff it is kBatch | i
EFL_IDSET_FN uint32_t settle(const uint32_t* slots, int64_t slot) { return slot < 0 ? kEmpty : slots[slot]; }
EFL_IDSET_FN bool won(uint32_t settled, int64_t i) { return settled == (kBatch | (uint32_t)i); }

// finish: row's position from what settle read and the winners' ranks
EFL_IDSET_FN int64_t position(uint32_t settled, int64_t size0, const uint32_t* rank) {
  if (settled == kEmpty) return -1;
  return (settled & kBatch) ? size0 + (int64_t)rank[settled & ~kBatch] : (int64_t)settled;
}

// find: the entry index of `row`, or -1. Nothing writes during a find launch: plain loads.
template <int WORDS>
EFL_IDSET_FN int64_t find(const uint32_t* slots, uint64_t capacity, uint64_t seed, const uint8_t* keys,
                          const Row<WORDS>& row) {
  uint64_t h = hash<WORDS>(seed, row) & (capacity - 1);
  for (uint64_t probes = 0; probes < capacity; ++probes, h = (h + 1) & (capacity - 1)) {
    const uint32_t e = slots[h];
    if (e == kEmpty) return -1;
    if (equal(row, load_row<WORDS>(keys, (int64_t)e))) return (int64_t)e;
  }
  return -1;
}

// rehash: entry e (unique among the entries) takes the first empty slot of its chain
template <class A, int WORDS>
EFL_IDSET_FN bool place(uint32_t* slots, uint64_t capacity, uint64_t seed, const uint8_t* keys, int64_t e) {
  uint64_t h = hash<WORDS>(seed, load_row<WORDS>(keys, e)) & (capacity - 1);
  for (uint64_t probes = 0; probes < capacity; ++probes, h = (h + 1) & (capacity - 1))
    if (A::load(slots + h) == kEmpty && A::cas(slots + h, kEmpty, (uint32_t)e) == kEmpty) return true;
  return false;
}

// efl_idset_hash: bytes of any alignment
inline uint64_t hash_bytes(uint64_t seed, const uint8_t* row, int width) {
  uint64_t w[4] = {0, 0, 0, 0};
  for (int b = 0; b < width; ++b) w[b >> 3] |= (uint64_t)row[b] << (8 * (b & 7));
  if (width == 8) {
    Row<1> r{{w[0]}};
    return hash<1>(seed, r);
  }
  Row<4> r{{w[0], w[1], w[2], w[3]}};
  return hash<4>(seed, r);
}

}  // namespace idset
}  // namespace efl
