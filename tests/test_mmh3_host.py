"""CPU: the host side of the bucket hash (efl.psi.bucket). csrc/mmh3.h, the header the efl_mmh3_* and
efl_bucket_* kernels are compiled from, is compiled by g++ under ASan and UBSan into a stand-alone
program that checks MurmurHash3_x86_32 (SMHasher's verification value, the published vectors, every
length at every start offset inside a guarded buffer, bytes >= 0x80 in every tail position), floor_mod
at the ends of the int32 range, the CheckSum step against the concatenation it stands for, and the
partition's serial steps (histogram in three row orders, scan, scatter) against std::stable_sort;
mmh3_hash / efl_mmh3_hash_host / efl_mmh3_hash_rows_host against tests/golden/mmh3_kat.json."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG

with open(os.path.join(GOLDEN, "mmh3_kat.json")) as _f:
    KAT = json.load(_f)

HOST_MAIN = r"""
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "mmh3.h"
using namespace efl::mmh3;

static int bad = 0;
#define CHECK(c, ...) do { if (!(c)) { ++bad; printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t lcg = 0x243F6A8885A308D3ull;
static uint64_t rnd() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg >> 11; }

static uint32_t hash_str(const char* s, uint32_t seed) { return murmur3_x86_32((const uint8_t*)s, (int64_t)strlen(s), seed); }

// the hash of a copy that ends exactly at the end of a heap block (ASan guards the byte after it)
static uint32_t hash_guarded(const uint8_t* p, int64_t len, uint32_t seed) {
  uint8_t* g = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(g, p, len);
  const uint32_t h = murmur3_x86_32(len ? g : g + 1, len, seed);     // len == 0: a pointer nothing may be read from
  free(g);
  return h;
}

struct Plain {
  static void add(uint32_t* p, uint32_t v) { *p += v; }
};

// the partition by its serial steps; perm: the order in which the rows of a tile run the histogram step
static void partition(const std::vector<int32_t>& bucket, int buckets, int perm) {
  const int64_t n = (int64_t)bucket.size(), tiles = tiles_of(n);
  const int S = buckets + 1;
  std::vector<uint32_t> counts((size_t)S * tiles, 0), hist(S);
  for (int64_t t = 0; t < tiles; ++t) {
    std::fill(hist.begin(), hist.end(), 0u);
    const int64_t lo = t * kTile, m = std::min<int64_t>(kTile, n - lo);
    for (int64_t k = 0; k < m; ++k) {
      const int64_t j = perm == 0 ? k : perm == 1 ? m - 1 - k : (k * 7919 + 13) % m;   // 7919 is prime: a permutation for m < 7919
      count_row<Plain>(hist.data(), bucket[lo + j], buckets);
    }
    for (int s = 0; s < S; ++s) counts[counts_index(s, t, tiles)] = hist[s];
  }
  const uint64_t total = exclusive_scan(counts.data(), (int64_t)counts.size());
  CHECK(total == (uint64_t)n, "the counts sum to %llu of %lld rows", (unsigned long long)total, (long long)n);
  std::vector<int64_t> order(n, -1), starts(S);
  for (int s = 0; s < S && tiles; ++s) starts[s] = counts[counts_index(s, 0, tiles)];
  std::vector<uint32_t> cursor(S);
  for (int64_t t = 0; t < tiles; ++t) {
    for (int s = 0; s < S; ++s) cursor[s] = counts[counts_index(s, t, tiles)];
    for (int64_t i = t * kTile; i < std::min<int64_t>(n, (t + 1) * kTile); ++i) scatter_row(cursor.data(), bucket[i], buckets, i, order.data());
  }
  // the model: a stable sort by slot
  std::vector<int64_t> want(n);
  for (int64_t i = 0; i < n; ++i) want[i] = i;
  std::stable_sort(want.begin(), want.end(), [&](int64_t a, int64_t b) { return slot_of(bucket[a], buckets) < slot_of(bucket[b], buckets); });
  CHECK(order == want, "n=%lld buckets=%d perm=%d: order differs from std::stable_sort", (long long)n, buckets, perm);
  std::vector<int64_t> sizes(S + 1, 0);
  for (int64_t i = 0; i < n; ++i) ++sizes[slot_of(bucket[i], buckets) + 1];
  for (int s = 0; s < S; ++s) sizes[s + 1] += sizes[s];
  for (int s = 0; s < S && tiles; ++s) CHECK(starts[s] == sizes[s], "starts[%d] = %lld, want %lld", s, (long long)starts[s], (long long)sizes[s]);
}

int main() {
  // SMHasher's verification value
  {
    uint8_t key[256], blob[1024];
    for (int i = 0; i < 256; ++i) {
      key[i] = (uint8_t)i;
      const uint32_t h = murmur3_x86_32(key, i, (uint32_t)(256 - i));
      for (int b = 0; b < 4; ++b) blob[4 * i + b] = (uint8_t)(h >> (8 * b));
    }
    const uint32_t v = murmur3_x86_32(blob, 1024, 0);
    CHECK(v == 0xB0F57EE3u, "verification value 0x%08X", v);
    printf("verification 0x%08X\n", v);
  }
  // the published vectors
  CHECK(hash_str("", 0) == 0u, "empty");
  CHECK(hash_str("test", 0) == 0xBA6BD213u, "test");
  CHECK(hash_str("Hello, world!", 0) == 0xC0363E43u, "Hello, world!");
  CHECK(hash_str("The quick brown fox jumps over the lazy dog", 0) == 0x2E4FF723u, "fox");
  CHECK((int32_t)hash_str("hello", 0) == 613153351, "hello");
  CHECK((int32_t)hash_str("foo", 0) == -156908512, "foo");
  CHECK(hash_str("abc", 0) == 0xB3DD93FAu, "abc");
  CHECK(hash_str("", 1) == 0x514E28B7u, "empty, seed 1");
  CHECK(hash_str("", 0xFFFFFFFFu) == 0x81F16F39u, "empty, seed -1");
  CHECK(hash_str("aaaa", 0x9747B28Cu) == 0x5A97808Au, "aaaa");
  // every length 0..67 at every start offset 0..7: the same bytes give the same hash wherever they start,
  // and nothing outside [p, p + len) is read (the guarded copy ends at the end of its heap block)
  {
    std::vector<uint8_t> data(80);
    for (auto& b : data) b = (uint8_t)rnd();
    for (int len = 0; len <= 67; ++len) {
      const uint32_t want = hash_guarded(data.data(), len, 7);
      for (int off = 0; off < 8; ++off) {
        uint8_t* g = (uint8_t*)malloc(off + len + (off + len ? 0 : 1));
        memcpy(g + off, data.data(), len);
        CHECK(murmur3_x86_32(g + off, len, 7) == want, "len %d at offset %d", len, off);
        free(g);
      }
    }
  }
  // a byte >= 0x80 in every tail position: read as unsigned (a sign-extended tail changes the higher bytes of k)
  for (int len = 1; len <= 7; ++len)
    for (int pos = len - len % 4; pos < len; ++pos)
      for (int v = 0x80; v < 0x100; v += 0x7F) {
        uint8_t d[8];
        memset(d, 'a', sizeof d);
        d[pos] = (uint8_t)v;
        // the definition, block by block, over unsigned bytes
        uint32_t h = 3;
        if (len >= 4) h = mix_block(h, d[0] | d[1] << 8 | d[2] << 16 | (uint32_t)d[3] << 24);
        uint32_t k = 0;
        for (int j = len - 1; j >= len - len % 4; --j) k = k << 8 | d[j];
        h ^= mix_k(k);
        CHECK(murmur3_x86_32(d, len, 3) == fmix32(h ^ (uint32_t)len), "0x%02X at %d of %d", v, pos, len);
      }
  // floor_mod: Python's % of the signed hash
  {
    const int64_t moduli[] = {1, 2, 3, 64, 1000, 2147483647};
    const int32_t hs[] = {INT32_MIN, -1, 0, INT32_MAX};
    // Python: [[h % m for m in moduli] for h in hs]
    const int64_t want[4][6] = {{0, 0, 1, 0, 352, 2147483646}, {0, 1, 2, 63, 999, 2147483646}, {0, 0, 0, 0, 0, 0}, {0, 1, 1, 63, 647, 0}};
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 6; ++b) {
        const int64_t r = floor_mod(hs[a], moduli[b]);
        CHECK(r == want[a][b], "floor_mod(%d, %lld) = %lld, want %lld", hs[a], (long long)moduli[b], (long long)r, (long long)want[a][b]);
        CHECK(r >= 0 && r < moduli[b], "floor_mod(%d, %lld) out of range", hs[a], (long long)moduli[b]);
      }
    CHECK(bucket_id(-1, 64 * 3, 3) == 63 && bucket_id(INT32_MIN, 6, 3) == 1 && bucket_id(-5, 6, 3) == 0 && bucket_id(-4, 6, 3) == 0 && bucket_id(-3, 6, 3) == 1, "bucket_id");
  }
  // CheckSum's step against the concatenation it stands for, at the ends of the range and value lengths 0..9
  {
    const int32_t curs[] = {0, 7, -7, 1234567890, -1234567890, INT32_MAX, INT32_MIN, 10, -10, 99999, -100000};
    for (int32_t cur : curs)
      for (int len = 0; len < 10; ++len) {
        uint8_t value[16];
        for (auto& b : value) b = (uint8_t)rnd();
        const std::string text = std::to_string(cur) + std::string((const char*)value, len);
        const int32_t want = (int32_t)murmur3_x86_32((const uint8_t*)text.data(), (int64_t)text.size(), 0);
        CHECK(checksum_add(cur, value, len) == want, "checksum_add(%d, %d bytes)", cur, len);
      }
  }
  // the partition
  int runs = 0;
  {
    const int64_t sizes[] = {0, 1, 63, 64, 65, kTile - 1, kTile, kTile + 1, 3 * kTile + 17};
    const int bucket_counts[] = {1, 2, 64, 4096};
    for (int64_t n : sizes)
      for (int buckets : bucket_counts)
        for (int perm = 0; perm < 3; ++perm) {
          std::vector<int32_t> b(n);
          for (auto& v : b) v = (int32_t)(rnd() % buckets);
          partition(b, buckets, perm);
          ++runs;
        }
    for (int perm = 0; perm < 3; ++perm) {
      const int64_t n = 2 * kTile + 5;
      std::vector<int32_t> b(n, 0);
      partition(b, 64, perm);                                    // all rows in the first bucket
      std::fill(b.begin(), b.end(), 63);
      partition(b, 64, perm);                                    // ... in the last
      for (int64_t i = 0; i < n; ++i) b[i] = (int32_t)(n - 1 - i);
      partition(b, 4096, perm);                                  // one row per bucket while they last, the rest in none
      for (int64_t i = 0; i < n; ++i) b[i] = (i % 7 == 0) ? -1 - (int32_t)i : (i % 5 == 0) ? 64 : (i % 3 ? 3 : 60);
      partition(b, 64, perm);                                    // many empty buckets, rows without a bucket
      b.assign(n, INT32_MIN);
      b[5] = INT32_MAX;
      partition(b, 2, perm);                                     // no row has a bucket
      runs += 5;
    }
  }
  printf("%d partitions\n", runs);
  printf("mmh3 host check: %d failures\n", bad);
  return bad ? 1 : 0;
}
"""


def test_mmh3_header_under_sanitizers(tmp_path):
    """The header the kernels are compiled from, as a host program of its own under ASan + UBSan."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = tmp_path / "mmh3_host.cpp"
    src.write_text(HOST_MAIN)
    exe = tmp_path / "mmh3_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "verification 0xB0F57EE3" in r.stdout
    assert "123 partitions" in r.stdout, r.stdout[-4000:]
    assert "mmh3 host check: 0 failures" in r.stdout, r.stdout[-4000:]


def test_golden_file_pins_the_hash():
    assert KAT["smhasher_verification"] == "0xB0F57EE3"
    assert KAT["decimal_ids"]["negative"] == 2129 and len(KAT["decimal_ids"]["hashes"]) == 4096
    by_input = {(bytes.fromhex(h["hex"]), h["seed"]): h["hash"] for h in KAT["hashes"]}
    assert by_input[(b"hello", 0)] == 613153351 and by_input[(b"foo", 0)] == -156908512
    assert by_input[(b"test", 0)] == 0xBA6BD213 - 2 ** 32 and by_input[(b"", 0xFFFFFFFF)] == 0x81F16F39 - 2 ** 32
    assert by_input[(b"aaaa", 0x9747B28C)] == 0x5A97808A


def test_mmh3_hash_against_the_golden_file():
    import efl
    lib = efl.lib.raw()
    for h in KAT["hashes"]:
        data = bytes.fromhex(h["hex"])
        assert efl.psi.mmh3_hash(data, h["seed"]) == h["hash"], h
        assert lib.efl_mmh3_hash_host(data, len(data), h["seed"]) == h["hash"], h
        assert efl.psi.mmh3_hash(bytearray(data), h["seed"]) == h["hash"]
        if "text" in h:
            assert efl.psi.mmh3_hash(h["text"], h["seed"]) == h["hash"]       # a str is hashed as UTF-8
    for i, want in enumerate(KAT["decimal_ids"]["hashes"]):
        assert efl.psi.mmh3_hash(str(i)) == want
    # a signed seed is the same 32 bits, as in mmh3
    assert efl.psi.mmh3_hash(b"", -1) == efl.psi.mmh3_hash(b"", 0xFFFFFFFF) == 0x81F16F39 - 2 ** 32
    assert efl.psi.mmh3_hash is efl.psi.bucket.mmh3_hash
    with pytest.raises(TypeError):
        efl.psi.mmh3_hash(5)
    # a null pointer and a negative length have no hash
    assert lib.efl_mmh3_hash_host(None, 3, 0) == 0 and lib.efl_mmh3_hash_host(b"abc", -1, 0) == 0
    assert lib.efl_mmh3_hash_host(None, 0, 1) == 0x514E28B7


def test_hash_rows_host_against_the_golden_file():
    """efl_mmh3_hash_rows_host over one packed buffer in which the strings start at every offset mod 4."""
    import efl
    lib = efl.lib.raw()
    for seed in (0, 1, 0xFFFFFFFF, 0x9747B28C):
        items = [h for h in KAT["hashes"] if h["seed"] == seed]
        data = [bytes.fromhex(h["hex"]) for h in items]
        offsets = np.zeros(len(data) + 1, dtype=np.int64)
        np.cumsum([len(d) for d in data], out=offsets[1:])
        chars = np.frombuffer(b"".join(data), dtype=np.uint8).copy()
        out = np.full(len(data), 12345, dtype=np.int32)
        assert lib.efl_mmh3_hash_rows_host(chars.ctypes.data, offsets.ctypes.data, len(data), seed, out.ctypes.data) == 0
        assert out.tolist() == [h["hash"] for h in items]
    assert lib.efl_mmh3_hash_rows_host(None, None, 0, 0, None) == 0
    assert lib.efl_mmh3_hash_rows_host(None, None, 3, 0, None) == -3
    assert lib.efl_mmh3_hash_rows_host(ctypes.c_void_p(8), ctypes.c_void_p(8), -1, 0, ctypes.c_void_p(8)) == -3
