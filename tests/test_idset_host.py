"""CPU: the host side of the signed-ID store (efl.psi.IdStore). csrc/idset.h, the header the
efl_idset_* kernels are compiled from, is compiled by g++ under ASan and UBSan into a stand-alone
program that runs the per-row steps of an insert (claim, settle, rank, append, finish), of a find and
of a rehash serially, in three different row orders of the claim step (each a legal schedule of the
kernel), and checks them against a std::map; efl_idset_hash; the argument checks of efl_idset_insert
/ find / rehash (they run before any HIP call); IdStore's constructor and empty inputs."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from conftest import PKG

HOST_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "idset.h"
using namespace efl::idset;

// one lane at a time: the plain forms of the three slot operations
struct Serial {
  static uint32_t load(uint32_t* p) { return *p; }
  static uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) {
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
  }
  static void min(uint32_t* p, uint32_t v) {
    if (v < *p) *p = v;
  }
};

struct alignas(16) Block { uint8_t b[32]; };
static int bad = 0;
#define CHECK(c, ...) do { if (!(c)) { ++bad; printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t lcg = 0x243F6A8885A308D3ull;
static uint64_t rnd() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg >> 11; }

template <int WORDS>
struct Store {
  static constexpr int W = 8 * WORDS;
  std::vector<uint32_t> slots;
  std::vector<Block> keys;          // W bytes per key, packed
  int64_t size = 0;
  uint64_t seed, capacity;
  std::map<std::string, int64_t> model;
  std::vector<std::string> order;

  Store(uint64_t cap, uint64_t s) : slots(cap, kEmpty), keys(cap / 2 * W / 32 + 1), seed(s), capacity(cap) {}
  uint8_t* kp() { return keys[0].b; }

  void grow(int64_t n) {
    if (capacity >= 2 * (uint64_t)(size + n)) return;
    while (capacity < 2 * (uint64_t)(size + n)) capacity *= 2;
    keys.resize(capacity / 2 * W / 32 + 1);
    slots.assign(capacity, kEmpty);
    for (int64_t e = 0; e < size; ++e) CHECK((place<Serial, WORDS>(slots.data(), capacity, seed, kp(), e)), "place %lld", (long long)e);
  }

  // perm: the order in which the rows run their claim step
  void insert(const std::vector<Block>& batch, int64_t n, int perm) {
    grow(n);
    const uint8_t* rows = batch[0].b;
    const int64_t size0 = size;
    std::vector<int64_t> slot(n), pos(n);
    std::vector<uint32_t> settled(n), rank(n);
    for (int64_t k = 0; k < n; ++k) {
      const int64_t i = perm == 0 ? k : perm == 1 ? n - 1 - k : (k * 7919 + 13) % n;   // 7919 is prime: a permutation for n < 7919
      slot[i] = claim<Serial, WORDS>(slots.data(), capacity, seed, kp(), rows, i);
      CHECK(slot[i] >= 0, "claim %lld", (long long)i);
    }
    for (int64_t i = 0; i < n; ++i) settled[i] = settle(slots.data(), slot[i]);
    uint32_t r = 0;
    for (int64_t i = 0; i < n; ++i) {
      rank[i] = r;
      if (won(settled[i], i)) store_row<WORDS>(kp(), size0 + r++, load_row<WORDS>(rows, i));
    }
    for (int64_t i = 0; i < n; ++i) {
      if (won(settled[i], i)) slots[slot[i]] = (uint32_t)(size0 + rank[i]);
      pos[i] = position(settled[i], size0, rank.data());
    }
    size += r;
    // the dict
    for (int64_t i = 0; i < n; ++i) {
      const std::string k((const char*)rows + i * W, W);
      auto it = model.find(k);
      if (it == model.end()) {
        it = model.emplace(k, (int64_t)model.size()).first;
        order.push_back(k);
      }
      CHECK(pos[i] == it->second, "row %lld at %lld, the dict says %lld", (long long)i, (long long)pos[i], (long long)it->second);
    }
    verify();
  }

  void verify() {
    CHECK(size == (int64_t)model.size(), "size %lld vs %zu", (long long)size, model.size());
    for (int64_t e = 0; e < size && e < (int64_t)order.size(); ++e)
      CHECK(!memcmp(kp() + e * W, order[e].data(), W), "key %lld out of insertion order", (long long)e);
    int64_t used = 0;
    for (uint32_t s : slots) {
      CHECK(s == kEmpty || (int64_t)s < size, "slot value %u left behind", s);
      used += s != kEmpty;
    }
    CHECK(used == size, "%lld slots used for %lld keys", (long long)used, (long long)size);
    for (int64_t e = 0; e < size; ++e)
      CHECK(find<WORDS>(slots.data(), capacity, seed, kp(), load_row<WORDS>(kp(), e)) == e, "find of key %lld", (long long)e);
  }

  void absent(const Block& b) {
    if (model.count(std::string((const char*)b.b, W))) return;
    CHECK(find<WORDS>(slots.data(), capacity, seed, kp(), load_row<WORDS>(b.b, 0)) == -1, "found an absent row");
  }
};

// rows of a batch, packed W bytes apart inside 16-byte aligned storage
template <int WORDS>
struct Batch {
  static constexpr int W = 8 * WORDS;
  std::vector<Block> mem;
  int64_t n = 0;
  void add(const uint8_t* row) {
    if ((size_t)((n + 1) * W + 31) / 32 > mem.size()) mem.resize(mem.size() * 2 + 8);
    memcpy(mem[0].b + n * W, row, W);
    ++n;
  }
};

template <int WORDS>
static void run(int perm, uint64_t cap, uint64_t seed) {
  constexpr int W = 8 * WORDS;
  Store<WORDS> st(cap, seed);
  uint8_t row[32];
  for (int round = 0; round < 6; ++round) {
    Batch<WORDS> b;
    // the edge rows, twice each, so every one is a duplicate inside its batch and across batches
    for (int rep = 0; rep < 2; ++rep) {
      memset(row, 0, sizeof row);
      b.add(row);
      memset(row, 0xFF, sizeof row);
      b.add(row);
      memset(row, 0x5A, sizeof row);
      b.add(row);
      row[0] ^= 1;                     // differs from the row before in byte 0 only
      b.add(row);
      row[0] ^= 1;
      row[W - 1] ^= 0x80;              // ... in byte W - 1 only
      b.add(row);
    }
    // random rows from a small key space (many duplicates) and fresh ones
    const int64_t n = 40 + 97 * round;
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t id = (rnd() % 3) ? rnd() % 150 : rnd();
      for (int j = 0; j < W; ++j) row[j] = (uint8_t)((id >> (8 * (j & 7))) ^ (uint64_t)(j >> 3) * 0x35);
      b.add(row);
    }
    st.insert(b.mem, b.n, perm);
    for (int k = 0; k < 50; ++k) {
      Block x;
      for (int j = 0; j < 32; ++j) x.b[j] = (uint8_t)rnd();
      st.absent(x);
    }
  }
  // 300 identical rows: one key, and with the reversed order every later claim lowers the slot
  {
    Batch<WORDS> b;
    memset(row, 0xC3, sizeof row);
    for (int i = 0; i < 300; ++i) b.add(row);
    const int64_t before = st.size;
    st.insert(b.mem, b.n, perm);
    CHECK(st.size == before + 1, "300 equal rows gave %lld keys", (long long)(st.size - before));
  }
  printf("W=%d perm=%d: %lld keys in %llu slots\n", W, perm, (long long)st.size, (unsigned long long)st.capacity);
}

int main() {
  for (int perm = 0; perm < 3; ++perm) {
    run<1>(perm, 8, 0x0123456789ABCDEFull + perm);
    run<4>(perm, 8, 0xFEDCBA9876543210ull - perm);
    run<4>(perm, 4096, 7);            // no growth: the table starts large enough
  }
  // hash_bytes is hash<> of the row's words
  Block x;
  for (int j = 0; j < 32; ++j) x.b[j] = (uint8_t)(j * 37 + 1);
  CHECK(hash_bytes(5, x.b, 32) == hash<4>(5, load_row<4>(x.b, 0)), "hash_bytes 32");
  CHECK(hash_bytes(5, x.b, 8) == hash<1>(5, load_row<1>(x.b, 0)), "hash_bytes 8");
  printf("idset host check: %d failures\n", bad);
  return bad ? 1 : 0;
}
"""


def test_idset_header_under_sanitizers(tmp_path):
    """The header the kernels are compiled from, as a host program of its own under ASan + UBSan."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = tmp_path / "idset_host.cpp"
    src.write_text(HOST_MAIN)
    exe = tmp_path / "idset_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "idset host check: 0 failures" in r.stdout, r.stdout[-4000:]
    assert r.stdout.count("keys in") == 9


def _hash(lib, seed, row):
    return lib.efl_idset_hash(seed, bytes(row), len(row))


@pytest.mark.parametrize("width", (8, 32))
def test_hash_depends_on_every_byte_and_on_the_seed(width):
    import efl
    lib = efl.lib.raw()
    seed = 0x1234_5678_9ABC_DEF0
    for base in (bytes(width), b"\xff" * width, bytes(range(7, 7 + width))):
        h = _hash(lib, seed, base)
        assert h == efl.psi.id_store.hash_row(seed, base)
        seen = {h}
        for i in range(width):
            for bit in (1, 0x80, 0xFF):
                row = bytearray(base)
                row[i] ^= bit
                assert _hash(lib, seed, row) != h, (i, bit)
                seen.add(_hash(lib, seed, row))
        assert len(seen) == 3 * width + 1
        for bit in range(64):
            assert _hash(lib, seed ^ (1 << bit), base) != h, bit
    # a null row and another width have no hash
    assert lib.efl_idset_hash(seed, None, width) == 0 and lib.efl_idset_hash(seed, b"x" * 16, 16) == 0


def test_hash_is_not_a_prefix_hash():
    """4,096 rows that agree in their first 24 bytes spread over the 8,192 home slots as a uniform
    hash spreads them (about 3,230 distinct; a prefix-only hash gives 1)."""
    import efl
    lib = efl.lib.raw()
    prefix = bytes(range(24))
    for seed in (0, 1, 0xDEADBEEF_00C0FFEE):
        homes = {_hash(lib, seed, prefix + i.to_bytes(8, "little")) & 8191 for i in range(4096)}
        assert len(homes) >= 3000, (seed, len(homes))
        # and the same for rows that agree in their LAST 24 bytes
        homes = {_hash(lib, seed, i.to_bytes(8, "big") + prefix) & 8191 for i in range(4096)}
        assert len(homes) >= 3000, (seed, len(homes))
    # width 8: 4,096 consecutive integers
    homes = {_hash(lib, 3, i.to_bytes(8, "little")) & 8191 for i in range(4096)}
    assert len(homes) >= 3000, len(homes)


def test_argument_errors_without_gpu():
    import efl
    lib = efl.lib.raw()
    P = ctypes.c_void_p
    P16, P8, P20, P4 = P(16), P(8), P(20), P(4)
    err = lambda: lib.efl_last_error().decode()
    big = 1 << 20

    def insert(rows=P16, n=5, width=32, keys=P16, key_capacity=64, size=P16, size_bound=10, slots=P16, capacity=128,
               pos=P16, scratch=P16, scratch_len=big):
        return lib.efl_idset_insert(rows, n, width, keys, key_capacity, size, size_bound, slots, capacity, 7, pos,
                                    scratch, scratch_len, None)

    def find(rows=P16, n=5, width=32, keys=P16, slots=P16, capacity=128, pos=P16):
        return lib.efl_idset_find(rows, n, width, keys, slots, capacity, 7, pos, None)

    def rehash(keys=P16, width=32, size=P16, size_bound=10, slots=P16, capacity=128):
        return lib.efl_idset_rehash(keys, width, size, size_bound, slots, capacity, 7, None)

    # n == 0 is a no-op, before anything else is looked at
    assert lib.efl_idset_insert(None, 0, 5, None, -1, None, -1, None, 3, 0, None, None, 0, None) == 0
    assert lib.efl_idset_find(None, 0, 5, None, None, 3, 0, None, None) == 0
    # negative counts
    assert insert(n=-1) == -3 and "negative" in err()
    assert find(n=-1) == -3 and "negative" in err()
    assert rehash(size_bound=-1) == -3 and "negative" in err()
    assert insert(size_bound=-1) == -3 and "negative" in err()
    # null buffers
    for name in ("rows", "keys", "size", "slots", "pos", "scratch"):
        assert insert(**{name: None}) == -3 and "null buffer" in err(), name
    for name in ("rows", "keys", "slots", "pos"):
        assert find(**{name: None}) == -3 and "null buffer" in err(), name
    for name in ("keys", "size", "slots"):
        assert rehash(**{name: None}) == -3 and "null buffer" in err(), name
    # rows of 32 bytes are 16-byte aligned, rows of 8 bytes 8-byte aligned
    assert insert(rows=P8) == -3 and "16-byte aligned" in err()
    assert insert(keys=P20) == -3 and "aligned" in err()
    assert insert(rows=P4, width=8) == -3 and "8-byte aligned" in err()
    assert insert(keys=P20, width=8) == -3 and "aligned" in err()
    assert find(rows=P8) == -3 and "aligned" in err()
    assert find(keys=P4, width=8) == -3 and "aligned" in err()
    assert rehash(keys=P8) == -3 and "aligned" in err()
    assert insert(size=P4) == -3 and "misaligned" in err()
    assert insert(pos=P4) == -3 and "misaligned" in err()
    assert find(pos=P20) == -3 and "misaligned" in err()
    # a width other than 8 or 32
    for w in (0, 4, 16, 31, 64, -8):
        assert insert(width=w) == -3 and "8 or 32" in err(), w
        assert find(width=w) == -3 and "8 or 32" in err(), w
        assert rehash(width=w) == -3 and "8 or 32" in err(), w
    # a capacity that is not a power of two
    for c in (0, 1, -128, 100, 127, 129, (1 << 32) + 2, 1 << 33):
        assert insert(capacity=c) == -3 and "power of two" in err(), c
        assert find(capacity=c) == -3 and "power of two" in err(), c
        assert rehash(capacity=c) == -3 and "power of two" in err(), c
    # a capacity that is too small: 2 * (size_bound + n) slots are needed
    assert insert(n=5, size_bound=60, capacity=128) == -3 and "capacity 128 is below twice the 65" in err()
    assert insert(n=4, size_bound=60, capacity=128, key_capacity=63) == -3 and "key_capacity" in err()
    assert rehash(size_bound=65, capacity=128) == -3 and "below twice" in err()
    assert insert(scratch_len=8) == -3 and "efl_idset_scratch_bytes" in err()
    # entries are limited to 2^31 - 2
    top = 2 ** 31 - 2
    assert insert(n=1, size_bound=top, capacity=1 << 32, key_capacity=1 << 31) == -8 and "2^31 - 2" in err()
    assert insert(n=top + 1, size_bound=0, capacity=1 << 32, key_capacity=1 << 31) == -8
    assert find(n=top + 1) == -8
    assert rehash(size_bound=top + 1, capacity=1 << 32) == -8
    with pytest.raises(efl.errors.ResourceExhaustedError, match="2\\^31 - 2"):
        efl.lib.check(rehash(size_bound=top + 1, capacity=1 << 32))
    # the scratch of a batch: two words per row, one per block of 256 rows, two more
    assert lib.efl_idset_scratch_bytes(0) == 0 and lib.efl_idset_scratch_bytes(-3) == 0
    assert lib.efl_idset_scratch_bytes(1) == 4 * (2 + 1 + 2)
    assert lib.efl_idset_scratch_bytes(257) == 4 * (514 + 2 + 2)


def test_id_store_constructor_and_empty_inputs_need_no_gpu():
    import efl
    psi = efl.psi
    assert psi.IdStore is psi.id_store.IdStore and psi.EcdhJoinServer is psi.ecdh_join.EcdhJoinServer
    assert psi.EcdhJoinClient is psi.ecdh_join.EcdhJoinClient
    assert {"IdStore", "EcdhJoinServer", "EcdhJoinClient", "id_store", "ecdh_join"} <= set(psi.__all__)
    for bad in (0, 16, 31, "32", None):
        with pytest.raises(efl.errors.InvalidArgumentError, match="8 or 32"):
            psi.IdStore(width=bad)
    for bad in (0, 1, 100, -64, 2 ** 33, 64.0):
        with pytest.raises(efl.errors.InvalidArgumentError, match="power of two"):
            psi.IdStore(capacity=bad)
    assert psi.IdStore().seed != psi.IdStore().seed             # a private seed per store
    for width in (8, 32):
        s = psi.IdStore(width=width, capacity=8, seed=2 ** 64 + 5)
        assert s.seed == 5 and s.width == width and s.capacity == 8
        empty = torch.empty((0, width), dtype=torch.uint8)
        assert s.put_rows(empty).shape == (0,) and s.put_rows(empty).dtype == torch.int64
        assert s.put_rows(empty, torch.empty(0, dtype=torch.int64)).shape == (0,)
        assert s.find(empty).shape == (0,) and s.find(empty).dtype == torch.int64
        assert s.exists(empty).dtype == torch.bool and s.exists(empty).shape == (0,) and s.exists([]) == []
        found, vals = s.get(empty)
        assert found.shape == (0,) and vals.shape == (0,) and vals.dtype == torch.int64
        assert s.put([], []) is True
        assert s.size() == 0
        assert tuple(s.keys().shape) == (0, width) and s.keys().dtype == torch.uint8
        assert tuple(s.values().shape) == (0,) and list(s.iter_batches(4)) == []
        s.clear()
        with pytest.raises(efl.errors.InvalidArgumentError, match="uint8"):
            s.find(torch.zeros((3, width + 1), dtype=torch.uint8))
        with pytest.raises(efl.errors.InvalidArgumentError, match="uint8"):
            s.put_rows(torch.zeros((3, width), dtype=torch.int8))
        with pytest.raises(efl.errors.InvalidArgumentError, match="values"):
            s.put_rows(torch.zeros((3, width), dtype=torch.uint8), torch.zeros(2, dtype=torch.int64))
        with pytest.raises(ValueError, match="item 1 is not"):
            s.exists([b"a" * width, b"a" * (width + 1)])
    # the join's halves: construction and the empty paths
    signer = psi.EccSigner(b"k" * 32)
    server, client = psi.EcdhJoinServer(signer, batch_size=4), psi.EcdhJoinClient(signer)
    server.add_ids([])
    assert client.join([], server) == []
    assert tuple(server.get_final_result().shape) == (0, 32) and server.get_final_ids() == []
    with pytest.raises(efl.errors.InvalidArgumentError, match="unexpected block_id: 3"):
        server.send_server_signed_data(torch.empty((0, 32), dtype=torch.uint8), 3)
    assert psi.ecdh_join.gather_res([b"a", b"b", b"c"], [True, False, True]) == [b"a", b"c"]
