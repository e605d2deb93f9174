"""CPU: the host side of the sort join's order (efl.psi.strsort). csrc/strsort.h, the header the
efl_strings_* kernels are compiled from, is compiled by g++ under ASan and UBSan into a stand-alone
program that checks fields, compare_bytes, compare_record, the 8-byte prefix with the cases a
prefix-only compare gets wrong, and the serial forms of the tile sort and the rank merge against
std::stable_sort (runs of unequal length, a run with no sibling); efl_strings_sort_host,
efl_strings_search_host and efl_strings_run_heads_host against Python's sorted() over the pool of
strsort_pool.py; the argument checks of every new entry point, which run before any HIP call; and what
the Python layer refuses and accepts."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG
from strsort_pool import POOL, draw, expected_order, fields, pack, random_keys

HOST_MAIN = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "strsort.h"
using namespace efl::strsort;

static int bad = 0;
#define CHECK(c, ...) do { if (!(c)) { ++bad; printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t lcg = 0x13198A2E03707344ull;
static uint64_t rnd() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg >> 11; }

typedef std::string S;
static S lit(const char* s, size_t n) { return S(s, n); }
#define L(s) lit(s, sizeof(s) - 1)

// a copy that ends exactly at the end of a heap block (ASan guards the bytes around it); an empty
// string gets a pointer nothing may be read from
struct Guarded {
  uint8_t* block;
  const uint8_t* p;
  int64_t len;
  explicit Guarded(const S& s) : block((uint8_t*)malloc(s.size() ? s.size() : 1)), len((int64_t)s.size()) {
    if (len) memcpy(block, s.data(), len);
    p = len ? block : block + 1;
  }
  ~Guarded() { free(block); }
};

static int sign(int c) { return c < 0 ? -1 : c > 0 ? 1 : 0; }

// the model of Python's bytes order
static int model_bytes(const S& a, const S& b) {
  const size_t m = std::min(a.size(), b.size());
  const int c = m ? memcmp(a.data(), b.data(), m) : 0;
  return c ? sign(c) : a.size() < b.size() ? -1 : a.size() > b.size() ? 1 : 0;
}

// split(b'#'): the first two pieces (the second empty when there is no '#')
static void model_split(const S& k, S* f0, S* f1, bool* has1) {
  const size_t h = k.find('#');
  *has1 = h != S::npos;
  *f0 = k.substr(0, h);
  *f1 = S();
  if (*has1) {
    const size_t h2 = k.find('#', h + 1);
    *f1 = k.substr(h + 1, h2 == S::npos ? S::npos : h2 - h - 1);
  }
}

static int model_record(const S& a, const S& b) {
  S a0, a1, b0, b1;
  bool x;
  model_split(a, &a0, &a1, &x);
  model_split(b, &b0, &b1, &x);
  const int c = model_bytes(a1, b1);
  return c ? c : model_bytes(a0, b0);
}

struct Packed {
  std::vector<int64_t> offsets;
  uint8_t* chars;
  explicit Packed(const std::vector<S>& keys, int lead) : offsets(keys.size() + 1) {
    int64_t at = lead;
    for (size_t i = 0; i < keys.size(); ++i) {
      offsets[i] = at;
      at += (int64_t)keys[i].size();
    }
    offsets[keys.size()] = at;
    chars = (uint8_t*)malloc(at ? at : 1);                  // exactly the bytes: the last string ends the block
    memset(chars, 0xEE, lead);
    for (size_t i = 0; i < keys.size(); ++i)
      if (keys[i].size()) memcpy(chars + offsets[i], keys[i].data(), keys[i].size());
  }
  ~Packed() { free(chars); }
};

// the sort by its serial steps: entries, every tile's bitonic network (the workers of a step in the
// order `perm`), the rank merges that ping-pong two buffers
static std::vector<int64_t> serial_sort(const Packed& P, const int32_t* segment, int64_t n, int mode, int perm, int* passes) {
  std::vector<int64_t> ext((size_t)n * 2, -1);
  if (mode == kSortRecord)
    for (int64_t r = 0; r < n; ++r) write_extents(P.chars, P.offsets.data(), r, ext.data());
  const Rows R{P.chars, P.offsets.data(), mode == kSortRecord ? ext.data() : nullptr, mode};
  std::vector<Entry> a(n), b(n);
  for (int64_t r = 0; r < n; ++r) a[r] = make_entry(R, segment, r);
  std::vector<Entry> tile(kTile);
  for (int64_t base = 0; base < n; base += kTile) {
    const int count = (int)std::min<int64_t>(kTile, n - base), span = tile_span(count);
    for (int x = 0; x < span; ++x) tile[x] = x < count ? a[base + x] : no_entry();
    for (int k = 2; k <= span; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1)
        for (int w = 0; w < span / 2; ++w) bitonic_exchange(R, tile.data(), k, j, perm ? span / 2 - 1 - w : w);
    for (int x = 0; x < count; ++x) a[base + x] = tile[x];
    for (int x = count; x < span; ++x) CHECK(tile[x].row == kNoRow, "a free place moved in front of a row");
  }
  *passes = 0;
  for (int64_t run = kTile; run < n; run *= 2, ++*passes) {
    std::vector<char> taken(n, 0);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t at = merge_place(R, a.data(), n, run, i);
      CHECK(at >= 0 && at < n && !taken[at], "merge_place(%lld) = %lld: outside or taken", (long long)i, (long long)at);
      if (at < 0 || at >= n) continue;
      taken[at] = 1;
      b[at] = a[i];
    }
    a.swap(b);
  }
  std::vector<int64_t> order(n);
  for (int64_t i = 0; i < n; ++i) order[i] = (int64_t)a[i].row;
  return order;
}

static std::vector<int64_t> model_sort(const std::vector<S>& keys, const int32_t* segment, int mode) {
  std::vector<int64_t> want(keys.size());
  for (size_t i = 0; i < keys.size(); ++i) want[i] = (int64_t)i;
  std::stable_sort(want.begin(), want.end(), [&](int64_t x, int64_t y) {
    if (segment && segment[x] != segment[y]) return segment[x] < segment[y];
    return (mode == kSortBytes ? model_bytes(keys[x], keys[y]) : model_record(keys[x], keys[y])) < 0;
  });
  return want;
}

int main() {
  const std::vector<S> pool = {
    L(""), L("a"), L("a\0"), L("a\0\0"), L("ab"), L("abc"), L("b"), L("abcdefgh"), L("abcdefghX"), L("abcdefghY"),
    L("abcdefgh\0"), L("abcdefghiJ"), L("abcdefghiK"), L("0123456789abcdefP"), L("0123456789abcdefQ"),
    L("0123456789abcdef"), L("\x7f"), L("\x80"), L("\xff"), L("\xff\0"), L("a\xff" "b"), L("a\x7f" "b"), L("\0"), L("\0\0"),
    L("a"), L("abc"), L("abcdefghX"), L(""), L("\x80"),
    L("#"), L("##"), L("#5"), L("id#"), L("id#5"), L("id#5#x"), L("id#5#y#z"), L("#5#"), L("#a#b"),
    L("x#9"), L("x#10"), L("x#100"), L("y#9"), L("y#10"), L("w#100"), L("x#9"),
    L("a#"), L("a#\0"), L("a\0#1"), L("a#1"), L("\x80#\x80"), L("\x7f#\x80"), L("\x80#\x7f"),
    L("k1#12345678"), L("k2#12345678"), L("k1#123456789"), L("k0#1234567890"), L("k3#12345678\0"),
    L("abcdefgh#12345678"), L("abcdefgi#12345678"), L("abcdefgh#1234567"), L("no hash at all")};

  // fields, as split(b'#') sees a key
  {
    struct Case { S key; S f0, f1; bool has1; };
    const Case cases[] = {
      {L(""), L(""), L(""), false}, {L("abc"), L("abc"), L(""), false}, {L("#"), L(""), L(""), true},
      {L("##"), L(""), L(""), true}, {L("a#"), L("a"), L(""), true}, {L("#b"), L(""), L("b"), true},
      {L("a#b"), L("a"), L("b"), true}, {L("a#b#c"), L("a"), L("b"), true}, {L("a#b#c#d"), L("a"), L("b"), true},
      {L("a##c"), L("a"), L(""), true}, {L("a\0#\0b#"), L("a\0"), L("\0b"), true}};
    for (const Case& c : cases) {
      const Guarded g(c.key);
      const Fields f = fields(g.p, g.len);
      CHECK(f.has1 == c.has1 && S((const char*)g.p + f.begin0, f.len0) == c.f0 && S((const char*)g.p + f.begin1, f.len1) == c.f1,
            "fields of a %d-byte key", (int)c.key.size());
    }
    for (const S& k : pool) {
      S f0, f1;
      bool has1;
      model_split(k, &f0, &f1, &has1);
      const Guarded g(k);
      const Fields f = fields(g.p, g.len);
      CHECK(f.has1 == has1 && S((const char*)g.p + f.begin0, f.len0) == f0 && S((const char*)g.p + f.begin1, f.len1) == f1, "fields over the pool");
    }
  }
  // the comparators over every pair of the pool, each string in a guarded block of its own
  {
    CHECK(compare_bytes((const uint8_t*)"a", 1, (const uint8_t*)"a\0", 2) < 0, "a proper prefix is smaller");
    CHECK(compare_bytes(nullptr, 0, (const uint8_t*)"\0", 1) < 0 && compare_bytes(nullptr, 0, nullptr, 0) == 0, "the empty string");
    CHECK(compare_bytes((const uint8_t*)"\x7f", 1, (const uint8_t*)"\x80", 1) < 0, "bytes compare unsigned");
    CHECK(compare_record((const uint8_t*)"x#10", 4, (const uint8_t*)"x#9", 3) < 0, "the order is lexicographic");
    CHECK(compare_record((const uint8_t*)"b#1", 3, (const uint8_t*)"a#2", 3) < 0, "field 1 comes first");
    CHECK(compare_record((const uint8_t*)"a#1#x", 5, (const uint8_t*)"a#1#y", 5) == 0, "a third field takes no part");
    int wrong_by_prefix = 0;
    for (const S& x : pool)
      for (const S& y : pool) {
        const Guarded a(x), b(y);
        const int cb = compare_bytes(a.p, a.len, b.p, b.len), cr = compare_record(a.p, a.len, b.p, b.len);
        CHECK(cb == model_bytes(x, y), "compare_bytes");
        CHECK(cr == model_record(x, y), "compare_record");
        // the prefix decides only when it differs, and then as the full comparison does
        const uint64_t pa = prefix8(a.p, a.len), pb = prefix8(b.p, b.len);
        if (pa != pb) CHECK((pa < pb) == (cb < 0), "prefix8 against compare_bytes");
        else if (cb != 0) ++wrong_by_prefix;
      }
    CHECK(wrong_by_prefix >= 20, "only %d pairs that a prefix-only compare gets wrong", wrong_by_prefix);
    CHECK(prefix8((const uint8_t*)"a", 1) == prefix8((const uint8_t*)"a\0\0", 3), "a and a NUL NUL share a prefix");
    CHECK(prefix8((const uint8_t*)"abcdefghX", 9) == 0x6162636465666768ull, "big-endian");
    printf("%d pairs tie on the prefix and differ\n", wrong_by_prefix);
  }
  // the sort by its serial steps against std::stable_sort
  int sorts = 0;
  {
    const int64_t sizes[] = {0, 1, 2, 3, 63, 64, 65, kTile - 1, kTile, kTile + 1, 2 * kTile, 3 * kTile, 4 * kTile + 1, 5 * kTile + 7};
    for (int64_t n : sizes)
      for (int mode = 0; mode < 2; ++mode)
        for (int segs = 0; segs < 3; ++segs) {               // no segments, 5 segments of both signs, a segment per row
          std::vector<S> keys(n);
          for (auto& k : keys) {
            if (rnd() % 2) { k = pool[rnd() % pool.size()]; continue; }
            const char letters[] = {'a', 'b', '#', '\0', '\xff', '1'};
            k.resize(rnd() % 41);
            for (auto& ch : k) ch = letters[rnd() % 6];
          }
          std::vector<int32_t> segment(n);
          for (int64_t i = 0; i < n; ++i) segment[i] = segs == 1 ? (int32_t)((int64_t)(rnd() % 5) * 1000000000 - 2000000000) : (int32_t)(n - i);
          const int32_t* seg = segs ? segment.data() : nullptr;
          const Packed P(keys, (int)(n % 4));
          int passes;
          const std::vector<int64_t> got = serial_sort(P, seg, n, mode, (int)(sorts % 2), &passes);
          CHECK(got == model_sort(keys, seg, mode), "n=%lld mode=%d segs=%d: order differs from std::stable_sort", (long long)n, mode, segs);
          int want_passes = 0;
          while (((int64_t)kTile << want_passes) < n) ++want_passes;
          CHECK(passes == want_passes, "n=%lld: %d passes", (long long)n, passes);
          ++sorts;
        }
    // already sorted, reversed and all equal
    for (int shape = 0; shape < 3; ++shape)
      for (int mode = 0; mode < 2; ++mode) {
        const int64_t n = 2 * kTile + 100;
        std::vector<S> keys(n);
        for (int64_t i = 0; i < n; ++i) {
          char text[32];
          snprintf(text, sizeof text, "id%06lld#%010lld", (long long)(shape == 0 ? i : n - i), (long long)(shape == 0 ? i : n - i));
          keys[i] = shape == 2 ? S("same#key") : S(text);
        }
        const Packed P(keys, 1);
        int passes;
        CHECK(serial_sort(P, nullptr, n, mode, 0, &passes) == model_sort(keys, nullptr, mode), "shape %d mode %d", shape, mode);
        ++sorts;
      }
  }
  printf("%d sorts\n", sorts);
  // search_one and run_head over the pool's bytes order
  {
    const Packed P(pool, 3);
    const int64_t m = (int64_t)pool.size();
    int passes;
    const std::vector<int64_t> order = serial_sort(P, nullptr, m, kSortBytes, 0, &passes);
    std::vector<S> queries = pool;
    for (const S& k : pool) {
      queries.push_back(k + S(1, '\0'));
      queries.push_back(k + "z");
      if (k.size()) queries.push_back(k.substr(0, k.size() - 1));
    }
    for (const S& q : queries) {
      int64_t want = -1;
      for (int64_t r = m - 1; r >= 0; --r)
        if (pool[r] == q) want = r;
      const Guarded g(q);
      const int64_t got = search_one(P.chars, P.offsets.data(), order.data(), m, g.p, g.len);
      CHECK(got == want, "search_one: row %lld, want %lld", (long long)got, (long long)want);
    }
    for (int64_t k = 0; k < m; ++k) {
      const uint8_t want = k == 0 || pool[order[k]] != pool[order[k - 1]];
      CHECK(run_head(P.chars, P.offsets.data(), order.data(), m, k) == want, "run_head(%lld)", (long long)k);
    }
  }
  printf("strsort host check: %d failures\n", bad);
  return bad ? 1 : 0;
}
"""


def test_strsort_header_under_sanitizers(tmp_path):
    """The header the kernels are compiled from, as a host program of its own under ASan + UBSan."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = tmp_path / "strsort_host.cpp"
    src.write_text(HOST_MAIN)
    exe = tmp_path / "strsort_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "90 sorts" in r.stdout, r.stdout[-4000:]
    assert "strsort host check: 0 failures" in r.stdout, r.stdout[-4000:]


# ---- the host entry points ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import efl
    return efl.lib.raw()


def sort_host(lib, keys, segment=None, mode="record", lead=1):
    chars, offsets = pack(keys, lead)
    order = np.full(len(keys), -7, dtype=np.int64)
    seg = None if segment is None else np.asarray(segment, dtype=np.int32)
    rc = lib.efl_strings_sort_host(chars.ctypes.data, offsets.ctypes.data, None if seg is None else seg.ctypes.data,
                                   len(keys), {"bytes": 0, "record": 1}[mode], order.ctypes.data)
    assert rc == 0
    return order.tolist()


def test_pool_covers_the_traps():
    assert b"" in POOL and b"#" in POOL and POOL.count(b"a") == 2
    assert {b"a", b"a\x00", b"a\x00\x00"} <= set(POOL)
    assert any(k.count(b"#") == 2 for k in POOL) and any(k.count(b"#") == 3 for k in POOL)
    assert any(max(k, default=0) >= 0x80 for k in POOL)
    for shared in (8, 9, 16):
        assert any(a != b and len(a) > shared and a[:shared] == b[:shared] and a[shared] != b[shared]
                   for a in POOL for b in POOL if len(b) > shared)
    assert fields(b"id#5#y#z") == (b"id", b"5") and fields(b"#") == (b"", b"") and fields(b"abc") == (b"abc", b"")
    # lexicographic, not numeric
    assert [POOL[i] for i in expected_order(POOL) if POOL[i] in (b"x#9", b"x#10", b"x#100")] == \
        [b"x#10", b"x#100", b"x#9", b"x#9"]


@pytest.mark.parametrize("mode", ("bytes", "record"))
def test_sort_host_over_the_pool(lib, mode):
    rng = np.random.default_rng(5)
    assert sort_host(lib, POOL, None, mode) == expected_order(POOL, None, mode)
    assert sort_host(lib, POOL, [0] * len(POOL), mode) == expected_order(POOL, None, mode)
    for n in (1, 2, 65, 700):
        keys = draw(rng, n)
        for segment in (None, rng.integers(-3, 4, size=n), np.arange(n)[::-1] - n // 2,
                        np.array([2 ** 31 - 1, -2 ** 31] * n)[:n]):
            assert sort_host(lib, keys, segment, mode, lead=n % 3) == expected_order(keys, segment, mode), (n, mode)
    # already sorted, reversed and all equal
    keys = [b"id%04d#%06d" % (i, i) for i in range(300)]
    assert sort_host(lib, keys, None, mode) == list(range(300))
    assert sort_host(lib, keys[::-1], None, mode) == list(range(300))[::-1]
    assert sort_host(lib, [b"same#key"] * 300, None, mode) == list(range(300))
    # mode "record" on keys that all have a '#' is sorted(keys, key=cmp_to_key(record_cmp))
    if mode == "record":
        def cmp(left, right):
            a, b = left.split(b"#"), right.split(b"#")
            return (a[1] > b[1]) - (a[1] < b[1]) or (a[0] > b[0]) - (a[0] < b[0])
        keys = draw(rng, 500, record=True)
        assert [keys[i] for i in sort_host(lib, keys)] == sorted(keys, key=functools.cmp_to_key(cmp))


def test_search_and_run_heads_host(lib):
    rng = np.random.default_rng(6)
    for table in (POOL, [], [b""], [b"a"], random_keys(rng, 257)):
        m = len(table)
        t_chars, t_offsets = pack(table, 1)
        t_order = np.array(expected_order(table, None, "bytes"), dtype=np.int64)
        queries = list(table) + [k + b"\x00" for k in table] + [k[:-1] for k in table if k] + \
            [b"", b"\x00", b"\xff" * 50, b"zzz"]
        q_chars, q_offsets = pack(queries, 2)
        out = np.full(len(queries), -7, dtype=np.int64)
        assert lib.efl_strings_search_host(t_chars.ctypes.data, t_offsets.ctypes.data, t_order.ctypes.data, m,
                                           q_chars.ctypes.data, q_offsets.ctypes.data, len(queries), out.ctypes.data) == 0
        assert out.tolist() == [table.index(q) if q in table else -1 for q in queries]
        if m:
            heads = np.full(m, 9, dtype=np.uint8)
            assert lib.efl_strings_run_heads_host(t_chars.ctypes.data, t_offsets.ctypes.data, t_order.ctypes.data, m,
                                                  heads.ctypes.data) == 0
            assert heads.tolist() == [int(k == 0 or table[t_order[k]] != table[t_order[k - 1]]) for k in range(m)]
            assert heads.sum() == len(set(table))
    # m == 0 with null table buffers: all -1
    q_chars, q_offsets = pack([b"a", b""])
    out = np.full(2, -7, dtype=np.int64)
    assert lib.efl_strings_search_host(None, None, None, 0, q_chars.ctypes.data, q_offsets.ctypes.data, 2, out.ctypes.data) == 0
    assert out.tolist() == [-1, -1]


def test_argument_checks_before_any_hip_call(lib):
    """No GPU is needed: every refusal comes before the first HIP call."""
    p8, p16, odd = ctypes.c_void_p(64), ctypes.c_void_p(64), ctypes.c_void_p(68)
    big = 2 ** 31 - 1
    err = lambda: lib.efl_last_error().decode()
    # scratch bytes: 48 per row, 0 out of range
    assert lib.efl_strings_sort_scratch_bytes(1) == 48 and lib.efl_strings_sort_scratch_bytes(2 ** 31 - 2) == 48 * (2 ** 31 - 2)
    assert [lib.efl_strings_sort_scratch_bytes(n) for n in (0, -1, big)] == [0, 0, 0]
    # the sort
    assert lib.efl_strings_sort(None, None, None, 0, 7, None, None, 0, None) == 0            # n == 0 comes first
    assert lib.efl_strings_sort(p8, p8, None, -1, 0, p8, p16, 1 << 20, None) == -3
    for args in ((None, p8, None, 5, 0, p8, p16), (p8, None, None, 5, 0, p8, p16), (p8, p8, None, 5, 0, None, p16),
                 (p8, p8, None, 5, 0, p8, None)):
        assert lib.efl_strings_sort(*args, 1 << 20, None) == -3 and "null" in err()
    for mode in (-1, 2):
        assert lib.efl_strings_sort(p8, p8, None, 5, mode, p8, p16, 1 << 20, None) == -3 and "mode" in err()
    for args in ((p8, odd, None, 5, 0, p8, p16), (p8, p8, ctypes.c_void_p(66), 5, 0, p8, p16), (p8, p8, None, 5, 0, odd, p16),
                 (p8, p8, None, 5, 0, p8, ctypes.c_void_p(72))):
        assert lib.efl_strings_sort(*args, 1 << 20, None) == -3 and "misaligned" in err()
    assert lib.efl_strings_sort(p8, p8, None, 5, 1, p8, p16, 5 * 48 - 1, None) == -3 and "scratch" in err()
    assert lib.efl_strings_sort(p8, p8, None, big, 1, p8, p16, 2 ** 62, None) == -8
    # the search
    assert lib.efl_strings_search(None, None, None, 5, None, None, 0, None, None) == 0
    assert lib.efl_strings_search(p8, p8, p8, 5, p8, p8, -1, p8, None) == -3
    assert lib.efl_strings_search(p8, p8, p8, -1, p8, p8, 5, p8, None) == -3
    for args in ((None, p8, p8, 5, p8, p8, 5, p8), (p8, None, p8, 5, p8, p8, 5, p8), (p8, p8, None, 5, p8, p8, 5, p8),
                 (p8, p8, p8, 5, None, p8, 5, p8), (p8, p8, p8, 5, p8, None, 5, p8), (p8, p8, p8, 5, p8, p8, 5, None),
                 (None, None, None, 0, p8, p8, 5, None)):
        assert lib.efl_strings_search(*args, None) == -3 and "null" in err()
    for args in ((p8, odd, p8, 5, p8, p8, 5, p8), (p8, p8, odd, 5, p8, p8, 5, p8), (p8, p8, p8, 5, p8, odd, 5, p8),
                 (p8, p8, p8, 5, p8, p8, 5, odd)):
        assert lib.efl_strings_search(*args, None) == -3 and "misaligned" in err()
    assert lib.efl_strings_search(p8, p8, p8, 5, p8, p8, big, p8, None) == -8
    assert lib.efl_strings_search(p8, p8, p8, big, p8, p8, 5, p8, None) == -8
    # the run heads
    assert lib.efl_strings_run_heads(None, None, None, 0, None, None) == 0
    assert lib.efl_strings_run_heads(p8, p8, p8, -1, p8, None) == -3
    for args in ((None, p8, p8, 5, p8), (p8, None, p8, 5, p8), (p8, p8, None, 5, p8), (p8, p8, p8, 5, None)):
        assert lib.efl_strings_run_heads(*args, None) == -3 and "null" in err()
    for args in ((p8, odd, p8, 5, p8), (p8, p8, odd, 5, p8)):
        assert lib.efl_strings_run_heads(*args, None) == -3 and "misaligned" in err()
    assert lib.efl_strings_run_heads(p8, p8, p8, big, p8, None) == -8
    # the host twins
    assert lib.efl_strings_sort_host(None, None, None, 0, 7, None) == 0
    assert lib.efl_strings_sort_host(None, None, None, 3, 0, None) == -3
    assert lib.efl_strings_sort_host(p8, p8, None, -1, 0, p8) == -3
    assert lib.efl_strings_sort_host(p8, p8, None, 3, 2, p8) == -3 and "mode" in err()
    assert lib.efl_strings_sort_host(p8, p8, None, big, 0, p8) == -8
    assert lib.efl_strings_search_host(None, None, None, 0, None, None, 0, None) == 0
    assert lib.efl_strings_search_host(None, None, None, 3, p8, p8, 3, p8) == -3
    assert lib.efl_strings_search_host(p8, p8, p8, -1, p8, p8, 3, p8) == -3
    assert lib.efl_strings_search_host(p8, p8, p8, 3, p8, p8, big, p8) == -8
    assert lib.efl_strings_run_heads_host(None, None, None, 0, None) == 0
    assert lib.efl_strings_run_heads_host(p8, p8, None, 3, p8) == -3
    assert lib.efl_strings_run_heads_host(p8, p8, p8, big, p8) == -8


# ---- the Python layer -----------------------------------------------------------------------------------

def test_record_keys_and_record_cmp():
    import efl
    psi = efl.psi
    assert psi.get_sample_store_key(5, 7) == b"5#7"
    assert psi.get_sample_store_key(b"id\xff", "té") == b"id\xff#t\xc3\xa9"
    assert psi.get_sample_store_key("a#b", 1.5) == b"a#b#1.5"
    assert psi.split_sample_store_key(b"a#b#c") == [b"a", b"b", b"c"] and psi.split_sample_store_key(b"abc") == [b"abc"]
    assert psi.gather_res([b"a", b"b", b"c"], [True, False, True]) == [b"a", b"c"]
    with pytest.raises(AssertionError, match="ids size 2, existence size 1"):
        psi.gather_res([b"a", b"b"], [True])
    assert psi.record_cmp is psi.strsort.record_cmp and psi.sort_keys is psi.strsort.sort_keys
    # record_cmp against the local definition on all pairs of a 60-key pool
    pool = [k for k in POOL if b"#" in k]
    pool += draw(np.random.default_rng(7), 60 - len(pool), record=True)
    assert len(pool) == 60
    for a in pool:
        for b in pool:
            ka, kb = (fields(a)[1], fields(a)[0]), (fields(b)[1], fields(b)[0])
            assert psi.record_cmp(a, b) == (ka > kb) - (ka < kb), (a, b)
    with pytest.raises(IndexError, match="list index out of range"):
        psi.record_cmp(b"abc", b"a#b")


def test_sort_keys_refuses_a_key_without_a_hash_sign():
    """The check runs on the packed bytes before the sort, so it needs no GPU."""
    import efl
    for keys in ([b"abc"], [b"a#1", b"abc", b"b#2"], [b"a#1", b""], [b"", b"#"], [b"a#1"] * 40 + [b"a1"]):
        with pytest.raises(IndexError, match="list index out of range"):
            efl.psi.sort_keys(keys)
        with pytest.raises(IndexError, match="list index out of range"):
            efl.psi.sort_keys(keys, mode="record")
    assert efl.psi.sort_keys([]) == [] and efl.psi.sort_keys([], mode="bytes") == []
    with pytest.raises(efl.errors.InvalidArgumentError, match="mode"):
        efl.psi.sort_keys([b"a#1"], mode="numeric")
    with pytest.raises(TypeError):
        efl.psi.sort_keys(["a#1"])
