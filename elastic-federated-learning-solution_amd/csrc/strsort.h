// The sort join's order of efl.psi (efl.psi.strsort): what the reference's default data-join does to
// its record keys `hash_col + b'#' + sort_col` (efls-data/xfl/data/utils.py:63-69) with
// sorted(keys, key=cmp_to_key(record_cmp)) (xfl/data/functions.py:49-60,261), as a comparison sort
// over packed byte strings of any length, a binary search in the sorted result and the heads of its
// runs of equal strings. Plain C++: the kernels of strsort.hip, the host entry points
// (efl_strings_*_host) and the host program of tests/test_strsort_host.py are all compiled from this
// header.
//
// The order. compare_bytes is Python's `bytes` order: unsigned bytes, the first difference decides,
// a proper prefix is smaller. compare_record is record_cmp: the key is split at '#', field 1 (the
// sort column) is compared first, then field 0 (the hash column), both by compare_bytes, so the order
// is lexicographic ("x#10" < "x#9"); what follows a second '#' takes no part. Rows are sorted by
// (segment as signed int32, key order, row index): the row index makes the order total, a total order
// makes the sort stable and gives every input exactly one correct output.
//
// The sort. Row r becomes an Entry (segment, row, the first 8 bytes of its primary field big-endian
// and zero-padded). Entries compare by segment, then prefix; equal prefixes fall through to the full
// comparison over the rows' bytes (the prefix cannot tell "a" from "a\0": the length decides), then
// to the row index. The steps are
//   entries  one row each: the field extents (record mode) and the Entry
//   tile     kTile entries sorted by a bitonic network, one compare-exchange per worker and step;
//            a tile's free places hold kNoRow entries, which sort after every row
//   merge    pass p merges runs of kTile 2^p entries pairwise: entry i's place is its offset in its
//            own run plus the number of entries of the sibling run that are less than it (one binary
//            search; the order is total, so "less than" serves both sides); a run without a sibling
//            is copied
// each a launch of its own on the device, so the only order between them is the launch boundary and
// every place is computed, not claimed.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define EFL_STRSORT_FN __host__ __device__ inline
#else
#define EFL_STRSORT_FN inline
#endif

namespace efl {
namespace strsort {

constexpr int kSortBytes = 0;                        // EFL_SORT_BYTES
constexpr int kSortRecord = 1;                       // EFL_SORT_RECORD
constexpr int kTile = 2048;                          // rows per tile: 256 lanes x 8
constexpr int64_t kMaxRows = 0x7FFFFFFE;             // 2^31 - 2, as the partition's
constexpr uint32_t kNoRow = 0xFFFFFFFFu;             // the row of a free place of a tile

// the two fields of a record key as split(b'#') and record_cmp see them, relative to the key's start
struct Fields {
  int64_t begin0, len0;      // the bytes before the first '#' (the whole key when it has none)
  int64_t begin1, len1;      // between the first and the second '#', or to the end
  bool has1;                 // false: no '#', field 1 is absent (and empty to the order)
};

EFL_STRSORT_FN Fields fields(const uint8_t* s, int64_t len) {
  Fields f;
  int64_t i = 0;
  while (i < len && s[i] != (uint8_t)'#') ++i;
  f.begin0 = 0;
  f.len0 = i;
  f.has1 = i < len;
  if (!f.has1) {
    f.begin1 = len;
    f.len1 = 0;
    return f;
  }
  int64_t j = i + 1;
  while (j < len && s[j] != (uint8_t)'#') ++j;
  f.begin1 = i + 1;
  f.len1 = j - (i + 1);
  return f;
}

// Python's bytes order: -1, 0, 1. Nothing is read of an empty string.
EFL_STRSORT_FN int compare_bytes(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb) {
  const int64_t m = la < lb ? la : lb;
  for (int64_t i = 0; i < m; ++i)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return la < lb ? -1 : la > lb ? 1 : 0;
}

// record_cmp: field 1, then field 0
EFL_STRSORT_FN int compare_record(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb) {
  const Fields fa = fields(a, la), fb = fields(b, lb);
  const int c = compare_bytes(a + fa.begin1, fa.len1, b + fb.begin1, fb.len1);
  return c ? c : compare_bytes(a + fa.begin0, fa.len0, b + fb.begin0, fb.len0);
}

// the first 8 bytes big-endian, zero-padded: prefix8(a) < prefix8(b) implies a < b in compare_bytes,
// equal prefixes decide nothing
EFL_STRSORT_FN uint64_t prefix8(const uint8_t* p, int64_t len) {
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v = v << 8 | (i < len ? (uint64_t)p[i] : 0u);
  return v;
}

// ---- rows of a packed buffer --------------------------------------------------------------------------

// string r is chars[offsets[r] .. offsets[r + 1]); ext (record mode; null: the fields are found again
// at every comparison) holds per row the absolute ends of field 0 and of field 1
struct Rows {
  const uint8_t* chars;
  const int64_t* offsets;
  const int64_t* ext;
  int mode;
};

EFL_STRSORT_FN int64_t row_len(const int64_t* offsets, int64_t r) {
  const int64_t d = offsets[r + 1] - offsets[r];
  return d > 0 ? d : 0;
}

// entries, one row: ext[2 r] <- the end of field 0, ext[2 r + 1] <- the end of field 1 (the end of
// field 0 when field 1 is absent: field 1 starts one past the '#' and is cut to that end)
EFL_STRSORT_FN void write_extents(const uint8_t* chars, const int64_t* offsets, int64_t r, int64_t* ext) {
  const int64_t lo = offsets[r];
  const Fields f = fields(chars + lo, row_len(offsets, r));
  ext[2 * r] = lo + f.len0;
  ext[2 * r + 1] = f.has1 ? lo + f.begin1 + f.len1 : lo + f.len0;
}

struct Span {
  const uint8_t* p;
  int64_t len;
};

EFL_STRSORT_FN Span whole_of(const Rows& R, int64_t r) { return Span{R.chars + R.offsets[r], row_len(R.offsets, r)}; }

// field f (0 or 1) of row r in record mode
EFL_STRSORT_FN Span field_of(const Rows& R, int64_t r, int f) {
  const int64_t lo = R.offsets[r];
  if (!R.ext) {
    const Fields x = fields(R.chars + lo, row_len(R.offsets, r));
    return f ? Span{R.chars + lo + x.begin1, x.len1} : Span{R.chars + lo, x.len0};
  }
  const int64_t e0 = R.ext[2 * r], e1 = R.ext[2 * r + 1];
  if (!f) return Span{R.chars + lo, e0 - lo};
  const int64_t b1 = e0 + 1 < e1 ? e0 + 1 : e1;
  return Span{R.chars + b1, e1 - b1};
}

// the key order of two rows: compare_bytes or compare_record by R.mode
EFL_STRSORT_FN int compare_rows(const Rows& R, int64_t ra, int64_t rb) {
  if (R.mode == kSortBytes) {
    const Span a = whole_of(R, ra), b = whole_of(R, rb);
    return compare_bytes(a.p, a.len, b.p, b.len);
  }
  const Span a1 = field_of(R, ra, 1), b1 = field_of(R, rb, 1);
  const int c = compare_bytes(a1.p, a1.len, b1.p, b1.len);
  if (c) return c;
  const Span a0 = field_of(R, ra, 0), b0 = field_of(R, rb, 0);
  return compare_bytes(a0.p, a0.len, b0.p, b0.len);
}

// ---- the sort -------------------------------------------------------------------------------------------

struct alignas(16) Entry {
  int32_t seg;
  uint32_t row;
  uint64_t prefix;
};

EFL_STRSORT_FN Entry no_entry() { return Entry{0, kNoRow, 0}; }

// entries, one row (after write_extents in record mode); segment may be null: one segment
EFL_STRSORT_FN Entry make_entry(const Rows& R, const int32_t* segment, int64_t r) {
  const Span s = R.mode == kSortBytes ? whole_of(R, r) : field_of(R, r, 1);
  return Entry{segment ? segment[r] : 0, (uint32_t)r, prefix8(s.p, s.len)};
}

// the total order (segment, key, row); a kNoRow entry follows every row
EFL_STRSORT_FN bool less(const Rows& R, const Entry& a, const Entry& b) {
  if (a.row == kNoRow) return false;
  if (b.row == kNoRow) return true;
  if (a.seg != b.seg) return a.seg < b.seg;
  if (a.prefix != b.prefix) return a.prefix < b.prefix;
  const int c = compare_rows(R, (int64_t)a.row, (int64_t)b.row);
  return c ? c < 0 : a.row < b.row;
}

// the power of two a tile of `count` entries is sorted as: at least 2, at most kTile
EFL_STRSORT_FN int tile_span(int64_t count) {
  int span = 2;
  while (span < count) span <<= 1;
  return span;
}

// tile: worker t (of span / 2) of step (k, j) of the bitonic network over e[0 .. span), k = 2, 4, ..
// span and for each k j = k / 2, k / 4, .. 1. The workers of one step touch disjoint pairs.
EFL_STRSORT_FN void bitonic_exchange(const Rows& R, Entry* e, int k, int j, int t) {
  const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
  const bool up = (i & k) == 0;
  const Entry a = e[i], b = e[l];
  if (up ? less(R, b, a) : less(R, a, b)) {
    e[i] = b;
    e[l] = a;
  }
}

// merge: the place of entry i of src (n entries, sorted runs of `run` entries each) after runs 2 q and
// 2 q + 1 have been merged
EFL_STRSORT_FN int64_t merge_place(const Rows& R, const Entry* src, int64_t n, int64_t run, int64_t i) {
  const int64_t r = i / run, mine = r * run, pair = (r >> 1) * 2 * run, sib = (r ^ 1) * run;
  if (sib >= n) return i;                          // a run with no sibling
  const Entry me = src[i];
  int64_t lo = sib, hi = sib + run < n ? sib + run : n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (less(R, src[mid], me)) lo = mid + 1;
    else hi = mid;
  }
  return pair + (i - mine) + (lo - sib);
}

// ---- search and run heads -------------------------------------------------------------------------------

// the table row of the first row in t_order (a kSortBytes order of the m table strings) whose string
// equals q, or -1; an entry of t_order outside [0, m) ends the search with -1
EFL_STRSORT_FN int64_t search_one(const uint8_t* t_chars, const int64_t* t_offsets, const int64_t* t_order, int64_t m,
                                  const uint8_t* q, int64_t lq) {
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2, r = t_order[mid];
    if (r < 0 || r >= m) return -1;
    if (compare_bytes(t_chars + t_offsets[r], row_len(t_offsets, r), q, lq) < 0) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= m) return -1;
  const int64_t r = t_order[lo];
  if (r < 0 || r >= m) return -1;
  return compare_bytes(t_chars + t_offsets[r], row_len(t_offsets, r), q, lq) == 0 ? r : -1;
}

// 1 when place k of `order` starts a run: k == 0, or the strings of rows order[k] and order[k - 1]
// differ in full bytes, length included (a row outside [0, n) equals nothing)
EFL_STRSORT_FN uint8_t run_head(const uint8_t* chars, const int64_t* offsets, const int64_t* order, int64_t n, int64_t k) {
  if (k == 0) return 1;
  const int64_t a = order[k], b = order[k - 1];
  if (a < 0 || a >= n || b < 0 || b >= n) return 1;
  return compare_bytes(chars + offsets[a], row_len(offsets, a), chars + offsets[b], row_len(offsets, b)) != 0;
}

}  // namespace strsort
}  // namespace efl
