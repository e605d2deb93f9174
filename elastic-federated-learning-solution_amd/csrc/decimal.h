// Python's str(int) of a number of up to 128 little-endian 32-bit words: what the reference hashes
// at the end of every RSA signature (efls-data/xfl/data/psi/rsa_signer.py, OneWayHash(str(v))). Plain
// C++: the kernels of decimal.hip, efl_rsa_decimal_digits and the host program of
// tests/test_decimal_host.py are all compiled from this header.
//
// Method. Repeated short division by 10^9 from the top non-zero word down: one pass replaces the
// number by its quotient and yields the remainder, a chunk of 9 decimal digits, least significant
// chunk first. The running remainder stays below 10^9 < 2^30, so a dividend (rem << 32 | word) is
// below 2^62 and its quotient fits a word; the divisor is a compile-time constant. The top word's
// quotient is below 5, and when it is 0 the word under it gets a non-zero one (its dividend is at
// least 2^32), so the number loses at most one word per pass and `top` follows without a scan.
//
// Bounds. A number of `words` words has at most D = max_digits(words) digits, so exactly
// max_chunks(words) = ceil(D / 9) passes run, each over at most `words` words; passes after the
// number has reached zero yield zero chunks. Nothing else loops.
//
// The text is RIGHT-aligned in a row of `stride` >= D bytes and left-padded with '0': digit d of
// chunk k (d = 0 the least significant) is the byte at column stride - 1 - (9 k + d), wherever the
// number's first digit falls, so chunks go out as they come and the byte at any column is a function
// of one chunk (text_byte).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define EFL_DEC_FN __host__ __device__ inline
#else
#define EFL_DEC_FN inline
#endif

namespace efl {
namespace decimal {

constexpr int kMaxWords = 128;
constexpr uint32_t kChunk = 1000000000u;   // 10^9
constexpr int kChunkDigits = 9;

// floor(32 words log10 2) + 1 = len(str(2^(32 words) - 1)); 0 unless 1 <= words <= 128. log10 2 to
// twelve places: the error over 4096 bits is below 2e-9, and no multiple of log10 2 up to 4096
// comes within 1e-5 of an integer.
EFL_DEC_FN int max_digits(int words) {
  if (words < 1 || words > kMaxWords) return 0;
  return (int)((uint64_t)(32 * words) * 301029995664ull / 1000000000000ull) + 1;
}

EFL_DEC_FN int max_chunks(int words) { return (max_digits(words) + kChunkDigits - 1) / kChunkDigits; }

EFL_DEC_FN uint32_t ten_to(int d) {
  switch (d) {
    case 0: return 1u;
    case 1: return 10u;
    case 2: return 100u;
    case 3: return 1000u;
    case 4: return 10000u;
    case 5: return 100000u;
    case 6: return 1000000u;
    case 7: return 10000000u;
    case 8: return 100000000u;
    default: return kChunk;
  }
}

// decimal digits of a chunk in [1, 10^9); 1 for 0
EFL_DEC_FN int chunk_digits(uint32_t c) {
  int n = 1;
  for (int d = 1; d < kChunkDigits; ++d)
    if (c >= ten_to(d)) n = d + 1;
  return n;
}

// digit d (0 = least significant, d < 9) of a chunk
EFL_DEC_FN uint32_t digit_of(uint32_t chunk, int d) { return chunk / ten_to(d) % 10u; }

// The number in rd(0) .. rd(words - 1) (destroyed: wr(j, v) stores its quotients) as max_chunks(words)
// chunks, put(k, chunk) for k = 0, 1, .. in that order. Returns the number of digits, 1 for zero.
// 1 <= words <= 128 is the caller's to check.
template <class Rd, class Wr, class Put>
EFL_DEC_FN int to_chunks(int words, Rd rd, Wr wr, Put put) {
  int top = words;
  while (top > 0 && rd(top - 1) == 0u) --top;
  const int passes = max_chunks(words);
  int len = 1;
  for (int k = 0; k < passes; ++k) {
    uint32_t rem = 0;
    if (top > 0) {
      uint32_t first = 0;
      for (int j = top - 1; j >= 0; --j) {
        const uint64_t cur = ((uint64_t)rem << 32) | rd(j);
        const uint32_t q = (uint32_t)(cur / kChunk);
        rem = (uint32_t)(cur - (uint64_t)q * kChunk);
        wr(j, q);
        if (j == top - 1) first = q;
      }
      if (first == 0u) --top;
    }
    put(k, rem);
    if (rem) len = kChunkDigits * k + chunk_digits(rem);
  }
  return len;
}

// The ASCII byte at column `col` (0 <= col < stride) of the right-aligned row, chunk(k) giving chunk
// k < chunks; columns left of the last chunk are padding.
template <class Chunk>
EFL_DEC_FN uint8_t text_byte(int64_t stride, int64_t col, int chunks, Chunk chunk) {
  const int64_t right = stride - 1 - col;
  if (right >= (int64_t)kChunkDigits * chunks) return (uint8_t)'0';
  const int p = (int)right;                      // below 9 * 138
  const int k = p / kChunkDigits;
  return (uint8_t)('0' + digit_of(chunk(k), p - k * kChunkDigits));
}

}  // namespace decimal
}  // namespace efl
