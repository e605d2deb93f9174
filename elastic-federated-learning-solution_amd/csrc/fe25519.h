// Arithmetic mod p = 2^255 - 19 and the X25519 function of RFC 7748 (what python-curve25519-donna's
// make_private / make_shared compute for the reference's efls-data/xfl/data/psi/ecc_signer.py): the
// scalar is clamped, bit 255 of u is ignored, any u below 2^255 is accepted, the output is fully
// reduced and a low-order u gives 32 zero bytes without an error.
//
// Plain C++: hipcc compiles it for the device (k_x25519 of x25519.hip, one element per lane) and
// for the host, g++ compiles it for the host test. No intrinsics: (uint64_t)a * b + c is one
// v_mad_u64_u32 on the device, as in bignum.h.
//
// Representation: 10 unsigned limbs, limb i holding the bits from ceil(25.5 i) on, 26 bits wide for
// even i and 25 for odd i (radix 2^25.5). Limbs are never negative; a difference adds 2 p first.
// Two classes of limb bounds are used:
//   tight: even limbs < 2^26, odd limbs < 2^25 + 2^16     (what mul, sqr, mul_a24, from_words give)
//   loose: even limbs < 3 2^26, odd limbs < 3 2^25 + 2^16 (one add or sub of two tight numbers)
// mul and sqr take loose operands: a column is at most 77 E^2 + 190 O^2 < 2^62.2 for even limbs
// below E = 3 2^26 and odd limbs below O = 3 2^25 + 2^16, and the premultiplied operands 19 E and
// 4 O stay below 2^32.
//
// FE_AUDIT(site, fe, cls) stands where a function states the class of an operand or of its result.
// It expands to nothing unless the includer defined it before this header: the host test defines it
// to a checker of every limb against the class, so the contracts are exercised and not only stated.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define FE_FN __host__ __device__ __forceinline__
#define FE_UNROLL _Pragma("unroll")
#define FE_LOOP _Pragma("unroll 1")
#else
#define FE_FN inline
#define FE_UNROLL
#define FE_LOOP
#endif

#ifndef FE_AUDIT
#define FE_AUDIT(site, fe, cls)
#endif

namespace efl {
namespace fe {

struct Fe {
  uint32_t v[10];
};

// what FE_AUDIT is handed: the class a site states, and the site
enum AuditClass { kTight, kLoose };
enum AuditSite { kMulF, kMulG, kSqrF, kA24F, kSubF, kSubG, kCarryH, kAuditSites };

// the clamped scalar as the ladder reads it: bit t is (w[t / 32] >> (t % 32)) & 1
struct Scalar {
  uint32_t w[8];
};

FE_FN constexpr int limb_pos(int i) { return (51 * i + 1) / 2; }
FE_FN constexpr int limb_bits(int i) { return (i & 1) ? 25 : 26; }
FE_FN constexpr uint32_t limb_mask(int i) { return (1u << limb_bits(i)) - 1u; }

// h = the low 255 bits of the little-endian words w (bit 255 is dropped; 2^255 - 1 is the largest
// value, p .. 2^255 - 1 are not reduced here). Gives tight limbs, each below 2^bits.
FE_FN void from_words(Fe& h, const uint32_t w[8]) {
  FE_UNROLL
  for (int i = 0; i < 10; ++i) {
    const int j = limb_pos(i) >> 5, s = limb_pos(i) & 31;
    uint64_t t = w[j];
    if (j + 1 < 8) t |= (uint64_t)w[j + 1] << 32;
    h.v[i] = (uint32_t)(t >> s) & limb_mask(i);
  }
}

// the words of a canonical h (freeze's output: limb i < 2^bits(i), value < p)
FE_FN void to_words(uint32_t w[8], const Fe& h) {
  FE_UNROLL
  for (int j = 0; j < 8; ++j) w[j] = 0;
  FE_UNROLL
  for (int i = 0; i < 10; ++i) {
    const int j = limb_pos(i) >> 5, s = limb_pos(i) & 31;
    const uint64_t t = (uint64_t)h.v[i] << s;
    w[j] |= (uint32_t)t;
    if (j + 1 < 8) w[j + 1] |= (uint32_t)(t >> 32);
  }
}

FE_FN void set_small(Fe& h, uint32_t x) {
  h.v[0] = x;
  FE_UNROLL
  for (int i = 1; i < 10; ++i) h.v[i] = 0;
}

// h = f + g, limb by limb without a carry: tight + tight -> loose
FE_FN void add(Fe& h, const Fe& f, const Fe& g) {
  FE_UNROLL
  for (int i = 0; i < 10; ++i) h.v[i] = f.v[i] + g.v[i];
}

// h = f - g + 2 p, limb by limb: f tight, g tight (every limb of g is at most 2 p's) -> loose
FE_FN void sub(Fe& h, const Fe& f, const Fe& g) {
  FE_AUDIT(kSubF, f, kTight);
  FE_AUDIT(kSubG, g, kTight);
  h.v[0] = f.v[0] + 0x7ffffdau - g.v[0];
  FE_UNROLL
  for (int i = 1; i < 10; ++i) h.v[i] = f.v[i] + ((i & 1) ? 0x3fffffeu : 0x7fffffeu) - g.v[i];
}

// swap f and g where mask is all ones, leave them where it is zero
FE_FN void cswap(Fe& f, Fe& g, uint32_t mask) {
  FE_UNROLL
  for (int i = 0; i < 10; ++i) {
    const uint32_t x = (f.v[i] ^ g.v[i]) & mask;
    f.v[i] ^= x;
    g.v[i] ^= x;
  }
}

// the columns t to tight limbs. Two interleaved chains (0 -> 5 and 4 -> 9 -> 0 -> 1) so that no
// carry waits for nine others: 0, 4, 1, 5, 2, 6, 3, 7, 4, 8, 9 (times 19 into limb 0), 0. Limbs 0
// and 4 are carried twice; limbs 1 and 5 take a last carry after they were masked, the rest end
// below 2^bits.
// Precondition: the columns mul, sqr and mul_a24 form of loose operands, each below 2^62.2 and
// column 9 (whose carry is the one multiplied by 19) below 2^57.5. For those limb 1 ends at most
// 2^25 + 1711 and limb 5 at most 2^25 + 1062, both below 2^25 + 2^11. Columns below 2^62 each
// would still end tight (limb 1 at most 2^25 + 38,912); columns merely below 2^63 would not: limb 1
// can reach 2^25 + 77,823, past the tight 2^25 + 2^16, and limb 5 2^25 + 4,095. The exact-integer
// model of tests/x25519_domain.py proves these figures.
FE_FN void carry(Fe& h, uint64_t t[10]) {
  uint64_t c;
#define FE_CARRY(i, j, m)             \
  c = t[i] >> limb_bits(i);           \
  t[j] += c * (m);                    \
  t[i] &= limb_mask(i);
  FE_CARRY(0, 1, 1u) FE_CARRY(4, 5, 1u) FE_CARRY(1, 2, 1u) FE_CARRY(5, 6, 1u) FE_CARRY(2, 3, 1u)
  FE_CARRY(6, 7, 1u) FE_CARRY(3, 4, 1u) FE_CARRY(7, 8, 1u) FE_CARRY(4, 5, 1u) FE_CARRY(8, 9, 1u)
  FE_CARRY(9, 0, 19u) FE_CARRY(0, 1, 1u)
#undef FE_CARRY
  FE_UNROLL
  for (int i = 0; i < 10; ++i) h.v[i] = (uint32_t)t[i];
  FE_AUDIT(kCarryH, h, kTight);
}

// h = f g: loose operands -> tight. 100 products; limb products whose positions are both odd count
// twice (25.5-bit radix) and those that wrap past limb 9 count 19 times.
FE_FN void mul(Fe& h, const Fe& f, const Fe& g) {
  FE_AUDIT(kMulF, f, kLoose);
  FE_AUDIT(kMulG, g, kLoose);
  uint32_t g19[10], f2[10];
  FE_UNROLL
  for (int i = 0; i < 10; ++i) {
    g19[i] = 19u * g.v[i];
    f2[i] = 2u * f.v[i];
  }
  uint64_t t[10];
  FE_UNROLL
  for (int k = 0; k < 10; ++k) t[k] = 0;
  FE_UNROLL
  for (int i = 0; i < 10; ++i) {
    FE_UNROLL
    for (int j = 0; j < 10; ++j) {
      const uint32_t a = (i & j & 1) ? f2[i] : f.v[i];
      const uint32_t b = (i + j >= 10) ? g19[j] : g.v[j];
      t[(i + j) % 10] += (uint64_t)a * b;
    }
  }
  carry(h, t);
}

// h = f^2: loose -> tight. 55 products: the cross products are doubled in the left operand.
FE_FN void sqr(Fe& h, const Fe& f) {
  FE_AUDIT(kSqrF, f, kLoose);
  uint32_t f19[10];
  FE_UNROLL
  for (int i = 0; i < 10; ++i) f19[i] = 19u * f.v[i];
  uint64_t t[10];
  FE_UNROLL
  for (int k = 0; k < 10; ++k) t[k] = 0;
  FE_UNROLL
  for (int i = 0; i < 10; ++i) {
    FE_UNROLL
    for (int j = i; j < 10; ++j) {
      const uint32_t a = f.v[i] << ((i != j ? 1 : 0) + (i & j & 1));
      const uint32_t b = (i + j >= 10) ? f19[j] : f.v[j];
      t[(i + j) % 10] += (uint64_t)a * b;
    }
  }
  carry(h, t);
}

// h = 121665 f (a24 = (486662 - 2) / 4): loose -> tight
FE_FN void mul_a24(Fe& h, const Fe& f) {
  FE_AUDIT(kA24F, f, kLoose);
  uint64_t t[10];
  FE_UNROLL
  for (int i = 0; i < 10; ++i) t[i] = (uint64_t)f.v[i] * 121665u;
  carry(h, t);
}

// h <- h^(2^n), n >= 1: a loop, not n copies (the inversion's runs of 5 to 100 squarings)
FE_FN void sqr_n(Fe& h, int n) {
  FE_LOOP
  for (int i = 0; i < n; ++i) sqr(h, h);
}

// h = z^(p - 2) = z^(2^255 - 21): 254 squarings and 11 products; z loose -> tight. 0 gives 0.
FE_FN void invert(Fe& h, const Fe& z) {
  Fe t0, t1, t2, t3;
  sqr(t0, z);                    // 2
  sqr(t1, t0);
  sqr(t1, t1);                   // 8
  mul(t1, z, t1);                // 9
  mul(t0, t0, t1);               // 11
  sqr(t2, t0);                   // 22
  mul(t1, t1, t2);               // 2^5 - 1
  t2 = t1;
  sqr_n(t2, 5);
  mul(t1, t2, t1);               // 2^10 - 1
  t2 = t1;
  sqr_n(t2, 10);
  mul(t2, t2, t1);               // 2^20 - 1
  t3 = t2;
  sqr_n(t3, 20);
  mul(t2, t3, t2);               // 2^40 - 1
  sqr_n(t2, 10);
  mul(t1, t2, t1);               // 2^50 - 1
  t2 = t1;
  sqr_n(t2, 50);
  mul(t2, t2, t1);               // 2^100 - 1
  t3 = t2;
  sqr_n(t3, 100);
  mul(t2, t3, t2);               // 2^200 - 1
  sqr_n(t2, 50);
  mul(t1, t2, t1);               // 2^250 - 1
  sqr_n(t1, 5);                  // 2^255 - 32
  mul(h, t1, t0);                // 2^255 - 21
}

// h <- the canonical value below p of h. Any limbs are taken (each a whole uint32_t); the largest
// value the representation admits, every limb 2^32 - 1, is below 2^262.
FE_FN void freeze(Fe& h) {
  uint64_t t[10];
  FE_UNROLL
  for (int i = 0; i < 10; ++i) t[i] = h.v[i];
  // one chain with the fold of limb 9's carry: value < 2^255 + 2^12 < 2 p, limbs 1 .. 9 masked
  FE_UNROLL
  for (int i = 0; i < 9; ++i) {
    t[i + 1] += t[i] >> limb_bits(i);
    t[i] &= limb_mask(i);
  }
  t[0] += 19u * (t[9] >> 25);
  t[9] &= limb_mask(9);
  // q = floor((value + 19) / 2^255) = 1 exactly when value >= p
  uint64_t q = (t[0] + 19u) >> 26;
  FE_UNROLL
  for (int i = 1; i < 10; ++i) q = (t[i] + q) >> limb_bits(i);
  // value - q p = value + 19 q - q 2^255: the carry out of limb 9 is that 2^255
  t[0] += 19u * q;
  FE_UNROLL
  for (int i = 0; i < 9; ++i) {
    t[i + 1] += t[i] >> limb_bits(i);
    t[i] &= limb_mask(i);
  }
  t[9] &= limb_mask(9);
  FE_UNROLL
  for (int i = 0; i < 10; ++i) h.v[i] = (uint32_t)t[i];
}

// One step of the Montgomery ladder (RFC 7748 §5): (x2 : z2), (x3 : z3) <- the double of the first
// and the sum of the two, their difference being x1. All five tight in, the four tight out.
// 5 products, 4 squarings and the product by a24.
FE_FN void ladder_step(const Fe& x1, Fe& x2, Fe& z2, Fe& x3, Fe& z3) {
  Fe a, b, c, d, aa, bb, e, da, cb;
  add(a, x2, z2);
  sub(b, x2, z2);
  add(c, x3, z3);
  sub(d, x3, z3);
  sqr(aa, a);
  sqr(bb, b);
  mul(da, d, a);
  mul(cb, c, b);
  sub(e, aa, bb);
  add(a, da, cb);
  sub(b, da, cb);
  sqr(x3, a);
  sqr(b, b);
  mul(z3, x1, b);
  mul(x2, aa, bb);
  mul_a24(c, e);
  add(c, aa, c);
  mul(z2, e, c);
}

// out = X25519(k, u) on little-endian words; k is already clamped. The bit of each step is the
// same for every caller of one k (wave-uniform in k_x25519); the swap is by mask, and nothing but
// the loop counter indexes memory.
FE_FN void x25519_words(uint32_t out[8], const Scalar& k, const uint32_t u[8]) {
  Fe x1, x2, z2, x3, z3;
  from_words(x1, u);
  set_small(x2, 1);
  set_small(z2, 0);
  x3 = x1;
  set_small(z3, 1);
  uint32_t swap = 0;
  FE_LOOP
  for (int t = 254; t >= 0; --t) {
    const uint32_t bit = (k.w[t >> 5] >> (t & 31)) & 1u;
    swap ^= bit;
    cswap(x2, x3, 0u - swap);
    cswap(z2, z3, 0u - swap);
    swap = bit;
    ladder_step(x1, x2, z2, x3, z3);
  }
  cswap(x2, x3, 0u - swap);
  cswap(z2, z3, 0u - swap);
  invert(z2, z2);
  mul(x2, x2, z2);
  freeze(x2);
  to_words(out, x2);
}

// RFC 7748 §5 decodeScalar25519 on the 32 bytes as words; idempotent
FE_FN void clamp(Scalar& k) {
  k.w[0] &= ~7u;
  k.w[7] = (k.w[7] & 0x7fffffffu) | 0x40000000u;
}

FE_FN void words_from_bytes(uint32_t w[8], const uint8_t b[32]) {
  for (int j = 0; j < 8; ++j)
    w[j] = (uint32_t)b[4 * j] | (uint32_t)b[4 * j + 1] << 8 | (uint32_t)b[4 * j + 2] << 16 |
           (uint32_t)b[4 * j + 3] << 24;
}

FE_FN void bytes_from_words(uint8_t b[32], const uint32_t w[8]) {
  for (int j = 0; j < 32; ++j) b[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
}

// the whole function on bytes, the scalar clamped here (host callers; the kernel works on words)
FE_FN void x25519(uint8_t out[32], const uint8_t scalar[32], const uint8_t u[32]) {
  Scalar k;
  uint32_t uw[8], ow[8];
  words_from_bytes(k.w, scalar);
  clamp(k);
  words_from_bytes(uw, u);
  x25519_words(ow, k, uw);
  bytes_from_words(out, ow);
}

}  // namespace fe
}  // namespace efl
