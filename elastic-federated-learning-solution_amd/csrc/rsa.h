// RSA blind-signature PSI (efl.psi): what the kernels of rsa.hip read from the key block that
// rsaset.hip derives, and the launchers between the two.
#pragma once

#include "common.h"

namespace efl {
namespace rsa {

// constants of one prime x (p or q): word offsets into the key block. L = 32-bit words of the
// primes' class (16, 32, 64), G the lanes an element's number mod x is spread over, L28 the
// radix-2^28 limbs of that family (csrc/sliced28.h)
struct Prime {
  int64_t off_x;        // x, L words
  int64_t off_r2;       // R^2 mod x, R = 2^(32 L)
  int64_t off_x28;      // x as L28 28-bit limbs
  int64_t off_r2_28;    // R28^2 mod x, R28 = 2^(28 L28)
  int64_t off_dx;       // d mod (x - 1), L words
  uint32_t minv;        // -x^-1 mod 2^32
  uint32_t minv28;      // -x^-1 mod 2^28
  int32_t dbits;        // bit length of d mod (x - 1)
};

struct Key {
  const uint32_t* base;
  int32_t W;            // words of a row: the class of N (32, 64, 128)
  int32_t L;            // words of the primes' class; W == 2 L, or W == L for unbalanced primes
  uint32_t n_minv;      // -N^-1 mod 2^32
  int64_t off_n;        // N, W words
  int64_t off_n_r2;     // R^2 mod N, R = 2^(32 W)
  int64_t off_qinvp;    // (q^-1 mod p) R mod p, R = 2^(32 L)
  Prime pr[2];          // p, q
  __device__ __forceinline__ const uint32_t* at(int64_t off) const { return base + off; }
};

// (C, G) of the sign kernel for primes of L words: the Paillier decryption's default family for a
// modulus of that width
inline int sign_lanes(int L) { return L == 16 ? 2 : L == 32 ? 1 : 2; }
// radix-2^28 limbs of that family
int sign_limbs28(int L);

// s = x^d mod N by CRT ([n][W] words each); takes stream-ordered scratch for the odd powers
hipError_t sign(const Key& k, const uint32_t* x, uint32_t* s, long long n, hipStream_t st);
// out = r^e h mod N
hipError_t blind(const Key& k, const uint32_t* h, const uint32_t* r, uint64_t e, uint32_t* out, long long n,
                 hipStream_t st);
hipError_t sha256_fdh(const char* chars, const long long* offsets, uint32_t* out, int words_per_row, long long n,
                      hipStream_t st);

}  // namespace rsa
}  // namespace efl
