// Sliding-window exponentiation by a wave-uniform secret exponent in radix-2^28 Montgomery form: the
// Paillier decryption's c^(x-1) mod x^2 (paillier_sliced.hip m_func) and the RSA signer's x^dp mod p
// (rsa.hip k_rsa_sign). The exponent is the same for every element, so the walk is wave-uniform.
//
// The element's odd powers c^1, c^3, ..., c^(2^kWin - 1) go to a global scratch slab (entry k at
// slot + k G CP, this lane's CP-word slice) and every multiply stages its entry in LDS. Products:
// bits - 1 squarings + about bits / (kWin + 1) multiplies + 2^(kWin-1) for the table, against
// bits - 1 + popcount - 1 for the binary method: 2404 instead of about 3071 at a 4096-bit Paillier n.
//
// The first part is plain C++ shared with the host (tests/test_powm_window_host.py replays the plan
// with the system compiler); the device part follows.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include "sliced28.h"
#define EFL_PW_FN __host__ __device__ __forceinline__
#else
#define EFL_PW_FN static inline
#endif

namespace efl {
namespace s28 {

// window width and odd-power entries of the walk
constexpr int kWin = 5, kEntries = 1 << (kWin - 1);

// bit b of a wave-uniform exponent
EFL_PW_FN uint32_t ebit(const uint32_t* ex, int b) { return (ex[b >> 5] >> (b & 31)) & 1u; }

// One step of the left-to-right walk: nsq squarings, then (mul) a multiply by the odd power
// 2 entry + 1 (table entry `entry`); the next step starts at bit `next` (< 0: the walk is done).
struct WinStep {
  int nsq;
  bool mul;
  uint32_t entry;
  int next;
};

// the step at bit b: a 0 bit's lone squaring, or a window of up to kWin bits that starts at the 1
// bit b and ends in a 1 bit
EFL_PW_FN WinStep win_next(const uint32_t* ex, int b) {
  if (!ebit(ex, b)) return {1, false, 0u, b - 1};
  int j = b - kWin + 1 > 0 ? b - kWin + 1 : 0;
  while (!ebit(ex, j)) ++j;
  uint32_t v = 0;
  for (int t = b; t >= j; --t) v = (v << 1) | ebit(ex, t);
  return {b - j + 1, true, v >> 1, j - 1};
}

// the top window of an exponent of ebits >= 1 bits (bit ebits - 1 set): its entry is the walk's
// starting value, so it has no squarings
EFL_PW_FN WinStep win_first(const uint32_t* ex, int ebits) {
  WinStep s = win_next(ex, ebits - 1);
  s.nsq = 0;
  return s;
}

#ifdef __HIPCC__

// padded radix-2^28 slice of one element in HBM: lane g's C28 limbs at [g * CP, g * CP + C28)
template <int C28>
constexpr int pad4() { return (C28 + 3) & ~3; }

template <int C28>
__device__ __forceinline__ void store28(uint32_t* __restrict__ q, const uint32_t (&t)[C28]) {
  constexpr int CP = pad4<C28>();
#pragma unroll
  for (int j = 0; j < CP; j += 4)
    *reinterpret_cast<uint4*>(q + j) = make_uint4(t[j], j + 1 < C28 ? t[j + 1] : 0u, j + 2 < C28 ? t[j + 2] : 0u,
                                                  j + 3 < C28 ? t[j + 3] : 0u);
}

template <int C28>
__device__ __forceinline__ void load28(uint32_t (&t)[C28], const uint32_t* __restrict__ q) {
  constexpr int CP = pad4<C28>();
#pragma unroll
  for (int j = 0; j < CP; j += 4) {
    const uint4 v = *reinterpret_cast<const uint4*>(q + j);
    t[j] = v.x;
    if (j + 1 < C28) t[j + 1] = v.y;
    if (j + 2 < C28) t[j + 2] = v.z;
    if (j + 3 < C28) t[j + 3] = v.w;
  }
}

// The odd powers T[k] = T[k-1] c^2, k = 1 .. kEntries - 1, into slot + k G CP: a holds T[0] = c
// (the caller stored it at slot) and c^2 is staged in BASE. a ends as the last entry.
template <int C28, int G>
__device__ __forceinline__ void build_odd_powers(uint32_t (&a)[C28], uint32_t* slot, uint32_t* BASE, int E,
                                                 const uint32_t (&m28)[C28], uint32_t minv28, int g) {
  constexpr int CP = pad4<C28>();
#pragma unroll 1
  for (int k = 1; k < kEntries; ++k) {
    s28::mont_mul<C28, G>(a, sl::LdsElem{BASE, E}, m28, minv28, g);
    store28<C28>(slot + (size_t)k * G * CP, a);
  }
  sl::lds_sync();
}

// a <- a^ex in radix-2^28 Montgomery form (lazy: < 2m), ex of ebits >= 1 bits, uniform over the
// wave. slot: this lane's slice of the element's slab. The loop has one site for its squarings (the
// table's c^2, a 0 bit's lone squaring, a window's run): the next step is planned at its end. SOS:
// the squarings are sos_sqr, which takes both LDS arrays (BASE and SCR, contiguous) as the square's
// 2 L words; its code is about 3,500 instructions, hence the one call site.
template <int C28, int G, bool SOS>
__device__ __forceinline__ void powm_window(uint32_t (&a)[C28], uint32_t* slot, const uint32_t* ex, int ebits,
                                            uint32_t* BASE, uint32_t* SCR, int E, const uint32_t (&m28)[C28],
                                            uint32_t minv28, int g) {
  constexpr int CP = pad4<C28>();
  store28<C28>(slot, a);
  WinStep s = win_first(ex, ebits);
  s.nsq = 1;                                       // the table's c^2 goes through the squaring site first
  bool build = true;
#pragma unroll 1
  for (;;) {
#pragma unroll 1
    for (int t = 0; t < s.nsq; ++t) {
      if constexpr (SOS) s28::sos_sqr<C28, G>(a, BASE, E, m28, minv28, g);
      else s28::mont_sqr<C28, G>(a, SCR, E, m28, minv28, g);
      sl::lds_sync();
    }
    if (build) {
      // a = c^2: stage it, then the odd powers from T[0] = c
      sl::to_lds<C28>(BASE, E, g, a);
      sl::lds_sync();
      load28<C28>(a, slot);
      build_odd_powers<C28, G>(a, slot, BASE, E, m28, minv28, g);
      load28<C28>(a, slot + (size_t)s.entry * G * CP);   // the top window
      build = false;
    } else if (s.mul) {
      uint32_t ent[C28];
      load28<C28>(ent, slot + (size_t)s.entry * G * CP);
      sl::to_lds<C28>(BASE, E, g, ent);
      sl::lds_sync();
      s28::mont_mul<C28, G>(a, sl::LdsElem{BASE, E}, m28, minv28, g);
      sl::lds_sync();
    }
    if (s.next < 0) break;
    s = win_next(ex, s.next);
  }
}

// The same walk with CIOS squarings at two sites (the decryption's families without SOS): a window's
// entry is loaded before its squarings, so the load is in flight during them.
template <int C28, int G>
__device__ __forceinline__ void powm_window_preload(uint32_t (&a)[C28], uint32_t* slot, const uint32_t* ex,
                                                    int ebits, uint32_t* BASE, uint32_t* SCR, int E,
                                                    const uint32_t (&m28)[C28], uint32_t minv28, int g) {
  constexpr int CP = pad4<C28>();
  store28<C28>(slot, a);
  uint32_t c2[C28];
#pragma unroll
  for (int j = 0; j < C28; ++j) c2[j] = a[j];
  s28::mont_sqr<C28, G>(c2, SCR, E, m28, minv28, g);
  sl::lds_sync();
  sl::to_lds<C28>(BASE, E, g, c2);
  sl::lds_sync();
  build_odd_powers<C28, G>(a, slot, BASE, E, m28, minv28, g);
  WinStep s = win_first(ex, ebits);
  load28<C28>(a, slot + (size_t)s.entry * G * CP);
#pragma unroll 1
  while (s.next >= 0) {
    s = win_next(ex, s.next);
    if (!s.mul) {
      s28::mont_sqr<C28, G>(a, SCR, E, m28, minv28, g);
      continue;
    }
    uint32_t ent[C28];
    load28<C28>(ent, slot + (size_t)s.entry * G * CP);   // in flight during the squarings
#pragma unroll 1
    for (int t = 0; t < s.nsq; ++t) s28::mont_sqr<C28, G>(a, SCR, E, m28, minv28, g);
    // (mul_fips1 here, for one-lane numbers, measured 3 % slower: the 1024-bit decryption's 256
    // VGPRs were already full, round 4)
    sl::to_lds<C28>(BASE, E, g, ent);
    sl::lds_sync();
    s28::mont_mul<C28, G>(a, sl::LdsElem{BASE, E}, m28, minv28, g);
    sl::lds_sync();
  }
}

// a <- a^ex by the binary method (no slab): square, and multiply by the base on a 1 bit
template <int C28, int G>
__device__ __forceinline__ void powm_binary(uint32_t (&a)[C28], const uint32_t* ex, int ebits, uint32_t* BASE,
                                            uint32_t* SCR, int E, const uint32_t (&m28)[C28], uint32_t minv28,
                                            int g) {
  sl::to_lds<C28>(BASE, E, g, a);
#pragma unroll 1
  for (int b = ebits - 2; b >= 0; --b) {
    s28::mont_sqr<C28, G>(a, SCR, E, m28, minv28, g);
    if (ebit(ex, b)) s28::mont_mul<C28, G>(a, sl::LdsElem{BASE, E}, m28, minv28, g);
  }
}

#endif  // __HIPCC__

}  // namespace s28
}  // namespace efl
