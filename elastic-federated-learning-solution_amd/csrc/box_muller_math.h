// Box-Muller's radius sqrt(-2 ln u1) (csrc/mask.hip, efl_dp_noise) over the arguments it can reach.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// u1 in [1e-7, 1) and -2 ln u1 in [2.38e-7, 32.24], normal and finite, so the library functions'
// denormal rescaling, logf's non-finite select and sqrtf's zero / infinity select are left out
// (round 5, about a dozen instructions per pair).
//
// Round 5 took the device library's own logf and sqrtf sequences: v_log_f32 times ln 2 as a
// double-float, rounded to a float, then v_sqrt_f32 made the correctly rounded root of that float.
// tests/test_box_muller_domain_gpu.py walks all 2^23 values of u1 through the kernel's functions and
// found that radius 2 ulp away from the oracle's (oracle/mask.py: float64 log and sqrt, each rounded
// to float) for 10,902 of them, k = 4070 the first, on both sides of u1 = 0.5, which lets the normal
// drift to 5 ulp where the project states 4. v_log_f32 is up to 1.0 ulp off log2 u (measured over
// every u1); the result y of it is a float whose rounding alone is 0.5 ulp when |y| >= 1; the
// product with ln 2 rounds again. log_unit was up to 2.14 ulp off ln u1 (2 ulp from the rounded
// logarithm for 201,397 u1), the radius up to 1.72 ulp off sqrt(-2 ln u1).
//
// Now (the instruction count per pair goes from 15 to 19, one v_log_f32 and one v_rsq_f32 as before
// one v_log_f32 and one v_sqrt_f32):
// * log_unit splits u1 = m 2^e, m in [0.5, 1), and takes v_log_f32 of m only, so the hardware's
//   error is an error of log2 m in [-1, 0) and the exponent's share e ln 2 is exact to 2^-40 (ln 2 =
//   L1 + L2 with e L1 exact); ln u1 comes back unrounded, as a head and a tail;
// * radius_unit takes the root of -2 (head + tail) with one Newton step from v_rsq_f32, whose last
//   addition is the only rounding after the logarithm's.
// Measured over every u1 on an MI355X: the radius is at most 1 ulp from the oracle's for all 2^23
// (0.71 ulp off the real sqrt(-2 ln u1) below u1 = 0.5, 1.17 ulp above) and non-increasing in k
// (DESIGN.md §5c has the counts). tests/test_box_muller_domain_gpu.py asserts both on every run;
// tools/dp_fastmath_check.hip is the round-5 comparison with the library's logf / sqrtf.
//
// ln u = head (returned) + tail. The tail carries e l2 whole, so it reaches 34 ulp of the head
// (2^-18 of it) at e = -23; radius_unit's step is first order in it and drops 2^-39 of the root.
// Measured: head + tail is at most 0.35 ulp off ln u1 below u1 = 0.5 and 1.32 ulp above, where
// v_log_f32's own error is all of it.
__device__ __forceinline__ float log_unit(float u, float& tail) {
#pragma clang fp contract(off)
  const float hi = __uint_as_float(0x3f317217u), lo = __uint_as_float(0x3377d1cfu);   // ln 2 = hi + lo
  const float l1 = __uint_as_float(0x3f317200u), l2 = __uint_as_float(0x35bfbe8eu);   // ln 2 = l1 + l2, l1 of 16 bits
  const float ef = (float)__builtin_amdgcn_frexp_expf(u);                // u = m 2^e, -23 <= e <= 0
  const float f = __builtin_amdgcn_logf(__builtin_amdgcn_frexp_mantf(u));   // log2 m in [-1, 0)
  const float h = f * hi;
  float t = __builtin_fmaf(f, hi, -h);
  t = __builtin_fmaf(lo, f, t);                 // f ln 2 = h + t
  t = __builtin_fmaf(ef, l2, t);
  const float s = __builtin_fmaf(ef, l1, h);    // e l1 is exact and |e l1| >= |h| unless e = 0
  tail = (__builtin_fmaf(ef, l1, -s) + h) + t;  // e l1 - s exactly, then what the sum s dropped, then t
  return s;
}

// sqrt(-2 (lg + tail)) for -2 lg in [2.38e-7, 32.24]: q = rsq(x), s = x q, and the step
// s + (x + xl - s^2) q / 2 with the residual from one fma.
__device__ __forceinline__ float radius_unit(float lg, float tail) {
#pragma clang fp contract(off)
  const float x = -2.0f * lg;
  const float q = __builtin_amdgcn_rsqf(x);
  const float s = x * q;
  float res = __builtin_fmaf(-s, s, x);
  res = __builtin_fmaf(-2.0f, tail, res);
  return __builtin_fmaf(res, 0.5f * q, s);
}

// r at the clamp u1 = 1e-7: the value the compiler folds sqrtf(-2 logf(1e-7f)) to (5.677 68...)
constexpr uint32_t kRClampBits = 0x40b5afa8u;

