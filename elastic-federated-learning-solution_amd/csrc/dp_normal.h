// The DP-SGD noise of one element, shared by the kernels that apply it (csrc/mask.hip k_dp_noise,
// csrc/dpclip.hip k_dp_clip_sum): TF's normal of a Philox block and the noise-and-divide step.
//
// TF's tf.random.normal (NormalDistribution<PhiloxRandom, float>, tensorflow/core/lib/random/
// random_distributions.h): every Philox4x32-10 block gives 4 normals, Box-Muller on the word pairs
// (0, 1) and (2, 3): u1 = max(Uint32ToFloat(x0), 1e-7), v1 = float(2 pi (double) * Uint32ToFloat(x1)),
// r = sqrt(-2 log u1), (f0, f1) = r (sin v1, cos v1). Element i takes normal i % 4 of block
// ctr0 + i / 4. The radius over the arguments Box-Muller reaches: box_muller_math.h; the angle's
// sine and cosine: sincos_angle.h.
#pragma once

#include <cmath>

#include "common.h"
#include "pl_common.h"
#include "box_muller_math.h"
#include "sincos_angle.h"

namespace efl {
namespace {

// TF's Uint32ToFloat: 23 mantissa bits under exponent 127, minus 1.0
__device__ __forceinline__ float u01(uint32_t w) {
  return __uint_as_float(0x3f800000u | (w & 0x7fffffu)) - 1.0f;
}

// KEEP hands out the stage values of a pair (efl_dp_box_muller); the production instances
// (KEEP = false) compute nothing for it.
struct bm_stages { float r, sn, cs; };

template <bool KEEP = false>
__device__ __forceinline__ void box_muller(uint32_t x0, uint32_t x1, float& f0, float& f1,
                                           bm_stages* st = nullptr) {
  const float u1 = u01(x0);
  const float v1 = efl_box_muller_angle(u01(x1));   // float(2 pi (double) u), no doubles
  // both arms computed and one selected: a branch around the logarithm costs more than it saves
  float tl;
  const float lg = log_unit(fmaxf(u1, 1.0e-7f), tl);
  const float rr = radius_unit(lg, tl);
  const float r = u1 < 1.0e-7f ? __uint_as_float(kRClampBits) : rr;
  float sn, cs;
  efl_sincos_angle(v1, &sn, &cs);   // v1 in [0, 2 pi]: <= 1 ulp of the rounded sin / cos (sincos_angle.h)
  f0 = sn * r;
  f1 = cs * r;
  if constexpr (KEEP) *st = bm_stages{r, sn, cs};
}

__device__ __forceinline__ void normal4(uint64_t seed, uint64_t blk, float (&z)[4]) {
  uint32_t c[4] = {(uint32_t)blk, (uint32_t)(blk >> 32), 0u, 0u};
  pl::philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  box_muller(c[0], c[1], z[0], z[1]);
  box_muller(c[2], c[3], z[2], z[3]);
}

// The staged form (csrc/mask.hip's comment on k_dp_noise tells why): the stages after the Philox rounds
// across 2 NB Box-Muller pairs, and the normals of the NB blocks blk0, blk0 + stride, ..., the same
// values as normal4 on each.
template <int NB, bool KEEP = false, class WORDS>
__device__ __forceinline__ void box_muller_staged(WORDS words, float (&z)[NB][4], bm_stages* st = nullptr) {
  constexpr int P = 2 * NB;
  uint32_t c[NB][4];
  words(c);
  float u1[P], v1[P], r[P], tl[P], sn[P], cs[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    u1[p] = u01(c[p >> 1][(p & 1) * 2]);
    v1[p] = efl_box_muller_angle(u01(c[p >> 1][(p & 1) * 2 + 1]));
  }
#pragma unroll
  for (int p = 0; p < P; ++p) r[p] = log_unit(fmaxf(u1[p], 1.0e-7f), tl[p]);
#pragma unroll
  for (int p = 0; p < P; ++p) r[p] = radius_unit(r[p], tl[p]);
#pragma unroll
  for (int p = 0; p < P; ++p) r[p] = u1[p] < 1.0e-7f ? __uint_as_float(kRClampBits) : r[p];
#pragma unroll
  for (int p = 0; p < P; ++p) efl_sincos_angle(v1[p], &sn[p], &cs[p]);
#pragma unroll
  for (int p = 0; p < P; ++p) {
    z[p >> 1][(p & 1) * 2] = sn[p] * r[p];
    z[p >> 1][(p & 1) * 2 + 1] = cs[p] * r[p];
  }
  if constexpr (KEEP) {
#pragma unroll
    for (int p = 0; p < P; ++p) st[p] = bm_stages{r[p], sn[p], cs[p]};
  }
}

template <int NB>
__device__ __forceinline__ void normals(uint64_t seed, uint64_t blk0, uint64_t stride, float (&z)[NB][4]) {
  box_muller_staged<NB>(
      [=](uint32_t (&c)[NB][4]) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const uint64_t blk = blk0 + (uint64_t)b * stride;
          c[b][0] = (uint32_t)blk;
          c[b][1] = (uint32_t)(blk >> 32);
          c[b][2] = 0u;
          c[b][3] = 0u;
        }
        pl::philox_n<NB>(c, (uint32_t)seed, (uint32_t)(seed >> 32));
      },
      z);
}

// MODE 0, ElementWiseGaussianSumQuery.add_noise (dp_optimizer.py:70-71): v + normal * v * sigma;
// MODE 1, GaussianSumQuery (tensorflow_privacy 0.3.0, TF 1.x branch): v + (normal * stddev + 0);
// then safe_normalize (dp_optimizer.py:210-214): / num_microbatches. Each op rounds on its own.
// POW2: the divisor is a power of two and `div` holds its reciprocal: x * 2^-k is the correctly
// rounded x / 2^k (the same exact real, one rounding), without the IEEE division sequence.
template <int MODE, bool POW2>
__device__ __forceinline__ float dp_one(float v, float z, float sigma, float div) {
#pragma clang fp contract(off)
  const float n = MODE == 0 ? (z * v) * sigma : z * sigma + 0.0f;
  return POW2 ? (v + n) * div : (v + n) / div;
}

// The divisor as dp_one takes it: the exact reciprocal of a power of two whose reciprocal is a
// normal float (returns true), the divisor itself otherwise.
inline bool dp_divisor(float divisor, float* d) {
  int ex = 0;
  const bool pow2 = std::isfinite(divisor) && std::frexp(std::fabs(divisor), &ex) == 0.5f &&
                    std::isnormal(1.0f / divisor);
  *d = pow2 ? 1.0f / divisor : divisor;
  return pow2;
}

}  // namespace
}  // namespace efl
