// The clip scales of a DP-SGD step from per-row partial sums of squares, shared by the two units
// that produce such partials (csrc/dpclip.hip from stacked gradients, csrc/dpdense.hip from a dense
// layer's inputs and output gradients).
#pragma once

#include "common.h"

namespace efl {
namespace {

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  return s;
}

// One wave per row: S = the row's slots (lane l takes l, l + 64, ... in order, then the wave's tree),
// scale = clip * min(1 / sqrt(S), 1 / clip) in double, rounded to float once. S = 0 gives 1, an
// infinite S gives 0, a NaN stays a NaN (torch.minimum's rule, as GaussianSumQuery.preprocess_record).
__global__ __launch_bounds__(64) void k_dp_scales(const double* __restrict__ work, long long slots, double clip,
                                                  float* __restrict__ scales) {
  const double* w = work + (long long)blockIdx.x * slots;
  double s = 0.0;
  for (long long i = threadIdx.x; i < slots; i += 64) s += w[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    const double inv = 1.0 / sqrt(s), ic = 1.0 / clip;
    scales[blockIdx.x] = (float)(clip * ((inv < ic || inv != inv) ? inv : ic));
  }
}

}  // namespace
}  // namespace efl
