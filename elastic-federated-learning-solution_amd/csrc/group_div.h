// Division of a lane-group index by the row length (csrc/mask.hip: which row and column, hence which
// output slot, a lane group of mask_cols / mask_rows owns), shared with the host so that
// tests/test_group_div_host.py can sweep it with the system compiler.
//
// q = g / d for g < 2^31 as one 64-bit product and a shift (Granlund-Montgomery: l = ceil(log2 d),
// m = floor(2^(31 + l) / d) + 1 < 2^32 is exact for every g < 2^31), from the magic (m, 31 + l) the
// host passes; m == 0 (more than 2^31 groups) takes the 64-bit division.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define EFL_GD_FN __host__ __device__ __forceinline__
#else
#define EFL_GD_FN static inline
#endif

EFL_GD_FN long long div_groups(long long g, long long d, uint32_t m, int sh) {
  if (m) return (long long)(((uint64_t)(uint32_t)g * m) >> sh);
  return g / d;
}

// the magic (m, shift) of div_groups for d, or m = 0 when the groups pass 2^31
static inline void group_magic(long long total, long long d, uint32_t* m, int* sh) {
  *m = 0;
  *sh = 0;
  if (total <= 0 || total >= (1ll << 31) || d <= 0) return;
  int l = 0;
  while ((1ll << l) < d) ++l;
  *m = (uint32_t)(((1ull << (31 + l)) / (unsigned long long)d) + 1ull);
  *sh = 31 + l;
}
