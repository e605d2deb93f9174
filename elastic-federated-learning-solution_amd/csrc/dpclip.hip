// DP-SGD's per-microbatch step in one pass over the stacked gradients: the
// global L2 norm of every microbatch's record, its clip scale, the row-ordered sum of the scaled
// rows, the noise and the division by the number of microbatches.
//
// Reference: efls-train/python/efl/privacy/dp_optimizer.py compute_gradients (:148-216), with
// tensorflow_privacy 0.3.0's GaussianSumQuery (clip_by_global_norm per record, then the sum):
//   for each microbatch i: g_i = grad(loss_i); s = s + g_i * clip * min(1 / ||g_i||, 1 / clip)
//   final = (s + noise(s)) / num_microbatches
// A record is the list of a model's variables; variable v's microbatch gradients lie stacked as
// [rows, numel_v] (row r at grads + r * row_stride).
//
// Launches (two or three whatever the model; a further set per 64 variables):
//   k_dp_sqnorm    grid (row, variable, 8,192-element tile of the row): the tile's sum of squares
//                  in double, wave shuffles then LDS, one partial per workgroup into its own slot
//                  of `work`; no atomics, so the same bytes on every run;
//   k_dp_scales    (dp_scales.h) one wave per row: the row's slots summed in a fixed order, still in double, and
//                  scale_i = float(clip * min(1 / sqrt(S_i), 1 / clip)) rounded once;
//   k_dp_clip_sum  one lane owns one 4-column group of one variable (one Philox block, as
//                  k_dp_noise): it walks the rows IN ORDER, acc = acc + g * scale_i in fp32 with no
//                  contraction from 0.0f, which is the float the reference's loop of `s + r` makes,
//                  then runs k_dp_noise's noise and division on acc and stores once. The scales are
//                  staged in LDS 1,024 rows at a time; the row loads go out eight at a time and are
//                  added in row order.
// The variables travel BY VALUE as a kernel argument (dp_chunk: at most 64 of them with the first
// workgroup of each), so there is no device-side descriptor table, no allocation and no copy; a
// workgroup finds its variable by a search over that table in scalar registers.
//
// Loads: 16 bytes per lane where a variable's rows allow it (grads 16-byte aligned and row_stride a
// multiple of 4), dwords otherwise (a contiguous [rows, 10] stack has misaligned odd rows) and for
// the ragged last group of a variable with numel % 4 != 0.
#include <cstdint>

#include "common.h"
#include "dp_normal.h"
#include "dp_scales.h"

// acc + g * scale rounds twice, as the reference's separate multiply and add do
#pragma clang fp contract(off)

namespace efl {
namespace {

constexpr int kMaxVars = 64;        // variables per launch: 64 x 40 B of the 4 KiB argument space
constexpr int kNormTile = 8192;     // elements of a row per k_dp_sqnorm workgroup (kBlock x 32)
constexpr int kScaleRows = 1024;    // rows of scales staged in LDS at a time
constexpr int kRowsInFlight = 8;    // row loads a lane issues before it adds them

struct dp_chunk {
  efl_dp_var v[kMaxVars];
  uint32_t first[kMaxVars + 1];     // variable i's first workgroup in the grid; first[n] = all of them
  uint64_t vec;                     // bit i: variable i takes 16-byte loads
  int n;
};

// the variable whose workgroups hold `tile`: the last i with first[i] <= tile (every variable of a
// chunk has at least one workgroup, so first[] is strictly increasing)
__device__ __forceinline__ int find_var(const dp_chunk& c, uint32_t tile) {
  int lo = 0, hi = c.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (c.first[mid] <= tile) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Pass 1. Workgroup (row, tile): sum of squares of up to kNormTile elements of one variable's row.
__global__ __launch_bounds__(kBlock) void k_dp_sqnorm(const dp_chunk c, uint32_t tiles, long long slot0,
                                                      long long slots, double* __restrict__ work) {
  const uint32_t row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
  const int vi = find_var(c, tile), tid = (int)threadIdx.x;
  const long long e0 = (long long)(tile - c.first[vi]) * kNormTile;
  const long long left = c.v[vi].numel - e0;
  const int n = left < kNormTile ? (int)left : kNormTile;
  const float* __restrict__ p = c.v[vi].grads + (long long)row * c.v[vi].row_stride + e0;
  double acc = 0.0;
  if ((c.vec >> vi) & 1) {
    constexpr int G = kNormTile / 4 / kBlock;   // 16-byte groups per lane, kBlock apart
    f4 x[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const int g = k * kBlock + tid;
      x[k] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      if (4 * g + 4 <= n) x[k] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p) + g);
    }
#pragma unroll
    for (int k = 0; k < G; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc += (double)x[k][j] * (double)x[k][j];
    const int full = n & ~3;                    // the ragged end of the row: n % 4 dwords
    if (tid < n - full) {
      const float t = p[full + tid];
      acc += (double)t * (double)t;
    }
  } else {
    for (int k0 = 0; k0 < kNormTile / kBlock; k0 += kRowsInFlight) {
      float x[kRowsInFlight];
#pragma unroll
      for (int u = 0; u < kRowsInFlight; ++u) {
        const int i = (k0 + u) * kBlock + tid;
        x[u] = i < n ? p[i] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < kRowsInFlight; ++u) acc += (double)x[u] * (double)x[u];
    }
  }
  __shared__ double part[kBlock / 64];
  acc = wave_sum(acc);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = part[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) s += part[w];
    work[(long long)row * slots + slot0 + tile] = s;
  }
}

// a lane's four columns of one row: one 16-byte load, or `cnt` (1..4) dwords and zeros
template <bool VEC>
__device__ __forceinline__ f4 load_group(const float* p, int cnt) {
  if constexpr (VEC) {
    return __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
  } else {
    f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) v[j] = p[j];
    return v;
  }
}

// rows [0, nr) from p (row stride `stride`), added in row order; sc: their scales (CLIP)
template <bool VEC, bool CLIP>
__device__ __forceinline__ void walk_rows(const float* p, long long stride, int nr, int cnt, const float* sc,
                                          f4& acc) {
  int r = 0;
  for (; r + kRowsInFlight <= nr; r += kRowsInFlight) {
    f4 x[kRowsInFlight];
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) x[u] = load_group<VEC>(p + (long long)(r + u) * stride, cnt);
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
      const float s = CLIP ? sc[r + u] : 1.0f;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = CLIP ? acc[j] + x[u][j] * s : acc[j] + x[u][j];
    }
  }
  for (; r < nr; ++r) {
    const f4 x = load_group<VEC>(p + (long long)r * stride, cnt);
    const float s = CLIP ? sc[r] : 1.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = CLIP ? acc[j] + x[j] * s : acc[j] + x[j];
  }
}

// Pass 2. Workgroup = 256 column groups (1,024 columns) of one variable, all rows.
template <bool CLIP, int MODE, bool POW2>
__global__ __launch_bounds__(kBlock) void k_dp_clip_sum(const dp_chunk c, long long rows,
                                                        const float* __restrict__ scales, uint64_t seed,
                                                        float sigma, float div) {
  __shared__ float sc[CLIP ? kScaleRows : 1];
  const int vi = find_var(c, blockIdx.x), tid = (int)threadIdx.x;
  const long long numel = c.v[vi].numel, stride = c.v[vi].row_stride;
  const long long g = (long long)(blockIdx.x - c.first[vi]) * kBlock + tid, j0 = 4 * g;
  const bool active = j0 < numel;
  const int cnt = !active ? 0 : numel - j0 < 4 ? (int)(numel - j0) : 4;
  const bool vec = ((c.vec >> vi) & 1) && cnt == 4;
  const float* p = c.v[vi].grads + j0;
  f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (long long r0 = 0; r0 < rows; r0 += kScaleRows) {
    const int nr = rows - r0 < kScaleRows ? (int)(rows - r0) : kScaleRows;
    if constexpr (CLIP) {
      if (r0) __syncthreads();                  // every lane is done with the chunk before
      for (int i = tid; i < nr; i += kBlock) sc[i] = scales[r0 + i];
      __syncthreads();
    }
    if (active) {
      if (vec) walk_rows<true, CLIP>(p + r0 * stride, stride, nr, cnt, sc, acc);
      else walk_rows<false, CLIP>(p + r0 * stride, stride, nr, cnt, sc, acc);
    }
  }
  if (!active) return;
  float z[4];
  normal4(seed, c.v[vi].ctr0 + (uint64_t)g, z);
  f4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = dp_one<MODE, POW2>(acc[j], z[j], sigma, div);
  float* out = c.v[vi].out + j0;
  if (cnt == 4) *reinterpret_cast<f4*>(out) = o;
  else
    for (int j = 0; j < cnt; ++j) out[j] = o[j];
}

template <bool CLIP>
void launch_clip_sum(int noise_mode, bool pow2, unsigned grid, hipStream_t s, const dp_chunk& c, long long rows,
                     const float* scales, uint64_t seed, float sigma, float d) {
  if (noise_mode == 0 && pow2) k_dp_clip_sum<CLIP, 0, true><<<grid, kBlock, 0, s>>>(c, rows, scales, seed, sigma, d);
  else if (noise_mode == 0) k_dp_clip_sum<CLIP, 0, false><<<grid, kBlock, 0, s>>>(c, rows, scales, seed, sigma, d);
  else if (pow2) k_dp_clip_sum<CLIP, 1, true><<<grid, kBlock, 0, s>>>(c, rows, scales, seed, sigma, d);
  else k_dp_clip_sum<CLIP, 1, false><<<grid, kBlock, 0, s>>>(c, rows, scales, seed, sigma, d);
}

long long norm_tiles(long long numel) { return (numel + kNormTile - 1) / kNormTile; }
long long sum_tiles(long long numel) { return ((numel + 3) / 4 + kBlock - 1) / kBlock; }

// fn(chunk) for every run of at most kMaxVars non-empty variables, each with tiles(numel) workgroups
// of a grid that has `per_tile` of them per tile; false when a grid would pass 2^31 - 1 workgroups
template <class F>
bool for_chunks(const efl_dp_var* vars, int64_t nvars, long long (*tiles)(long long), long long per_tile, F fn) {
  int64_t i = 0;
  while (i < nvars) {
    dp_chunk c;
    long long total = 0;
    c.n = 0;
    c.vec = 0;
    for (; i < nvars && c.n < kMaxVars; ++i) {
      if (vars[i].numel == 0) continue;
      c.v[c.n] = vars[i];
      c.first[c.n] = (uint32_t)total;
      if (aligned(vars[i].grads, 16) && vars[i].row_stride % 4 == 0) c.vec |= 1ull << c.n;
      total += tiles(vars[i].numel);
      if (total * per_tile > 0x7fffffffll) return false;
      ++c.n;
    }
    if (c.n == 0) break;
    c.first[c.n] = (uint32_t)total;
    fn(c);
  }
  return true;
}

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API int64_t efl_dp_clip_work_elems(const int64_t* numels, int64_t nvars, int64_t rows) {
  if (nvars < 0 || rows <= 0 || (nvars > 0 && !numels)) {
    set_error("efl_dp_clip_work_elems: nvars must be >= 0 and rows > 0");
    return EFL_E_INVALID_ARGUMENT;
  }
  long long tiles = 0;
  for (int64_t i = 0; i < nvars; ++i) {
    if (numels[i] < 0) { set_error("efl_dp_clip_work_elems: negative element count"); return EFL_E_INVALID_ARGUMENT; }
    tiles += norm_tiles(numels[i]);
    if (tiles > INT64_MAX / 16 / rows) { set_error("efl_dp_clip_work_elems: record too large"); return EFL_E_INVALID_ARGUMENT; }
  }
  return rows * tiles;
}

EFL_API int efl_dp_clip_sum(const efl_dp_var* vars, int64_t nvars, int64_t rows, int clip_mode, float l2_norm_clip,
                            int noise_mode, float sigma, float divisor, uint64_t seed, float* scales, double* work,
                            int64_t work_elems, void* stream) {
  if (clip_mode < 0 || clip_mode > 2) { set_error("efl_dp_clip_sum: clip_mode must be 0 (none), 1 (from the norms) or 2 (given scales)"); return EFL_E_INVALID_ARGUMENT; }
  if (noise_mode < 0 || noise_mode > 1) { set_error("efl_dp_clip_sum: noise_mode must be 0 (element-wise) or 1 (Gaussian sum)"); return EFL_E_INVALID_ARGUMENT; }
  if (!(divisor == divisor) || divisor == 0.0f) { set_error("efl_dp_clip_sum: divisor must be non-zero"); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode == 1 && !(l2_norm_clip > 0.0f)) { set_error("efl_dp_clip_sum: l2_norm_clip must be positive"); return EFL_E_INVALID_ARGUMENT; }
  if (nvars < 0 || rows <= 0) { set_error("efl_dp_clip_sum: nvars must be >= 0 and rows > 0"); return EFL_E_INVALID_ARGUMENT; }
  if (nvars == 0) return EFL_OK;
  if (!vars) { set_error("efl_dp_clip_sum: null variable table"); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode != 0 && (!scales || !aligned(scales, 4))) { set_error("efl_dp_clip_sum: clip modes 1 and 2 need a scales buffer"); return EFL_E_INVALID_ARGUMENT; }
  long long slots = 0;
  for (int64_t i = 0; i < nvars; ++i) {
    const efl_dp_var& v = vars[i];
    if (v.numel < 0) { set_error("efl_dp_clip_sum: variable %lld: negative element count", (long long)i); return EFL_E_INVALID_ARGUMENT; }
    if (v.numel == 0) continue;
    if (!v.grads || !v.out) { set_error("efl_dp_clip_sum: variable %lld: null buffer", (long long)i); return EFL_E_INVALID_ARGUMENT; }
    if (!aligned(v.grads, 4) || !aligned(v.out, 16)) {
      set_error("efl_dp_clip_sum: variable %lld: grads must be 4-byte and out 16-byte aligned", (long long)i);
      return EFL_E_INVALID_ARGUMENT;
    }
    if (v.row_stride < v.numel) {
      set_error("efl_dp_clip_sum: variable %lld: row_stride %lld < numel %lld", (long long)i, (long long)v.row_stride, (long long)v.numel);
      return EFL_E_INVALID_ARGUMENT;
    }
    slots += norm_tiles(v.numel);
    if (slots > INT64_MAX / 16 / rows) { set_error("efl_dp_clip_sum: record too large"); return EFL_E_INVALID_ARGUMENT; }
  }
  if (clip_mode == 1 && (!work || !aligned(work, 8) || work_elems < rows * slots)) {
    set_error("efl_dp_clip_sum: work must hold efl_dp_clip_work_elems() = %lld doubles, got %lld", (long long)(rows * slots), (long long)work_elems);
    return EFL_E_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  float d;
  const bool pow2 = dp_divisor(divisor, &d);
  // every grid is checked before the first launch
  const auto none = [](const dp_chunk&) {};
  if (rows > 0x7fffffffll || (clip_mode == 1 && !for_chunks(vars, nvars, norm_tiles, rows, none)) ||
      !for_chunks(vars, nvars, sum_tiles, 1, none)) {
    set_error("efl_dp_clip_sum: record too large for one grid");
    return EFL_E_INVALID_ARGUMENT;
  }
  if (slots == 0) return EFL_OK;                  // every variable is empty
  if (clip_mode == 1) {
    long long slot0 = 0;
    for_chunks(vars, nvars, norm_tiles, rows, [&](const dp_chunk& c) {
      const uint32_t tiles = c.first[c.n];
      k_dp_sqnorm<<<(unsigned)(tiles * rows), kBlock, 0, s>>>(c, tiles, slot0, slots, work);
      slot0 += tiles;
    });
    k_dp_scales<<<(unsigned)rows, 64, 0, s>>>(work, slots, (double)l2_norm_clip, scales);
  }
  for_chunks(vars, nvars, sum_tiles, 1, [&](const dp_chunk& c) {
    if (clip_mode == 0) launch_clip_sum<false>(noise_mode, pow2, c.first[c.n], s, c, rows, scales, seed, sigma, d);
    else launch_clip_sum<true>(noise_mode, pow2, c.first[c.n], s, c, rows, scales, seed, sigma, d);
  });
  return hip_status(hipGetLastError(), "efl_dp_clip_sum");
}

EFL_API int efl_dp_scales(const double* work, int64_t slots, int64_t rows, float l2_norm_clip, float* scales,
                          void* stream) {
  if (!(l2_norm_clip > 0.0f)) { set_error("efl_dp_scales: l2_norm_clip must be positive"); return EFL_E_INVALID_ARGUMENT; }
  if (rows <= 0 || rows > 0x7fffffffll || slots < 0) { set_error("efl_dp_scales: 0 < rows < 2^31 and slots >= 0"); return EFL_E_INVALID_ARGUMENT; }
  if (!work || !aligned(work, 8) || !scales || !aligned(scales, 4)) { set_error("efl_dp_scales: null or misaligned buffer"); return EFL_E_INVALID_ARGUMENT; }
  k_dp_scales<<<(unsigned)rows, 64, 0, (hipStream_t)stream>>>(work, slots, (double)l2_norm_clip, scales);
  return hip_status(hipGetLastError(), "efl_dp_scales");
}
