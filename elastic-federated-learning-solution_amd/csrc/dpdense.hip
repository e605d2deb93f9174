// DP-SGD for dense layers without the per-microbatch gradient stack: the clip norms
// and the clipped, noised sum of a Linear layer's weight and bias gradients straight from the layer's
// input X [B, in] and the gradient D [B, out] of the summed loss with respect to its output.
//
// Reference: efls-train/python/efl/privacy/dp_optimizer.py compute_gradients (:148-216); the models
// of example/criteo/criteo_dp_leader_dense.py and example/dp_mnist/leader.py are dense layers.
// Microbatch i is the r = B / rows consecutive batch rows [i r, (i + 1) r); its weight gradient is
// G_i = D_i^T X_i [out, in] and its bias gradient is g_i = sum_a d_a. Then
//   ||G_i||_F^2 = sum_{a, b in i} (x_a . x_b)(d_a . d_b)     (two r x r Gram matrices),
//   sum_i s_i G_i = D^T diag(s_{k / r}) X                    (one GEMM with K = B),
// so nothing of size rows x in x out is ever formed.
//
// Launches (a further set per 32 layers):
//   k_dp_dense_sqnorm  grid (microbatch, layer). r = 1: ||x||^2 ||d||^2 (+ ||d||^2 for the bias), the
//                      lanes striding the columns with 16-byte loads, no LDS Grams. r > 1: X_i and D_i
//                      go through LDS 256 columns at a time (row length 257, so the r rows of one
//                      column lie in r different banks); one thread owns one (matrix, column half,
//                      pair a <= b) and adds its products in double; the bias term is the column sums
//                      of the same D tile. The pair sums meet in LDS, Gx[a,b] Gd[a,b] is taken once
//                      for a = b and twice for a < b (the mirrored half), and the workgroup reduces by
//                      wave shuffles, then LDS, into its own slot work[row][layer]. No atomics.
//   k_dp_scales        (dp_scales.h) one wave per row, as efl_dp_clip_sum.
//   k_dp_dense_sum     one wave = one 32x32 block of W^T [in, out] = X^T diag(s) D on
//                      v_mfma_f32_32x32x2_f32, M = in, N = out, K = B. Both operands are K-major in
//                      memory as they lie: lane l of a k pair reads X[k + l / 32][m0 + l % 32] and
//                      D[k + l / 32][n0 + l % 32], two 128-byte runs per operand, no transpose and no
//                      LDS. The accumulator gives lane l the rows m0 + 8 g + 4 (l / 32) + {0..3} at
//                      column n0 + l % 32: four consecutive `in` of one `out`, which is one 16-byte
//                      store into w_out[out][in] and, with in % 4 == 0, exactly one Philox block.
//                      The scale s[k / r] goes onto the D fragment (one fp32 rounding) from a per-k
//                      table in LDS, 1,024 k at a time. The loads of the next 16 k are issued before
//                      the 8 MFMAs of the current 16. Rows k >= B, m >= in and n >= out are clamped
//                      loads turned into zeros, and are never stored. The blocks with m0 = 0 also add
//                      their scaled D fragments into the bias gradient (two fp32 chains, even and
//                      odd k, joined once) and noise and store it.
// Epilogue: with in % 4 == 0 the lane runs normal4 / dp_one on its sums (dp_normal.h, as
// k_dp_clip_sum). Otherwise a Philox block straddles two weight rows: the kernel stores the plain
// sums and efl_dp_noise finishes them in place, the same functions over the same sums.
// One wave per block and a fixed k order: the same inputs give the same bytes.
#include <cstdint>

#include "common.h"
#include "dp_normal.h"
#include "dp_scales.h"

#pragma clang fp contract(off)

namespace efl {
namespace {

typedef float acc16 __attribute__((ext_vector_type(16)));

constexpr int kMaxLayers = 32;      // layers per launch: 32 x 80 B of the 4 KiB argument space
constexpr int kMaxR = 16;           // batch rows per microbatch
constexpr int kPairs = kMaxR * (kMaxR + 1) / 2;
constexpr int kCols = 256;          // columns of X_i / D_i in LDS at a time
constexpr int kLd = kCols + 1;      // LDS row length: row a of column c in bank (a + c) % 64
constexpr int kItems = (4 * kPairs + kBlock - 1) / kBlock;   // (matrix, half, pair) items per thread
constexpr int kKChunk = 1024;       // k whose scales are staged in LDS at a time
constexpr int kU = 8;               // MFMAs (k pairs) per register buffer

struct dd_chunk {
  efl_dp_dense v[kMaxLayers];
  uint32_t first[kMaxLayers + 1];   // layer i's first 32x32 block in the GEMM grid
  uint32_t vecx, vecd;              // bit i: layer i's x / d rows take 16-byte loads
  int n;
};

__device__ __forceinline__ int find_layer(const dd_chunk& c, uint32_t tile) {
  int lo = 0, hi = c.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (c.first[mid] <= tile) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the workgroup's sum of s, in every thread of wave 0 (fixed order: the wave trees, then waves 0..3)
__device__ __forceinline__ double block_sum(double s, double* part) {
  const int tid = (int)threadIdx.x;
  s = wave_sum(s);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  double t = part[0];
#pragma unroll
  for (int w = 1; w < kBlock / 64; ++w) t += part[w];
  __syncthreads();
  return t;
}

// sum of squares of p[0, n) over the workgroup's lanes, each lane's share in double
__device__ __forceinline__ double lane_sumsq(const float* __restrict__ p, int n, bool vec) {
  const int tid = (int)threadIdx.x;
  double acc = 0.0;
  if (vec) {
    const int full = n & ~3;
    for (int g = 4 * tid; g < full; g += 4 * kBlock) {
      const f4 x = *reinterpret_cast<const f4*>(p + g);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc += (double)x[j] * (double)x[j];
    }
    if (tid < n - full) acc += (double)p[full + tid] * (double)p[full + tid];
  } else {
    for (int i = tid; i < n; i += kBlock) acc += (double)p[i] * (double)p[i];
  }
  return acc;
}

// columns [c0, c0 + nc) of r rows (row a at p + a * stride) into t[a * kLd + c]
__device__ __forceinline__ void stage_rows(const float* __restrict__ p, long long stride, int r, int c0, int nc,
                                           bool vec, float* t) {
  const int tid = (int)threadIdx.x;
  if (vec) {
    const int full = nc & ~3;
    for (int e = tid; e < r * (kCols / 4); e += kBlock) {
      const int a = e / (kCols / 4), c = 4 * (e % (kCols / 4));
      if (c < full) {
        const f4 x = *reinterpret_cast<const f4*>(p + a * stride + c0 + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) t[a * kLd + c + j] = x[j];
      } else {
        for (int j = 0; c + j < nc; ++j) t[a * kLd + c + j] = p[a * stride + c0 + c + j];
      }
    }
  } else {
    for (int e = tid; e < r * kCols; e += kBlock) {
      const int a = e / kCols, c = e % kCols;
      if (c < nc) t[a * kLd + c] = p[a * stride + c0 + c];
    }
  }
}

// Pass 1. Workgroup (microbatch, layer): ||D_i^T X_i||_F^2 (+ ||sum_a d_a||^2 with a bias) in double.
__global__ __launch_bounds__(kBlock) void k_dp_dense_sqnorm(const dd_chunk c, int r, long long slot0,
                                                            long long slots, double* __restrict__ work) {
  __shared__ double part[kBlock / 64];
  const int li = (int)blockIdx.y, tid = (int)threadIdx.x;
  const long long row = blockIdx.x;
  const efl_dp_dense& L = c.v[li];
  const int in = (int)L.in, out = (int)L.out;
  const bool vx = (c.vecx >> li) & 1, vd = (c.vecd >> li) & 1, bias = L.b_out != nullptr;
  const float* __restrict__ x = L.x + row * r * L.x_row_stride;
  const float* __restrict__ d = L.d + row * r * L.d_row_stride;
  double* slot = work + row * slots + slot0 + li;
  if (r == 1) {
    const double sx = block_sum(lane_sumsq(x, in, vx), part);
    const double sd = block_sum(lane_sumsq(d, out, vd), part);
    if (tid == 0) *slot = bias ? sx * sd + sd : sx * sd;
    return;
  }
  __shared__ float tx[kMaxR * kLd], td[kMaxR * kLd];
  __shared__ double gram[4][kPairs];            // [matrix * 2 + half][pair]
  __shared__ unsigned char pa[kPairs], pb[kPairs];
  const int np = r * (r + 1) / 2;
  if (tid < r)                                  // pairs (a, b), a <= b, in row-major order
    for (int b = tid, p = tid * r - tid * (tid - 1) / 2; b < r; ++b, ++p) { pa[p] = (unsigned char)tid; pb[p] = (unsigned char)b; }
  __syncthreads();
  // this thread's items: matrix (0 = X, 1 = D), column half, pair
  int ia[kItems], ib[kItems], ihalf[kItems], imat[kItems];
  double g[kItems];
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int it = tid + j * kBlock;
    g[j] = 0.0;
    imat[j] = -1;
    ia[j] = ib[j] = ihalf[j] = 0;
    if (it < 4 * np) {
      imat[j] = it / (2 * np);
      ihalf[j] = it % (2 * np) / np;
      ia[j] = pa[it % np];
      ib[j] = pb[it % np];
    }
  }
  double bs = 0.0;                              // this thread's columns of ||sum_a d_a||^2
  const int wide = in > out ? in : out;
  for (int c0 = 0; c0 < wide; c0 += kCols) {
    const int nx = in - c0 < 0 ? 0 : in - c0 < kCols ? in - c0 : kCols;
    const int nd = out - c0 < 0 ? 0 : out - c0 < kCols ? out - c0 : kCols;
    if (c0) __syncthreads();                    // every thread is done with the tiles before
    if (nx) stage_rows(x, L.x_row_stride, r, c0, nx, vx, tx);
    if (nd) stage_rows(d, L.d_row_stride, r, c0, nd, vd, td);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      if (imat[j] < 0) continue;
      const float* t = imat[j] ? td : tx;
      const int n = imat[j] ? nd : nx;
      const int lo = ihalf[j] * (kCols / 2), hi = n < lo + kCols / 2 ? n : lo + kCols / 2;
      const float* ta = t + ia[j] * kLd;
      const float* tb = t + ib[j] * kLd;
      double s = g[j];
      for (int cc = lo; cc < hi; ++cc) s += (double)ta[cc] * (double)tb[cc];
      g[j] = s;
    }
    if (bias && tid < nd) {
      double cs = 0.0;
      for (int a = 0; a < r; ++a) cs += (double)td[a * kLd + tid];
      bs += cs * cs;
    }
  }
#pragma unroll
  for (int j = 0; j < kItems; ++j)
    if (imat[j] >= 0) gram[imat[j] * 2 + ihalf[j]][(tid + j * kBlock) % np] = g[j];
  __syncthreads();
  double v = bs;
  if (tid < np) {
    const double gx = gram[0][tid] + gram[1][tid], gd = gram[2][tid] + gram[3][tid];
    v += pa[tid] == pb[tid] ? gx * gd : 2.0 * (gx * gd);   // the mirrored half of the symmetric Grams
  }
  v = block_sum(v, part);
  if (tid == 0) *slot = v;
}

// Pass 2. One wave: a 32x32 block of W^T = X^T diag(s) D of one layer, its noise and its store.
template <bool CLIP, int MODE, bool POW2>
__global__ __launch_bounds__(64) void k_dp_dense_sum(const dd_chunk c, long long B, int r,
                                                     const float* __restrict__ scales, uint64_t seed, float sigma,
                                                     float div) {
  __shared__ float sk[CLIP ? kKChunk : 1];      // sk[k % kKChunk] = scales[k / r]
  const int lane = (int)threadIdx.x, h = lane >> 5, l = lane & 31;
  const int li = find_layer(c, blockIdx.x);
  const efl_dp_dense& L = c.v[li];
  const long long in = L.in, out = L.out, xs = L.x_row_stride, ds = L.d_row_stride;
  const uint32_t t = blockIdx.x - c.first[li], tiles_m = (uint32_t)((in + 31) / 32);
  const uint32_t bn = t / tiles_m, bm = t - bn * tiles_m;
  const long long m = (long long)bm * 32 + l, n = (long long)bn * 32 + l;
  const bool mok = m < in, nok = n < out;
  const bool do_bias = bm == 0 && L.b_out != nullptr;
  // clamped, so that every load is in bounds and unconditional; the edges become zeros at use
  const float* __restrict__ xp = L.x + (mok ? m : 0);
  const float* __restrict__ dp = L.d + (nok ? n : 0);

  float a0[kU], b0[kU], a1[kU], b1[kU];
  auto load = [&](long long kb, float (&a)[kU], float (&b)[kU]) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      long long k = kb + 2 * u + h;
      k = k < B ? k : B - 1;
      a[u] = xp[k * xs];
      b[u] = dp[k * ds];
    }
  };

  acc16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
  float bsum = 0.0f;

  load(0, a0, b0);
  for (long long kb = 0; kb < B; kb += 2 * kU) {
    const int ko = (int)(kb % kKChunk);
    if constexpr (CLIP) {
      if (ko == 0) {
        if (kb) __syncthreads();                // the wave is done with the chunk before
        const long long left = B - kb;
        const int nk = left < kKChunk ? (int)left : kKChunk;
        for (int i = lane; i < nk; i += 64) sk[i] = scales[(kb + i) / r];
        __syncthreads();
      }
    }
    const bool more = kb + 2 * kU < B;
    if (more) load(kb + 2 * kU, a1, b1);        // the next step's loads travel under the MFMAs
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const bool kok = kb + 2 * u + h < B;
      const float a = (kok && mok) ? a0[u] : 0.0f;
      float b = 0.0f;
      if (kok && nok) b = CLIP ? b0[u] * sk[ko + 2 * u + h] : b0[u];
      if (do_bias) bsum = bsum + b;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < kU; ++u) { a0[u] = a1[u]; b0[u] = b1[u]; }
    }
  }

  // weights: register 4 g + j of lane (h, l) is W^T[m0 + 8 g + 4 h + j][n0 + l]
  const bool fused = (in & 3) == 0;
  if (nok) {
    float* wrow = L.w_out + n * in;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const long long mm = (long long)bm * 32 + 8 * g4 + 4 * h;
      if (fused) {
        if (mm < in) {                          // in % 4 == 0: all four or none
          float z[4];
          normal4(seed, L.ctr0_w + (uint64_t)((n * in + mm) >> 2), z);
          f4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = dp_one<MODE, POW2>(acc[4 * g4 + j], z[j], sigma, div);
          *reinterpret_cast<f4*>(wrow + mm) = o;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (mm + j < in) wrow[mm + j] = acc[4 * g4 + j];
      }
    }
  }
  // bias: lane (0, l) joins the two k chains; the lane of every fourth column takes its Philox block
  if (do_bias) {                                // uniform over the wave
    const float tot = bsum + __shfl_xor(bsum, 32);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __shfl(tot, (lane + j) & 63);
    if (h == 0 && (l & 3) == 0 && nok) {
      float z[4];
      normal4(seed, L.ctr0_b + (uint64_t)(n >> 2), z);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (n + j < out) L.b_out[n + j] = dp_one<MODE, POW2>(v[j], z[j], sigma, div);
    }
  }
}

template <bool CLIP>
void launch_dense_sum(int mode, bool pow2, unsigned grid, hipStream_t s, const dd_chunk& c, long long B, int r,
                      const float* scales, uint64_t seed, float sigma, float d) {
  if (mode == 0 && pow2) k_dp_dense_sum<CLIP, 0, true><<<grid, 64, 0, s>>>(c, B, r, scales, seed, sigma, d);
  else if (mode == 0) k_dp_dense_sum<CLIP, 0, false><<<grid, 64, 0, s>>>(c, B, r, scales, seed, sigma, d);
  else if (pow2) k_dp_dense_sum<CLIP, 1, true><<<grid, 64, 0, s>>>(c, B, r, scales, seed, sigma, d);
  else k_dp_dense_sum<CLIP, 1, false><<<grid, 64, 0, s>>>(c, B, r, scales, seed, sigma, d);
}

// fn(chunk, index of its first layer) for every run of at most kMaxLayers layers; false when a
// chunk's GEMM grid would pass 2^31 - 1 blocks
template <class F>
bool for_chunks(const efl_dp_dense* layers, int64_t nlayers, F fn) {
  for (int64_t i0 = 0; i0 < nlayers; i0 += kMaxLayers) {
    dd_chunk c;
    long long total = 0;
    c.n = (int)(nlayers - i0 < kMaxLayers ? nlayers - i0 : kMaxLayers);
    c.vecx = c.vecd = 0;
    for (int i = 0; i < c.n; ++i) {
      const efl_dp_dense& L = layers[i0 + i];
      c.v[i] = L;
      c.first[i] = (uint32_t)total;
      if (aligned(L.x, 16) && L.x_row_stride % 4 == 0) c.vecx |= 1u << i;
      if (aligned(L.d, 16) && L.d_row_stride % 4 == 0) c.vecd |= 1u << i;
      total += ((L.in + 31) / 32) * ((L.out + 31) / 32);
      if (total > 0x7fffffffll) return false;
    }
    c.first[c.n] = (uint32_t)total;
    fn(c, i0);
  }
  return true;
}

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API int64_t efl_dp_dense_work_elems(int64_t nlayers, int64_t rows) {
  if (nlayers < 0 || rows <= 0 || (nlayers > 0 && rows > INT64_MAX / 16 / nlayers)) {
    set_error("efl_dp_dense_work_elems: nlayers must be >= 0 and rows > 0 (and their product below 2^59)");
    return EFL_E_INVALID_ARGUMENT;
  }
  return nlayers * rows;
}

EFL_API int efl_dp_dense_sqnorm(const efl_dp_dense* layers, int64_t nlayers, int64_t B, int64_t rows, double* work,
                                int64_t slot0, int64_t slots, void* stream) {
  constexpr int64_t kMax = 0x7fffffff;
  if (nlayers < 0 || rows <= 0 || B <= 0 || B > kMax) { set_error("efl_dp_dense_sqnorm: nlayers must be >= 0, rows > 0 and 0 < B < 2^31"); return EFL_E_INVALID_ARGUMENT; }
  if (B % rows != 0 || B / rows > kMaxR) { set_error("efl_dp_dense_sqnorm: rows (%lld) must divide B (%lld) into at most %d batch rows each", (long long)rows, (long long)B, kMaxR); return EFL_E_INVALID_ARGUMENT; }
  if (nlayers == 0) return EFL_OK;
  if (!layers) { set_error("efl_dp_dense_sqnorm: null layer table"); return EFL_E_INVALID_ARGUMENT; }
  for (int64_t i = 0; i < nlayers; ++i) {
    const efl_dp_dense& L = layers[i];
    if (L.in <= 0 || L.out <= 0 || L.in > kMax || L.out > kMax || !L.x || !L.d || !aligned(L.x, 4) || !aligned(L.d, 4) ||
        L.x_row_stride < L.in || L.d_row_stride < L.out) {
      set_error("efl_dp_dense_sqnorm: layer %lld: null or misaligned x / d, in or out < 1, or a row stride below its width", (long long)i);
      return EFL_E_INVALID_ARGUMENT;
    }
  }
  if (!work || !aligned(work, 8) || slot0 < 0 || slots > INT64_MAX / 16 / rows || slot0 > slots - nlayers) {
    set_error("efl_dp_dense_sqnorm: work must hold rows x slots doubles with the layers' %lld slots in [slot0, slots)", (long long)nlayers);
    return EFL_E_INVALID_ARGUMENT;
  }
  for_chunks(layers, nlayers, [&](const dd_chunk& c, int64_t i0) {
    k_dp_dense_sqnorm<<<dim3((unsigned)rows, (unsigned)c.n), kBlock, 0, (hipStream_t)stream>>>(c, (int)(B / rows), slot0 + i0, slots, work);
  });
  return hip_status(hipGetLastError(), "efl_dp_dense_sqnorm");
}

EFL_API int efl_dp_dense_clip_sum(const efl_dp_dense* layers, int64_t nlayers, int64_t B, int64_t rows, int clip_mode,
                                  float l2_norm_clip, int mode, float sigma, float divisor, uint64_t seed,
                                  float* scales, double* work, int64_t work_elems, void* stream) {
  constexpr int64_t kMax = 0x7fffffff;
  if (clip_mode < 0 || clip_mode > 2) { set_error("efl_dp_dense_clip_sum: clip_mode must be 0 (none), 1 (from the norms) or 2 (given scales)"); return EFL_E_INVALID_ARGUMENT; }
  if (mode < 0 || mode > 1) { set_error("efl_dp_dense_clip_sum: mode must be 0 (element-wise) or 1 (Gaussian sum)"); return EFL_E_INVALID_ARGUMENT; }
  if (!(divisor == divisor) || divisor == 0.0f) { set_error("efl_dp_dense_clip_sum: divisor must be non-zero"); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode == 1 && !(l2_norm_clip > 0.0f)) { set_error("efl_dp_dense_clip_sum: l2_norm_clip must be positive"); return EFL_E_INVALID_ARGUMENT; }
  if (nlayers < 0 || rows <= 0 || B <= 0 || B > kMax) { set_error("efl_dp_dense_clip_sum: nlayers must be >= 0, rows > 0 and 0 < B < 2^31"); return EFL_E_INVALID_ARGUMENT; }
  if (B % rows != 0) { set_error("efl_dp_dense_clip_sum: rows (%lld) must divide B (%lld)", (long long)rows, (long long)B); return EFL_E_INVALID_ARGUMENT; }
  const int64_t r = B / rows;
  if (r > kMaxR) { set_error("efl_dp_dense_clip_sum: %lld batch rows per microbatch, at most %d", (long long)r, kMaxR); return EFL_E_INVALID_ARGUMENT; }
  if (nlayers == 0) return EFL_OK;
  if (!layers) { set_error("efl_dp_dense_clip_sum: null layer table"); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode != 0 && (!scales || !aligned(scales, 4))) { set_error("efl_dp_dense_clip_sum: clip modes 1 and 2 need a scales buffer"); return EFL_E_INVALID_ARGUMENT; }
  for (int64_t i = 0; i < nlayers; ++i) {
    const efl_dp_dense& L = layers[i];
    if (L.in <= 0 || L.out <= 0 || L.in > kMax || L.out > kMax) { set_error("efl_dp_dense_clip_sum: layer %lld: in and out must be in 1 .. 2^31 - 1", (long long)i); return EFL_E_INVALID_ARGUMENT; }
    if (!L.x || !L.d || !L.w_out) { set_error("efl_dp_dense_clip_sum: layer %lld: null buffer", (long long)i); return EFL_E_INVALID_ARGUMENT; }
    if (!aligned(L.x, 4) || !aligned(L.d, 4) || !aligned(L.w_out, 16) || !aligned(L.b_out, 4)) {
      set_error("efl_dp_dense_clip_sum: layer %lld: x, d and b_out must be 4-byte and w_out 16-byte aligned", (long long)i);
      return EFL_E_INVALID_ARGUMENT;
    }
    if (L.x_row_stride < L.in || L.d_row_stride < L.out) {
      set_error("efl_dp_dense_clip_sum: layer %lld: a row stride (%lld, %lld) below its width (%lld, %lld)", (long long)i,
                (long long)L.x_row_stride, (long long)L.d_row_stride, (long long)L.in, (long long)L.out);
      return EFL_E_INVALID_ARGUMENT;
    }
  }
  if (clip_mode == 1 && (!work || !aligned(work, 8) || rows > INT64_MAX / 16 / nlayers || work_elems < rows * nlayers)) {
    set_error("efl_dp_dense_clip_sum: work must hold efl_dp_dense_work_elems() = %lld doubles, got %lld", (long long)(rows * nlayers), (long long)work_elems);
    return EFL_E_INVALID_ARGUMENT;
  }
  if (!for_chunks(layers, nlayers, [](const dd_chunk&, int64_t) {})) {   // every grid, before the first launch
    set_error("efl_dp_dense_clip_sum: layers too large for one grid");
    return EFL_E_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  float d;
  const bool pow2 = dp_divisor(divisor, &d);
  if (clip_mode == 1) {
    for_chunks(layers, nlayers, [&](const dd_chunk& c, int64_t i0) {
      k_dp_dense_sqnorm<<<dim3((unsigned)rows, (unsigned)c.n), kBlock, 0, s>>>(c, (int)r, i0, nlayers, work);
    });
    k_dp_scales<<<(unsigned)rows, 64, 0, s>>>(work, nlayers, (double)l2_norm_clip, scales);
  }
  for_chunks(layers, nlayers, [&](const dd_chunk& c, int64_t) {
    if (clip_mode == 0) launch_dense_sum<false>(mode, pow2, c.first[c.n], s, c, B, (int)r, scales, seed, sigma, d);
    else launch_dense_sum<true>(mode, pow2, c.first[c.n], s, c, B, (int)r, scales, seed, sigma, d);
  });
  const int rc = hip_status(hipGetLastError(), "efl_dp_dense_clip_sum");
  if (rc != EFL_OK) return rc;
  // a weight matrix whose rows are no multiple of 4 long: its Philox blocks straddle rows, so the
  // GEMM stored the plain sums and the noise kernel finishes them in place
  for (int64_t i = 0; i < nlayers; ++i) {
    const efl_dp_dense& L = layers[i];
    if (L.in % 4 == 0) continue;
    const int e = efl_dp_noise(L.w_out, L.w_out, L.in * L.out, mode, sigma, divisor, seed, L.ctr0_w, stream);
    if (e != EFL_OK) return e;
  }
  return EFL_OK;
}
