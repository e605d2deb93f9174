// DP-SGD for Linear layers applied at every position of a sequence, without the per-microbatch
// gradient stack: the clip norms and the clipped, noised sum of the layer's weight and
// bias gradients straight from its input x [B, T, in] and the gradient d [B, T, out] of the summed loss
// with respect to its output, both channel-minor as torch.nn.Linear leaves them.
//
// Reference: efls-train/python/efl/privacy/dp_optimizer.py compute_gradients (:148-216). Microbatch i is
// the P = r T consecutive rows from i P of the flattened [B T, .] matrices, r = B / rows. Its weight
// gradient is G_i = D_i^T X_i [out, in] and its bias gradient g_i = sum_p d_p, and with the Grams
// Gx = X_i X_i^T and Gd = D_i D_i^T [P, P]
//   ||G_i||_F^2 + ||g_i||^2 = sum_{p, p'} Gd[p, p'] (Gx[p, p'] + beta),   beta = 1 with a bias, else 0
// ("ghost clipping": the sum of all entries of Gd is ||sum_p d_p||^2, so the bias needs no pass of its
// own). That is P^2 (in + out) products against the P in out of forming G_i, the cheaper side while
// P < 2 in out / (in + out); it is taken for every P (the result is the same, a direct route is not built).
//   sum_i s_i G_i = D^T diag(s_{k / P}) X,   one GEMM with K = B T.
//
// Launches (a further set per 24 layers):
//   k_dp_seq_sqnorm  workgroup (microbatch, layer, pair of 64-position tiles I <= J): 4 waves, each a
//                    32 x 32 quarter of the pair's 64 x 64 block of both Grams as 2 x 2 tiles of
//                    v_mfma_f64_16x16x4_f64, Gx over K = in and then Gd over K = out, 8 accumulators of 4
//                    doubles in all. The 64 rows of tile I and of tile J (one copy when I = J) pass
//                    through LDS 64 columns at a time, row length 68 floats: lane (i, k) of a fragment
//                    reads word 68 i + k, bank 4 i + k, all 64 different, and a row starts 16-byte
//                    aligned for the staging stores. The fp32 operands widen exactly. Both Grams lie
//                    in the same lanes, so Gd (Gx + beta) is lane-local and neither is stored; an
//                    off-diagonal pair counts twice (an exact doubling). Rows >= P and columns >= the
//                    width are clamped loads turned into zeros, which add nothing. The workgroup reduces
//                    by wave shuffles, then LDS, into its own slot. No atomics: the same bytes on every run.
//   k_dp_scales      (dp_scales.h) one wave per row of slots.
//   k_dp_seq_sum     one wave = (split, 32 x 32 block of W^T [in, out] = X^T diag(s) D) on
//                    v_mfma_f32_32x32x2_f32, as k_dp_dense_sum: both operands K-major in memory as they
//                    lie, no LDS but for the scales (sk[k] = s[k / P], 1,024 k at a time), the loads of
//                    the next 16 k issued before the 8 MFMAs of the current 16. K = B T is cut into
//                    min(rows, 16) groups of consecutive microbatches (seq_splits: a function of `rows`
//                    alone, so the bytes do not depend on the device); every (split, block) stores its
//                    plain sums to partials[split][...], the blocks with m0 = 0 their bias sums too.
//   k_dp_clip_sum    (csrc/dpclip.hip, through efl_dp_clip_sum, clip_mode 0, rows = splits) adds the
//                    splits in order, noises and divides: efl_dp_noise's functions at the same stream
//                    positions as every other family.
// Rounding contract. Scales: S in double in a fixed order, rounded once to the float scale
// (k_dp_scales: S = 0 gives 1, an infinite S gives 0). Sum: s d rounded once, fp32 accumulation in a fixed
// order within a split, the splits added in order, then the noise add and the divide:
//   |got - exact| <= (B T + splits + 3) 2^-24 (sum |s d x| + |noise|) / |divisor|   per element.
#include <cstdint>
#include <vector>

#include "common.h"
#include "dp_scales.h"

#pragma clang fp contract(off)

namespace efl {
namespace {

typedef float acc16 __attribute__((ext_vector_type(16)));
typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kMaxLayers = 24;      // layers per launch: 24 x 88 B of the 4 KiB argument space
constexpr int kMaxR = 16;           // examples per microbatch
constexpr int kMaxP = 8192;         // rows (example, position) per microbatch
constexpr int kTP = 64;             // positions per tile of the Grams
constexpr int kKC = 64;             // columns of a tile in LDS at a time
constexpr int kLd = kKC + 4;        // LDS row length: word 68 i + k lies in bank 4 i + k
constexpr int kSplitCap = 16;       // most splits of the sum's reduction
constexpr int kKChunk = 1024;       // k whose scales are staged in LDS at a time
constexpr int kU = 8;               // MFMAs (k pairs) per register buffer

struct sq_chunk {
  efl_dp_seq v[kMaxLayers];
  uint32_t first[kMaxLayers + 1];   // layer i's first tile pair (= norm slot) among the chunk's
  uint32_t bfirst[kMaxLayers + 1];  // layer i's first 32x32 block in the GEMM grid
  long long poff[kMaxLayers];       // layer i's weight sums in a row of partials (the bias follows, 4-padded)
  uint32_t vecx, vecd;              // bit i: layer i's x / d rows take 16-byte loads
  int n;
};

__host__ __device__ inline long long pad4(long long n) { return (n + 3) & ~3ll; }

// Microbatches per split and the number of splits: a function of `rows` alone. At most kSplitCap
// splits, every one non-empty, the last one ragged.
inline void seq_splits(long long rows, long long* per, long long* splits) {
  const long long cap = rows < kSplitCap ? rows : kSplitCap;
  *per = (rows + cap - 1) / cap;
  *splits = (rows + *per - 1) / *per;
}

__device__ __forceinline__ int find_layer(const uint32_t* first, int n, uint32_t tile) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= tile) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Columns [k0, k0 + kKC) of the tile's 64 rows [p0, p0 + 64) of a microbatch (row p at base + p stride)
// into t[row * kLd + column]. Every load is clamped into the matrix; rows >= P and columns >= width
// become zeros.
__device__ __forceinline__ void stage_tile(const float* __restrict__ base, long long stride, int P, int p0, int width,
                                           int k0, bool vec, float* t) {
  for (int e = (int)threadIdx.x; e < kTP * (kKC / 4); e += kBlock) {
    const int rr = e / (kKC / 4), c = 4 * (e % (kKC / 4)), col = k0 + c;
    const bool pok = p0 + rr < P;
    const float* __restrict__ src = base + (long long)(pok ? p0 + rr : 0) * stride;
    f4 v;
    if (vec && col + 4 <= width) {
      v = *reinterpret_cast<const f4*>(src + col);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = col + j < width;
        const float u = src[ok ? col + j : 0];
        v[j] = ok ? u : 0.0f;
      }
    }
    if (!pok) v = f4{0.0f, 0.0f, 0.0f, 0.0f};
    *reinterpret_cast<f4*>(t + rr * kLd + c) = v;
  }
}

// acc[a][b] += rows [rs + 16 a, +16) of ti times rows [cs + 16 b, +16) of tj, over the chunk's first nk columns
__device__ __forceinline__ void gram_chunk(const float* ti, const float* tj, int rs, int cs, int nk, d4 (&acc)[2][2]) {
  const int lane = (int)threadIdx.x & 63, i16 = lane & 15, kk = lane >> 4;
  const float* a0 = ti + (rs + i16) * kLd + kk;
  const float* b0 = tj + (cs + i16) * kLd + kk;
  for (int k = 0; k < nk; k += 4) {
    const double A0 = (double)a0[k], A1 = (double)a0[16 * kLd + k];
    const double B0 = (double)b0[k], B1 = (double)b0[16 * kLd + k];
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(A0, B0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(A0, B1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(A1, B0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(A1, B1, acc[1][1], 0, 0, 0);
  }
}

// the 64 x 64 block (tile I, tile J) of M M^T, M the microbatch's rows of `width` columns: this wave's quarter
__device__ __forceinline__ void gram_block(const float* __restrict__ base, long long stride, int P, int I, int J,
                                           int width, bool vec, float* ti, float* tjbuf, d4 (&acc)[2][2]) {
  const int w = (int)threadIdx.x >> 6;
  const float* tj = I == J ? ti : tjbuf;
  for (int k0 = 0; k0 < width; k0 += kKC) {
    __syncthreads();                            // every thread is done with the chunk before
    stage_tile(base, stride, P, I * kTP, width, k0, vec, ti);
    if (I != J) stage_tile(base, stride, P, J * kTP, width, k0, vec, tjbuf);
    __syncthreads();
    const int left = width - k0, nk = left < kKC ? (left + 3) & ~3 : kKC;
    gram_chunk(ti, tj, 32 * (w >> 1), 32 * (w & 1), nk, acc);
  }
}

// Pass 1. Workgroup (microbatch, tile pair of a layer): sum over the pair's block of Gd (Gx + beta), in double.
__global__ __launch_bounds__(kBlock) void k_dp_seq_sqnorm(const sq_chunk c, int r, long long slot0, long long slots,
                                                          double* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) float ti[kTP * kLd];
  __shared__ __attribute__((aligned(16))) float tj[kTP * kLd];
  __shared__ double part[kBlock / 64];
  const uint32_t npair = c.first[c.n];
  const long long row = blockIdx.x / npair;
  const uint32_t blk = blockIdx.x - (uint32_t)row * npair;
  const int li = find_layer(c.first, c.n, blk), tid = (int)threadIdx.x;
  const efl_dp_seq& L = c.v[li];
  const int P = r * (int)L.T, nt = (P + kTP - 1) / kTP;
  int I = 0;                                    // pairs (I, J), I <= J, in row-major order
  uint32_t rem = blk - c.first[li];
  while (rem >= (uint32_t)(nt - I)) { rem -= (uint32_t)(nt - I); ++I; }
  const int J = I + (int)rem;
  d4 gx[2][2], gd[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) gx[a][b] = gd[a][b] = d4{0.0, 0.0, 0.0, 0.0};
  gram_block(L.x + row * P * L.x_row_stride, L.x_row_stride, P, I, J, (int)L.in, (c.vecx >> li) & 1, ti, tj, gx);
  gram_block(L.d + row * P * L.d_row_stride, L.d_row_stride, P, I, J, (int)L.out, (c.vecd >> li) & 1, ti, tj, gd);
  const double beta = L.b_out != nullptr ? 1.0 : 0.0;
  double v = 0.0;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int j = 0; j < 4; ++j) v += gd[a][b][j] * (gx[a][b][j] + beta);
  if (I != J) v = 2.0 * v;                      // the mirrored block of the symmetric Grams
  v = wave_sum(v);
  if ((tid & 63) == 0) part[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    double t = part[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) t += part[w];
    work[row * slots + slot0 + blk] = t;
  }
}

// Pass 2. One wave: a 32x32 block of W^T = X^T diag(s) D of one layer over one split's rows, stored plain.
template <bool CLIP>
__global__ __launch_bounds__(64) void k_dp_seq_sum(const sq_chunk c, long long rows, int r, long long per,
                                                   const float* __restrict__ scales, float* __restrict__ partials,
                                                   long long prow) {
  __shared__ float sk[CLIP ? kKChunk : 1];      // sk[k % kKChunk] = scales[k / P], k counted from the split's first row
  const int lane = (int)threadIdx.x, h = lane >> 5, l = lane & 31;
  const int li = find_layer(c.bfirst, c.n, blockIdx.x);
  const efl_dp_seq& L = c.v[li];
  const long long in = L.in, out = L.out, xs = L.x_row_stride, ds = L.d_row_stride, P = (long long)r * L.T;
  const uint32_t t = blockIdx.x - c.bfirst[li], tiles_m = (uint32_t)((in + 31) / 32);
  const uint32_t bn = t / tiles_m, bm = t - bn * tiles_m;
  const long long m = (long long)bm * 32 + l, n = (long long)bn * 32 + l;
  const bool mok = m < in, nok = n < out;
  const bool do_bias = bm == 0 && L.b_out != nullptr;
  const long long mb0 = (long long)blockIdx.y * per, mb1 = mb0 + per < rows ? mb0 + per : rows;
  const long long K = (mb1 - mb0) * P;          // this split's rows, from row mb0 P
  // clamped, so that every load is in bounds and unconditional; the edges become zeros at use
  const float* __restrict__ xp = L.x + mb0 * P * xs + (mok ? m : 0);
  const float* __restrict__ dp = L.d + mb0 * P * ds + (nok ? n : 0);
  const float* __restrict__ sc = scales + (CLIP ? mb0 : 0);

  float a0[kU], b0[kU], a1[kU], b1[kU];
  auto load = [&](long long kb, float (&a)[kU], float (&b)[kU]) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      long long k = kb + 2 * u + h;
      k = k < K ? k : K - 1;
      a[u] = xp[k * xs];
      b[u] = dp[k * ds];
    }
  };

  acc16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
  float bsum = 0.0f;

  load(0, a0, b0);
  for (long long kb = 0; kb < K; kb += 2 * kU) {
    const int ko = (int)(kb % kKChunk);
    if constexpr (CLIP) {
      if (ko == 0) {
        if (kb) __syncthreads();                // the wave is done with the chunk before
        const long long left = K - kb;
        const int nk = left < kKChunk ? (int)left : kKChunk;
        for (int i = lane; i < nk; i += 64) sk[i] = sc[(kb + i) / P];
        __syncthreads();
      }
    }
    const bool more = kb + 2 * kU < K;
    if (more) load(kb + 2 * kU, a1, b1);        // the next step's loads travel under the MFMAs
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const bool kok = kb + 2 * u + h < K;
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
  float* prt = partials + (long long)blockIdx.y * prow + c.poff[li];
  if (nok) {
    float* wrow = prt + n * in;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const long long mm = (long long)bm * 32 + 8 * g4 + 4 * h;
      if ((in & 3) == 0) {
        if (mm < in) *reinterpret_cast<f4*>(wrow + mm) = f4{acc[4 * g4], acc[4 * g4 + 1], acc[4 * g4 + 2], acc[4 * g4 + 3]};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (mm + j < in) wrow[mm + j] = acc[4 * g4 + j];
      }
    }
  }
  // bias: the two k chains (even and odd k) joined once
  if (do_bias) {                                // uniform over the wave
    const float tot = bsum + __shfl_xor(bsum, 32);
    if (h == 0 && nok) prt[pad4(out * in) + n] = tot;
  }
}

long long layer_pairs(const efl_dp_seq& L, long long r) {
  const long long nt = (r * L.T + kTP - 1) / kTP;
  return nt * (nt + 1) / 2;
}

long long layer_blocks(const efl_dp_seq& L) { return ((L.in + 31) / 32) * ((L.out + 31) / 32); }

// floats of one layer in a row of partials: the weight sums, then the bias sums, each 4-padded
long long layer_partials(const efl_dp_seq& L) { return pad4(L.in * L.out) + (L.b_out ? pad4(L.out) : 0); }

// The checks the entry points share, before any HIP call. On success *pairs is the number of tile pairs
// (= norm slots per microbatch) and *prow the floats in a row of partials.
int check_layers(const char* who, const efl_dp_seq* layers, int64_t nlayers, int64_t B, int64_t rows, long long* pairs,
                 long long* prow) {
  constexpr int64_t kMax = 0x7fffffff;
  *pairs = *prow = 0;
  if (nlayers < 0 || rows <= 0 || B <= 0 || B > kMax) { set_error("%s: nlayers must be >= 0, rows > 0 and 0 < B < 2^31", who); return EFL_E_INVALID_ARGUMENT; }
  if (B % rows != 0) { set_error("%s: rows (%lld) must divide B (%lld)", who, (long long)rows, (long long)B); return EFL_E_INVALID_ARGUMENT; }
  const int64_t r = B / rows;
  if (r > kMaxR) { set_error("%s: %lld examples per microbatch, at most %d", who, (long long)r, kMaxR); return EFL_E_INVALID_ARGUMENT; }
  if (nlayers == 0) return EFL_OK;
  if (!layers) { set_error("%s: null layer table", who); return EFL_E_INVALID_ARGUMENT; }
  long long blocks = 0;
  for (int64_t i = 0; i < nlayers; ++i) {
    const efl_dp_seq& L = layers[i];
    const long long li = (long long)i;
    if (L.T < 1 || L.in <= 0 || L.out <= 0 || L.in > kMax || L.out > kMax) { set_error("%s: layer %lld: T must be >= 1, in and out in 1 .. 2^31 - 1", who, li); return EFL_E_INVALID_ARGUMENT; }
    if (L.T > kMaxP || r * L.T > kMaxP) { set_error("%s: layer %lld: %lld examples of %lld positions per microbatch, at most %d rows", who, li, (long long)r, (long long)L.T, kMaxP); return EFL_E_INVALID_ARGUMENT; }
    if (!L.x || !L.d || !L.w_out) { set_error("%s: layer %lld: null buffer", who, li); return EFL_E_INVALID_ARGUMENT; }
    if (!aligned(L.x, 4) || !aligned(L.d, 4) || !aligned(L.w_out, 16) || !aligned(L.b_out, 16)) {
      set_error("%s: layer %lld: x and d must be 4-byte, w_out and b_out 16-byte aligned", who, li);
      return EFL_E_INVALID_ARGUMENT;
    }
    if (L.x_row_stride < L.in || L.d_row_stride < L.out) {
      set_error("%s: layer %lld: a row stride (%lld, %lld) below its width (%lld, %lld)", who, li, (long long)L.x_row_stride,
                (long long)L.d_row_stride, (long long)L.in, (long long)L.out);
      return EFL_E_INVALID_ARGUMENT;
    }
    *pairs += layer_pairs(L, r);
    *prow += layer_partials(L);
    blocks += layer_blocks(L);
    if (*pairs > kMax / rows || blocks > kMax || *prow > INT64_MAX / 64) { set_error("%s: layers too large for one grid", who); return EFL_E_INVALID_ARGUMENT; }
  }
  return EFL_OK;
}

// fn(chunk, tile pairs before it) for every run of at most kMaxLayers layers
template <class F>
void for_chunks(const efl_dp_seq* layers, int64_t nlayers, long long r, F fn) {
  long long before = 0, poff = 0;
  for (int64_t i0 = 0; i0 < nlayers; i0 += kMaxLayers) {
    sq_chunk c;
    long long pairs = 0, blocks = 0;
    c.n = (int)(nlayers - i0 < kMaxLayers ? nlayers - i0 : kMaxLayers);
    c.vecx = c.vecd = 0;
    for (int i = 0; i < c.n; ++i) {
      const efl_dp_seq& L = layers[i0 + i];
      c.v[i] = L;
      c.first[i] = (uint32_t)pairs;
      c.bfirst[i] = (uint32_t)blocks;
      c.poff[i] = poff;
      if (aligned(L.x, 16) && L.x_row_stride % 4 == 0) c.vecx |= 1u << i;
      if (aligned(L.d, 16) && L.d_row_stride % 4 == 0) c.vecd |= 1u << i;
      pairs += layer_pairs(L, r);
      blocks += layer_blocks(L);
      poff += layer_partials(L);
    }
    c.first[c.n] = (uint32_t)pairs;
    c.bfirst[c.n] = (uint32_t)blocks;
    fn(c, before);
    before += pairs;
  }
}

void launch_sqnorm(const efl_dp_seq* layers, int64_t nlayers, int64_t rows, int r, double* work, long long slot0,
                   long long slots, hipStream_t s) {
  for_chunks(layers, nlayers, r, [&](const sq_chunk& c, long long before) {
    k_dp_seq_sqnorm<<<(unsigned)(rows * c.first[c.n]), kBlock, 0, s>>>(c, r, slot0 + before, slots, work);
  });
}

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API int64_t efl_dp_seq_work_elems(const efl_dp_seq* layers, int64_t nlayers, int64_t B, int64_t rows) {
  long long pairs, prow;
  const int rc = check_layers("efl_dp_seq_work_elems", layers, nlayers, B, rows, &pairs, &prow);
  return rc != EFL_OK ? rc : rows * pairs;
}

EFL_API int64_t efl_dp_seq_partial_elems(const efl_dp_seq* layers, int64_t nlayers, int64_t B, int64_t rows) {
  long long pairs, prow, per, splits;
  const int rc = check_layers("efl_dp_seq_partial_elems", layers, nlayers, B, rows, &pairs, &prow);
  if (rc != EFL_OK) return rc;
  seq_splits(rows, &per, &splits);
  return splits * prow;
}

EFL_API int efl_dp_seq_sqnorm(const efl_dp_seq* layers, int64_t nlayers, int64_t B, int64_t rows, double* work,
                              int64_t slot0, int64_t slots, void* stream) {
  long long pairs, prow;
  const int rc = check_layers("efl_dp_seq_sqnorm", layers, nlayers, B, rows, &pairs, &prow);
  if (rc != EFL_OK) return rc;
  if (nlayers == 0) return EFL_OK;
  if (!work || !aligned(work, 8) || slot0 < 0 || slots > INT64_MAX / 16 / rows || slot0 > slots - pairs) {
    set_error("efl_dp_seq_sqnorm: work must hold rows x slots doubles with the layers' %lld slots in [slot0, slots)", pairs);
    return EFL_E_INVALID_ARGUMENT;
  }
  launch_sqnorm(layers, nlayers, rows, (int)(B / rows), work, slot0, slots, (hipStream_t)stream);
  return hip_status(hipGetLastError(), "efl_dp_seq_sqnorm");
}

EFL_API int efl_dp_seq_clip_sum(const efl_dp_seq* layers, int64_t nlayers, int64_t B, int64_t rows, int clip_mode,
                                float l2_norm_clip, int mode, float sigma, float divisor, uint64_t seed, float* scales,
                                double* work, int64_t work_elems, float* partials, int64_t partial_elems, void* stream) {
  const char* who = "efl_dp_seq_clip_sum";
  if (clip_mode < 0 || clip_mode > 2) { set_error("%s: clip_mode must be 0 (none), 1 (from the norms) or 2 (given scales)", who); return EFL_E_INVALID_ARGUMENT; }
  if (mode < 0 || mode > 1) { set_error("%s: mode must be 0 (element-wise) or 1 (Gaussian sum)", who); return EFL_E_INVALID_ARGUMENT; }
  if (!(divisor == divisor) || divisor == 0.0f) { set_error("%s: divisor must be non-zero", who); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode == 1 && !(l2_norm_clip > 0.0f)) { set_error("%s: l2_norm_clip must be positive", who); return EFL_E_INVALID_ARGUMENT; }
  long long pairs, prow, per, splits;
  const int rc = check_layers(who, layers, nlayers, B, rows, &pairs, &prow);
  if (rc != EFL_OK) return rc;
  if (nlayers == 0) return EFL_OK;
  if (clip_mode != 0 && (!scales || !aligned(scales, 4))) { set_error("%s: clip modes 1 and 2 need a scales buffer", who); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode == 1 && (!work || !aligned(work, 8) || work_elems < rows * pairs)) {
    set_error("%s: work must hold efl_dp_seq_work_elems() = %lld doubles, got %lld", who, (long long)(rows * pairs), (long long)work_elems);
    return EFL_E_INVALID_ARGUMENT;
  }
  seq_splits(rows, &per, &splits);
  if (!partials || !aligned(partials, 16) || partial_elems < splits * prow) {
    set_error("%s: partials must hold efl_dp_seq_partial_elems() = %lld floats, 16-byte aligned, got %lld", who, (long long)(splits * prow), (long long)partial_elems);
    return EFL_E_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  const int r = (int)(B / rows);
  if (clip_mode == 1) {
    launch_sqnorm(layers, nlayers, rows, r, work, 0, pairs, s);
    k_dp_scales<<<(unsigned)rows, 64, 0, s>>>(work, pairs, (double)l2_norm_clip, scales);
  }
  std::vector<efl_dp_var> vars;
  for_chunks(layers, nlayers, r, [&](const sq_chunk& c, long long) {
    const dim3 grid(c.bfirst[c.n], (unsigned)splits);
    if (clip_mode == 0) k_dp_seq_sum<false><<<grid, 64, 0, s>>>(c, rows, r, per, scales, partials, prow);
    else k_dp_seq_sum<true><<<grid, 64, 0, s>>>(c, rows, r, per, scales, partials, prow);
    for (int i = 0; i < c.n; ++i) {
      const efl_dp_seq& L = c.v[i];
      vars.push_back(efl_dp_var{partials + c.poff[i], L.w_out, L.in * L.out, prow, L.ctr0_w});
      if (L.b_out) vars.push_back(efl_dp_var{partials + c.poff[i] + pad4(L.in * L.out), L.b_out, L.out, prow, L.ctr0_b});
    }
  });
  const int e = hip_status(hipGetLastError(), who);
  if (e != EFL_OK) return e;
  // the splits in order, the noise and the divide: one launch over every variable
  return efl_dp_clip_sum(vars.data(), (int64_t)vars.size(), splits, 0, 0.0f, mode, sigma, divisor, seed, nullptr, nullptr,
                         0, stream);
}
