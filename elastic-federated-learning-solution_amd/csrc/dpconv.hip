// DP-SGD for Conv2d layers without the per-microbatch gradient stack: the clip norms
// and the clipped, noised sum of a convolution's weight and bias gradients straight from the layer's
// input x [B, Cin, H, W] and the gradient d [B, Cout, Ho, Wo] of the summed loss by its output.
//
// Reference: efls-train/python/efl/privacy/dp_optimizer.py compute_gradients (:148-216); the model of
// example/dp_mnist/dp_cnn.py is two convolutions and two dense layers. groups = 1, zero padding.
// With T = Ho Wo, K = Cin kh kw, q = (c kh + i) kw + j and the im2col row
//   U[b][t][q] = x[b][c][oy sh - ph + i dh][ox sw - pw + j dw]   (0 outside the image),
// microbatch m (the r = B / rows consecutive examples from m r) has the weight gradient
//   G_m [Cout, K] = sum_{a in m} sum_t d[a][.][t] (x) U[a][t][.]   and   g_m[o] = sum_{a, t} d[a][o][t],
// and sum_m s_m G_m is one implicit GEMM whose reduction runs over all B T (example, position) pairs.
// Cout K is small and T large, so a T x T Gram costs more than G_m itself: the norm pass forms G_m in
// registers, squares it and drops it. Nothing of size rows x Cout x K reaches memory.
//
// Both kernels cut the [K, Cout] plane into 32 x 32 blocks and walk an example's output positions
// in rectangles of R rows x C columns (R C <= 128, chosen on the host from the shapes alone so that
// the input window of a rectangle fits: conv_geometry). Per (example, rectangle) a workgroup stages
//   xw  the input window [channels the block's q touch][(R-1) sh + (kh-1) dh + 1][(C-1) sw + (kw-1) dw + 1],
//       rows read along W, positions outside the image stored as zeros (so the gather has no branch),
//   dt  the block's 32 rows of d [o][ry C + cx], row length 129 (bank o + t), read along Wo, already
//       multiplied by the example's clip scale in the sum pass (the one fp32 rounding of s d),
// and a lane gathers its im2col operand as xw[qoff(lane's q) + toff[t]], two LDS tables of offsets.
// No rectangle is assumed to cover an image: any H and W work.
//
// Launches (a further set per 24 layers):
//   k_dp_conv_sqnorm  workgroup (microbatch, block): 4 waves, each a 16 x 16 quarter of the block on
//                     v_mfma_f64_16x16x4_f64 (the fp32 operands widen exactly, the accumulator is
//                     double), over the microbatch's r examples; then sum of squares, wave shuffles,
//                     LDS, one slot per workgroup. The blocks with q = 0 add ||g_m||^2 of their 32
//                     channels from the same dt. No atomics: the same bytes on every run.
//   k_dp_conv_sum     one wave = (split, block) on v_mfma_f32_32x32x2_f32, M = q, N = Cout: the lane
//                     ends with four consecutive q of one o, one 16-byte store. The reduction is
//                     split over contiguous groups of microbatches (conv_splits: a function of `rows`
//                     alone); every (split, block) stores its plain sums to partials[split][...].
//   k_dp_clip_sum     (csrc/dpclip.hip, through efl_dp_clip_sum, clip_mode 0, rows = splits) adds the
//                     splits in order, noises and divides: efl_dp_noise's functions, any K.
#include <cstdint>
#include <vector>

#include "common.h"
#include "dp_scales.h"

#pragma clang fp contract(off)

namespace efl {
namespace {

typedef float acc16 __attribute__((ext_vector_type(16)));
typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kMaxLayers = 24;      // layers per launch: 24 x 128 B of the 4 KiB argument space
constexpr int kMaxR = 16;           // examples per microbatch
constexpr int kTile = 32;           // block edge in q and in o
constexpr int kTC = 128;            // output positions per rectangle
constexpr int kLd = kTC + 1;        // dt row length
constexpr int kXW = 8192;           // floats of input window in LDS
constexpr int kSplitCap = 16;       // most splits of the reduction

struct cv_geom { int R, C, WR, WC; };   // rectangle of output positions and its input window

struct cv_chunk {
  efl_dp_conv v[kMaxLayers];
  cv_geom g[kMaxLayers];
  uint32_t first[kMaxLayers + 1];   // layer i's first 32x32 block among the chunk's
  long long poff[kMaxLayers];       // layer i's weight sums in a row of partials (the bias follows, 4-padded)
  int n;
};

__host__ __device__ inline long long pad4(long long n) { return (n + 3) & ~3ll; }

// Microbatches per split and the number of splits: a function of `rows` alone, so that the bytes do
// not depend on the device. At most kSplitCap splits, every one non-empty, the last one ragged.
inline void conv_splits(long long rows, long long* per, long long* splits) {
  const long long cap = rows < kSplitCap ? rows : kSplitCap;
  *per = (rows + cap - 1) / cap;
  *splits = (rows + *per - 1) / *per;
}

// The rectangle of output positions a workgroup stages at a time: as wide as the output row allows
// (at most kTC), then as many rows as keep R C <= kTC and the input window of the most channels a
// block's 32 q can touch within kXW floats. False when one output position's window does not fit.
bool conv_geometry(const efl_dp_conv& L, cv_geom* g) {
  const double eh = ((double)L.kh - 1) * L.dh + 1, ew = ((double)L.kw - 1) * L.dw + 1;
  const long long khkw = (long long)L.kh * L.kw;
  const long long span = (kTile - 1) / khkw + 2;
  const double nch = (double)(L.cin < span ? L.cin : span);
  auto fits = [&](int R, int C) { return nch * ((R - 1.0) * L.sh + eh) * ((C - 1.0) * L.sw + ew) <= kXW; };
  int C = L.wo < kTC ? L.wo : kTC;
  while (C > 1 && !fits(1, C)) C = (C + 1) / 2;
  if (!fits(1, C)) return false;
  int R = kTC / C < L.ho ? kTC / C : L.ho;
  while (R > 1 && !fits(R, C)) --R;
  g->R = R;
  g->C = C;
  g->WR = (R - 1) * L.sh + (L.kh - 1) * L.dh + 1;
  g->WC = (C - 1) * L.sw + (L.kw - 1) * L.dw + 1;
  return true;
}

__device__ __forceinline__ int find_layer(const cv_chunk& c, uint32_t tile) {
  int lo = 0, hi = c.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (c.first[mid] <= tile) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int log2_ceil(int n) {   // smallest l with 2^l >= n, at most 6
  int l = 0;
  while (l < 6 && (1 << l) < n) ++l;
  return l;
}

// One workgroup's view of its 32x32 block of one layer, and the LDS it stages into.
struct cv_block {
  int H, W, Cout, Ho, Wo, sh, sw, ph, pw;
  int R, C, WR, WC, lw, lc, nt, nt4;   // nt = R C positions per rectangle, nt4 = nt rounded up to 4
  int q0, o0, c0, nch, no;             // first q and o; channels [c0, c0 + nch); no = valid o in the block
  long long K, xs, ds;                 // floats per example of x and of d
};

__device__ __forceinline__ cv_block make_block(const efl_dp_conv& L, const cv_geom& g, uint32_t t) {
  cv_block b;
  b.H = L.h; b.W = L.w; b.Cout = L.cout; b.Ho = L.ho; b.Wo = L.wo;
  b.sh = L.sh; b.sw = L.sw; b.ph = L.ph; b.pw = L.pw;
  b.R = g.R; b.C = g.C; b.WR = g.WR; b.WC = g.WC;
  b.lw = log2_ceil(g.WC);
  b.lc = log2_ceil(g.C);
  b.nt = g.R * g.C;
  b.nt4 = (b.nt + 3) & ~3;
  const int khkw = L.kh * L.kw;
  b.K = (long long)L.cin * khkw;
  const uint32_t tiles_q = (uint32_t)((b.K + kTile - 1) / kTile);
  const uint32_t bo = t / tiles_q, bq = t - bo * tiles_q;
  b.q0 = (int)bq * kTile;
  b.o0 = (int)bo * kTile;
  const long long qlast = b.q0 + kTile - 1 < b.K - 1 ? b.q0 + kTile - 1 : b.K - 1;
  b.c0 = b.q0 / khkw;
  b.nch = (int)(qlast / khkw) - b.c0 + 1;
  b.no = L.cout - b.o0 < kTile ? L.cout - b.o0 : kTile;
  b.xs = (long long)L.cin * L.h * L.w;
  b.ds = (long long)L.cout * L.ho * L.wo;
  return b;
}

// a lane's q as an offset into xw: (c - c0) WR WC + i dh WC + j dw; 0 and *ok = false past K
__device__ __forceinline__ int q_offset(const efl_dp_conv& L, const cv_block& b, int q, bool* ok) {
  *ok = q < b.K;
  if (!*ok) return 0;
  const int khkw = L.kh * L.kw, c = q / khkw, rem = q - c * khkw, i = rem / L.kw, j = rem - i * L.kw;
  return ((c - b.c0) * b.WR + i * L.dh) * b.WC + j * L.dw;
}

// toff[t] = ry sh WC + cx sw for position t = ry C + cx of a rectangle (0 for the padding up to nt4),
// and zeros in dt's padding columns [nt, nt4) of all 32 rows: both hold for every rectangle
template <int NTH>
__device__ __forceinline__ void stage_tables(const cv_block& b, int* toff, float* dt) {
  const int tid = (int)threadIdx.x;
  for (int t = tid; t < b.nt4; t += NTH) {
    const int ry = t / b.C, cx = t - ry * b.C;
    toff[t] = t < b.nt ? ry * b.sh * b.WC + cx * b.sw : 0;
  }
  const int pad = b.nt4 - b.nt;
  for (int e = tid; e < kTile * pad; e += NTH) dt[(e / pad) * kLd + b.nt + e % pad] = 0.0f;
}

// the input window of the rectangle at (oy0, ox0) of one example: xb = its channel c0. Every load is
// clamped into the image and unconditional; what lies outside becomes a zero.
template <int NTH>
__device__ __forceinline__ void stage_x(const cv_block& b, const float* __restrict__ xb, int oy0, int ox0, float* xw) {
  const int tid = (int)threadIdx.x, step = 1 << b.lw;
  const int sub = tid >> b.lw, wx0 = tid & (step - 1), rpi = NTH >> b.lw, nrows = b.nch * b.WR;
  const int iy0 = oy0 * b.sh - b.ph, ix0 = ox0 * b.sw - b.pw;
  for (int rw = sub; rw < nrows; rw += rpi) {
    const int c = rw / b.WR, iy = iy0 + (rw - c * b.WR);
    const bool yok = iy >= 0 && iy < b.H;
    const float* __restrict__ src = xb + ((long long)c * b.H + (yok ? iy : 0)) * b.W;
    for (int wx = wx0; wx < b.WC; wx += step) {
      const int ix = ix0 + wx;
      const bool ok = yok && ix >= 0 && ix < b.W;
      const float v = src[ok ? ix : 0];
      xw[rw * b.WC + wx] = ok ? v : 0.0f;
    }
  }
}

// the block's rows of d over the same rectangle, times s (SCALE): db = the example's channel o0
template <int NTH, bool SCALE>
__device__ __forceinline__ void stage_d(const cv_block& b, const float* __restrict__ db, int oy0, int ox0, float s,
                                        float* dt) {
  const int tid = (int)threadIdx.x, step = 1 << b.lc;
  const int sub = tid >> b.lc, cx0 = tid & (step - 1), rpi = NTH >> b.lc, nrows = kTile * b.R;
  for (int rd = sub; rd < nrows; rd += rpi) {
    const int ol = rd / b.R, ry = rd - ol * b.R, oy = oy0 + ry;
    const bool rok = ol < b.no && oy < b.Ho;
    const float* __restrict__ src = db + ((long long)(rok ? ol : 0) * b.Ho + (rok ? oy : 0)) * b.Wo;
    for (int cx = cx0; cx < b.C; cx += step) {
      const bool ok = rok && ox0 + cx < b.Wo;
      float v = src[ok ? ox0 + cx : 0];
      v = ok ? v : 0.0f;
      dt[ol * kLd + ry * b.C + cx] = SCALE ? v * s : v;
    }
  }
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
  return t;
}

// Pass 1. Workgroup (microbatch, block): the sum of squares of a 32x32 block of G_m (+ of 32 channels
// of g_m in the blocks with q = 0), in double.
__global__ __launch_bounds__(kBlock) void k_dp_conv_sqnorm(const cv_chunk c, int r, long long slot0, long long slots,
                                                           double* __restrict__ work) {
  __shared__ float xw[kXW];
  __shared__ float dt[kTile * kLd];
  __shared__ int toff[kTC];
  __shared__ double part[kBlock / 64];
  const uint32_t nblk = c.first[c.n];
  const long long row = blockIdx.x / nblk;
  const uint32_t blk = blockIdx.x - (uint32_t)row * nblk;
  const int li = find_layer(c, blk), tid = (int)threadIdx.x;
  const efl_dp_conv& L = c.v[li];
  const cv_block b = make_block(L, c.g[li], blk - c.first[li]);
  const int w = tid >> 6, lane = tid & 63, i16 = lane & 15, kk = lane >> 4;
  const int qsub = b.q0 + 16 * (w & 1), osub = 16 * (w >> 1);
  const bool live = qsub < b.K && osub < b.no;   // this wave's quarter holds something
  bool qok;
  const int qoff = q_offset(L, b, qsub + i16, &qok);
  const float* drow = dt + (osub + i16) * kLd;
  const bool bias = b.q0 == 0 && L.b_out != nullptr;
  const float* brow = dt + (tid >> 3) * kLd;    // the bias: 8 threads share one o
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  double bs = 0.0;
  stage_tables<kBlock>(b, toff, dt);
  for (int a = 0; a < r; ++a) {
    const long long ex = row * r + a;
    const float* __restrict__ xb = L.x + ex * b.xs + (long long)b.c0 * b.H * b.W;
    const float* __restrict__ db = L.d + ex * b.ds + (long long)b.o0 * b.Ho * b.Wo;
    for (int oy0 = 0; oy0 < b.Ho; oy0 += b.R)
      for (int ox0 = 0; ox0 < b.Wo; ox0 += b.C) {
        __syncthreads();                        // every thread is done with the rectangle before
        stage_x<kBlock>(b, xb, oy0, ox0, xw);
        stage_d<kBlock, false>(b, db, oy0, ox0, 1.0f, dt);
        __syncthreads();
        if (live)
          for (int k = kk; k < b.nt4; k += 4) {
            const float u = xw[qoff + toff[k]];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(qok ? (double)u : 0.0, (double)drow[k], acc, 0, 0, 0);
          }
        if (bias)
          for (int k = tid & 7; k < b.nt; k += 8) bs += (double)brow[k];
      }
  }
  double v = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) v += acc[j] * acc[j];
  if (bias) {                                   // uniform over the workgroup
    bs += __shfl_xor(bs, 1);
    bs += __shfl_xor(bs, 2);
    bs += __shfl_xor(bs, 4);
    if ((tid & 7) == 0) v += bs * bs;
  }
  v = block_sum(v, part);
  if (tid == 0) work[row * slots + slot0 + blk] = v;
}

// Pass 2. One wave: a 32x32 block of sum_{b, t} s d (x) U over one split's microbatches, stored plain.
template <bool CLIP>
__global__ __launch_bounds__(64) void k_dp_conv_sum(const cv_chunk c, long long rows, int r, long long per,
                                                    const float* __restrict__ scales, float* __restrict__ partials,
                                                    long long prow) {
  __shared__ float xw[kXW];
  __shared__ float dt[kTile * kLd];
  __shared__ int toff[kTC];
  const int lane = (int)threadIdx.x, h = lane >> 5, l = lane & 31;
  const int li = find_layer(c, blockIdx.x);
  const efl_dp_conv& L = c.v[li];
  const cv_block b = make_block(L, c.g[li], blockIdx.x - c.first[li]);
  bool qok;
  const int qoff = q_offset(L, b, b.q0 + l, &qok);
  const float* drow = dt + l * kLd;
  const bool do_bias = b.q0 == 0 && L.b_out != nullptr;
  const long long m0 = (long long)blockIdx.y * per, m1 = m0 + per < rows ? m0 + per : rows;
  acc16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
  float bsum = 0.0f;
  stage_tables<64>(b, toff, dt);
  for (long long m = m0; m < m1; ++m) {
    const float s = CLIP ? scales[m] : 1.0f;
    for (int a = 0; a < r; ++a) {
      const long long ex = m * r + a;
      const float* __restrict__ xb = L.x + ex * b.xs + (long long)b.c0 * b.H * b.W;
      const float* __restrict__ db = L.d + ex * b.ds + (long long)b.o0 * b.Ho * b.Wo;
      for (int oy0 = 0; oy0 < b.Ho; oy0 += b.R)
        for (int ox0 = 0; ox0 < b.Wo; ox0 += b.C) {
          __syncthreads();                      // the wave is done with the rectangle before
          stage_x<64>(b, xb, oy0, ox0, xw);
          stage_d<64, CLIP>(b, db, oy0, ox0, s, dt);
          __syncthreads();
          for (int k = h; k < b.nt4; k += 2) {
            const float u = xw[qoff + toff[k]];
            const float dv = drow[k];
            if (do_bias) bsum = bsum + dv;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qok ? u : 0.0f, dv, acc, 0, 0, 0);
          }
        }
    }
  }
  // weights: register 4 g + j of lane (h, l) is the sum at q = q0 + 8 g + 4 h + j, o = o0 + l
  float* prt = partials + (long long)blockIdx.y * prow + c.poff[li];
  const bool ook = l < b.no;
  if (ook) {
    float* wrow = prt + (long long)(b.o0 + l) * b.K;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const long long qq = b.q0 + 8 * g4 + 4 * h;
      if ((b.K & 3) == 0) {
        if (qq < b.K) *reinterpret_cast<f4*>(wrow + qq) = f4{acc[4 * g4], acc[4 * g4 + 1], acc[4 * g4 + 2], acc[4 * g4 + 3]};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (qq + j < b.K) wrow[qq + j] = acc[4 * g4 + j];
      }
    }
  }
  // bias: the two k chains (even and odd positions) joined once
  if (do_bias) {                                // uniform over the wave
    const float tot = bsum + __shfl_xor(bsum, 32);
    if (h == 0 && ook) prt[pad4((long long)L.cout * b.K) + b.o0 + l] = tot;
  }
}

long long layer_blocks(const efl_dp_conv& L) {
  const long long K = (long long)L.cin * L.kh * L.kw;
  return ((K + kTile - 1) / kTile) * (((long long)L.cout + kTile - 1) / kTile);
}

// floats of one layer in a row of partials: the weight sums, then the bias sums, each 4-padded
long long layer_partials(const efl_dp_conv& L) {
  return pad4((long long)L.cout * L.cin * L.kh * L.kw) + (L.b_out ? pad4(L.cout) : 0);
}

// The checks the entry points share, before any HIP call. On success *blocks is the number of 32x32
// blocks (= norm slots per microbatch) and *prow the floats in a row of partials.
int check_layers(const char* who, const efl_dp_conv* layers, int64_t nlayers, int64_t B, int64_t rows,
                 long long* blocks, long long* prow) {
  constexpr int64_t kMax = 0x7fffffff;
  *blocks = *prow = 0;
  if (nlayers < 0 || rows <= 0 || B <= 0 || B > kMax) { set_error("%s: nlayers must be >= 0, rows > 0 and 0 < B < 2^31", who); return EFL_E_INVALID_ARGUMENT; }
  if (B % rows != 0) { set_error("%s: rows (%lld) must divide B (%lld)", who, (long long)rows, (long long)B); return EFL_E_INVALID_ARGUMENT; }
  if (B / rows > kMaxR) { set_error("%s: %lld examples per microbatch, at most %d", who, (long long)(B / rows), kMaxR); return EFL_E_INVALID_ARGUMENT; }
  if (nlayers == 0) return EFL_OK;
  if (!layers) { set_error("%s: null layer table", who); return EFL_E_INVALID_ARGUMENT; }
  for (int64_t i = 0; i < nlayers; ++i) {
    const efl_dp_conv& L = layers[i];
    const long long li = (long long)i;
    if (L.cin <= 0 || L.h <= 0 || L.w <= 0 || L.cout <= 0 || L.ho <= 0 || L.wo <= 0 || L.kh <= 0 || L.kw <= 0 ||
        L.sh <= 0 || L.sw <= 0 || L.dh <= 0 || L.dw <= 0 || L.ph < 0 || L.pw < 0) {
      set_error("%s: layer %lld: sizes, strides and dilations must be positive and paddings >= 0", who, li);
      return EFL_E_INVALID_ARGUMENT;
    }
    const long long eh = ((long long)L.kh - 1) * L.dh + 1, ew = ((long long)L.kw - 1) * L.dw + 1;
    const long long nh = (long long)L.h + 2ll * L.ph - eh, nw = (long long)L.w + 2ll * L.pw - ew;
    if (nh < 0 || nw < 0 || nh / L.sh + 1 != L.ho || nw / L.sw + 1 != L.wo) {
      set_error("%s: layer %lld: ho x wo = %d x %d is not the output of a %d x %d input under its kernel, stride, padding and dilation", who, li, L.ho, L.wo, L.h, L.w);
      return EFL_E_INVALID_ARGUMENT;
    }
    const long long K = (long long)L.cin * L.kh * L.kw;
    if ((long long)L.h + 2ll * L.ph > kMax || (long long)L.w + 2ll * L.pw > kMax || K > kMax || K * L.cout > kMax || (long long)L.cin * L.h * L.w > kMax || (long long)L.cout * L.ho * L.wo > kMax) {
      set_error("%s: layer %lld: a weight or an example of 2^31 floats or more", who, li);
      return EFL_E_INVALID_ARGUMENT;
    }
    if (!L.x || !L.d || !L.w_out) { set_error("%s: layer %lld: null buffer", who, li); return EFL_E_INVALID_ARGUMENT; }
    if (!aligned(L.x, 4) || !aligned(L.d, 4) || !aligned(L.w_out, 16) || !aligned(L.b_out, 16)) {
      set_error("%s: layer %lld: x and d must be 4-byte, w_out and b_out 16-byte aligned", who, li);
      return EFL_E_INVALID_ARGUMENT;
    }
    cv_geom g;
    if (!conv_geometry(L, &g)) {
      set_error("%s: layer %lld: the input window of one output position (%lld x %lld over the channels of 32 weights) exceeds %d floats", who, li, eh, ew, kXW);
      return EFL_E_INVALID_ARGUMENT;
    }
    *blocks += layer_blocks(L);
    *prow += layer_partials(L);
    if (*blocks > kMax / rows || *prow > INT64_MAX / 64) { set_error("%s: layers too large for one grid", who); return EFL_E_INVALID_ARGUMENT; }
  }
  return EFL_OK;
}

// fn(chunk, blocks before it) for every run of at most kMaxLayers layers
template <class F>
void for_chunks(const efl_dp_conv* layers, int64_t nlayers, F fn) {
  long long before = 0, poff = 0;
  for (int64_t i0 = 0; i0 < nlayers; i0 += kMaxLayers) {
    cv_chunk c;
    long long total = 0;
    c.n = (int)(nlayers - i0 < kMaxLayers ? nlayers - i0 : kMaxLayers);
    for (int i = 0; i < c.n; ++i) {
      const efl_dp_conv& L = layers[i0 + i];
      c.v[i] = L;
      conv_geometry(L, &c.g[i]);
      c.first[i] = (uint32_t)total;
      c.poff[i] = poff;
      total += layer_blocks(L);
      poff += layer_partials(L);
    }
    c.first[c.n] = (uint32_t)total;
    fn(c, before);
    before += total;
  }
}

void launch_sqnorm(const efl_dp_conv* layers, int64_t nlayers, int64_t rows, int r, double* work, long long slot0,
                   long long slots, hipStream_t s) {
  for_chunks(layers, nlayers, [&](const cv_chunk& c, long long before) {
    k_dp_conv_sqnorm<<<(unsigned)(rows * c.first[c.n]), kBlock, 0, s>>>(c, r, slot0 + before, slots, work);
  });
}

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API int64_t efl_dp_conv_work_elems(const efl_dp_conv* layers, int64_t nlayers, int64_t rows) {
  long long blocks, prow;
  const int rc = check_layers("efl_dp_conv_work_elems", layers, nlayers, rows > 0 ? rows : 1, rows, &blocks, &prow);
  return rc != EFL_OK ? rc : rows * blocks;
}

EFL_API int64_t efl_dp_conv_partial_elems(const efl_dp_conv* layers, int64_t nlayers, int64_t B, int64_t rows) {
  long long blocks, prow, per, splits;
  const int rc = check_layers("efl_dp_conv_partial_elems", layers, nlayers, B, rows, &blocks, &prow);
  if (rc != EFL_OK) return rc;
  conv_splits(rows, &per, &splits);
  return splits * prow;
}

EFL_API int efl_dp_conv_sqnorm(const efl_dp_conv* layers, int64_t nlayers, int64_t B, int64_t rows, double* work,
                               int64_t slot0, int64_t slots, void* stream) {
  long long blocks, prow;
  const int rc = check_layers("efl_dp_conv_sqnorm", layers, nlayers, B, rows, &blocks, &prow);
  if (rc != EFL_OK) return rc;
  if (nlayers == 0) return EFL_OK;
  if (!work || !aligned(work, 8) || slot0 < 0 || slots > INT64_MAX / 16 / rows || slot0 > slots - blocks) {
    set_error("efl_dp_conv_sqnorm: work must hold rows x slots doubles with the layers' %lld slots in [slot0, slots)", blocks);
    return EFL_E_INVALID_ARGUMENT;
  }
  launch_sqnorm(layers, nlayers, rows, (int)(B / rows), work, slot0, slots, (hipStream_t)stream);
  return hip_status(hipGetLastError(), "efl_dp_conv_sqnorm");
}

EFL_API int efl_dp_conv_clip_sum(const efl_dp_conv* layers, int64_t nlayers, int64_t B, int64_t rows, int clip_mode,
                                 float l2_norm_clip, int mode, float sigma, float divisor, uint64_t seed, float* scales,
                                 double* work, int64_t work_elems, float* partials, int64_t partial_elems,
                                 void* stream) {
  const char* who = "efl_dp_conv_clip_sum";
  if (clip_mode < 0 || clip_mode > 2) { set_error("%s: clip_mode must be 0 (none), 1 (from the norms) or 2 (given scales)", who); return EFL_E_INVALID_ARGUMENT; }
  if (mode < 0 || mode > 1) { set_error("%s: mode must be 0 (element-wise) or 1 (Gaussian sum)", who); return EFL_E_INVALID_ARGUMENT; }
  if (!(divisor == divisor) || divisor == 0.0f) { set_error("%s: divisor must be non-zero", who); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode == 1 && !(l2_norm_clip > 0.0f)) { set_error("%s: l2_norm_clip must be positive", who); return EFL_E_INVALID_ARGUMENT; }
  long long blocks, prow, per, splits;
  const int rc = check_layers(who, layers, nlayers, B, rows, &blocks, &prow);
  if (rc != EFL_OK) return rc;
  if (nlayers == 0) return EFL_OK;
  if (clip_mode != 0 && (!scales || !aligned(scales, 4))) { set_error("%s: clip modes 1 and 2 need a scales buffer", who); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode == 1 && (!work || !aligned(work, 8) || work_elems < rows * blocks)) {
    set_error("%s: work must hold efl_dp_conv_work_elems() = %lld doubles, got %lld", who, (long long)(rows * blocks), (long long)work_elems);
    return EFL_E_INVALID_ARGUMENT;
  }
  conv_splits(rows, &per, &splits);
  if (!partials || !aligned(partials, 16) || partial_elems < splits * prow) {
    set_error("%s: partials must hold efl_dp_conv_partial_elems() = %lld floats, 16-byte aligned, got %lld", who, (long long)(splits * prow), (long long)partial_elems);
    return EFL_E_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  const int r = (int)(B / rows);
  if (clip_mode == 1) {
    launch_sqnorm(layers, nlayers, rows, r, work, 0, blocks, s);
    k_dp_scales<<<(unsigned)rows, 64, 0, s>>>(work, blocks, (double)l2_norm_clip, scales);
  }
  std::vector<efl_dp_var> vars;
  for_chunks(layers, nlayers, [&](const cv_chunk& c, long long) {
    const dim3 grid(c.first[c.n], (unsigned)splits);
    if (clip_mode == 0) k_dp_conv_sum<false><<<grid, 64, 0, s>>>(c, rows, r, per, scales, partials, prow);
    else k_dp_conv_sum<true><<<grid, 64, 0, s>>>(c, rows, r, per, scales, partials, prow);
    for (int i = 0; i < c.n; ++i) {
      const efl_dp_conv& L = c.v[i];
      const long long wn = (long long)L.cout * L.cin * L.kh * L.kw;
      vars.push_back(efl_dp_var{partials + c.poff[i], L.w_out, wn, prow, L.ctr0_w});
      if (L.b_out) vars.push_back(efl_dp_var{partials + c.poff[i] + pad4(wn), L.b_out, L.cout, prow, L.ctr0_b});
    }
  });
  const int e = hip_status(hipGetLastError(), who);
  if (e != EFL_OK) return e;
  // the splits in order, the noise and the divide: one launch over every variable
  return efl_dp_clip_sum(vars.data(), (int64_t)vars.size(), splits, 0, 0.0f, mode, sigma, divisor, seed, nullptr, nullptr,
                         0, stream);
}
