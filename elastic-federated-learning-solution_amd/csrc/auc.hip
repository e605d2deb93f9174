// efl.metrics on the device: the thresholded AUC of tf.metrics.auc (TF 1.15) as a
// histogram, and the grouped AUC as a sort and a segmented rank sum.
//
// Reference: efls-train/python/efl/utils/metrics.py:25-58 exports metrics.auc (tf.metrics.auc: every
// prediction against every one of T thresholds, a [T, n] boolean tensor per batch) and metrics.gauc
// (an op the reference never defines; the definition here is include/efl_hip.h's).
//
// AUC. thr[0] = -1e-7, thr[T - 1] = 1 + 1e-7, thr[i] = i / (T - 1), each formed in double and rounded
// once to float. An element's bucket is k(p) = #{t : p > thr[t]} in [0, T] (thr is non-decreasing, so
// the set is a prefix; a NaN compares false everywhere and lands in 0); its key is label (T + 1) + k.
// The metric's state is the summed weight per key, double [2][T + 1].
//   k_auc_count   no weights. A workgroup strides over tiles of 2,048 elements: two 16-byte prediction
//                 loads and the labels' own width per lane, the bucket from the guess floor(p (T - 1))
//                 corrected against the threshold table in LDS, then one LDS integer add into the
//                 wave's copy of the histogram (4, 2 or 1 copies, as T lets them fit). An integer sum
//                 does not depend on order. The copies are added and written as doubles (exact) to the
//                 workgroup's row of the work buffer.
//   k_auc_wsum    weights. A tile's (key, weight) pairs are staged in LDS in element order. Lane l owns
//                 the keys base + l + 256 q, q < KPT, their sums in registers; every lane walks the
//                 staged tile (a broadcast LDS read per element) and adds the weights of its own keys
//                 as it meets them: in element order, no atomics. blockIdx.y picks the range of
//                 256 KPT keys (two ranges only for T = 4096).
//   k_auc_reduce  one lane per key adds the workgroups' rows to the state in workgroup order.
//   k_auc_value   one workgroup: prefix and suffix sums of the buckets in double (a lane owns a run of
//                 buckets; the runs' totals go through LDS and are added in order), tp, fp, tn, fn
//                 [4][T] to the caller, then the curve's terms, lane-strided, reduced in a fixed tree.
//
// GAUC. Keys of 16 bytes (indicator with its sign bit flipped; order-preserving prediction bits << 32 |
// label) are sorted ascending: a bitonic network per tile of 2,048 in LDS, then rank-merge passes
// (an element's place is its offset in its own run plus its rank in the sibling run: lower bound for
// the left run, upper bound for the right one, so equal keys keep a total order). In the sorted order a
// positive's pairs are counted from the exclusive prefix count of negatives:
//   2U += 2 (neg[run start] - neg[group start]) + (neg[run end] - neg[run start]),
// the three places found by binary search. Both prefix sums (negatives, then the positives' int64
// contributions) are tile-local scans plus a scanned table of tile totals, which is how a group that
// spans any number of tiles is carried. A group's head forms AUC_g = 2U / (2 P N) in double once; the
// workgroups' (total, count) go through one slot each, added in slot order.
// No kernel waits for another lane, wave or workgroup, and nothing is claimed by an atomic on global
// memory: the same inputs give the same bytes.
#include <cstdint>
#include <type_traits>

#include "common.h"

namespace efl {
namespace {

constexpr int kTile = EFL_AUC_TILE;          // elements per tile of both metrics
constexpr int kPer = kTile / kBlock;         // 8 per lane
constexpr int kMaxT = 4096;
constexpr int kMaxGroups = 512;              // workgroups of an update: two per CU
constexpr long long kMaxPartial = 1 << 20;   // doubles of the work buffer, at most
constexpr long long kMaxGauc = 1 << 22;      // elements of one efl_gauc_update
static_assert(kTile == 2048 && kPer == 8, "a lane takes two 16-byte loads of predictions per tile");

__host__ __device__ inline int keys_of(int T) { return 2 * (T + 1); }

int groups_of(long long n, int T) {
  const long long tiles = (n + kTile - 1) / kTile;
  long long cap = kMaxPartial / keys_of(T);
  if (cap > kMaxGroups) cap = kMaxGroups;
  return (int)(tiles < cap ? tiles : cap);
}

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  return s;
}

__device__ __forceinline__ void fill_thresholds(int T, float* thr) {
  for (int i = (int)threadIdx.x; i < T; i += kBlock)
    thr[i] = i == 0 ? (float)-1e-7 : i == T - 1 ? (float)(1.0 + 1e-7) : (float)((double)i / (double)(T - 1));
}

// #{t : p > thr[t]}: exact for every float, whatever the guess
__device__ __forceinline__ int bucket(float p, int T, const float* thr) {
  const float x = p * (float)(T - 1);
  int k = x >= (float)(T - 1) ? T : x > 0.0f ? (int)x + 1 : 0;
  while (k < T && p > thr[k]) ++k;
  while (k > 0 && !(p > thr[k - 1])) --k;
  return k;
}

template <class L>
struct alignas(sizeof(L) * 4 < 16 ? sizeof(L) * 4 : 16) lab4 {
  L v[4];
};

// f(element's index in the tile, prediction, label != 0, weight) for the lane's 8 elements of the tile
// from `base`: 16-byte loads where four elements are there, single ones at the end of the input
template <class L, bool W, class F>
__device__ __forceinline__ void lane_elements(const float* __restrict__ pred, const L* __restrict__ labels,
                                              const float* __restrict__ weights, long long base, long long n, F f) {
#pragma unroll
  for (int j = 0; j < kPer / 4; ++j) {
    const int e = (j * kBlock + (int)threadIdx.x) * 4;
    const long long i = base + e;
    if (i + 4 <= n) {
      const f4 p = *reinterpret_cast<const f4*>(pred + i);
      const lab4<L> l = *reinterpret_cast<const lab4<L>*>(labels + i);
      f4 w = {0.0f, 0.0f, 0.0f, 0.0f};
      if (W) w = *reinterpret_cast<const f4*>(weights + i);
#pragma unroll
      for (int c = 0; c < 4; ++c) f(e + c, p[c], l.v[c] != (L)0, w[c]);
    } else {
      for (int c = 0; i + c < n; ++c) f(e + c, pred[i + c], labels[i + c] != (L)0, W ? weights[i + c] : 0.0f);
    }
  }
}

template <class L>
__global__ __launch_bounds__(kBlock) void k_auc_count(const float* __restrict__ pred, const L* __restrict__ labels,
                                                      long long n, int T, int copies, double* __restrict__ partial) {
  extern __shared__ uint32_t lds[];
  float* thr = reinterpret_cast<float*>(lds);
  uint32_t* hist = lds + T;
  const int keys = keys_of(T), tid = (int)threadIdx.x;
  fill_thresholds(T, thr);
  for (int i = tid; i < copies * keys; i += kBlock) hist[i] = 0;
  __syncthreads();
  uint32_t* mine = hist + ((tid >> 6) & (copies - 1)) * keys;
  const long long tiles = (n + kTile - 1) / kTile;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x)
    lane_elements<L, false>(pred, labels, nullptr, t * kTile, n, [&](int, float p, bool pos, float) {
      atomicAdd(&mine[(pos ? T + 1 : 0) + bucket(p, T, thr)], 1u);
    });
  __syncthreads();
  for (int i = tid; i < keys; i += kBlock) {
    uint32_t s = 0;
    for (int c = 0; c < copies; ++c) s += hist[c * keys + i];
    partial[(long long)blockIdx.x * keys + i] = (double)s;
  }
}

template <class L, int KPT>
__global__ __launch_bounds__(kBlock) void k_auc_wsum(const float* __restrict__ pred, const L* __restrict__ labels,
                                                     const float* __restrict__ weights, long long n, int T,
                                                     double* __restrict__ partial) {
  extern __shared__ uint32_t lds[];
  float* thr = reinterpret_cast<float*>(lds);
  uint2* stage = reinterpret_cast<uint2*>(lds + ((T + 3) & ~3));
  const int keys = keys_of(T), tid = (int)threadIdx.x;
  const unsigned base = blockIdx.y * (unsigned)(kBlock * KPT);
  double acc[KPT];
#pragma unroll
  for (int q = 0; q < KPT; ++q) acc[q] = 0.0;
  fill_thresholds(T, thr);
  __syncthreads();
  const long long tiles = (n + kTile - 1) / kTile;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long left = n - t * kTile;
    const int count = left < kTile ? (int)left : kTile;
    lane_elements<L, true>(pred, labels, weights, t * kTile, n, [&](int e, float p, bool pos, float w) {
      stage[e] = make_uint2((unsigned)((pos ? T + 1 : 0) + bucket(p, T, thr)), __float_as_uint(w));
    });
    __syncthreads();
#pragma unroll 4
    for (int e = 0; e < count; ++e) {
      const uint2 s = stage[e];
      const unsigned rel = s.x - base;           // below base: wraps past every range
      if ((rel & (kBlock - 1)) == (unsigned)tid && rel < (unsigned)(kBlock * KPT)) {
        const int slot = (int)(rel >> 8);
        const double w = (double)__uint_as_float(s.y);
#pragma unroll
        for (int q = 0; q < KPT; ++q)
          if (slot == q) acc[q] += w;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < KPT; ++q) {
    const unsigned key = base + (unsigned)(q * kBlock + tid);
    if (key < (unsigned)keys) partial[(long long)blockIdx.x * keys + key] = acc[q];
  }
}
static_assert(kBlock == 256, "k_auc_wsum takes a key's slot from rel >> 8");

__global__ __launch_bounds__(kBlock) void k_auc_reduce(const double* __restrict__ partial, int groups, int keys,
                                                       double* __restrict__ state) {
  const int j = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (j >= keys) return;
  double s = state[j];
  for (int g = 0; g < groups; ++g) s += partial[(long long)g * keys + j];
  state[j] = s;
}

__device__ __forceinline__ double div0(double a, double b) { return b == 0.0 ? 0.0 : a / b; }

__global__ __launch_bounds__(kBlock) void k_auc_value(const double* __restrict__ state, int T, int curve, int method,
                                                      float* __restrict__ value, double* __restrict__ value64,
                                                      double* conf) {
  __shared__ double tot[2][kBlock];
  __shared__ double red[kBlock / 64];
  const int tid = (int)threadIdx.x, B = T + 1, per = (B + kBlock - 1) / kBlock;
  const int k0 = tid * per, k1 = k0 + per < B ? k0 + per : B;     // k1 <= k0: no buckets for this lane
  for (int lab = 0; lab < 2; ++lab) {
    const double* h = state + lab * B;
    double s = 0.0;
    for (int k = k0; k < k1; ++k) s += h[k];
    tot[lab][tid] = s;
  }
  __syncthreads();
  for (int lab = 0; lab < 2; ++lab) {
    const double* h = state + lab * B;
    double* above = conf + (lab ? 0 : 1) * T;                     // tp, fp: the buckets over t
    double* below = conf + (lab ? 3 : 2) * T;                     // fn, tn: the buckets up to t
    double lo = 0.0, hi = 0.0;
    for (int i = 0; i < tid; ++i) lo += tot[lab][i];
    for (int i = kBlock - 1; i > tid; --i) hi += tot[lab][i];
    for (int k = k0; k < k1; ++k) {
      lo += h[k];
      if (k < T) below[k] = lo;
    }
    for (int k = k1 - 1; k >= k0; --k) {
      hi += h[k];
      if (k >= 1) above[k - 1] = hi;
    }
  }
  __threadfence_block();
  __syncthreads();
  const double *tp = conf, *fp = conf + T, *tn = conf + 2 * T, *fn = conf + 3 * T;
  constexpr double eps = 1e-6;
  double s = 0.0;
  for (int t = tid; t < T - 1; t += kBlock) {
    const int u = t + 1;
    if (curve == 1 && method == 1) {                              // TF's interpolate_pr_auc
      const double p0 = tp[t] + fp[t], p1 = tp[u] + fp[u], dtp = tp[t] - tp[u], dp = p0 - p1;
      const double slope = div0(dtp, dp > 0.0 ? dp : 0.0), intercept = tp[u] - slope * p1;
      const double ratio = p0 > 0.0 && p1 > 0.0 ? p0 / p1 : 1.0, den = tp[u] + fn[u];
      s += div0(slope * (dtp + intercept * log(ratio)), den > 0.0 ? den : 0.0);
      continue;
    }
    const double r0 = (tp[t] + eps) / (tp[t] + fn[t] + eps), r1 = (tp[u] + eps) / (tp[u] + fn[u] + eps);
    double x0, x1, y0, y1;
    if (curve == 0) {
      x0 = fp[t] / (fp[t] + tn[t] + eps), x1 = fp[u] / (fp[u] + tn[u] + eps), y0 = r0, y1 = r1;
    } else {
      x0 = r0, x1 = r1, y0 = (tp[t] + eps) / (tp[t] + fp[t] + eps), y1 = (tp[u] + eps) / (tp[u] + fp[u] + eps);
    }
    const double h = method == 2 ? (y0 < y1 ? y0 : y1) : method == 3 ? (y0 > y1 ? y0 : y1) : (y0 + y1) / 2.0;
    s += (x0 - x1) * h;
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double v = red[0];
    for (int w = 1; w < kBlock / 64; ++w) v += red[w];
    *value64 = v;
    *value = (float)v;
  }
}

// ---------------------------------------------------------------------------------------------------
// GAUC
// ---------------------------------------------------------------------------------------------------

struct alignas(16) gkey {
  uint64_t g;      // the indicator, sign bit flipped
  uint64_t v;      // order-preserving prediction bits << 32 | label
};

__device__ __forceinline__ bool key_less(const gkey& a, const gkey& b) { return a.g < b.g || (a.g == b.g && a.v < b.v); }
__device__ __forceinline__ bool is_neg(const gkey& k) { return (k.v & 1) == 0; }

// -0.0 is +0.0; every NaN is the one value above +inf
__device__ __forceinline__ uint32_t ordered_bits(float p) {
  if (p != p) return 0xFFFFFFFFu;
  const uint32_t u = p == 0.0f ? 0u : __float_as_uint(p);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the scratch of one call, every part 16-byte aligned
struct gauc_scratch {
  long long a, b, neg, cloc, tneg, tc, slots, bytes;
  explicit gauc_scratch(long long n) {
    const long long tiles = (n + kTile - 1) / kTile, blocks = (n + kBlock - 1) / kBlock;
    auto pad = [](long long x) { return (x + 15) & ~15ll; };
    a = 0;
    b = a + 16 * n;
    neg = b + 16 * n;                       // int32 [n + 1]: negatives before each place
    cloc = neg + pad(4 * (n + 1));          // int64 [n]: contributions before each place, within its tile
    tneg = cloc + pad(8 * n);               // int64 [tiles + 1]: negatives before each tile
    tc = tneg + pad(8 * (tiles + 1));       // int64 [tiles + 1]: contributions before each tile
    slots = tc + pad(8 * (tiles + 1));      // double [blocks][2]
    bytes = slots + 16 * blocks;
  }
};

template <class L>
__global__ __launch_bounds__(kBlock) void k_gauc_tile_sort(const float* __restrict__ pred, const L* __restrict__ labels,
                                                           const long long* __restrict__ ind, int n,
                                                           gkey* __restrict__ out) {
  __shared__ gkey tile[kTile];
  const int tid = (int)threadIdx.x, base = (int)blockIdx.x * kTile;
  const int count = n - base < kTile ? n - base : kTile;
  int span = 1;
  while (span < count) span <<= 1;
  for (int x = tid; x < span; x += kBlock) {
    gkey k = {~0ull, ~0ull};                 // a free place: after every key
    if (x < count) {
      k.g = (uint64_t)ind[base + x] ^ 0x8000000000000000ull;
      k.v = ((uint64_t)ordered_bits(pred[base + x]) << 32) | (labels[base + x] != (L)0 ? 1u : 0u);
    }
    tile[x] = k;
  }
  for (int k = 2; k <= span; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < span / 2; i += kBlock) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
        const gkey a = tile[lo], b = tile[hi];
        if (key_less(b, a) == ((lo & k) == 0)) { tile[lo] = b; tile[hi] = a; }
      }
    }
  __syncthreads();
  for (int x = tid; x < count; x += kBlock) out[base + x] = tile[x];
}

// the first place of keys[lo, hi) that is not less than (g, v); with v + 1 the place after the equal ones
__device__ __forceinline__ int lower_bound(const gkey* __restrict__ keys, int lo, int hi, const gkey& key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (key_less(keys[mid], key)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int upper_bound(const gkey* __restrict__ keys, int lo, int hi, const gkey& key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (!key_less(key, keys[mid])) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// one lane per key: its place after the pairwise merge of sorted runs of `run` keys
__global__ __launch_bounds__(kBlock) void k_gauc_merge(const gkey* __restrict__ src, gkey* __restrict__ dst, int n, int run) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i >= n) return;
  const int start = i / (2 * run) * (2 * run);
  const int mid = start + run < n ? start + run : n, end = start + 2 * run < n ? start + 2 * run : n;
  const gkey key = src[i];
  const int at = i < mid ? i + (lower_bound(src, mid, end, key) - mid)
                         : start + (i - mid) + (upper_bound(src, start, mid, key) - start);
  dst[at] = key;                                   // at is in [start, end): see the header's contract
}

// v's exclusive prefix over the workgroup's lanes; *total its sum. sh holds kBlock values.
__device__ __forceinline__ long long block_scan(long long v, long long* sh, long long* total) {
  const int tid = (int)threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {
    const long long x = tid >= d ? sh[tid - d] : 0;
    __syncthreads();
    sh[tid] += x;
    __syncthreads();
  }
  *total = sh[kBlock - 1];
  const long long incl = sh[tid];
  __syncthreads();
  return incl - v;
}

// one workgroup per tile: the tile's negatives
__global__ __launch_bounds__(kBlock) void k_gauc_tile_neg(const gkey* __restrict__ keys, int n, long long* __restrict__ tneg) {
  __shared__ long long sh[kBlock];
  const int i0 = (int)blockIdx.x * kTile + (int)threadIdx.x * kPer;
  long long c = 0, total;
  for (int i = i0; i < i0 + kPer && i < n; ++i) c += is_neg(keys[i]);
  block_scan(c, sh, &total);
  if (threadIdx.x == 0) tneg[blockIdx.x] = total;
}

// one workgroup: t[0, m) becomes its exclusive prefix and t[m] the sum; m <= 2,048
__global__ __launch_bounds__(kBlock) void k_gauc_scan_tiles(long long* t, int m) {
  __shared__ long long sh[kBlock];
  const int per = (m + kBlock - 1) / kBlock, i0 = (int)threadIdx.x * per;
  long long c = 0, total;
  for (int i = i0; i < i0 + per && i < m; ++i) c += t[i];
  long long run = block_scan(c, sh, &total);
  for (int i = i0; i < i0 + per && i < m; ++i) {
    const long long x = t[i];
    t[i] = run;
    run += x;
  }
  if (threadIdx.x == 0) t[m] = total;
}

// one workgroup per tile: neg[i] = the negatives before place i, neg[n] = all of them
__global__ __launch_bounds__(kBlock) void k_gauc_neg_prefix(const gkey* __restrict__ keys, int n,
                                                            const long long* __restrict__ tneg, int* __restrict__ neg) {
  __shared__ long long sh[kBlock];
  const int i0 = (int)blockIdx.x * kTile + (int)threadIdx.x * kPer;
  long long c = 0, total;
  for (int i = i0; i < i0 + kPer && i < n; ++i) c += is_neg(keys[i]);
  long long run = tneg[blockIdx.x] + block_scan(c, sh, &total);
  for (int i = i0; i < i0 + kPer && i < n; ++i) {
    neg[i] = (int)run;
    run += is_neg(keys[i]);
    if (i == n - 1) neg[n] = (int)run;
  }
}

// one workgroup per tile: a positive's pairs, doubled: 2 for each negative of its group below its run
// of equal predictions, 1 for each negative in the run. cloc[i] = the tile's contributions before i.
__global__ __launch_bounds__(kBlock) void k_gauc_contrib(const gkey* __restrict__ keys, int n, const int* __restrict__ neg,
                                                         long long* __restrict__ cloc, long long* __restrict__ tc) {
  __shared__ long long sh[kBlock];
  const int i0 = (int)blockIdx.x * kTile + (int)threadIdx.x * kPer;
  long long c[kPer], sum = 0, total;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int i = i0 + q;
    c[q] = 0;
    if (i < n && !is_neg(keys[i])) {
      const gkey k = keys[i];
      const gkey run_lo = {k.g, k.v & ~0xFFFFFFFFull}, run_hi = {k.g, k.v | 0xFFFFFFFFull}, grp = {k.g, 0};
      const int gs = lower_bound(keys, 0, i, grp), rs = lower_bound(keys, gs, i, run_lo);
      const int re = upper_bound(keys, i + 1, n, run_hi);
      c[q] = 2ll * (neg[rs] - neg[gs]) + (neg[re] - neg[rs]);
    }
    sum += c[q];
  }
  long long run = block_scan(sum, sh, &total);
#pragma unroll
  for (int q = 0; q < kPer; ++q)
    if (i0 + q < n) {
      cloc[i0 + q] = run;
      run += c[q];
    }
  if (threadIdx.x == 0) tc[blockIdx.x] = total;
}

// one lane per place; a group's first place forms AUC_g. slots[block] = the block's (total, count).
__global__ __launch_bounds__(kBlock) void k_gauc_groups(const gkey* __restrict__ keys, int n, const int* __restrict__ neg,
                                                        const long long* __restrict__ cloc, const long long* __restrict__ tc,
                                                        double* __restrict__ slots) {
  __shared__ double red[2][kBlock / 64];
  const int tid = (int)threadIdx.x, i = (int)(blockIdx.x * kBlock + threadIdx.x);
  const int tiles = (n + kTile - 1) / kTile;
  double total = 0.0, count = 0.0;
  if (i < n && (i == 0 || keys[i - 1].g != keys[i].g)) {
    const gkey last = {keys[i].g, ~0ull};
    const int ge = upper_bound(keys, i + 1, n, last);
    const long long N = neg[ge] - neg[i], P = (ge - i) - N;
    if (P > 0 && N > 0) {
      const long long c1 = ge == n ? tc[tiles] : tc[ge / kTile] + cloc[ge], c0 = tc[i / kTile] + cloc[i];
      total = (double)(ge - i) * ((double)(c1 - c0) / (2.0 * (double)P * (double)N));
      count = (double)(ge - i);
    }
  }
  total = wave_sum(total);
  count = wave_sum(count);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = total;
    red[1][tid >> 6] = count;
  }
  __syncthreads();
  if (tid < 2) {
    double s = red[tid][0];
    for (int w = 1; w < kBlock / 64; ++w) s += red[tid][w];
    slots[2 * (long long)blockIdx.x + tid] = s;
  }
}

// one workgroup: the slots in slot order (a lane adds a run of them, lane 0 the lanes' sums), into the
// call's (total, count), the running state and its value
__global__ __launch_bounds__(kBlock) void k_gauc_final(const double* __restrict__ slots, int blocks, double* __restrict__ state,
                                                       double* __restrict__ call_out, float* __restrict__ value,
                                                       double* __restrict__ value64) {
  __shared__ double part[2][kBlock];
  const int tid = (int)threadIdx.x, per = (blocks + kBlock - 1) / kBlock;
  double t = 0.0, c = 0.0;
  for (int b = tid * per; b < tid * per + per && b < blocks; ++b) {
    t += slots[2 * b];
    c += slots[2 * b + 1];
  }
  part[0][tid] = t;
  part[1][tid] = c;
  __syncthreads();
  if (tid == 0) {
    t = c = 0.0;
    for (int l = 0; l < kBlock; ++l) {
      t += part[0][l];
      c += part[1][l];
    }
    if (call_out) {
      call_out[0] = t;
      call_out[1] = c;
    }
    const double T = state[0] + t, C = state[1] + c, v = C > 0.0 ? T / C : 0.0;
    state[0] = T;
    state[1] = C;
    *value64 = v;
    *value = (float)v;
  }
}

// TensorFlow DataType numbers of the labels: DT_FLOAT, DT_INT32, DT_UINT8, DT_INT64, DT_BOOL
template <class F>
bool with_label_type(int dtype, F f) {
  switch (dtype) {
    case 1: f((const float*)nullptr); return true;
    case 3: f((const int32_t*)nullptr); return true;
    case 4: case 10: f((const uint8_t*)nullptr); return true;
    case 9: f((const int64_t*)nullptr); return true;
  }
  return false;
}

int label_align(int dtype) { return dtype == 4 || dtype == 10 ? 4 : 16; }

int invalid(const char* who, const char* text) {
  set_error("%s: %s", who, text);
  return EFL_E_INVALID_ARGUMENT;
}

template <class L, int KPT>
void launch_wsum(const float* pred, const L* labels, const float* weights, long long n, int T, int groups, double* work,
                 hipStream_t s) {
  const int parts = (keys_of(T) + kBlock * KPT - 1) / (kBlock * KPT);
  const size_t lds = 4 * (size_t)((T + 3) & ~3) + 8 * (size_t)kTile;
  k_auc_wsum<L, KPT><<<dim3((unsigned)groups, (unsigned)parts), kBlock, lds, s>>>(pred, labels, weights, n, T, work);
}

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API int64_t efl_auc_work_elems(int64_t n, int num_thresholds) {
  if (n < 0 || n > 0x7fffffffll || num_thresholds < 2 || num_thresholds > kMaxT) {
    set_error("efl_auc_work_elems: 0 <= n < 2^31 and 2 <= num_thresholds <= 4096");
    return EFL_E_INVALID_ARGUMENT;
  }
  return (int64_t)groups_of(n, num_thresholds) * keys_of(num_thresholds);
}

EFL_API int efl_auc_update(const float* predictions, const void* labels, int label_dtype, const float* weights, int64_t n,
                           int num_thresholds, double* state, double* work, int64_t work_elems, void* stream) {
  const char* who = "efl_auc_update";
  const int T = num_thresholds;
  if (T < 2 || T > kMaxT) return invalid(who, "num_thresholds must be in [2, 4096]");
  if (n < 0 || n > 0x7fffffffll) return invalid(who, "n must be in [0, 2^31 - 1]");
  if (!with_label_type(label_dtype, [](auto) {})) return invalid(who, "labels must be uint8 / bool (4, 10), int32 (3), int64 (9) or float32 (1)");
  if (!state || !aligned(state, 8)) return invalid(who, "null or misaligned state");
  if (n == 0) return EFL_OK;
  if (!predictions || !labels) return invalid(who, "null predictions or labels");
  if (!aligned(predictions, 16) || !aligned(labels, label_align(label_dtype)) || !aligned(weights, 16))
    return invalid(who, "predictions, weights and labels must be 16-byte aligned (byte labels: 4)");
  const int groups = groups_of(n, T), keys = keys_of(T);
  if (!work || !aligned(work, 8) || work_elems < (int64_t)groups * keys) {
    set_error("%s: work must hold efl_auc_work_elems() = %lld doubles, got %lld", who, (long long)groups * keys, (long long)work_elems);
    return EFL_E_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  with_label_type(label_dtype, [&](auto tag) {
    using L = std::remove_const_t<std::remove_pointer_t<decltype(tag)>>;
    const L* lab = static_cast<const L*>(labels);
    if (!weights) {
      int copies = 4;
      while (copies > 1 && 4 * (size_t)T + 4 * (size_t)copies * keys > 65536) copies >>= 1;
      k_auc_count<L><<<groups, kBlock, 4 * (size_t)T + 4 * (size_t)copies * keys, s>>>(predictions, lab, n, T, copies, work);
    } else if (keys <= kBlock * 2) {
      launch_wsum<L, 2>(predictions, lab, weights, n, T, groups, work, s);
    } else if (keys <= kBlock * 8) {
      launch_wsum<L, 8>(predictions, lab, weights, n, T, groups, work, s);
    } else {
      launch_wsum<L, 32>(predictions, lab, weights, n, T, groups, work, s);
    }
  });
  k_auc_reduce<<<(keys + kBlock - 1) / kBlock, kBlock, 0, s>>>(work, groups, keys, state);
  return hip_status(hipGetLastError(), who);
}

EFL_API int efl_auc_value(const double* state, int num_thresholds, int curve, int summation_method, float* value,
                          double* value64, double* confusion, void* stream) {
  const char* who = "efl_auc_value";
  if (num_thresholds < 2 || num_thresholds > kMaxT) return invalid(who, "num_thresholds must be in [2, 4096]");
  if (curve < 0 || curve > 1) return invalid(who, "curve must be 0 (ROC) or 1 (PR)");
  if (summation_method < 0 || summation_method > 3)
    return invalid(who, "summation_method must be 0 (trapezoidal), 1 (careful_interpolation), 2 (minoring) or 3 (majoring)");
  if (!state || !value || !value64 || !confusion) return invalid(who, "null state, value, value64 or confusion");
  if (!aligned(state, 8) || !aligned(value, 4) || !aligned(value64, 8) || !aligned(confusion, 8))
    return invalid(who, "misaligned state, value, value64 or confusion");
  k_auc_value<<<1, kBlock, 0, (hipStream_t)stream>>>(state, num_thresholds, curve, summation_method, value, value64, confusion);
  return hip_status(hipGetLastError(), who);
}

EFL_API int64_t efl_gauc_scratch_bytes(int64_t n) {
  if (n < 0 || n > kMaxGauc) {
    set_error("efl_gauc_scratch_bytes: n must be in [0, 2^22]");
    return EFL_E_INVALID_ARGUMENT;
  }
  return n == 0 ? 0 : gauc_scratch(n).bytes;
}

EFL_API int efl_gauc_update(const float* predictions, const void* labels, int label_dtype, const int64_t* indicators,
                            int64_t n, double* state, double* call_out, float* value, double* value64, void* scratch,
                            int64_t scratch_bytes, void* stream) {
  const char* who = "efl_gauc_update";
  if (n < 0) return invalid(who, "negative n");
  if (n > kMaxGauc) {
    set_error("%s: %lld elements: one call takes at most 2^22", who, (long long)n);
    return EFL_E_INVALID_ARGUMENT;
  }
  if (!with_label_type(label_dtype, [](auto) {})) return invalid(who, "labels must be uint8 / bool (4, 10), int32 (3), int64 (9) or float32 (1)");
  if (!state || !value || !value64) return invalid(who, "null state, value or value64");
  if (!aligned(state, 8) || !aligned(call_out, 8) || !aligned(value, 4) || !aligned(value64, 8))
    return invalid(who, "misaligned state, call_out, value or value64");
  if (n > 0) {
    if (!predictions || !labels || !indicators) return invalid(who, "null predictions, labels or indicators");
    const int la = label_dtype == 4 || label_dtype == 10 ? 1 : label_dtype == 9 ? 8 : 4;
    if (!aligned(predictions, 4) || !aligned(labels, la) || !aligned(indicators, 8))
      return invalid(who, "misaligned predictions, labels or indicators");
    if (!scratch || !aligned(scratch, 16) || scratch_bytes < gauc_scratch(n).bytes) {
      set_error("%s: scratch must be 16-byte aligned and hold efl_gauc_scratch_bytes() = %lld bytes, got %lld", who,
                gauc_scratch(n).bytes, (long long)scratch_bytes);
      return EFL_E_INVALID_ARGUMENT;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const int N = (int)n, tiles = (N + kTile - 1) / kTile, blocks = (N + kBlock - 1) / kBlock;
  const double* slots = nullptr;
  if (N > 0) {
    const gauc_scratch L(N);
    unsigned char* base = static_cast<unsigned char*>(scratch);
    gkey* a = reinterpret_cast<gkey*>(base + L.a);
    gkey* b = reinterpret_cast<gkey*>(base + L.b);
    int* neg = reinterpret_cast<int*>(base + L.neg);
    long long* cloc = reinterpret_cast<long long*>(base + L.cloc);
    long long* tneg = reinterpret_cast<long long*>(base + L.tneg);
    long long* tc = reinterpret_cast<long long*>(base + L.tc);
    double* sl = reinterpret_cast<double*>(base + L.slots);
    with_label_type(label_dtype, [&](auto tag) {
      using Lt = std::remove_const_t<std::remove_pointer_t<decltype(tag)>>;
      k_gauc_tile_sort<Lt><<<tiles, kBlock, 0, s>>>(predictions, static_cast<const Lt*>(labels),
                                                   reinterpret_cast<const long long*>(indicators), N, a);
    });
    for (long long run = kTile; run < N; run *= 2) {
      k_gauc_merge<<<blocks, kBlock, 0, s>>>(a, b, N, (int)run);
      gkey* t = a;
      a = b;
      b = t;
    }
    k_gauc_tile_neg<<<tiles, kBlock, 0, s>>>(a, N, tneg);
    k_gauc_scan_tiles<<<1, kBlock, 0, s>>>(tneg, tiles);
    k_gauc_neg_prefix<<<tiles, kBlock, 0, s>>>(a, N, tneg, neg);
    k_gauc_contrib<<<tiles, kBlock, 0, s>>>(a, N, neg, cloc, tc);
    k_gauc_scan_tiles<<<1, kBlock, 0, s>>>(tc, tiles);
    k_gauc_groups<<<blocks, kBlock, 0, s>>>(a, N, neg, cloc, tc, sl);
    slots = sl;
  }
  k_gauc_final<<<1, kBlock, 0, s>>>(slots, blocks, state, call_out, value, value64);
  return hip_status(hipGetLastError(), who);
}
