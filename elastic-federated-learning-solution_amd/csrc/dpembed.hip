// DP-SGD for embedding tables without a dense per-microbatch gradient: the clip norms
// and the clipped, noised sum of a table's gradient straight from the looked-up ids [B, L] and the
// gradient d of the summed loss with respect to the layer's output (torch.nn.Embedding: [B, L, dim];
// torch.nn.EmbeddingBag, modes "sum" and "mean": [B, dim], every entry of a bag sharing its row).
//
// Reference: efls-train/python/efl/privacy/dp_optimizer.py compute_gradients (:148-216); the model of
// example/criteo is hashed embedding tables (combiner "mean") under a small MLP.
// Entry e = b L + l has id ids[e] and gradient row d_e = d[b][l] (or d[b]) times the layer's weight w
// (1, or 1 / L for "mean"). Microbatch m owns the r = B / rows consecutive examples from m r. Its
// gradient of the table is zero but for the rows its ids name, so
//   S_m = sum over distinct v of || sum_{e in m, id_e = v} w d_e ||^2,
//   sum_m s_m G_m [v] = sum_{e, id_e = v} (s_{m(e)} w) d_e,
// and the only dense work is the noise, which every row of the table gets: one write and no read.
//
// NOTHING IS ADDRESSED BY AN ID. Ids are sort keys and take part in comparisons only; an id outside
// [0, V) becomes the key V, which equals no table row: it enters neither the norm nor the sum.
//
// Launches (a further set per 32 layers; no matrix instructions: a sort, a segmented reduction and a
// store stream have no GEMM in them):
//   k_dp_embed_sqnorm  workgroup (microbatch, layer). The microbatch's n = r L keys (id << 13 | entry)
//                      go into LDS, padded to a power of two with all-ones keys, and through a bitonic
//                      network (the key is unique, so the order is total and entries of one id stay in
//                      entry order). Item (position p, column c), the lanes striding the items: where
//                      p heads a run of equal ids the lane adds the run's (double) w (double) d_e[c] in
//                      entry order, squares the sum and keeps it; the workgroup reduces by wave
//                      shuffles, then LDS, into its own slot work[m][layer]. No atomics.
//   k_dp_scales        (dp_scales.h) one wave per row, as efl_dp_clip_sum.
//   k_dp_embed_group   one workgroup of 1,024 lanes per layer sorts all N = B L <= 8,192 keys the same
//                      way (64 KiB of LDS at most). It writes the sorted ids sid[p], at every run head p
//                      the combined row U[p][c] = sum of the run in fp32 from 0.0f in entry order,
//                      acc = acc + t_e d_e[c] with t_e = s_{m(e)} w rounded once (entry order is
//                      microbatch order: the loop's `sum = sum + g_m s_m` on the rows that are hit), and
//                      for every tile of the noise pass the range [lo, hi) of sorted positions whose
//                      ids lie in the tile's rows (two searches of the keys in LDS). The runs are not
//                      compacted: U is indexed by the head's position, so no count has to be formed or
//                      read anywhere.
//   k_dp_embed_noise   workgroup = one tile of 4,096 consecutive elements of out [V, dim]; a lane owns 4
//                      Philox blocks kBlock lanes apart, as k_dp_noise. It reads its tile's [lo, hi): empty
//                      for nearly every tile, and then the tile is normals<4>, dp_one(0, z) and four
//                      16-byte non-temporal stores, with nothing read. Otherwise the lane finds each of
//                      its elements' rows among sid[lo, hi) and takes U[p][c] where the row is there.
//                      A row may straddle blocks, stores and tiles (dim is any value >= 1); the ragged
//                      end of V dim goes out as dwords.
// Fixed orders everywhere: the same inputs give the same bytes.
#include <cstdint>

#include "common.h"
#include "dp_normal.h"
#include "dp_scales.h"

// acc + t * d rounds twice, as the reference's separate multiply and add do
#pragma clang fp contract(off)

namespace efl {
namespace {

constexpr int kMaxLayers = 32;       // layers per launch: 32 x (72 + 8 + 4) B of the 4 KiB argument space
constexpr int kMaxR = 16;            // examples per microbatch
constexpr int kEntryBits = 13;       // an entry's index in its key
constexpr int kMaxEntries = 1 << kEntryBits;   // 8,192 keys of 8 bytes: the 64 KiB of LDS
constexpr int kGroupBlock = 1024;    // lanes of k_dp_embed_group
constexpr int kNB = 4;               // Philox blocks per lane of the noise pass
constexpr int kNoiseTile = EFL_DP_EMBED_NOISE_TILE;   // elements of out per workgroup of the noise pass
static_assert(kNoiseTile == kBlock * kNB * 4, "a tile is kNB Philox blocks per lane");
constexpr uint64_t kEntryMask = kMaxEntries - 1;

struct de_chunk {
  efl_dp_embed v[kMaxLayers];
  uint64_t off[kMaxLayers];          // layer i's scratch, in bytes from the scratch base
  uint32_t first[kMaxLayers + 1];    // layer i's first tile in the noise grid
  int n;
};

// a layer's scratch: sid [N] int64, U [N, dim] float, tile ranges [tiles] int2, each 16-byte aligned
__host__ __device__ inline long long pad16(long long b) { return (b + 15) & ~15ll; }
__host__ __device__ inline long long tiles_of(const efl_dp_embed& L) { return (L.V * L.dim + kNoiseTile - 1) / kNoiseTile; }
__host__ __device__ inline long long u_offset(long long N) { return pad16(8 * N); }
__host__ __device__ inline long long tr_offset(const efl_dp_embed& L, long long N) { return u_offset(N) + pad16(4 * N * L.dim); }
__host__ __device__ inline long long layer_bytes(const efl_dp_embed& L, long long N) { return tr_offset(L, N) + pad16(8 * tiles_of(L)); }

__host__ __device__ inline int pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

__device__ __forceinline__ int find_layer(const de_chunk& c, uint32_t tile) {
  int lo = 0, hi = c.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (c.first[mid] <= tile) lo = mid;
    else hi = mid;
  }
  return lo;
}

// keys[i] = (id, i) for the n entries from ids, all ones for i in [n, P); then the bitonic network
__device__ __forceinline__ void sort_entries(const int64_t* __restrict__ ids, int n, int P, long long V, uint64_t* keys) {
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  for (int i = tid; i < P; i += nt) {
    uint64_t key = ~0ull;
    if (i < n) {
      const long long id = ids[i];
      key = ((uint64_t)(id >= 0 && id < V ? id : V) << kEntryBits) | (uint64_t)i;
    }
    keys[i] = key;
  }
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < P / 2; i += nt) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
        const uint64_t a = keys[lo], b = keys[hi];
        if ((a > b) == ((lo & k) == 0)) { keys[lo] = b; keys[hi] = a; }
      }
    }
  __syncthreads();
}

// the first position of keys[lo, hi) whose key is >= key
__device__ __forceinline__ int lower_bound(const uint64_t* keys, int lo, int hi, uint64_t key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// position p heads a run of a table row's entries
__device__ __forceinline__ bool run_head(const uint64_t* keys, int p, long long V) {
  const uint64_t id = keys[p] >> kEntryBits;
  return id != (uint64_t)V && (p == 0 || (keys[p - 1] >> kEntryBits) != id);
}

// Pass 1. Workgroup (microbatch, layer): S_{m, layer} in double into its slot.
__global__ __launch_bounds__(kBlock) void k_dp_embed_sqnorm(const de_chunk c, int r, long long slot0, long long slots,
                                                            double* __restrict__ work) {
  extern __shared__ uint64_t keys[];
  const int li = (int)blockIdx.y, tid = (int)threadIdx.x;
  const long long m = blockIdx.x;
  const efl_dp_embed& L = c.v[li];
  const int Lc = L.L, n = r * Lc, P = pow2_at_least(n);
  const long long dim = L.dim, e0 = m * n;
  sort_entries(L.ids + e0, n, P, L.V, keys);
  const double w = (double)L.w;
  double sq = 0.0;
  for (long long it = tid; it < n * dim; it += kBlock) {
    const int p = (int)(it / dim);
    const long long col = it - p * dim;
    if (!run_head(keys, p, L.V)) continue;
    const uint64_t id = keys[p] >> kEntryBits;
    double acc = 0.0;
    for (int q = p; q < n && (keys[q] >> kEntryBits) == id; ++q) {
      const long long e = e0 + (long long)(keys[q] & kEntryMask), b = e / Lc, l = e - b * Lc;
      acc += w * (double)L.d[b * L.d_row_stride + l * L.d_l_stride + col];
    }
    sq += acc * acc;
  }
  __syncthreads();                              // every lane is done with the keys: their LDS takes the partials
  double* part = reinterpret_cast<double*>(keys);
  sq = wave_sum(sq);
  if ((tid & 63) == 0) part[tid >> 6] = sq;
  __syncthreads();
  if (tid == 0) {
    double s = part[0];
#pragma unroll
    for (int wv = 1; wv < kBlock / 64; ++wv) s += part[wv];
    work[m * slots + slot0 + li] = s;
  }
}

// Pass 2. Workgroup = layer: the sorted ids, the combined row of every run and the tiles' ranges.
template <bool CLIP>
__global__ __launch_bounds__(kGroupBlock) void k_dp_embed_group(const de_chunk c, long long B, int r,
                                                                const float* __restrict__ scales,
                                                                unsigned char* __restrict__ scratch) {
  extern __shared__ uint64_t keys[];
  const int li = (int)blockIdx.x, tid = (int)threadIdx.x;
  const efl_dp_embed& L = c.v[li];
  const int Lc = L.L, N = (int)(B * Lc), P = pow2_at_least(N);
  const long long dim = L.dim, V = L.V;
  unsigned char* base = scratch + c.off[li];
  long long* __restrict__ sid = reinterpret_cast<long long*>(base);
  float* __restrict__ U = reinterpret_cast<float*>(base + u_offset(N));
  i2* __restrict__ tr = reinterpret_cast<i2*>(base + tr_offset(L, N));
  sort_entries(L.ids, N, P, V, keys);
  for (long long it = tid; it < N * dim; it += kGroupBlock) {
    const int p = (int)(it / dim);
    const long long col = it - p * dim;
    const uint64_t id = keys[p] >> kEntryBits;
    if (col == 0) sid[p] = (long long)id;
    if (!run_head(keys, p, V)) continue;
    float acc = 0.0f;
    for (int q = p; q < N && (keys[q] >> kEntryBits) == id; ++q) {
      const long long e = (long long)(keys[q] & kEntryMask), b = e / Lc, l = e - b * Lc;
      const float t = CLIP ? scales[b / r] * L.w : L.w;
      acc = acc + t * L.d[b * L.d_row_stride + l * L.d_l_stride + col];
    }
    U[p * dim + col] = acc;
  }
  const long long numel = V * dim, tiles = tiles_of(L);
  for (long long t = tid; t < tiles; t += kGroupBlock) {
    const long long j0 = t * kNoiseTile, j1 = j0 + kNoiseTile < numel ? j0 + kNoiseTile : numel;
    const uint64_t v0 = (uint64_t)(j0 / dim), v1 = (uint64_t)((j1 - 1) / dim);
    const int lo = lower_bound(keys, 0, N, v0 << kEntryBits);
    tr[t] = i2{lo, lower_bound(keys, lo, N, (v1 + 1) << kEntryBits)};
  }
}

// Pass 3. Workgroup = one tile of out: the noise of every element, over U where a row was hit.
template <int MODE, bool POW2>
__global__ __launch_bounds__(kBlock) void k_dp_embed_noise(const de_chunk c, long long B,
                                                           const unsigned char* __restrict__ scratch, uint64_t seed,
                                                           float sigma, float div) {
  const int li = find_layer(c, blockIdx.x), tid = (int)threadIdx.x;
  const efl_dp_embed& L = c.v[li];
  const long long dim = L.dim, numel = L.V * dim, N = B * L.L;
  const long long tile = blockIdx.x - c.first[li], g0 = tile * (kBlock * kNB) + tid;
  const unsigned char* base = scratch + c.off[li];
  const long long* __restrict__ sid = reinterpret_cast<const long long*>(base);
  const float* __restrict__ U = reinterpret_cast<const float*>(base + u_offset(N));
  const i2 range = reinterpret_cast<const i2*>(base + tr_offset(L, N))[tile];   // uniform over the workgroup
  float z[kNB][4];
  normals<kNB>(seed, L.ctr0 + (uint64_t)g0, kBlock, z);
#pragma unroll
  for (int b = 0; b < kNB; ++b) {
    const long long g = g0 + b * kBlock, i0 = 4 * g;
    if (i0 >= numel) break;
    f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (range[0] != range[1]) {                 // rare: rows of this tile were hit
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long row = (i0 + j) / dim, col = i0 + j - row * dim;
        int lo = range[0], hi = range[1];
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (sid[mid] < row) lo = mid + 1;
          else hi = mid;
        }
        if (i0 + j < numel && lo < range[1] && sid[lo] == row) v[j] = U[lo * dim + col];
      }
    }
    f4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = dp_one<MODE, POW2>(v[j], z[b][j], sigma, div);
    if (i0 + 4 <= numel) __builtin_nontemporal_store(o, reinterpret_cast<f4*>(L.out) + g);
    else
      for (int j = 0; i0 + j < numel; ++j) L.out[i0 + j] = o[j];
  }
}

const char* check_layer(const efl_dp_embed& L, int64_t B, bool need_out) {
  constexpr int64_t kMax = 0x7fffffff;
  if (L.V < 1 || L.dim < 1 || L.L < 1 || L.V > kMax) return "V, dim and L must be >= 1 (V below 2^31)";
  if (B * (int64_t)L.L > kMaxEntries) return "more than 8192 entries (B L)";
  if (!L.ids || !L.d || (need_out && !L.out)) return "null ids, d or out";
  if (!aligned(L.ids, 8) || !aligned(L.d, 4) || (need_out && !aligned(L.out, 16))) return "ids must be 8-byte, d 4-byte and out 16-byte aligned";
  if (L.d_l_stride != 0 && (L.d_l_stride < L.dim || L.d_l_stride > (1ll << 40))) return "d's l stride must be 0 (a bag) or at least dim";
  if (L.d_row_stride < (int64_t)(L.L - 1) * L.d_l_stride + L.dim) return "d's row stride is below its width";
  return nullptr;
}

// fn(chunk, index of its first layer) for every run of at most kMaxLayers layers, their scratch laid
// out in layer order; false when a chunk's noise grid would pass 2^31 - 1 tiles. *bytes: all of it.
template <class F>
bool for_chunks(const efl_dp_embed* layers, int64_t nlayers, int64_t B, long long* bytes, F fn) {
  long long off = 0;
  for (int64_t i0 = 0; i0 < nlayers; i0 += kMaxLayers) {
    de_chunk c;
    long long total = 0;
    c.n = (int)(nlayers - i0 < kMaxLayers ? nlayers - i0 : kMaxLayers);
    for (int i = 0; i < c.n; ++i) {
      const efl_dp_embed& L = layers[i0 + i];
      c.v[i] = L;
      c.off[i] = (uint64_t)off;
      c.first[i] = (uint32_t)total;
      off += layer_bytes(L, B * L.L);
      total += tiles_of(L);
      if (total > 0x7fffffffll) return false;
    }
    c.first[c.n] = (uint32_t)total;
    fn(c, i0);
  }
  if (bytes) *bytes = off;
  return true;
}

// the dynamic LDS of a chunk's sort kernels: the widest layer's padded keys (and the norm's partials)
size_t lds_bytes(const de_chunk& c, long long examples) {
  int p = 4;
  for (int i = 0; i < c.n; ++i) {
    const int q = pow2_at_least((int)(examples * c.v[i].L));
    p = q > p ? q : p;
  }
  return (size_t)p * 8;
}

bool check_batch(const char* who, int64_t nlayers, int64_t B, int64_t rows) {
  if (nlayers < 0 || rows <= 0 || B <= 0 || B > kMaxEntries) { set_error("%s: nlayers must be >= 0, rows > 0 and 0 < B <= 8192", who); return false; }
  if (B % rows != 0 || B / rows > kMaxR) { set_error("%s: rows (%lld) must divide B (%lld) into at most %d examples each", who, (long long)rows, (long long)B, kMaxR); return false; }
  return true;
}

template <int MODE, bool POW2>
void launch_noise(const de_chunk& c, long long B, const unsigned char* scratch, uint64_t seed, float sigma, float d,
                  hipStream_t s) {
  k_dp_embed_noise<MODE, POW2><<<c.first[c.n], kBlock, 0, s>>>(c, B, scratch, seed, sigma, d);
}

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API int64_t efl_dp_embed_work_elems(int64_t nlayers, int64_t rows) {
  if (nlayers < 0 || rows <= 0 || (nlayers > 0 && rows > INT64_MAX / 16 / nlayers)) {
    set_error("efl_dp_embed_work_elems: nlayers must be >= 0 and rows > 0 (and their product below 2^59)");
    return EFL_E_INVALID_ARGUMENT;
  }
  return nlayers * rows;
}

EFL_API int64_t efl_dp_embed_scratch_bytes(const efl_dp_embed* layers, int64_t nlayers, int64_t B) {
  if (nlayers < 0 || B <= 0 || B > kMaxEntries || (nlayers > 0 && !layers)) {
    set_error("efl_dp_embed_scratch_bytes: nlayers must be >= 0, 0 < B <= 8192 and the table given");
    return EFL_E_INVALID_ARGUMENT;
  }
  for (int64_t i = 0; i < nlayers; ++i) {
    const efl_dp_embed& L = layers[i];
    if (L.V < 1 || L.dim < 1 || L.L < 1 || L.V > 0x7fffffff || B * (int64_t)L.L > kMaxEntries) {
      set_error("efl_dp_embed_scratch_bytes: layer %lld: V, dim and L must be >= 1 and B L <= 8192", (long long)i);
      return EFL_E_INVALID_ARGUMENT;
    }
  }
  long long bytes = 0;
  if (!for_chunks(layers, nlayers, B, &bytes, [](const de_chunk&, int64_t) {})) {
    set_error("efl_dp_embed_scratch_bytes: tables too large for one grid");
    return EFL_E_INVALID_ARGUMENT;
  }
  return bytes;
}

EFL_API int efl_dp_embed_sqnorm(const efl_dp_embed* layers, int64_t nlayers, int64_t B, int64_t rows, double* work,
                                int64_t slot0, int64_t slots, void* stream) {
  if (!check_batch("efl_dp_embed_sqnorm", nlayers, B, rows)) return EFL_E_INVALID_ARGUMENT;
  if (nlayers == 0) return EFL_OK;
  if (!layers) { set_error("efl_dp_embed_sqnorm: null layer table"); return EFL_E_INVALID_ARGUMENT; }
  for (int64_t i = 0; i < nlayers; ++i)
    if (const char* why = check_layer(layers[i], B, false)) { set_error("efl_dp_embed_sqnorm: layer %lld: %s", (long long)i, why); return EFL_E_INVALID_ARGUMENT; }
  if (!work || !aligned(work, 8) || slot0 < 0 || slots > INT64_MAX / 16 / rows || slot0 > slots - nlayers) {
    set_error("efl_dp_embed_sqnorm: work must hold rows x slots doubles with the layers' %lld slots in [slot0, slots)", (long long)nlayers);
    return EFL_E_INVALID_ARGUMENT;
  }
  if (!for_chunks(layers, nlayers, B, nullptr, [](const de_chunk&, int64_t) {})) { set_error("efl_dp_embed_sqnorm: tables too large for one grid"); return EFL_E_INVALID_ARGUMENT; }
  const int r = (int)(B / rows);
  for_chunks(layers, nlayers, B, nullptr, [&](const de_chunk& c, int64_t i0) {
    k_dp_embed_sqnorm<<<dim3((unsigned)rows, (unsigned)c.n), kBlock, lds_bytes(c, r), (hipStream_t)stream>>>(c, r, slot0 + i0, slots, work);
  });
  return hip_status(hipGetLastError(), "efl_dp_embed_sqnorm");
}

EFL_API int efl_dp_embed_clip_sum(const efl_dp_embed* layers, int64_t nlayers, int64_t B, int64_t rows, int clip_mode,
                                  float l2_norm_clip, int mode, float sigma, float divisor, uint64_t seed,
                                  float* scales, double* work, int64_t work_elems, void* scratch,
                                  int64_t scratch_bytes, void* stream) {
  const char* who = "efl_dp_embed_clip_sum";
  if (clip_mode < 0 || clip_mode > 2) { set_error("%s: clip_mode must be 0 (none), 1 (from the norms) or 2 (given scales)", who); return EFL_E_INVALID_ARGUMENT; }
  if (mode < 0 || mode > 1) { set_error("%s: mode must be 0 (element-wise) or 1 (Gaussian sum)", who); return EFL_E_INVALID_ARGUMENT; }
  if (!(divisor == divisor) || divisor == 0.0f) { set_error("%s: divisor must be non-zero", who); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode == 1 && !(l2_norm_clip > 0.0f)) { set_error("%s: l2_norm_clip must be positive", who); return EFL_E_INVALID_ARGUMENT; }
  if (!check_batch(who, nlayers, B, rows)) return EFL_E_INVALID_ARGUMENT;
  if (nlayers == 0) return EFL_OK;
  if (!layers) { set_error("%s: null layer table", who); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode != 0 && (!scales || !aligned(scales, 4))) { set_error("%s: clip modes 1 and 2 need a scales buffer", who); return EFL_E_INVALID_ARGUMENT; }
  for (int64_t i = 0; i < nlayers; ++i)
    if (const char* why = check_layer(layers[i], B, true)) { set_error("%s: layer %lld: %s", who, (long long)i, why); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode == 1 && (!work || !aligned(work, 8) || rows > INT64_MAX / 16 / nlayers || work_elems < rows * nlayers)) {
    set_error("%s: work must hold efl_dp_embed_work_elems() = %lld doubles, got %lld", who, (long long)(rows * nlayers), (long long)work_elems);
    return EFL_E_INVALID_ARGUMENT;
  }
  long long need = 0;
  if (!for_chunks(layers, nlayers, B, &need, [](const de_chunk&, int64_t) {})) { set_error("%s: tables too large for one grid", who); return EFL_E_INVALID_ARGUMENT; }
  if (!scratch || !aligned(scratch, 16) || scratch_bytes < need) {
    set_error("%s: scratch must be 16-byte aligned and hold efl_dp_embed_scratch_bytes() = %lld bytes, got %lld", who, need, (long long)scratch_bytes);
    return EFL_E_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  unsigned char* sc = static_cast<unsigned char*>(scratch);
  const int r = (int)(B / rows);
  float d;
  const bool pow2 = dp_divisor(divisor, &d);
  if (clip_mode == 1) {
    for_chunks(layers, nlayers, B, nullptr, [&](const de_chunk& c, int64_t i0) {
      k_dp_embed_sqnorm<<<dim3((unsigned)rows, (unsigned)c.n), kBlock, lds_bytes(c, r), s>>>(c, r, i0, nlayers, work);
    });
    k_dp_scales<<<(unsigned)rows, 64, 0, s>>>(work, nlayers, (double)l2_norm_clip, scales);
  }
  for_chunks(layers, nlayers, B, nullptr, [&](const de_chunk& c, int64_t) {
    if (clip_mode == 0) k_dp_embed_group<false><<<c.n, kGroupBlock, lds_bytes(c, B), s>>>(c, B, r, scales, sc);
    else k_dp_embed_group<true><<<c.n, kGroupBlock, lds_bytes(c, B), s>>>(c, B, r, scales, sc);
    if (mode == 0 && pow2) launch_noise<0, true>(c, B, sc, seed, sigma, d, s);
    else if (mode == 0) launch_noise<0, false>(c, B, sc, seed, sigma, d, s);
    else if (pow2) launch_noise<1, true>(c, B, sc, seed, sigma, d, s);
    else launch_noise<1, false>(c, B, sc, seed, sigma, d, s);
  });
  return hip_status(hipGetLastError(), who);
}
