// DP-SGD for the scale and bias of per-example normalisation layers: the clip norms and the
// clipped, noised sum of a LayerNorm's or GroupNorm's weight and bias gradients straight from the layer's
// input x and the gradient d of the summed loss with respect to its output.
//
// Reference: efls-train/python/efl/privacy/dp_optimizer.py compute_gradients (:148-216). With mu and var
// the mean and the biased variance of an element's statistics group and xh = (x - mu) / sqrt(var + eps),
// microbatch i (the r = B / rows consecutive examples from i r) has
//   ggamma_i[c] = sum d xh,   gbeta_i[c] = sum d   over the microbatch's elements of channel c,
//   S_i = sum_c ggamma_i[c]^2 + beta sum_c gbeta_i[c]^2,   beta = 1 with a bias, else 0.
// That is a column reduction, not a GEMM, so none of the matrix-core families takes it.
//   kind 0, channel-last (torch.nn.LayerNorm over the last dimension): x, d [B, T, C], row p = b T + t at
//           x + p x_row_stride; the statistics group of an element is its row, n = C.
//   kind 1, channel-first (torch.nn.GroupNorm): x, d [B, C, L] contiguous; the statistics group is (b, g),
//           the C / G channels of group g times the L positions, one contiguous run of n = (C / G) L floats.
//
// Launches (a further set per 24 layers):
//   k_dp_norm_stats  one wave per statistics group: the mean, then sum (x - mu)^2 in a second pass over the
//                    same run (no cancellation), both in double, a lane's terms in order and then the wave's
//                    tree; (mu, 1 / sqrt(var + eps)) stored as two doubles. 16-byte loads where the run's
//                    base and length allow, dwords otherwise and for a ragged end.
//   k_dp_norm_grad   channel-last: a workgroup of 4 waves owns (microbatch, layer, tile of 256 columns). A
//                    lane holds 4 adjacent columns, so a wave reads a row of the tile as one coalesced
//                    1 KiB; wave w takes the microbatch's rows w, w + 4, ... of P = r T, four of them in
//                    flight, with the row's (mu, rstd) from one uniform 16-byte load. d (x - mu) rstd is
//                    formed and accumulated in double (the fp32 inputs widen exactly). The 4 waves' sums
//                    meet in 16 KiB of LDS and thread t adds column t's in wave order.
//                    channel-first: a workgroup owns (microbatch, layer, 4 channels), one wave each; the
//                    wave walks its channel's r runs of L floats, fetches the group's stats once per
//                    example, and reduces by the wave's tree.
//                    Both write the microbatch's ggamma, gbeta, rounded once to fp32, into the layer's
//                    columns of a stack [rows, sum of pad4(C) (+ pad4(C))], and the workgroup's share of
//                    S_i, from the double sums, into its own slot of `work`: no atomics, the same bytes on
//                    every run.
//   k_dp_scales      (dp_scales.h) one wave per row of slots.
//   k_dp_clip_sum    (csrc/dpclip.hip, through efl_dp_clip_sum over the stack, clip_mode 2 with the scales,
//                    0 without) the rows in order, the noise and the divide: efl_dp_noise's functions at
//                    the same stream positions as every other family.
// Rounding contract. Statistics and sums in double: S_i differs from the exact one by far less than
// 2^-32 sum_c [(sum |d| |xh|)^2 + beta (sum |d|)^2]. Sum: each stacked row rounded once, then
// efl_dp_clip_sum's row-ordered fp32 sum:
//   |got - exact| <= (rows + 4) 2^-24 (sum_i s_i sum |d xh| + |noise|) / |divisor|   per element.
#include <cstdint>
#include <vector>

#include "common.h"
#include "dp_scales.h"

#pragma clang fp contract(off)

namespace efl {
namespace {

constexpr int kMaxLayers = 24;      // layers per launch: 24 x 96 B of the 4 KiB argument space
constexpr int kMaxR = 16;           // examples per microbatch
constexpr int kTile = 256;          // channel-last: columns per workgroup, 4 per lane
constexpr int kWaves = kBlock / 64;
constexpr int kChan = kWaves;       // channel-first: channels per workgroup, one per wave
constexpr int kRowsInFlight = 4;    // channel-last: rows a wave loads before it adds them

struct nm_chunk {
  efl_dp_norm v[kMaxLayers];
  uint32_t gfirst[kMaxLayers + 1];  // layer i's first statistics group among the chunk's
  uint32_t tfirst[kMaxLayers + 1];  // layer i's first workgroup (= norm slot) of a microbatch
  long long soff[kMaxLayers];       // layer i's first float in a row of the stack
  uint32_t vs, vx, vd;              // bit i: layer i's statistics runs / x rows / d rows take 16-byte loads
  int n;
};

__host__ __device__ inline long long pad4(long long n) { return (n + 3) & ~3ll; }

__device__ __forceinline__ int find_layer(const uint32_t* first, int n, uint32_t at) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= at) lo = mid;
    else hi = mid;
  }
  return lo;
}

// sum over the wave of f(p[i]), i < n, in double: lane l takes the 4-groups (or dwords) l, l + 64, ...
template <class F>
__device__ __forceinline__ double wave_run_sum(const float* __restrict__ p, long long n, bool vec, int lane, F f) {
  double s = 0.0;
  if (vec) {
    const long long nv = n >> 2;
    for (long long g = lane; g < nv; g += 64) {
      const f4 v = *reinterpret_cast<const f4*>(p + 4 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) s += f(v[j]);
    }
    if (lane < n - 4 * nv) s += f(p[4 * nv + lane]);    // the ragged end: n % 4 dwords
  } else {
    for (long long i = lane; i < n; i += 64) s += f(p[i]);
  }
  return wave_sum(s);
}

// One wave per statistics group: (mu, 1 / sqrt(var + eps)) in double, two passes.
__global__ __launch_bounds__(kBlock) void k_dp_norm_stats(const nm_chunk c, long long gbase, double* __restrict__ stats) {
  const uint32_t g = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (g >= c.gfirst[c.n]) return;                       // a whole wave; the kernel has no barrier
  const int li = find_layer(c.gfirst, c.n, g), lane = (int)threadIdx.x & 63;
  const efl_dp_norm& L = c.v[li];
  const long long local = g - c.gfirst[li];
  const long long n = L.kind == 0 ? L.C : L.C / L.groups * L.T_or_L;
  const float* __restrict__ p = L.x + local * (L.kind == 0 ? L.x_row_stride : n);
  const bool vec = (c.vs >> li) & 1;
  const double mu = wave_run_sum(p, n, vec, lane, [](float v) { return (double)v; }) / (double)n;
  const double q = wave_run_sum(p, n, vec, lane, [mu](float v) { const double t = (double)v - mu; return t * t; });
  if (lane == 0) {
    d2* o = reinterpret_cast<d2*>(stats) + gbase + g;
    *o = d2{mu, 1.0 / sqrt(q / (double)n + L.eps)};
  }
}

// a lane's `cnt` (0..4) columns of one row: one 16-byte load, or dwords and zeros
__device__ __forceinline__ f4 load_cols(const float* __restrict__ p, int cnt, bool vec) {
  if (vec && cnt == 4) return *reinterpret_cast<const f4*>(p);
  f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < cnt) v[j] = p[j];
  return v;
}

// the workgroup's share of S_i into its slot, the waves' shares added in wave order
__device__ __forceinline__ void store_slot(double s, double* part, double* __restrict__ work, long long at) {
  const int tid = (int)threadIdx.x;
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0 && work) {
    double t = part[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += part[w];
    work[at] = t;
  }
}

// channel-last: columns [256 tile, +256) of microbatch `row`, all its P = r T rows
__device__ __forceinline__ void grad_channel_last(const efl_dp_norm& L, bool vx, bool vd, int r, long long row, uint32_t tile,
                                                  const d2* __restrict__ st, d2 (*red)[kTile], double* part,
                                                  double* __restrict__ work, long long slot, float* __restrict__ srow) {
  const int tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63;
  const long long P = (long long)r * L.T_or_L, C = L.C, col = (long long)tile * kTile + 4 * lane;
  const int cnt = col >= C ? 0 : C - col < 4 ? (int)(C - col) : 4;
  const float* __restrict__ xp = L.x + row * P * L.x_row_stride + col;
  const float* __restrict__ dp = L.d + row * P * L.d_row_stride + col;
  st += row * P;
  double gw[4] = {0.0, 0.0, 0.0, 0.0}, gb[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long p0 = w; p0 < P; p0 += kWaves * kRowsInFlight) {
    f4 x[kRowsInFlight], d[kRowsInFlight];
    d2 ms[kRowsInFlight];
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
      const long long p = p0 + kWaves * u;
      const bool ok = p < P;                            // uniform over the wave
      x[u] = load_cols(xp + p * L.x_row_stride, ok ? cnt : 0, vx);
      d[u] = load_cols(dp + p * L.d_row_stride, ok ? cnt : 0, vd);
      ms[u] = ok ? st[p] : d2{0.0, 0.0};
    }
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double dd = (double)d[u][j], xh = ((double)x[u][j] - ms[u][0]) * ms[u][1];
        gw[j] += dd * xh;
        gb[j] += dd;
      }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[w][4 * lane + j] = d2{gw[j], gb[j]};
  __syncthreads();
  d2 t = red[0][tid];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) t += red[k][tid];
  const long long c = (long long)tile * kTile + tid;
  const bool ok = c < C, bias = L.b_out != nullptr;
  double s = 0.0;
  if (ok) {
    s = t[0] * t[0] + (bias ? t[1] * t[1] : 0.0);
    if (srow) {
      srow[c] = (float)t[0];
      if (bias) srow[pad4(C) + c] = (float)t[1];
    }
  }
  store_slot(wave_sum(s), part, work, slot);
}

// channel-first: channel 4 quad + wave of microbatch `row`, its r runs of L floats
__device__ __forceinline__ void grad_channel_first(const efl_dp_norm& L, bool vx, bool vd, int r, long long row, uint32_t quad,
                                                   const d2* __restrict__ st, double* part, double* __restrict__ work,
                                                   long long slot, float* __restrict__ srow) {
  const int tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63;
  const long long C = L.C, len = L.T_or_L, ch = (long long)quad * kChan + w, G = L.groups;
  const bool ok = ch < C, bias = L.b_out != nullptr;    // uniform over the wave
  double gw = 0.0, gb = 0.0;
  if (ok) {
    const long long grp = ch / (C / G);
    for (int e = 0; e < r; ++e) {
      const long long b = row * r + e;
      const d2 ms = st[b * G + grp];
      const float* __restrict__ xp = L.x + (b * C + ch) * len;
      const float* __restrict__ dp = L.d + (b * C + ch) * len;
      if (vx && vd) {                                   // len % 4 == 0
        for (long long q = lane; q < (len >> 2); q += 64) {
          const f4 x = *reinterpret_cast<const f4*>(xp + 4 * q), d = *reinterpret_cast<const f4*>(dp + 4 * q);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double dd = (double)d[j];
            gw += dd * (((double)x[j] - ms[0]) * ms[1]);
            gb += dd;
          }
        }
      } else {
        for (long long i = lane; i < len; i += 64) {
          const double dd = (double)dp[i];
          gw += dd * (((double)xp[i] - ms[0]) * ms[1]);
          gb += dd;
        }
      }
    }
  }
  gw = wave_sum(gw);
  gb = wave_sum(gb);
  if (ok && lane == 0 && srow) {
    srow[ch] = (float)gw;
    if (bias) srow[pad4(C) + ch] = (float)gb;
  }
  store_slot(ok ? gw * gw + (bias ? gb * gb : 0.0) : 0.0, part, work, slot);
}

// Workgroup (microbatch, workgroup of a layer). work == nullptr: no norm slots; stack == nullptr: no stack.
__global__ __launch_bounds__(kBlock) void k_dp_norm_grad(const nm_chunk c, int r, long long gbase,
                                                         const double* __restrict__ stats, long long slot0, long long slots,
                                                         double* __restrict__ work, float* __restrict__ stack, long long srow) {
  __shared__ d2 red[kWaves][kTile];
  __shared__ double part[kWaves];
  const uint32_t per = c.tfirst[c.n];
  const long long row = blockIdx.x / per;
  const uint32_t blk = blockIdx.x - (uint32_t)row * per;
  const int li = find_layer(c.tfirst, c.n, blk);
  const efl_dp_norm& L = c.v[li];
  const d2* st = reinterpret_cast<const d2*>(stats) + gbase + c.gfirst[li];
  float* sr = stack ? stack + row * srow + c.soff[li] : nullptr;
  const long long slot = row * slots + slot0 + blk;
  const bool vx = (c.vx >> li) & 1, vd = (c.vd >> li) & 1;
  if (L.kind == 0) grad_channel_last(L, vx, vd, r, row, blk - c.tfirst[li], st, red, part, work, slot, sr);
  else grad_channel_first(L, vx, vd, r, row, blk - c.tfirst[li], st, part, work, slot, sr);
}

long long layer_groups(const efl_dp_norm& L, long long B) { return B * (L.kind == 0 ? L.T_or_L : (long long)L.groups); }
long long layer_slots(const efl_dp_norm& L) { return L.kind == 0 ? (L.C + kTile - 1) / kTile : (L.C + kChan - 1) / kChan; }
long long layer_stack(const efl_dp_norm& L) { return pad4(L.C) * (L.b_out ? 2 : 1); }

// The checks the entry points share, before any HIP call. On success: the statistics groups, the norm
// slots per microbatch and the floats in a row of the stack.
int check_layers(const char* who, const efl_dp_norm* layers, int64_t nlayers, int64_t B, int64_t rows, long long* groups,
                 long long* slots, long long* srow) {
  constexpr int64_t kMax = 0x7fffffff;
  *groups = *slots = *srow = 0;
  if (nlayers < 0 || rows <= 0 || B <= 0 || B > kMax) { set_error("%s: nlayers must be >= 0, rows > 0 and 0 < B < 2^31", who); return EFL_E_INVALID_ARGUMENT; }
  if (B % rows != 0) { set_error("%s: rows (%lld) must divide B (%lld)", who, (long long)rows, (long long)B); return EFL_E_INVALID_ARGUMENT; }
  const int64_t r = B / rows;
  if (r > kMaxR) { set_error("%s: %lld examples per microbatch, at most %d", who, (long long)r, kMaxR); return EFL_E_INVALID_ARGUMENT; }
  if (nlayers == 0) return EFL_OK;
  if (!layers) { set_error("%s: null layer table", who); return EFL_E_INVALID_ARGUMENT; }
  for (int64_t i = 0; i < nlayers; ++i) {
    const efl_dp_norm& L = layers[i];
    const long long li = (long long)i;
    if (L.kind != 0 && L.kind != 1) { set_error("%s: layer %lld: kind must be 0 (channel-last) or 1 (channel-first)", who, li); return EFL_E_INVALID_ARGUMENT; }
    if (L.C < 1 || L.C > kMax || L.T_or_L < 1 || L.T_or_L > kMax) { set_error("%s: layer %lld: C and T_or_L in 1 .. 2^31 - 1", who, li); return EFL_E_INVALID_ARGUMENT; }
    if (L.groups < 1 || L.C % L.groups != 0 || (L.kind == 0 && L.groups != 1)) {
      set_error("%s: layer %lld: groups (%d) must divide C (%lld), and be 1 for the channel-last kind", who, li, (int)L.groups, (long long)L.C);
      return EFL_E_INVALID_ARGUMENT;
    }
    if (!(L.eps >= 0.0) || L.eps > 1.0e300) { set_error("%s: layer %lld: eps must be finite and >= 0", who, li); return EFL_E_INVALID_ARGUMENT; }
    if (!L.x || !L.d || !L.w_out) { set_error("%s: layer %lld: null buffer", who, li); return EFL_E_INVALID_ARGUMENT; }
    if (!aligned(L.x, 4) || !aligned(L.d, 4) || !aligned(L.w_out, 16) || !aligned(L.b_out, 16)) {
      set_error("%s: layer %lld: x and d must be 4-byte, w_out and b_out 16-byte aligned", who, li);
      return EFL_E_INVALID_ARGUMENT;
    }
    if (L.kind == 0 && (L.x_row_stride < L.C || L.d_row_stride < L.C)) {
      set_error("%s: layer %lld: a row stride (%lld, %lld) below C (%lld)", who, li, (long long)L.x_row_stride, (long long)L.d_row_stride, (long long)L.C);
      return EFL_E_INVALID_ARGUMENT;
    }
    if (L.kind == 1 && L.C / L.groups > kMax / L.T_or_L) { set_error("%s: layer %lld: a statistics group of 2^31 elements or more", who, li); return EFL_E_INVALID_ARGUMENT; }
    if (L.T_or_L > kMax / B || r * L.T_or_L > kMax) { set_error("%s: layer %lld: too many rows for one grid", who, li); return EFL_E_INVALID_ARGUMENT; }
    *groups += layer_groups(L, B);
    *slots += layer_slots(L);
    *srow += layer_stack(L);
    if (*groups > kMax || *slots > kMax / rows || *srow > INT64_MAX / 64 / rows) { set_error("%s: layers too large for one grid", who); return EFL_E_INVALID_ARGUMENT; }
  }
  return EFL_OK;
}

long long scratch_bytes(long long groups, long long rows, long long srow) { return 16 * groups + 4 * rows * srow; }

// fn(chunk, statistics groups before it, norm slots before it) for every run of at most kMaxLayers layers
template <class F>
void for_chunks(const efl_dp_norm* layers, int64_t nlayers, long long B, F fn) {
  long long gbefore = 0, sbefore = 0, soff = 0;
  for (int64_t i0 = 0; i0 < nlayers; i0 += kMaxLayers) {
    nm_chunk c;
    long long groups = 0, slots = 0;
    c.n = (int)(nlayers - i0 < kMaxLayers ? nlayers - i0 : kMaxLayers);
    c.vs = c.vx = c.vd = 0;
    for (int i = 0; i < c.n; ++i) {
      const efl_dp_norm& L = layers[i0 + i];
      c.v[i] = L;
      c.gfirst[i] = (uint32_t)groups;
      c.tfirst[i] = (uint32_t)slots;
      c.soff[i] = soff;
      const bool cl = L.kind == 0;
      if (aligned(L.x, 16) && (cl ? L.x_row_stride : L.C / L.groups * L.T_or_L) % 4 == 0) c.vs |= 1u << i;
      if (aligned(L.x, 16) && (cl ? L.x_row_stride : L.T_or_L) % 4 == 0) c.vx |= 1u << i;
      if (aligned(L.d, 16) && (cl ? L.d_row_stride : L.T_or_L) % 4 == 0) c.vd |= 1u << i;
      groups += layer_groups(L, B);
      slots += layer_slots(L);
      soff += layer_stack(L);
    }
    c.gfirst[c.n] = (uint32_t)groups;
    c.tfirst[c.n] = (uint32_t)slots;
    fn(c, gbefore, sbefore);
    gbefore += groups;
    sbefore += slots;
  }
}

// the statistics, then every microbatch's gradients: norm slots into `work` (or none), rows into `stack` (or none)
void launch(const efl_dp_norm* layers, int64_t nlayers, int64_t B, int64_t rows, double* work, long long slot0,
            long long slots, double* stats, float* stack, long long srow, hipStream_t s) {
  const int r = (int)(B / rows);
  for_chunks(layers, nlayers, B, [&](const nm_chunk& c, long long gbefore, long long sbefore) {
    k_dp_norm_stats<<<(c.gfirst[c.n] + kWaves - 1) / kWaves, kBlock, 0, s>>>(c, gbefore, stats);
    k_dp_norm_grad<<<(unsigned)(rows * c.tfirst[c.n]), kBlock, 0, s>>>(c, r, gbefore, stats, slot0 + sbefore, slots, work,
                                                                      stack, srow);
  });
}

bool scratch_ok(const void* scratch, int64_t bytes, long long need) { return scratch && aligned(scratch, 16) && bytes >= need; }

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API int64_t efl_dp_norm_work_elems(const efl_dp_norm* layers, int64_t nlayers, int64_t B, int64_t rows) {
  long long groups, slots, srow;
  const int rc = check_layers("efl_dp_norm_work_elems", layers, nlayers, B, rows, &groups, &slots, &srow);
  return rc != EFL_OK ? rc : rows * slots;
}

EFL_API int64_t efl_dp_norm_scratch_bytes(const efl_dp_norm* layers, int64_t nlayers, int64_t B, int64_t rows) {
  long long groups, slots, srow;
  const int rc = check_layers("efl_dp_norm_scratch_bytes", layers, nlayers, B, rows, &groups, &slots, &srow);
  return rc != EFL_OK ? rc : scratch_bytes(groups, rows, srow);
}

EFL_API int efl_dp_norm_sqnorm(const efl_dp_norm* layers, int64_t nlayers, int64_t B, int64_t rows, double* work,
                               int64_t slot0, int64_t slots, void* scratch, int64_t scratch_bytes_, void* stream) {
  const char* who = "efl_dp_norm_sqnorm";
  long long groups, own, srow;
  const int rc = check_layers(who, layers, nlayers, B, rows, &groups, &own, &srow);
  if (rc != EFL_OK) return rc;
  if (nlayers == 0) return EFL_OK;
  if (!work || !aligned(work, 8) || slot0 < 0 || slots > INT64_MAX / 16 / rows || slot0 > slots - own) {
    set_error("%s: work must hold rows x slots doubles with the layers' %lld slots in [slot0, slots)", who, own);
    return EFL_E_INVALID_ARGUMENT;
  }
  if (!scratch_ok(scratch, scratch_bytes_, scratch_bytes(groups, rows, srow))) {
    set_error("%s: scratch must hold efl_dp_norm_scratch_bytes() = %lld bytes, 16-byte aligned, got %lld", who, scratch_bytes(groups, rows, srow), (long long)scratch_bytes_);
    return EFL_E_INVALID_ARGUMENT;
  }
  launch(layers, nlayers, B, rows, work, slot0, slots, static_cast<double*>(scratch), nullptr, 0, (hipStream_t)stream);
  return hip_status(hipGetLastError(), who);
}

EFL_API int efl_dp_norm_clip_sum(const efl_dp_norm* layers, int64_t nlayers, int64_t B, int64_t rows, int clip_mode,
                                 float l2_norm_clip, int mode, float sigma, float divisor, uint64_t seed, float* scales,
                                 double* work, int64_t work_elems, void* scratch, int64_t scratch_bytes_, void* stream) {
  const char* who = "efl_dp_norm_clip_sum";
  if (clip_mode < 0 || clip_mode > 2) { set_error("%s: clip_mode must be 0 (none), 1 (from the norms) or 2 (given scales)", who); return EFL_E_INVALID_ARGUMENT; }
  if (mode < 0 || mode > 1) { set_error("%s: mode must be 0 (element-wise) or 1 (Gaussian sum)", who); return EFL_E_INVALID_ARGUMENT; }
  if (!(divisor == divisor) || divisor == 0.0f) { set_error("%s: divisor must be non-zero", who); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode == 1 && !(l2_norm_clip > 0.0f)) { set_error("%s: l2_norm_clip must be positive", who); return EFL_E_INVALID_ARGUMENT; }
  long long groups, slots, srow;
  const int rc = check_layers(who, layers, nlayers, B, rows, &groups, &slots, &srow);
  if (rc != EFL_OK) return rc;
  if (nlayers == 0) return EFL_OK;
  if (clip_mode != 0 && (!scales || !aligned(scales, 4))) { set_error("%s: clip modes 1 and 2 need a scales buffer", who); return EFL_E_INVALID_ARGUMENT; }
  if (clip_mode == 1 && (!work || !aligned(work, 8) || work_elems < rows * slots)) {
    set_error("%s: work must hold efl_dp_norm_work_elems() = %lld doubles, got %lld", who, (long long)(rows * slots), (long long)work_elems);
    return EFL_E_INVALID_ARGUMENT;
  }
  if (!scratch_ok(scratch, scratch_bytes_, scratch_bytes(groups, rows, srow))) {
    set_error("%s: scratch must hold efl_dp_norm_scratch_bytes() = %lld bytes, 16-byte aligned, got %lld", who, scratch_bytes(groups, rows, srow), (long long)scratch_bytes_);
    return EFL_E_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  double* stats = static_cast<double*>(scratch);
  float* stack = reinterpret_cast<float*>(static_cast<char*>(scratch) + 16 * groups);
  launch(layers, nlayers, B, rows, clip_mode == 1 ? work : nullptr, 0, slots, stats, stack, srow, s);
  if (clip_mode == 1) k_dp_scales<<<(unsigned)rows, 64, 0, s>>>(work, slots, (double)l2_norm_clip, scales);
  const int e = hip_status(hipGetLastError(), who);
  if (e != EFL_OK) return e;
  std::vector<efl_dp_var> vars;
  long long soff = 0;
  for (int64_t i = 0; i < nlayers; ++i) {
    const efl_dp_norm& L = layers[i];
    vars.push_back(efl_dp_var{stack + soff, L.w_out, L.C, srow, L.ctr0_w});
    if (L.b_out) vars.push_back(efl_dp_var{stack + soff + pad4(L.C), L.b_out, L.C, srow, L.ctr0_b});
    soff += layer_stack(L);
  }
  // the stacked rows in order with their scales, the noise and the divide: one launch over every variable
  return efl_dp_clip_sum(vars.data(), (int64_t)vars.size(), rows, clip_mode == 0 ? 0 : 2, 0.0f, mode, sigma, divisor, seed,
                         scales, nullptr, 0, stream);
}
