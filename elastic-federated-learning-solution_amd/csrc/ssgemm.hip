// The products of the secret-sharing matmul (efls-train/python/efl/privacy/secret_sharing.py
// _matmul, :30-77) as ONE kernel: z[R, N] = sum_t s_t * A_t[R, K_t] @ B_t[K_t, N] for up to 8 terms.
// A mode-C forward is five products into one [R, N] result,
//   z = a@b + (a - e)@b1' + (e_odd - e_even)@f1' + a1'@(b/2 + f) - e1'@(f_odd + f_even),
// over operands that are slices and transposes of a few tensors (the received one is cut four
// ways). As library GEMMs that is five launches, two additions and copies of the transposed
// slices; here it is one GEMM over the concatenated inner dimension whose operands are strided
// views, read where they lie.
//
// Design (gfx950, fp32 MFMA):
//  * v_mfma_f32_32x32x2_f32: one wave owns a 32x32 block of z in 16 accumulator VGPRs. Lane l gives
//    A[i = l % 32][k = l / 32] and B[k = l / 32][j = l % 32]; accumulator register v of lane l is
//    D[8 (v / 4) + 4 (l / 32) + v % 4][l % 32] (the CDNA ISA guide's 32x32x2 layout; the asymmetric
//    shapes of tests/test_ss_products_gpu.py fail on any other).
//  * Two instances: 256 lanes (2 x 2 waves) on a 64x64 tile in k steps of 32, and one wave on a
//    32x32 tile in k steps of 64 for a result that fits one such tile (the host picks; see there).
//  * The terms run back to back as one long K in those steps; each term is padded to whole steps
//    with zeros as it is staged, so K_t may be odd or 0. The accumulators stay in registers from
//    the first term to the last, and the sign of a term is applied to its A elements on the way
//    into LDS (a negation: exact).
//  * global -> registers -> LDS -> MFMA fragments, double-buffered: the global loads of step s + 1
//    are issued before the MFMAs of step s and land in the other LDS buffer after them; one
//    barrier per step.
//  * Strides. Each operand is a view with a row and a column stride. The lanes of a staging pass
//    run along the dimension whose stride is 1 (k for a row-major A, m for its transpose; n for a
//    row-major B, k for its transpose), so a plain view and a transposed one both load in
//    contiguous runs (16 floats along k, 32 or 64 along m / n). Element offsets are 32-bit when
//    every view is shorter than 2^31 elements (the host checks), 64-bit otherwise. Other strides load correctly,
//    uncoalesced.
//  * LDS is k-major: As[k][m], Bs[k][n], row length LD, element (k, x) at k LD + (x ^ 4 ((k / 2) % 8)).
//    A fragment read takes 32 consecutive x of row k (lanes 0-31) and of row k + 1 (lanes 32-63),
//    k even. LD = 32 for the 32-wide tile and 64 + 32 = 96 for the 64-wide one, so that LD % 64 == 32:
//    the two rows fall on the two different halves of 64 banks (with 32 banks a half wave is a
//    pass, conflict-free for any LD). The XOR permutes x inside its aligned group of 32, the same
//    for rows k and k + 1, so reads stay conflict-free, and it spreads the k-contiguous staging
//    pass (16 k x 4 x per wave, which would hit 8 banks 8 ways) over 64 different banks: the 8 row
//    pairs take 8 different groups of 4 and the two parities of k the two halves.
//  * Edges: rows >= R, columns >= N and k >= K_t are staged as zeros and never stored.
//  * No split-K, no atomics, no lane waits for another: the same inputs give the same bytes.
#include "common.h"

namespace efl {
namespace {

typedef float acc16 __attribute__((ext_vector_type(16)));


struct ss_args {
  efl_ss_term t[EFL_SS_MAX_TERMS];
  float* z;
  long long zrs;
  int R, N, count, tiles_n;
};

constexpr int lds_row(int tile) { return tile % 64 == 32 ? tile : tile + 32; }   // LD % 64 == 32

__device__ __forceinline__ int lds_at(int k, int x, int ld) { return k * ld + (x ^ (((k >> 1) & 7) << 2)); }

// Element e of a staging pass over a [KS][T] tile: lanes along x (the m or n of the tile) when
// that dimension has stride 1; otherwise along k in runs of 16, one [16][T] slab after the other,
// so that a wave's pass is the 16 k x 4 x the XOR of lds_at spreads over all banks.
template <int T>
__device__ __forceinline__ void tile_pos(int e, bool along_x, int& k, int& x) {
  if (along_x) { x = e % T; k = e / T; }
  else { k = e / (16 * T) * 16 + e % 16; x = e % (16 * T) / 16; }
}

// KS: k per staged step (KS / 2 MFMAs of 32x32x2 per wave between two barriers). OFF: the type of
// an element offset inside a view: int when the host found every view shorter than 2^31 elements
// (two 32-bit multiplies per load), long long otherwise (the 64-bit products cost about 80 VALU
// instructions per load and bound the kernel: measured 188 us against 144 us at 256 x 392 x 10, 32x32 tile).
template <int WM, int WN, int KS, class OFF>
__global__ __launch_bounds__(64 * WM * WN) void k_ss_products(const ss_args g) {
  constexpr int TM = 32 * WM, TN = 32 * WN, NT = 64 * WM * WN, kStep = KS;
  constexpr int LDA = lds_row(TM), LDB = lds_row(TN);
  constexpr int EA = TM * kStep / NT, EB = TN * kStep / NT;   // staged elements per lane
  __shared__ float As[2][kStep * LDA];
  __shared__ float Bs[2][kStep * LDB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int bm = blockIdx.x / g.tiles_n, bn = blockIdx.x - bm * g.tiles_n;
  const long long m0 = (long long)bm * TM, n0 = (long long)bn * TN;

  // (t, k0): the term and the k offset inside it of a step; empty terms are passed over
  int t = 0;
  long long k0 = 0;
  auto settle = [&]() {
    while (t < g.count && k0 >= g.t[t].k) { ++t; k0 = 0; }
  };
  settle();

  // load() only issues loads: every index is clamped into the view, so each load is in bounds and
  // unconditional, and nothing reads ra / rb before stage(), which zeroes the elements outside the
  // edges and applies the sign, so the wave never waits on a load while it still has loads to issue.
  float ra[EA], rb[EB];
  bool a_along_m = false, b_along_n = false, neg = false;   // of the step held in ra / rb,
  long long hk0 = 0, hK = 0;                                // with its k offset and its term's K
  auto load = [&]() {
    const efl_ss_term& T = g.t[t];
    a_along_m = T.a_rs == 1;
    b_along_n = T.b_cs == 1;
    neg = T.sign < 0;
    hk0 = k0;
    hK = T.k;
    // last row, column and k of this tile and step that lie inside the views (uniform)
    const int mlim = (int)min((long long)g.R - 1 - m0, (long long)TM - 1);
    const int nlim = (int)min((long long)g.N - 1 - n0, (long long)TN - 1);
    const int klim = (int)min(hK - 1 - k0, (long long)kStep - 1);
    const OFF ars = (OFF)T.a_rs, acs = (OFF)T.a_cs, brs = (OFF)T.b_rs, bcs = (OFF)T.b_cs;
#pragma unroll
    for (int j = 0; j < EA; ++j) {
      int kk, m;
      tile_pos<TM>(tid + j * NT, a_along_m, kk, m);
      ra[j] = T.a[((OFF)m0 + min(m, mlim)) * ars + ((OFF)k0 + min(kk, klim)) * acs];
    }
#pragma unroll
    for (int j = 0; j < EB; ++j) {
      int kk, n;
      tile_pos<TN>(tid + j * NT, b_along_n, kk, n);
      rb[j] = T.b[((OFF)k0 + min(kk, klim)) * brs + ((OFF)n0 + min(n, nlim)) * bcs];
    }
    k0 += kStep;
    settle();
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int j = 0; j < EA; ++j) {
      int kk, m;
      tile_pos<TM>(tid + j * NT, a_along_m, kk, m);
      const float v = (m0 + m < g.R && hk0 + kk < hK) ? ra[j] : 0.0f;
      As[buf][lds_at(kk, m, LDA)] = neg ? -v : v;
    }
#pragma unroll
    for (int j = 0; j < EB; ++j) {
      int kk, n;
      tile_pos<TN>(tid + j * NT, b_along_n, kk, n);
      Bs[buf][lds_at(kk, n, LDB)] = (n0 + n < g.N && hk0 + kk < hK) ? rb[j] : 0.0f;
    }
  };

  acc16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.0f;

  if (t < g.count) {
    load();
    stage(0);
    __syncthreads();
    int cur = 0;
    for (;;) {
      const bool more = t < g.count;   // uniform over the workgroup
      if (more) load();                // the next step's global loads travel under the MFMAs
#pragma unroll
      for (int kk = 0; kk < kStep; kk += 2) {
        const int kr = kk + (lane >> 5);
        const float a = As[cur][lds_at(kr, wm * 32 + (lane & 31), LDA)];
        const float b = Bs[cur][lds_at(kr, wn * 32 + (lane & 31), LDB)];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
      }
      if (!more) break;
      stage(cur ^ 1);    // last read before the barrier that ended the previous step
      __syncthreads();
      cur ^= 1;
    }
  }

  const long long col = n0 + wn * 32 + (lane & 31);
  if (col < g.N) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const long long row = m0 + wm * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
      if (row < g.R) g.z[row * g.zrs + col] = acc[v];
    }
  }
}

// Byte range [lo, hi) of a [rows, cols] float view; false when it does not fit 2^62 bytes.
// *narrow is cleared when an element offset of the view does not fit an int.
bool view_range(const float* p, long long rows, long long cols, long long rs, long long cs, uintptr_t* lo,
                uintptr_t* hi, bool* narrow) {
  const __int128 last = (__int128)(rows - 1) * rs + (__int128)(cols - 1) * cs;
  if (last >= ((__int128)1 << 60)) return false;
  if (last > 0x7fffffff) *narrow = false;
  *lo = reinterpret_cast<uintptr_t>(p);
  *hi = *lo + ((uintptr_t)last + 1) * sizeof(float);
  return *hi >= *lo;
}

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API int efl_ss_products(const efl_ss_term* terms, int count, float* z, int64_t z_row_stride, int64_t rows,
                            int64_t cols, int tile, void* stream) {
  constexpr int64_t kMax = 0x7fffffff;
  if (count < 0 || count > EFL_SS_MAX_TERMS) {
    set_error("efl_ss_products: 0 to %d terms, got %d", EFL_SS_MAX_TERMS, count);
    return EFL_E_INVALID_ARGUMENT;
  }
  if (rows < 0 || cols < 0 || rows > kMax || cols > kMax) {
    set_error("efl_ss_products: result [%lld, %lld] outside 0 .. 2^31 - 1", (long long)rows, (long long)cols);
    return EFL_E_INVALID_ARGUMENT;
  }
  if (tile != 0 && tile != 32 && tile != 64) {
    set_error("efl_ss_products: tile must be 0 (chosen here), 32 or 64, got %d", tile);
    return EFL_E_INVALID_ARGUMENT;
  }
  if (count > 0 && !terms) { set_error("efl_ss_products: null term list"); return EFL_E_INVALID_ARGUMENT; }
  for (int i = 0; i < count; ++i) {
    if (terms[i].k < 0 || terms[i].k > kMax) {
      set_error("efl_ss_products: term %d: inner dimension %lld outside 0 .. 2^31 - 1", i, (long long)terms[i].k);
      return EFL_E_INVALID_ARGUMENT;
    }
    if (terms[i].sign != 1 && terms[i].sign != -1) {
      set_error("efl_ss_products: term %d: sign must be +1 or -1, got %d", i, terms[i].sign);
      return EFL_E_INVALID_ARGUMENT;
    }
  }
  if (rows == 0 || cols == 0) return EFL_OK;
  if (!z) { set_error("null buffer"); return EFL_E_INVALID_ARGUMENT; }
  if (z_row_stride < cols) {
    set_error("efl_ss_products: row stride of z (%lld) below its width (%lld)", (long long)z_row_stride, (long long)cols);
    return EFL_E_INVALID_ARGUMENT;
  }
  uintptr_t zlo, zhi;
  bool narrow = true, znarrow = true;
  if (!view_range(z, rows, cols, z_row_stride, 1, &zlo, &zhi, &znarrow)) {
    set_error("efl_ss_products: z too large");
    return EFL_E_INVALID_ARGUMENT;
  }
  ss_args g;
  g.count = 0;
  for (int i = 0; i < count; ++i) {
    const efl_ss_term& T = terms[i];
    if (T.k == 0) continue;   // contributes nothing; its pointers are not looked at
    if (!T.a || !T.b) { set_error("efl_ss_products: term %d: null operand", i); return EFL_E_INVALID_ARGUMENT; }
    if (T.a_rs < 1 || T.a_cs < 1 || T.b_rs < 1 || T.b_cs < 1) {
      set_error("efl_ss_products: term %d: strides must be positive", i);
      return EFL_E_INVALID_ARGUMENT;
    }
    uintptr_t lo, hi;
    if (!view_range(T.a, rows, T.k, T.a_rs, T.a_cs, &lo, &hi, &narrow) || (lo < zhi && zlo < hi) ||
        !view_range(T.b, T.k, cols, T.b_rs, T.b_cs, &lo, &hi, &narrow) || (lo < zhi && zlo < hi)) {
      set_error("efl_ss_products: term %d: an operand overlaps z (or spans more than 2^62 bytes)", i);
      return EFL_E_INVALID_ARGUMENT;
    }
    g.t[g.count++] = T;
  }
  g.z = z;
  g.zrs = z_row_stride;
  g.R = (int)rows;
  g.N = (int)cols;

  // The one-wave tile only where a 32x32 tile holds the whole result. Spreading a small result
  // over four times as many CUs with it did not pay: at 256 x {10, 64, 256} (8 to 64 one-wave
  // workgroups against 4 to 16 of four waves) the 64x64 tile ran in 105 us and the 32x32 one in
  // 144 us, both bound by the serial walk of K in a workgroup, which four waves stage faster.
  const int T = tile ? tile : (rows <= 32 && cols <= 32 ? 32 : 64);
  const long long tn = (cols + T - 1) / T, tiles = ((rows + T - 1) / T) * tn;
  if (tiles > kMax) { set_error("efl_ss_products: result too large for one launch"); return EFL_E_INVALID_ARGUMENT; }
  g.tiles_n = (int)tn;
  hipStream_t s = (hipStream_t)stream;
  if (T == 64 && narrow) k_ss_products<2, 2, 32, int><<<(unsigned)tiles, 256, 0, s>>>(g);
  else if (T == 64) k_ss_products<2, 2, 32, long long><<<(unsigned)tiles, 256, 0, s>>>(g);
  else if (narrow) k_ss_products<1, 1, 64, int><<<(unsigned)tiles, 64, 0, s>>>(g);
  else k_ss_products<1, 1, 64, long long><<<(unsigned)tiles, 64, 0, s>>>(g);
  return hip_status(hipGetLastError(), "efl_ss_products");
}
