// RSA blind-signature PSI, the kernels (efl.psi; reference: efls-data/xfl/data/psi/rsa_signer.py,
// one gmpy2.powmod(x, d, n) per ID on the server, powmod(r, e, n) * x and divm(s, r, n) on the client,
// sha256 as the full-domain hash).
//
// k_rsa_sign: s = x^d mod N by CRT, an element's number mod p (then mod q) spread over G lanes in
// radix 2^28 exactly as the Paillier decryption's number mod p^2 is (csrc/sliced28.h; one 64-lane wave
// per workgroup, E = 64 / G elements per wave): x mod p -> x R28 -> x^dp by left-to-right sliding
// windows over the element's odd powers in a stream-ordered scratch slab -> sp; the same for q; then
// Garner's join h = (sp - sq) (q^-1 mod p) mod p, s = h q + sq at full width. dp and dq are the same
// for every element, so the window walk is wave-uniform. Squarings are those of the decryption of the
// same width: product scanning in one lane (sqr_fips1), SOS over two lanes (sos_sqr), CIOS for the
// short slices.
//
// The exponent walk is NOT constant-time: its sequence of squarings and multiplies, and the table
// entries it loads, follow the bits of dp and dq (as the reference's gmpy2.powmod does). The signer
// is a batch service on the key owner's own machine; it is no defence against a co-tenant who can
// time the GPU.
//
// k_rsa_blind: out = r^e h mod N, binary square-and-multiply over the public exponent (up to 64
// bits) in the 32-bit sliced arithmetic of csrc/sliced.h; with e = 1 it is the product s r^-1 of the
// unblinding (rsaset.hip composes it with the batched inversion of paillier.hip).
// k_sha256_fdh: FIPS 180-4 SHA-256 of n packed byte strings, one lane per string, the digest as the
// low 8 words of a row.
#include "powm28.h"
#include "rsa.h"
#include "sha256.h"
#include "sliced.h"
#include "sliced28.h"

namespace efl {
namespace rsa {
namespace {

using namespace sl;
using s28::kEntries;
using s28::pad4;

constexpr int kWave = 64;
// elements per launch (the slab holds kEntries + 1 numbers for each)
constexpr long long kChunk = 1 << 18;

// C 32-bit words per lane of a number mod p (L = C G words); rows of x and s have k.W words, 2 L
// (balanced primes) or L (p or q longer than half of N's class: the high half of x is absent)
template <int C, int G>
__global__ __launch_bounds__(kWave, C >= 32 ? 2 : 4) void k_rsa_sign(Key k, const uint32_t* x, uint32_t* out,
                                                                     long long N, uint32_t* win) {
  constexpr int L = C * G, E = kWave / G;
  constexpr int C28 = s28::limbs_per_lane(L, G), L28 = C28 * G, CP = pad4<C28>();
  constexpr bool kSos = G == 2 && C == 32 && EFL_SQR_SOS;
  extern __shared__ uint32_t lds[];
  const int g = (int)threadIdx.x % G;
  const int e = (int)threadIdx.x / G;
  const long long i = (long long)blockIdx.x * E + e;
  if (i >= N) return;
  uint32_t* BASE = lds + e;
  uint32_t* SCR = lds + L28 * E + e;            // contiguous with BASE: word L28 + w of BASE is word w of SCR
  const bool wide = k.W == 2 * L;
  const uint32_t* xi = x + i * k.W;
  // this lane's slice of the element's slab: kEntries odd powers (p's, then reused for q's) and sp
  uint32_t* slot = win + (size_t)i * (kEntries + 1) * G * CP + g * CP;
  uint32_t* keep = slot + (size_t)kEntries * G * CP;
  uint32_t sq[C];
#pragma unroll 1
  for (int second = 0; second < 2; ++second) {
    const Prime& p0 = k.pr[0];
    const Prime& p1 = k.pr[1];
    const uint32_t minv = second ? p1.minv : p0.minv;
    const uint32_t minv28 = second ? p1.minv28 : p0.minv28;
    const uint32_t* r2 = k.at(second ? p1.off_r2 : p0.off_r2);
    uint32_t t[C];
    {
      // x mod m, x = hi R + lo, R = 2^(32 L): hi R mod m = mont(hi, R^2); lo mod m = redc(mont(lo, R^2))
      uint32_t m[C], lo[C];
      slice_uniform<C>(m, k.at(second ? p1.off_x : p0.off_x), g);
      load_slice<C>(lo, xi, g);
      sl::mont_mul<C, G>(lo, Uniform{r2}, m, minv, g);
      sl::redc<C, G>(lo, m, minv, g);
      if (wide) {
        load_slice<C>(t, xi + L, g);
        sl::mont_mul<C, G>(t, Uniform{r2}, m, minv, g);
        const uint32_t top = sl::add<C, G>(t, lo, g);
        sl::csub<C, G>(t, m, top != 0 || sl::geq<C, G>(t, m, g), g);
      } else {
#pragma unroll
        for (int j = 0; j < C; ++j) t[j] = lo[j];
      }
    }
    to_lds<C>(SCR, E, g, t);
    lds_sync();
    // keep the 32-bit constants above from being held in VGPRs across the exponentiation
    asm volatile("" ::: "memory");
    uint32_t a[C28], m28[C28];
    s28::from_words<C28>(a, SCR, E, L, g);
    slice_uniform<C28>(m28, k.at(second ? p1.off_x28 : p0.off_x28), g);
    lds_sync();
    s28::mont_mul<C28, G>(a, Uniform{k.at(second ? p1.off_r2_28 : p0.off_r2_28)}, m28, minv28, g);   // x R28
    lds_sync();
    s28::powm_window<C28, G, kSos>(a, slot, k.at(second ? p1.off_dx : p0.off_dx), second ? p1.dbits : p0.dbits, BASE,
                                   SCR, E, m28, minv28, g);
    s28::mont_mul<C28, G>(a, Unit{}, m28, minv28, g);   // x^dx mod m, fully reduced
    lds_sync();
    to_lds<C28>(SCR, E, g, a);
    lds_sync();
    s28::to_words<C>(sq, SCR, E, L28, g);
    lds_sync();
    if (!second) store_slice<C>(keep, 0, sq);             // sp waits in the slab
  }
  asm volatile("" ::: "memory");
  // Garner: h = (sp - sq) (q^-1 mod p) mod p; s = h q + sq. sq < q may exceed p (p < q, or a q
  // longer than p): it is reduced mod p first, as hi and lo were.
  uint32_t ph[C], d[C], r[C];
  slice_uniform<C>(ph, k.at(k.pr[0].off_x), g);
  const uint32_t p_minv = k.pr[0].minv;
#pragma unroll
  for (int j = 0; j < C; ++j) d[j] = sq[j];
  sl::mont_mul<C, G>(d, Uniform{k.at(k.pr[0].off_r2)}, ph, p_minv, g);
  sl::redc<C, G>(d, ph, p_minv, g);                        // sq mod p
  load_slice<C>(r, keep, 0);                               // sp
  if (sl::sub<C, G>(r, d, g)) sl::add<C, G>(r, ph, g);
  sl::mont_mul<C, G>(r, Uniform{k.at(k.off_qinvp)}, ph, p_minv, g);   // h (< p, normal form)
  // s = h q + sq by operand scanning over the words of h (in SCR); low words leave lane 0 into
  // BASE, the high half follows them there (past L28 words it lies over the words of h already read)
  lds_sync();
  to_lds<C>(SCR, E, g, r);
  lds_sync();
  uint32_t qh[C], t[C];
  slice_uniform<C>(qh, k.at(k.pr[1].off_x), g);
#pragma unroll
  for (int j = 0; j < C; ++j) t[j] = sq[j];
  scan_mul_add<C, G>(t, qh, SCR, BASE, E, g);
  if (wide) {
    uint32_t o[2 * C];
    from_lds<2 * C>(o, BASE, E, g);
    store_slice<2 * C>(out + i * 2 * L, g, o);
  } else {
    uint32_t o[C];                                         // s < N < 2^(32 L): the high half is zero
    from_lds<C>(o, BASE, E, g);
    store_slice<C>(out + i * L, g, o);
  }
}

// out = r^ex h mod N (ex >= 1), numbers of L = C G = k.W words over G lanes in 32-bit limbs. h and
// r may be any W-word values: a product with an operand below N is below 2 N before its subtraction
template <int C, int G>
__global__ __launch_bounds__(kWave) void k_rsa_blind(Key k, const uint32_t* h, const uint32_t* r,
                                                     uint64_t ex, uint32_t* out, long long N) {
  constexpr int L = C * G, E = kWave / G;
  extern __shared__ uint32_t lds[];
  const int g = (int)threadIdx.x % G;
  const int e = (int)threadIdx.x / G;
  const long long i = (long long)blockIdx.x * E + e;
  if (i >= N) return;
  uint32_t* BASE = lds + e;
  uint32_t* SCR = lds + L * E + e;
  uint32_t n[C], t[C];
  slice_uniform<C>(n, k.at(k.off_n), g);
  const uint32_t minv = k.n_minv;
  load_slice<C>(t, r + i * L, g);
  sl::mont_mul<C, G>(t, Uniform{k.at(k.off_n_r2)}, n, minv, g);   // r R mod N
  to_lds<C>(BASE, E, g, t);
  lds_sync();
  const int ebits = 64 - __clzll((long long)ex);
#pragma unroll 1
  for (int b = ebits - 2; b >= 0; --b) {
    sl::mont_sqr<C, G>(t, SCR, E, n, minv, g);
    if ((ex >> b) & 1ull) sl::mont_mul<C, G>(t, LdsElem{BASE, E}, n, minv, g);
    lds_sync();
  }
  lds_sync();
  to_lds<C>(SCR, E, g, t);                                        // r^e R mod N
  lds_sync();
  load_slice<C>(t, h + i * L, g);
  sl::mont_mul<C, G>(t, LdsElem{SCR, E}, n, minv, g);             // h r^e mod N
  store_slice<C>(out + i * L, g, t);
}

// ---- SHA-256 full-domain hash (the compression is sha256.h's) ---------------------------------------
// row i of out = int(sha256(string i).hexdigest(), 16): the digest is a big-endian number, so word
// j (little-endian) is state word H[7 - j]; words 8 .. wpr - 1 are zero. One lane per string; any
// length.
__global__ __launch_bounds__(256) void k_sha256_fdh(const char* __restrict__ chars,
                                                    const long long* __restrict__ offsets,
                                                    uint32_t* __restrict__ out, int wpr, long long N) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const unsigned char* s = reinterpret_cast<const unsigned char*>(chars) + offsets[i];
  const long long len = offsets[i + 1] - offsets[i];
  uint32_t H[8];
  sha256::digest(H, len, [s](long long p) { return s[p]; });
  uint32_t* o = out + i * wpr;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = H[7 - j];
  for (int j = 8; j < wpr; ++j) o[j] = 0u;
}

inline unsigned grid_of(long long N, int G) {
  const long long E = kWave / G;
  return (unsigned)((N + E - 1) / E);
}

template <int C, int G>
hipError_t run_sign(const Key& k, const uint32_t* x, uint32_t* s, long long N, hipStream_t st) {
  constexpr int L = C * G, C28 = s28::limbs_per_lane(L, G);
  constexpr size_t slab = (size_t)(kEntries + 1) * G * pad4<C28>();
  const size_t lds = (size_t)(2 * C28 * G) * (kWave / G) * 4;
  const long long chunk = N < kChunk ? N : kChunk;
  uint32_t* win = nullptr;
  hipError_t err = hipMallocAsync(reinterpret_cast<void**>(&win), (size_t)chunk * slab * 4, st);
  if (err != hipSuccess) return err;
  for (long long o = 0; o < N && err == hipSuccess; o += chunk) {
    const long long n = N - o < chunk ? N - o : chunk;
    hipLaunchKernelGGL((k_rsa_sign<C, G>), dim3(grid_of(n, G)), dim3(kWave), lds, st, k, x + o * k.W, s + o * k.W, n,
                       win);
    err = hipGetLastError();
  }
  const hipError_t ferr = hipFreeAsync(win, st);
  return err == hipSuccess ? ferr : err;
}

template <int C, int G>
hipError_t run_blind(const Key& k, const uint32_t* h, const uint32_t* r, uint64_t e, uint32_t* out, long long N,
                     hipStream_t st) {
  const size_t lds = (size_t)(2 * C * G) * (kWave / G) * 4;
  hipLaunchKernelGGL((k_rsa_blind<C, G>), dim3(grid_of(N, G)), dim3(kWave), lds, st, k, h, r, e, out, N);
  return hipGetLastError();
}

}  // namespace

int sign_limbs28(int L) {
  const int G = sign_lanes(L);
  return s28::limbs_per_lane(L, G) * G;
}

hipError_t sign(const Key& k, const uint32_t* x, uint32_t* s, long long n, hipStream_t st) {
  switch (k.L) {
    case 16: return run_sign<8, 2>(k, x, s, n, st);
    case 32: return run_sign<32, 1>(k, x, s, n, st);
    case 64: return run_sign<32, 2>(k, x, s, n, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t blind(const Key& k, const uint32_t* h, const uint32_t* r, uint64_t e, uint32_t* out, long long n,
                 hipStream_t st) {
  if (e == 0) return hipErrorInvalidValue;
  switch (k.W) {
    case 32: return run_blind<32, 1>(k, h, r, e, out, n, st);
    case 64: return run_blind<32, 2>(k, h, r, e, out, n, st);
    case 128: return run_blind<32, 4>(k, h, r, e, out, n, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t sha256_fdh(const char* chars, const long long* offsets, uint32_t* out, int words_per_row, long long n,
                      hipStream_t st) {
  hipLaunchKernelGGL(k_sha256_fdh, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, chars, offsets, out,
                     words_per_row, n);
  return hipGetLastError();
}

}  // namespace rsa
}  // namespace efl
