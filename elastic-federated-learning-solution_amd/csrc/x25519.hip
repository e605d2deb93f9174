// ECDH PSI (efl.psi.EccSigner): batched X25519 with one scalar for the whole batch, what the
// reference's efls-data/xfl/data/psi/ecc_signer.py does one ID at a time through
// python-curve25519-donna, and the C ABI efl_x25519 / efl_x25519_hash (include/efl_hip.h).
//
// k_x25519 runs one element per lane: the field arithmetic and the ladder are fe25519.h, plain C++
// that the host test compiles too. The clamped scalar travels as eight 32-bit kernel arguments, so
// each ladder step's bit is wave-uniform; the conditional swap is by mask and no branch or address
// depends on the scalar beyond the uniform loop. u is public. No LDS, no scratch.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "fe25519.h"
#include "sha256.h"

namespace efl {
namespace {

constexpr int kMaxPrefix = 64;           // bytes of efl_x25519_hash's prefix, carried as kernel arguments
constexpr long long kChunk = 1ll << 30;  // rows per launch (a grid of 2^22 blocks)

struct Prefix {
  uint32_t w[kMaxPrefix / 4];            // little-endian: byte p is (w[p / 4] >> 8 (p % 4)) & 255
  int32_t len;
};

// out[i] = X25519(k, u[i]) on rows of 8 little-endian words, 16-byte aligned; out may be u (a lane
// reads its own row before it writes it, and touches no other)
__global__ __launch_bounds__(kBlock) void k_x25519(fe::Scalar k, const uint32_t* u, uint32_t* out, long long N) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const uint4* src = reinterpret_cast<const uint4*>(u + i * 8);
  const uint4 lo = src[0], hi = src[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t r[8];
  fe::x25519_words(r, k, w);
  uint4* dst = reinterpret_cast<uint4*>(out + i * 8);
  dst[0] = make_uint4(r[0], r[1], r[2], r[3]);
  dst[1] = make_uint4(r[4], r[5], r[6], r[7]);
}

// row i of out = the 32 bytes of sha256(prefix || string i) in digest order: word j is the
// byte-swapped state word H[j] (not efl_sha256_fdh's number form). One lane per string.
__global__ __launch_bounds__(kBlock) void k_sha256_rows(Prefix pre, const char* __restrict__ chars,
                                                        const long long* __restrict__ offsets,
                                                        uint32_t* __restrict__ out, long long N) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const unsigned char* s = reinterpret_cast<const unsigned char*>(chars) + offsets[i];
  const long long plen = pre.len, len = plen + (offsets[i + 1] - offsets[i]);
  uint32_t H[8];
  sha256::digest(H, len, [&](long long p) -> uint32_t {
    return p < plen ? (pre.w[p >> 2] >> (8 * (int)(p & 3))) & 255u : (uint32_t)s[p - plen];
  });
  uint4* dst = reinterpret_cast<uint4*>(out + i * 8);
  dst[0] = make_uint4(__builtin_bswap32(H[0]), __builtin_bswap32(H[1]), __builtin_bswap32(H[2]),
                      __builtin_bswap32(H[3]));
  dst[1] = make_uint4(__builtin_bswap32(H[4]), __builtin_bswap32(H[5]), __builtin_bswap32(H[6]),
                      __builtin_bswap32(H[7]));
}

fe::Scalar clamped(const uint8_t scalar[32]) {
  fe::Scalar k;
  fe::words_from_bytes(k.w, scalar);
  fe::clamp(k);
  return k;
}

hipError_t run_x25519(const fe::Scalar& k, const uint32_t* u, uint32_t* out, long long N, hipStream_t st) {
  for (long long o = 0; o < N; o += kChunk) {
    const long long n = std::min(N - o, kChunk);
    hipLaunchKernelGGL(k_x25519, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, k, u + o * 8,
                       out + o * 8, n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int check_rows(int64_t n, const void* scalar, std::initializer_list<const void*> bufs,
               std::initializer_list<const void*> rows) {
  if (n < 0) {
    set_error("negative count");
    return EFL_E_INVALID_ARGUMENT;
  }
  if (n == 0) return 1;
  if (!scalar) {
    set_error("null scalar");
    return EFL_E_INVALID_ARGUMENT;
  }
  for (const void* p : bufs)
    if (!p) {
      set_error("null buffer");
      return EFL_E_INVALID_ARGUMENT;
    }
  for (const void* p : rows)
    if (!aligned(p, 16)) {
      set_error("rows of 32 bytes must be 16-byte aligned");
      return EFL_E_INVALID_ARGUMENT;
    }
  return EFL_OK;
}

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API int efl_x25519(const uint8_t scalar[32], const uint8_t* u, uint8_t* out, int64_t n, void* stream) {
  const int rc = check_rows(n, scalar, {u, out}, {u, out});
  if (rc) return rc > 0 ? EFL_OK : rc;
  return hip_status(run_x25519(clamped(scalar), reinterpret_cast<const uint32_t*>(u),
                               reinterpret_cast<uint32_t*>(out), (long long)n, (hipStream_t)stream),
                    "efl_x25519");
}

EFL_API int efl_x25519_hash(const uint8_t scalar[32], const char* prefix, int prefix_len, const char* chars,
                            const int64_t* offsets, uint8_t* out, int64_t n, void* stream) {
  if (prefix_len < 0 || prefix_len > kMaxPrefix) {
    set_error("prefix_len %d is outside 0 .. %d", prefix_len, kMaxPrefix);
    return EFL_E_INVALID_ARGUMENT;
  }
  const int rc = check_rows(n, scalar, {chars, offsets, out}, {out});
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (prefix_len > 0 && !prefix) {
    set_error("null prefix");
    return EFL_E_INVALID_ARGUMENT;
  }
  Prefix pre{};
  pre.len = prefix_len;
  uint8_t bytes[kMaxPrefix] = {0};
  if (prefix_len > 0) memcpy(bytes, prefix, (size_t)prefix_len);
  for (int j = 0; j < kMaxPrefix / 4; ++j)
    pre.w[j] = (uint32_t)bytes[4 * j] | (uint32_t)bytes[4 * j + 1] << 8 | (uint32_t)bytes[4 * j + 2] << 16 |
               (uint32_t)bytes[4 * j + 3] << 24;
  hipStream_t st = (hipStream_t)stream;
  uint32_t* rows = reinterpret_cast<uint32_t*>(out);
  const long long* offs = reinterpret_cast<const long long*>(offsets);
  for (long long o = 0; o < n; o += kChunk) {
    const long long m = std::min((long long)n - o, kChunk);
    hipLaunchKernelGGL(k_sha256_rows, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, pre, chars,
                       offs + o, rows + o * 8, m);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_status(e, "efl_x25519_hash");
  }
  // the ladder in place over the digests
  return hip_status(run_x25519(clamped(scalar), rows, rows, (long long)n, st), "efl_x25519_hash");
}
