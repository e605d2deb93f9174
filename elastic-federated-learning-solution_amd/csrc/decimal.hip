// The tail of every RSA PSI signature on the device (efl.psi; reference:
// efls-data/xfl/data/psi/rsa_signer.py, hex(OneWayHash(str(v)))[2:]): the decimal text of each row
// (csrc/decimal.h) and a 64-bit one-way hash over it, behind efl_rsa_decimal / efl_rsa_oneway.
//
// k_decimal_chunks  one lane per number, one 64-lane wave per workgroup. The number sits column-major
//                   in LDS, word j of the lane's element at lds[j * 64 + lane] (the layout
//                   sl::to_lds uses), so the wave's 64 accesses of a word fall in 64 different banks;
//                   4 * 64 * words bytes, 32 KiB at 128 words, and nothing else is in LDS. A lane
//                   touches its own column only: no barrier, no atomic, no lane waits for another,
//                   and lanes diverge only in how many words are still non-zero. Each of the
//                   ceil(D / 9) passes ends in ONE store of the pass's chunk (9 digits as a number
//                   below 10^9) to chunks[k * N + i], a k-major matrix in stream-ordered scratch:
//                   the wave's lanes write 64 consecutive dwords.
// k_decimal_text    one lane per aligned dword of the text: each byte is a digit of one chunk
//                   (decimal::text_byte) or padding, the wave stores 256 consecutive bytes; the few
//                   bytes before the first and after the last aligned dword go out singly.
// k_oneway_sha256   one lane per number: SHA-256 (sha256.h) whose byte getter reads the digits from
//                   the chunk matrix, so for efl_rsa_oneway the text is never written anywhere.
#include "decimal.h"
#include "sha256.h"

namespace efl {
namespace {

constexpr int kWave = 64;
constexpr long long kSlab = 1 << 18;            // rows per launch (the scratch holds their chunks)
constexpr int64_t kMaxStride = (int64_t)1 << 30;

__global__ __launch_bounds__(kWave) void k_decimal_chunks(const uint32_t* __restrict__ x, int words, long long N,
                                                          uint32_t* __restrict__ chunks, int32_t* __restrict__ len) {
  extern __shared__ uint32_t lds[];
  const long long i = (long long)blockIdx.x * kWave + threadIdx.x;
  if (i >= N) return;
  uint32_t* mine = lds + threadIdx.x;
  const uint32_t* xi = x + i * words;
  if ((words & 3) == 0 && aligned(x, 16)) {
    const uint4* v = reinterpret_cast<const uint4*>(xi);
    for (int j = 0; j < words / 4; ++j) {
      const uint4 w = v[j];
      mine[(4 * j + 0) * kWave] = w.x;
      mine[(4 * j + 1) * kWave] = w.y;
      mine[(4 * j + 2) * kWave] = w.z;
      mine[(4 * j + 3) * kWave] = w.w;
    }
  } else {
    for (int j = 0; j < words; ++j) mine[j * kWave] = xi[j];
  }
  len[i] = decimal::to_chunks(
      words, [mine](int j) { return mine[j * kWave]; }, [mine](int j, uint32_t v) { mine[j * kWave] = v; },
      [chunks, N, i](int k, uint32_t c) { chunks[(long long)k * N + i] = c; });
}

// text - lead is 4-byte aligned (0 <= lead < 4); lane t owns the dword at flat bytes 4 t - lead ..
__global__ __launch_bounds__(256) void k_decimal_text(const uint32_t* __restrict__ chunks, long long N, int nchunks,
                                                      uint8_t* __restrict__ text, long long stride, int lead) {
  const long long total = N * stride;
  const long long f0 = 4 * ((long long)blockIdx.x * 256 + threadIdx.x) - lead;
  if (f0 >= total) return;
  const long long first = f0 < 0 ? 0 : f0;
  long long row = first / stride, col = first - row * stride;
  uint32_t word = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const long long f = f0 + b;
    if (f < 0 || f >= total) continue;
    const uint32_t byte =
        decimal::text_byte(stride, col, nchunks, [chunks, N, row](int k) { return chunks[(long long)k * N + row]; });
    word |= byte << (8 * b);
    if (++col == stride) {
      col = 0;
      ++row;
    }
  }
  if (f0 >= 0 && f0 + 4 <= total) {
    *reinterpret_cast<uint32_t*>(text + f0) = word;
    return;
  }
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (f0 + b >= 0 && f0 + b < total) text[f0 + b] = (uint8_t)(word >> (8 * b));
}

// out[i] <- the first 8 bytes of sha256(the len[i] digits of row i) as a big-endian number, stored
// little-endian
__global__ __launch_bounds__(256) void k_oneway_sha256(const uint32_t* __restrict__ chunks,
                                                       const int32_t* __restrict__ len, long long N, int nchunks,
                                                       uint8_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int L = len[i];
  uint32_t H[8];
  sha256::digest(H, L, [chunks, N, i, L, nchunks](long long p) {
    return decimal::text_byte(L, p, nchunks, [chunks, N, i](int k) { return chunks[(long long)k * N + i]; });
  });
  *reinterpret_cast<uint64_t*>(out + 8 * i) = ((uint64_t)H[0] << 32) | H[1];
}

// the rows in slabs: chunks (and, for the hash, the lengths) in stream-ordered scratch, then the text
// (text != nullptr) or the hash (out != nullptr) of the slab
hipError_t run(const uint32_t* x, int words, long long n, uint8_t* text, long long stride, int32_t* len, uint8_t* out,
               hipStream_t st) {
  const int nchunks = decimal::max_chunks(words);
  long long slab = n < kSlab ? n : kSlab;
  if (text) {
    // the text kernel's grid stays below 2^31 blocks of 1 KiB
    const long long most = ((1ll << 31) - 2) * 1024 / stride;
    if (slab > most) slab = most;
  }
  uint32_t* scratch = nullptr;
  hipError_t err = hipMallocAsync(reinterpret_cast<void**>(&scratch), (size_t)slab * (nchunks + 1) * 4, st);
  if (err != hipSuccess) return err;
  int32_t* slab_len = reinterpret_cast<int32_t*>(scratch + (size_t)slab * nchunks);
  for (long long o = 0; o < n && err == hipSuccess; o += slab) {
    const long long m = n - o < slab ? n - o : slab;
    hipLaunchKernelGGL(k_decimal_chunks, dim3((unsigned)((m + kWave - 1) / kWave)), dim3(kWave),
                       (size_t)words * kWave * 4, st, x + o * words, words, m, scratch, len ? len + o : slab_len);
    err = hipGetLastError();
    if (err != hipSuccess) break;
    if (text) {
      uint8_t* t = text + o * stride;
      const int lead = (int)(reinterpret_cast<uintptr_t>(t) & 3);
      const long long dwords = (m * stride + lead + 3) / 4;
      hipLaunchKernelGGL(k_decimal_text, dim3((unsigned)((dwords + 255) / 256)), dim3(256), 0, st, scratch, m,
                         nchunks, t, stride, lead);
    } else {
      hipLaunchKernelGGL(k_oneway_sha256, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, scratch, slab_len, m,
                         nchunks, out + o * 8);
    }
    err = hipGetLastError();
  }
  const hipError_t ferr = hipFreeAsync(scratch, st);
  return err == hipSuccess ? ferr : err;
}

// the checks both entry points share; > 0: nothing to do
int rows_args(const uint32_t* x, int words, int64_t n) {
  if (n < 0) {
    set_error("negative count");
    return EFL_E_INVALID_ARGUMENT;
  }
  if (n == 0) return 1;
  if (words < 1 || words > decimal::kMaxWords) {
    set_error("a row has 1 to %d words, got %d", decimal::kMaxWords, words);
    return EFL_E_INVALID_ARGUMENT;
  }
  if (!x) {
    set_error("null buffer");
    return EFL_E_INVALID_ARGUMENT;
  }
  if (!aligned(x, 4)) {
    set_error("rows are misaligned (4 bytes)");
    return EFL_E_INVALID_ARGUMENT;
  }
  return EFL_OK;
}

int finish(hipError_t e, const char* what) {
  if (e == hipErrorOutOfMemory) {
    set_error("%s: out of device memory", what);
    return EFL_E_RESOURCE_EXHAUSTED;
  }
  return hip_status(e, what);
}

}  // namespace
}  // namespace efl

using namespace efl;

EFL_API int efl_rsa_decimal_digits(int words) { return decimal::max_digits(words); }

EFL_API int efl_rsa_decimal(const uint32_t* x, int words, int64_t n, uint8_t* text, int64_t stride, int32_t* len,
                            void* stream) {
  const int rc = rows_args(x, words, n);
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (!text || !len) {
    set_error("null buffer");
    return EFL_E_INVALID_ARGUMENT;
  }
  if (!aligned(len, 4)) {
    set_error("len is misaligned (4 bytes)");
    return EFL_E_INVALID_ARGUMENT;
  }
  if (stride < decimal::max_digits(words) || stride > kMaxStride) {
    set_error("stride %lld: a row of %d words takes %d to 2^30 bytes", (long long)stride, words,
              decimal::max_digits(words));
    return EFL_E_INVALID_ARGUMENT;
  }
  return finish(run(x, words, (long long)n, text, (long long)stride, len, nullptr, (hipStream_t)stream),
                "efl_rsa_decimal");
}

EFL_API int efl_rsa_oneway(const uint32_t* x, int words, int64_t n, int hash, uint8_t* out, void* stream) {
  const int rc = rows_args(x, words, n);
  if (rc) return rc > 0 ? EFL_OK : rc;
  if (hash != EFL_ONEWAY_SHA256_64) {
    set_error("one-way hash %d is not one of the device's (EFL_ONEWAY_SHA256_64 = 1)", hash);
    return EFL_E_INVALID_ARGUMENT;
  }
  if (!out) {
    set_error("null buffer");
    return EFL_E_INVALID_ARGUMENT;
  }
  if (!aligned(out, 8)) {
    set_error("out is misaligned (8 bytes)");
    return EFL_E_INVALID_ARGUMENT;
  }
  return finish(run(x, words, (long long)n, nullptr, 0, nullptr, out, (hipStream_t)stream), "efl_rsa_oneway");
}
