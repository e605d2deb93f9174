// The RSA key context of efl.psi and its C ABI (include/efl_hip.h, efl_rsa_*): what
// rsa.PublicKey / rsa.PrivateKey are to the reference's signers (efls-data/xfl/data/psi/rsa_signer.py),
// with every constant the kernels of rsa.hip read derived on the host from the hex text (hostbig.h)
// into ONE device block, as the Paillier context does (keyset.hip). d itself never reaches the
// device and no call gives it back: the block holds d mod (p - 1) and d mod (q - 1).
#include <memory>
#include <mutex>
#include <vector>

#include "hostbig.h"
#include "rsa.h"

namespace efl {
namespace {

using hb::Big;

int64_t put(std::vector<uint32_t>& h, const Big& x, int L) {
  const int64_t off = (int64_t)h.size();
  h.resize(h.size() + ((L + 3) & ~3));          // every constant starts 16-byte aligned
  hb::put_words(x, L, h.data() + off);
  return off;
}
int64_t put28(std::vector<uint32_t>& h, const Big& x, int L) {
  const int64_t off = (int64_t)h.size();
  h.resize(h.size() + ((L + 3) & ~3));
  hb::put_limbs28(x, L, h.data() + off);
  return off;
}

int parse_hex(const char* s, const char* what, Big* out) {
  if (!s) {
    set_error("%s: null text", what);
    return EFL_E_INVALID_ARGUMENT;
  }
  if (!hb::from_hex(s, strlen(s), out)) {
    set_error("%s is not a hex integer", what);
    return EFL_E_INVALID_ARGUMENT;
  }
  return EFL_OK;
}

// words of the class that holds `bits` bits among `classes`
int class_of(int bits, std::initializer_list<int> classes) {
  for (int c : classes)
    if (32 * c >= bits) return c;
  return 0;
}

int hip_fail(hipError_t e, const char* what) {
  if (e == hipErrorOutOfMemory) {
    set_error("%s: out of device memory", what);
    return EFL_E_RESOURCE_EXHAUSTED;
  }
  return hip_status(e, what);
}

}  // namespace
}  // namespace efl

using namespace efl;

struct efl_rsa_ctx {
  std::mutex mu;
  uint32_t* dev = nullptr;            // the key block
  rsa::Key key{};
  efl_pl_key inv{};                   // N as the modulus of the batched inversion (efl_pl_invert)
  bool has_public = false, has_private = false;
  int n_bits = 0;
  uint64_t e = 0;

  ~efl_rsa_ctx() {
    if (dev) (void)hipFree(dev);      // synchronises with work that still reads the block
  }
};

namespace {

// derive, upload, and only then replace the context's key (a refused key leaves the previous one)
int set_key(efl_rsa_ctx* ctx, const char* n_hex, const char* e_hex, const char* d_hex, const char* p_hex,
            const char* q_hex, bool priv, hipStream_t s) {
  if (!ctx) {
    set_error("null context");
    return EFL_E_INVALID_ARGUMENT;
  }
  Big n, e, d, p, q;
  int rc = parse_hex(n_hex, "n", &n);
  if (rc == EFL_OK) rc = parse_hex(e_hex, "e", &e);
  if (rc == EFL_OK && priv) rc = parse_hex(d_hex, "d", &d);
  if (rc == EFL_OK && priv) rc = parse_hex(p_hex, "p", &p);
  if (rc == EFL_OK && priv) rc = parse_hex(q_hex, "q", &q);
  if (rc != EFL_OK) return rc;
  if (!n.odd() || n.bits() < 16) {
    set_error("n must be odd and of at least 16 bits");
    return EFL_E_INVALID_ARGUMENT;
  }
  const int W = class_of(n.bits(), {32, 64, 128});
  if (!W) {
    set_error("n of %d bits is not supported on the GPU (max 4096)", n.bits());
    return EFL_E_INVALID_ARGUMENT;
  }
  if (e.zero() || e.bits() > 64) {
    set_error("e must be in [1, 2^64)");
    return EFL_E_INVALID_ARGUMENT;
  }
  const uint64_t e64 = (uint64_t)e.w[0] | (e.w.size() > 1 ? (uint64_t)e.w[1] << 32 : 0);

  std::vector<uint32_t> h;
  rsa::Key k{};
  k.W = W;
  k.L = W / 2;
  k.off_n = put(h, n, W);
  k.off_n_r2 = put(h, hb::mod(hb::pow2(2 * 32 * W), n), W);
  k.n_minv = hb::minv32(n);
  if (priv) {
    if (hb::mul(p, q) != n) {
      set_error("p q != n");
      return EFL_E_INVALID_ARGUMENT;
    }
    if (!p.odd() || !q.odd() || p == q || p == Big(1) || q == Big(1)) {
      set_error("p and q must be distinct odd primes");
      return EFL_E_INVALID_ARGUMENT;
    }
    const Big one(1);
    const Big pm1 = hb::sub(p, one), qm1 = hb::sub(q, one);
    if (hb::mod(hb::mul(e, d), pm1) != hb::mod(one, pm1) || hb::mod(hb::mul(e, d), qm1) != hb::mod(one, qm1)) {
      set_error("e d != 1 mod (p - 1) or mod (q - 1)");
      return EFL_E_INVALID_ARGUMENT;
    }
    // the primes' class: half of N's for balanced primes; N's own when one prime is longer than
    // that (python-rsa draws p an eighth longer than q)
    const int L = class_of(std::max(p.bits(), q.bits()), {16, 32, 64});
    if (!L || (L != W / 2 && L != W)) {
      set_error("primes of %d and %d bits do not fit a kernel family for n of %d bits", p.bits(), q.bits(),
                n.bits());
      return EFL_E_INVALID_ARGUMENT;
    }
    k.L = L;
    const int L28 = rsa::sign_limbs28(L);
    const Big* xs[2] = {&p, &q};
    const Big* xm1[2] = {&pm1, &qm1};
    for (int t = 0; t < 2; ++t) {
      const Big& x = *xs[t];
      rsa::Prime& pr = k.pr[t];
      pr.off_x = put(h, x, L);
      pr.off_r2 = put(h, hb::mod(hb::pow2(2 * 32 * L), x), L);
      pr.off_x28 = put28(h, x, L28);
      pr.off_r2_28 = put28(h, hb::mod(hb::pow2(2 * 28 * L28), x), L28);
      const Big dx = hb::mod(d, *xm1[t]);
      pr.off_dx = put(h, dx, L);
      pr.dbits = dx.bits();
      pr.minv = hb::minv32(x);
      pr.minv28 = hb::minv28(x);
    }
    Big qinv;
    if (!hb::modinv(hb::mod(q, p), p, &qinv)) {
      set_error("q has no inverse mod p");
      return EFL_E_INVALID_ARGUMENT;
    }
    k.off_qinvp = put(h, hb::mod(hb::mul(qinv, hb::pow2(32 * L)), p), L);
  }

  uint32_t* dev = nullptr;
  hipError_t err = hipMalloc((void**)&dev, h.size() * 4);
  if (err != hipSuccess) return hip_fail(err, "RSA key block");
  err = hipMemcpyAsync(dev, h.data(), h.size() * 4, hipMemcpyHostToDevice, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  if (err != hipSuccess) {
    (void)hipFree(dev);
    return hip_fail(err, "RSA key upload");
  }
  k.base = dev;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (ctx->dev) (void)hipFree(ctx->dev);   // waits for queued work that reads the previous key
  ctx->dev = dev;
  ctx->key = k;
  ctx->inv = efl_pl_key{};
  ctx->inv.ln = W / 2;                     // the inversion's modulus ("n^2") has 2 ln = W words
  ctx->inv.a_bits = 1;
  ctx->inv.off_n2 = k.off_n;
  ctx->inv.n2_minv = k.n_minv;
  ctx->has_public = true;
  ctx->has_private = priv;
  ctx->n_bits = n.bits();
  ctx->e = e64;
  return EFL_OK;
}

// the checks every batch op shares; > 0: nothing to do
int batch_args(efl_rsa_ctx* ctx, int64_t n, std::initializer_list<const void*> bufs, bool need_private,
               rsa::Key* k) {
  if (!ctx) {
    set_error("null context");
    return EFL_E_INVALID_ARGUMENT;
  }
  if (n < 0) {
    set_error("negative count");
    return EFL_E_INVALID_ARGUMENT;
  }
  if (n == 0) return 1;
  for (const void* b : bufs)
    if (!b || !aligned(b, 16)) {
      set_error(b ? "buffers must be 16-byte aligned" : "null buffer");
      return EFL_E_INVALID_ARGUMENT;
    }
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (need_private && !ctx->has_private) {
    set_error("No private key.");
    return EFL_E_ABORTED;
  }
  if (!ctx->has_public) {
    set_error("No public key.");
    return EFL_E_ABORTED;
  }
  *k = ctx->key;
  return EFL_OK;
}

}  // namespace

EFL_API int efl_rsa_ctx_create(efl_rsa_ctx** out) {
  if (!out) {
    set_error("null context pointer");
    return EFL_E_INVALID_ARGUMENT;
  }
  *out = new efl_rsa_ctx();
  return EFL_OK;
}

EFL_API int efl_rsa_ctx_destroy(efl_rsa_ctx* ctx) {
  delete ctx;                              // hipFree of the block synchronises with work still using it
  return EFL_OK;
}

EFL_API int efl_rsa_set_public(efl_rsa_ctx* ctx, const char* n_hex, const char* e_hex, void* stream) {
  return set_key(ctx, n_hex, e_hex, nullptr, nullptr, nullptr, false, (hipStream_t)stream);
}

EFL_API int efl_rsa_set_private(efl_rsa_ctx* ctx, const char* n_hex, const char* e_hex, const char* d_hex,
                                const char* p_hex, const char* q_hex, void* stream) {
  return set_key(ctx, n_hex, e_hex, d_hex, p_hex, q_hex, true, (hipStream_t)stream);
}

EFL_API int efl_rsa_ctx_query(efl_rsa_ctx* ctx, efl_rsa_ctx_info* info) {
  if (!ctx || !info) {
    set_error("null context or info");
    return EFL_E_INVALID_ARGUMENT;
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  *info = efl_rsa_ctx_info{};
  info->has_public = ctx->has_public;
  info->has_private = ctx->has_private;
  info->n_bits = ctx->n_bits;
  info->words = ctx->has_public ? ctx->key.W : 0;
  info->byte_len = ctx->n_bits / 8;
  info->e = ctx->e;
  return EFL_OK;
}

EFL_API int efl_rsa_sign(efl_rsa_ctx* ctx, const uint32_t* x, uint32_t* s, int64_t n, void* stream) {
  rsa::Key k;
  const int rc = batch_args(ctx, n, {x, s}, true, &k);
  if (rc) return rc > 0 ? EFL_OK : rc;
  const hipError_t e = rsa::sign(k, x, s, (long long)n, (hipStream_t)stream);
  return e == hipErrorOutOfMemory ? hip_fail(e, "efl_rsa_sign") : hip_status(e, "efl_rsa_sign");
}

EFL_API int efl_rsa_blind(efl_rsa_ctx* ctx, const uint32_t* h, const uint32_t* r, uint32_t* out, int64_t n,
                          void* stream) {
  rsa::Key k;
  const int rc = batch_args(ctx, n, {h, r, out}, false, &k);
  if (rc) return rc > 0 ? EFL_OK : rc;
  uint64_t e;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    e = ctx->e;
  }
  return hip_status(rsa::blind(k, h, r, e, out, (long long)n, (hipStream_t)stream), "efl_rsa_blind");
}

EFL_API int efl_rsa_unblind(efl_rsa_ctx* ctx, const uint32_t* s, const uint32_t* r, uint32_t* out, int64_t n,
                            int64_t* bad, void* stream) {
  rsa::Key k;
  int rc = batch_args(ctx, n, {s, r, out, bad}, false, &k);
  hipStream_t st = (hipStream_t)stream;
  if (rc) return rc > 0 ? EFL_OK : rc;     // n == 0: nothing is written, bad included
  efl_pl_key inv;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    inv = ctx->inv;
  }
  // r^-1 mod N by the batched binary GCD (bad <- the first r without an inverse; its inverse reads 0,
  // and so does its product), then s r^-1: the blind product with e = 1
  uint32_t* rinv = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&rinv), (size_t)n * k.W * 4, st);
  if (e != hipSuccess) return hip_fail(e, "efl_rsa_unblind");
  rc = efl_pl_invert(k.base, &inv, r, rinv, n, bad, stream);
  if (rc == EFL_OK) rc = hip_status(rsa::blind(k, s, rinv, 1, out, (long long)n, st), "efl_rsa_unblind");
  const hipError_t fe = hipFreeAsync(rinv, st);
  return rc != EFL_OK ? rc : hip_status(fe, "efl_rsa_unblind");
}

EFL_API int efl_sha256_fdh(const char* chars, const int64_t* offsets, uint32_t* out, int words_per_row, int64_t n,
                           void* stream) {
  if (n < 0) {
    set_error("negative count");
    return EFL_E_INVALID_ARGUMENT;
  }
  if (n == 0) return EFL_OK;
  if (!chars || !offsets || !out) {
    set_error("null buffer");
    return EFL_E_INVALID_ARGUMENT;
  }
  if (words_per_row < 8) {
    set_error("a row holds the 8 words of the digest at least");
    return EFL_E_INVALID_ARGUMENT;
  }
  return hip_status(rsa::sha256_fdh(chars, (const long long*)offsets, out, words_per_row, (long long)n,
                                    (hipStream_t)stream),
                    "efl_sha256_fdh");
}
