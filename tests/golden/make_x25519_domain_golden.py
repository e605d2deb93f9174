#!/usr/bin/env python3
"""Writes tests/golden/x25519_domain.json: the crafted-output family W of tests/x25519_domain.py and
one digest per input family.

The families and the reference are tests/x25519_domain.py (Python integers). This script does what
the tests should not repeat: it filters the w candidates down to u-coordinates of prime-order points
(one 253-step ladder each), and it asserts every non-zero expected row of U x two scalars, K x two u
values, W x two scalars and the 1,024-lane batch against OpenSSL (libcrypto's EVP_PKEY_derive through
ctypes, or `openssl pkeyutl -derive` where the library does not load). The tests recompute the rows
and compare their digests with the ones written here.

    python tests/golden/make_x25519_domain_golden.py
"""
import ctypes
import ctypes.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import x25519_domain as xd                      # noqa: E402
from make_x25519_golden import openssl_x25519   # noqa: E402

EVP_PKEY_X25519 = 1034


def load_crypto():
    for name in ("libcrypto.so.3", ctypes.util.find_library("crypto")):
        if not name:
            continue
        try:
            c = ctypes.CDLL(name)
            c.EVP_PKEY_new_raw_private_key.restype = ctypes.c_void_p
            c.EVP_PKEY_new_raw_public_key.restype = ctypes.c_void_p
            c.EVP_PKEY_CTX_new.restype = ctypes.c_void_p
            c.EVP_PKEY_new_raw_private_key.argtypes = c.EVP_PKEY_new_raw_public_key.argtypes = \
                [ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
            c.EVP_PKEY_CTX_new.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            c.EVP_PKEY_derive_init.argtypes = c.EVP_PKEY_CTX_free.argtypes = c.EVP_PKEY_free.argtypes = [ctypes.c_void_p]
            c.EVP_PKEY_derive_set_peer.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            c.EVP_PKEY_derive.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t)]
            return c
        except (OSError, AttributeError):
            continue
    return None


CRYPTO = load_crypto()


def openssl(k: bytes, u: bytes) -> bytes:
    if CRYPTO is None:
        return openssl_x25519(k, u)
    c = CRYPTO
    prv = c.EVP_PKEY_new_raw_private_key(EVP_PKEY_X25519, None, k, 32)
    pub = c.EVP_PKEY_new_raw_public_key(EVP_PKEY_X25519, None, u, 32)
    ctx = c.EVP_PKEY_CTX_new(prv, None)
    out, n = ctypes.create_string_buffer(32), ctypes.c_size_t(32)
    ok = c.EVP_PKEY_derive_init(ctx) == 1 and c.EVP_PKEY_derive_set_peer(ctx, pub) == 1 and \
        c.EVP_PKEY_derive(ctx, out, ctypes.byref(n)) == 1
    c.EVP_PKEY_CTX_free(ctx)
    c.EVP_PKEY_free(pub)
    c.EVP_PKEY_free(prv)
    assert ok and n.value == 32, (k.hex(), u.hex())
    return out.raw


def check(k: bytes, u: bytes, want: bytes) -> int:
    """1 when the row was compared (OpenSSL refuses to derive the all-zero secret)."""
    if not any(want):
        return 0
    got = openssl(k, u)
    assert got == want, (k.hex(), u.hex(), want.hex(), got.hex())
    return 1


def main():
    kept = {"curve": [], "twist": []}
    cands = xd.w_candidates()
    for w in cands:
        cls = xd.prime_order_class(w)
        if cls:
            kept[cls].append(w)
    xd.check_w_conditions(kept)
    doc = {"about": "The crafted outputs (family W) and the per-family digests of tests/x25519_domain.py; made by "
                    "make_x25519_domain_golden.py, every non-zero expected row checked against OpenSSL. w values "
                    "are hexadecimal numbers; scalars and points are the 32 bytes in order.",
           "seed": xd.SEED, "u_scalars": [k.hex() for k in xd.U_SCALARS], "w_scalars": [k.hex() for k in xd.W_SCALARS],
           "lane_scalar": xd.LANE_SCALAR.hex(), "k_points": [u.hex() for u in xd.k_points()],
           "candidates": len(cands), "w": {cls: ["%x" % w for w in ws] for cls, ws in kept.items()}}
    # the families read the w values from the fixture: write them before the rows are computed
    path = xd.FIXTURE
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    xd.family_w.cache_clear()
    xd.crafted_w.cache_clear()

    n = 0
    for k, rows in zip(xd.U_SCALARS, xd.expected_u()):
        n += sum(check(k, xd.le(u), want) for (_, _, u), want in zip(xd.family_u(), rows))
    for (_, _, k), rows in zip(xd.family_k(), xd.expected_k()):
        n += sum(check(k, u, want) for u, want in zip(xd.k_points(), rows))
    for k, us in zip(xd.W_SCALARS, xd.crafted_w()):
        n += sum(check(k, u, xd.le(w)) for u, (_, w) in zip(us, xd.family_w()))
    n += sum(check(xd.LANE_SCALAR, u, want) for u, want in zip(*xd.lane_us()))
    doc["openssl_checked_rows"] = n
    doc["digests"] = xd.digests()
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    assert os.path.getsize(path) < 64 * 1024
    print(path, os.path.getsize(path), "bytes;", n, "rows checked against",
          "libcrypto EVP_PKEY_derive" if CRYPTO is not None else "openssl pkeyutl -derive",
          {cls: len(ws) for cls, ws in kept.items()})


if __name__ == "__main__":
    main()
