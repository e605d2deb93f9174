#!/usr/bin/env python3
"""Writes tests/golden/x25519_kat.json: the known answers of efl.psi's X25519 (csrc/fe25519.h,
csrc/x25519.hip, efl.psi.EccSigner).

Everything is computed here with Python integers (the ladder formulas of RFC 7748 §5) and hashlib,
and every vector whose answer is not all zero is also asserted against `openssl pkeyutl -derive`,
the raw keys wrapped in the fixed DER prefixes of an X25519 PKCS#8 private key and SubjectPublicKeyInfo.
The tests read only the JSON.

    python tests/golden/make_x25519_golden.py
"""
import hashlib
import json
import os
import random
import subprocess
import tempfile

P = 2 ** 255 - 19
A24 = 121665
PKCS8 = bytes.fromhex("302e020100300506032b656e04220420")
SPKI = bytes.fromhex("302a300506032b656e032100")
HERE = os.path.dirname(os.path.abspath(__file__))


def clamp(k: bytes) -> bytes:
    b = bytearray(k)
    b[0] &= 248
    b[31] &= 127
    b[31] |= 64
    return bytes(b)


def x25519(k: bytes, u: bytes) -> bytes:
    """RFC 7748 §5: decodeScalar25519, decodeUCoordinate (bit 255 masked, no reduction check), the
    ladder with cswap, x2 * z2^(p - 2), fully reduced."""
    kn = int.from_bytes(clamp(k), "little")
    x1 = (int.from_bytes(u, "little") & ((1 << 255) - 1)) % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        kt = (kn >> t) & 1
        swap ^= kt
        if swap:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b = (x2 + z2) % P, (x2 - z2) % P
        aa, bb = a * a % P, b * b % P
        e = (aa - bb) % P
        c, d = (x3 + z3) % P, (x3 - z3) % P
        da, cb = d * a % P, c * b % P
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + A24 * e) % P
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


def openssl_x25519(k: bytes, u: bytes) -> bytes:
    with tempfile.TemporaryDirectory() as d:
        prv, pub = os.path.join(d, "k.der"), os.path.join(d, "u.der")
        with open(prv, "wb") as f:
            f.write(PKCS8 + k)
        with open(pub, "wb") as f:
            f.write(SPKI + u)
        return subprocess.check_output(["openssl", "pkeyutl", "-derive", "-keyform", "DER", "-inkey", prv,
                                        "-peerform", "DER", "-peerkey", pub], stderr=subprocess.PIPE)


def checked(k: bytes, u: bytes) -> bytes:
    out = x25519(k, u)
    if any(out):                      # OpenSSL refuses to derive the all-zero secret
        got = openssl_x25519(k, u)
        assert got == out, (k.hex(), u.hex(), out.hex(), got.hex())
    return out


def le(v: int) -> bytes:
    return v.to_bytes(32, "little")


def limbs_of(v: int):
    """v in the 25.5-bit limbs of csrc/fe25519.h, the excess above 2^255 left in limb 9."""
    out = []
    for i in range(10):
        pos, bits = (51 * i + 1) // 2, 25 if i & 1 else 26
        out.append((v >> pos) & ((1 << bits) - 1) if i < 9 else v >> pos)
    return out


def limbs_value(limbs):
    return sum(x << ((51 * i + 1) // 2) for i, x in enumerate(limbs))


def main():
    rng = random.Random(25519)
    rb = lambda: bytes(rng.randrange(256) for _ in range(32))

    # ---- known answers -------------------------------------------------------------------
    known = []

    def add_known(name, k, u, want):
        out = checked(bytes.fromhex(k) if isinstance(k, str) else k, bytes.fromhex(u) if isinstance(u, str) else u)
        assert out.hex() == want, (name, out.hex())
        known.append({"name": name, "scalar": k if isinstance(k, str) else k.hex(),
                      "u": u if isinstance(u, str) else u.hex(), "out": want})

    add_known("rfc7748-5.2-1", "a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4",
              "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
              "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552")
    add_known("rfc7748-5.2-2", "4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d",
              "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493",
              "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957")
    nine = le(9).hex()
    alice = "77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a"
    bob = "5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb"
    apub = "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a"
    bpub = "de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f"
    shared = "4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742"
    add_known("rfc7748-6.1-alice-public", alice, nine, apub)
    add_known("rfc7748-6.1-bob-public", bob, nine, bpub)
    add_known("rfc7748-6.1-alice-shared", alice, bpub, shared)
    add_known("rfc7748-6.1-bob-shared", bob, apub, shared)
    # the reference's test/test_ecc_signer.py: secret b'p' * 32, the hash forced to b'a' * 32
    add_known("reference-test", b"p" * 32, b"a" * 32, "8bb21ae817643480a77910370fab9d8d0fccf8ec05bb9412531adb3983348104")

    # RFC 7748 §5.2's iteration: k, u = X25519(k, u), k
    k = u = le(9)
    after = {}
    for it in range(1, 1001):
        k, u = x25519(k, u), k
        if it in (1, 1000):
            after[it] = k.hex()
    assert after[1] == "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"
    assert after[1000] == "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"
    iterated = {"start": nine, "after_1": after[1], "after_1000": after[1000]}

    # ---- scalars x u values, the edge values first --------------------------------------------
    order8 = [325606250916557431795983626356110631294008115727848805560023387167927233504,
              39382357235489614581723060781553021112529911719440698176882885853963445705823]
    us = [le(0), le(1), le(9), le(P - 1), le(P), le(P + 1), le(2 ** 255 - 1), le(2 ** 255 + 9)]
    us += [le(v) for v in order8]
    # RFC 7748 §7 also lists these plus p; neither fits in 255 bits (both are above 18), so there is
    # no such encoding to add
    assert all(v + P >= 2 ** 255 for v in order8)
    us += [rb() for _ in range(3)]
    us.append(le(int.from_bytes(rb(), "little") | 1 << 255))      # a random one with bit 255 set
    unclamped = bytes([rng.randrange(256) | 7]) + bytes(rng.randrange(256) for _ in range(30)) + bytes([0x80 | 0x3f & rng.randrange(256)])
    assert clamp(unclamped) != unclamped
    named = [("zeros", bytes(32)), ("ones", b"\xff" * 32), ("unclamped", unclamped), ("clamped-twin", clamp(unclamped)),
             ("random", rb())]
    scalars = []
    for name, s in named:
        outs = [checked(s, u) for u in us]
        scalars.append({"name": name, "scalar": s.hex(), "outs": [o.hex() for o in outs]})
        assert outs[7] == outs[2]                                   # bit 255 of u is ignored
        assert outs[4] == outs[0] == bytes(32) and outs[5] == outs[1]   # p = 0, p + 1 = 1
        assert all(not any(outs[i]) for i in (0, 1, 3, 8, 9))       # low order: all zero
        assert any(outs[2]) and any(outs[10])
    assert scalars[2]["outs"] == scalars[3]["outs"]

    # ---- hash vectors: lengths that cross SHA-256's padding boundaries with the 10-byte prefix ----
    prefix = b"curve25519"
    secret = rb()
    hashes = []
    for total in (10, 55, 56, 63, 64, 119, 120):
        n = total - len(prefix)
        ident = bytes(rng.randrange(0x80, 0x100) for _ in range(n)) if total == 63 else \
            bytes(rng.choice(b"0123456789abcdef_-") for _ in range(n))
        dg = hashlib.sha256(prefix + ident).digest()
        hashes.append({"id": ident.hex(), "digest": dg.hex(), "signed": checked(secret, dg).hex()})

    # ---- field vectors for the host test -------------------------------------------------------
    vals = [0, 1, 19, P - 1, P, 2 ** 255 - 1, 2 ** 255 - 20] + [int.from_bytes(rb(), "little") >> 1 for _ in range(4)]
    pairs = [(P - 1, P - 1), (2 ** 255 - 1, 2 ** 255 - 1), (P - 1, 2 ** 255 - 1), (2 ** 255 - 1, 0), (0, 2 ** 255 - 1)]
    pairs += [(rng.choice(vals), rng.choice(vals)) for _ in range(12)] + [(vals[-1], vals[-2]), (vals[-3], vals[-4])]
    mul = [{"a": le(a).hex(), "b": le(b).hex(), "sum": le((a + b) % P).hex(), "diff": le((a - b) % P).hex(),
            "prod": le(a * b % P).hex(), "sq": le(a * a % P).hex(), "loose": le((a + b) * (a - b) % P).hex(),
            "a24": le(A24 * (a - b) % P).hex(), "inv": le(pow(a, P - 2, P)).hex()} for a, b in pairs]
    freeze = [limbs_of(v) for v in (0, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 ** 255 - 1, 2 ** 255, 2 ** 256 - 1)]
    freeze.append([2 ** 32 - 1] * 10)                               # the largest value the limbs admit
    freeze.append([2 ** 26, 2 ** 25 + 2 ** 16] + [2 ** 26, 2 ** 25] * 4)
    freeze = [{"limbs": f, "out": le(limbs_value(f) % P).hex()} for f in freeze]

    doc = {"about": "X25519 (RFC 7748) known answers; made by make_x25519_golden.py from Python integers, "
                    "checked against openssl pkeyutl -derive. Hex strings are the 32 bytes in order.",
           "known": known, "iterated": iterated, "us": [u.hex() for u in us], "scalars": scalars,
           "hash": {"prefix": prefix.decode(), "secret": secret.hex(), "vectors": hashes},
           "field": {"mul": mul, "freeze": freeze}}
    path = os.path.join(HERE, "x25519_kat.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    assert os.path.getsize(path) < 64 * 1024
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
