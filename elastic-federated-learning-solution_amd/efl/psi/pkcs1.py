"""PKCS#1 (RFC 8017, appendix A.1) RSA keys as PEM / DER, the two forms the reference's signers
pass around (rsa.PublicKey.load_pkcs1 / save_pkcs1, efls-data/xfl/data/psi/rsa_signer.py:44-53):

  RSA PUBLIC KEY   SEQUENCE { n, e }
  RSA PRIVATE KEY  SEQUENCE { 0, n, e, d, p, q, d mod (p-1), d mod (q-1), q^-1 mod p }

Only what those two need of DER: definite lengths, SEQUENCE and non-negative INTEGER.
"""
from __future__ import annotations

import base64
import collections
import re

PublicKey = collections.namedtuple("PublicKey", "n e")
PrivateKey = collections.namedtuple("PrivateKey", "n e d p q")

_PEM = re.compile(rb"-----BEGIN (RSA (?:PUBLIC|PRIVATE) KEY)-----(.*?)-----END \1-----", re.S)


def _read_tlv(buf: bytes, at: int, tag: int):
    if at + 2 > len(buf) or buf[at] != tag:
        raise ValueError(f"PKCS#1: expected DER tag 0x{tag:02x} at byte {at}")
    ln = buf[at + 1]
    at += 2
    if ln & 0x80:
        k = ln & 0x7F
        if k == 0 or k > 4 or at + k > len(buf):
            raise ValueError("PKCS#1: unsupported DER length")
        ln = int.from_bytes(buf[at:at + k], "big")
        at += k
    if at + ln > len(buf):
        raise ValueError("PKCS#1: truncated DER")
    return buf[at:at + ln], at + ln


def der_integers(der: bytes) -> list:
    """The INTEGERs of one DER SEQUENCE of INTEGERs."""
    body, end = _read_tlv(der, 0, 0x30)
    if end != len(der):
        raise ValueError("PKCS#1: bytes after the key")
    out, at = [], 0
    while at < len(body):
        v, at = _read_tlv(body, at, 0x02)
        if not v or v[0] & 0x80:
            raise ValueError("PKCS#1: empty or negative INTEGER")
        out.append(int.from_bytes(v, "big"))
    return out


def _tlv(tag: int, body: bytes) -> bytes:
    n = len(body)
    if n < 0x80:
        return bytes([tag, n]) + body
    ln = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([tag, 0x80 | len(ln)]) + ln + body


def integers_der(values) -> bytes:
    # minimal two's complement: one more byte when the top bit is set
    return _tlv(0x30, b"".join(_tlv(0x02, int(v).to_bytes(int(v).bit_length() // 8 + 1, "big")) for v in values))


def pem_to_der(data):
    """(label, DER bytes) of the first RSA key block of a PEM text; DER input passes through."""
    if isinstance(data, str):
        data = data.encode()
    m = _PEM.search(data)
    if m is None:
        if data[:1] == b"\x30":
            return None, bytes(data)
        raise ValueError("PKCS#1: no RSA PUBLIC KEY / RSA PRIVATE KEY block")
    return m.group(1).decode(), base64.b64decode(b"".join(m.group(2).split()))


def der_to_pem(der: bytes, label: str) -> bytes:
    b64 = base64.b64encode(der)
    lines = [b64[i:i + 64] for i in range(0, len(b64), 64)]
    return b"-----BEGIN " + label.encode() + b"-----\n" + b"\n".join(lines) + b"\n-----END " + \
        label.encode() + b"-----\n"


def load_public(data) -> PublicKey:
    label, der = pem_to_der(data)
    if label not in (None, "RSA PUBLIC KEY"):
        raise ValueError(f"PKCS#1: {label} where a public key is expected")
    v = der_integers(der)
    if len(v) != 2:
        raise ValueError("PKCS#1: a public key is SEQUENCE { n, e }")
    return PublicKey(*v)


def load_private(data) -> PrivateKey:
    label, der = pem_to_der(data)
    if label not in (None, "RSA PRIVATE KEY"):
        raise ValueError(f"PKCS#1: {label} where a private key is expected")
    v = der_integers(der)
    if len(v) != 9 or v[0] != 0:
        raise ValueError("PKCS#1: a private key is SEQUENCE { 0, n, e, d, p, q, dp, dq, qinv } (two primes)")
    return PrivateKey(*v[1:6])


def public_der(n: int, e: int) -> bytes:
    return integers_der([n, e])


def private_der(n: int, e: int, d: int, p: int, q: int) -> bytes:
    return integers_der([0, n, e, d, p, q, d % (p - 1), d % (q - 1), pow(q, -1, p)])


def save_public(n: int, e: int) -> bytes:
    return der_to_pem(public_der(n, e), "RSA PUBLIC KEY")


def save_private(n: int, e: int, d: int, p: int, q: int) -> bytes:
    return der_to_pem(private_der(n, e, d, p, q), "RSA PRIVATE KEY")
