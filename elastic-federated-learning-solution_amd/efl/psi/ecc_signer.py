"""EccSigner: the reference's ECDH PSI signer (efls-data/xfl/data/psi/ecc_signer.py) on the GPU.

The reference signs one ID per call through python-curve25519-donna, whose make_private /
make_shared are RFC 7748's X25519: `sign_hash(x)` for every local ID and `sign(i)` for every item the
peer sends (xfl/data/ecdh_psi.py). Here a whole list goes through one launch (`sign_hash_list`,
`sign_list`); `sign_hash` and `sign` keep the reference's signatures as batches of one.

As in the reference, a low-order point (u = 0, 1, p - 1, p, p + 1 or one of the two order-8
u-coordinates of RFC 7748 §7) gives 32 zero bytes without an error: all such IDs collide.
"""
from __future__ import annotations

import os

from efl.psi import ecc_cipher


class EccSigner(object):
    def __init__(self, secret=None, hashfunc=None):
        """secret: 32 bytes (os.urandom(32) when None); clamped by the library as make_private does.
        hashfunc: bytes -> 32 bytes, run on the host per item; None for sha256(b"curve25519" + value)
        on the GPU. Needs no GPU."""
        if secret is not None:
            if not isinstance(secret, bytes) or len(secret) != 32:
                raise TypeError("secret must be 32-byte string")
            self._private = secret
        else:
            self._private = os.urandom(32)
        self._hashfunc = hashfunc
        if hashfunc is not None:
            t = hashfunc(b'test')
            if not isinstance(t, bytes) or len(t) != 32:
                raise TypeError("the return value of hashfunc  must be 32 bytes!")

    def sign_hash_list(self, values):
        """X25519(secret, hash(value)) for every byte string of `values`, as a list of 32-byte bytes."""
        values = list(values)
        if not values:
            return []
        if self._hashfunc is not None:
            return self.sign_list([self._hashfunc(v) for v in values], _what="hashfunc's result")
        chars, offsets = ecc_cipher.pack_strings(values)
        return ecc_cipher.bytes_from_rows(ecc_cipher.x25519_hash(self._private, chars, offsets))

    def sign_list(self, values, _what="sign"):
        """X25519(secret, value) for every 32-byte string of `values`; ValueError naming the index of
        an item that is not 32 bytes."""
        values = list(values)
        if not values:
            return []
        rows = ecc_cipher.rows_from_bytes(values, _what)
        return ecc_cipher.bytes_from_rows(ecc_cipher.x25519(self._private, rows))

    def sign_hash(self, value):
        """sign random bytes array, return 32-bytes"""
        return self.sign_hash_list([value])[0]

    def sign(self, value):
        """sign 32-bytes array, return 32-bytes"""
        return self.sign_list([value])[0]
