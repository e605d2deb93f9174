"""RSA blind-signature PSI signers on the GPU, with the names of the reference's
(efls-data/xfl/data/psi/rsa_signer.py): RsaSigner, ServerRsaSigner, ClientRsaSigner.

The server signs the full-domain hash of its own IDs, and the blinded hashes a client sends; the
client blinds its hashes with fresh random numbers, has them signed and unblinds. Both end with a
one-way hash of the signature, and equal IDs give equal strings. The hashes, every modular
exponentiation, the blinding and the unblinding run on the GPU (efl.psi.rsa_cipher.RsaKey); byte
strings on the wire are the reference's, int(v).to_bytes(n.bit_length() // 8, 'little').

Deviations from the reference, all at its edges:
  - Keys are PKCS#1 PEM / DER read and written by efl.psi.pkcs1 (the `rsa` package is not needed);
    load_key returns its named tuples (fields n, e and, private, d, p, q).
  - The final one-way hash is a constructor argument, `oneway_hash=`: a callable from str to int, or
    the name of a device hash (rsa_cipher.ONEWAY_HASHES: "sha256", whose host twin is
    rsa_cipher.oneway_sha256). The default, None, is cityhash.CityHash64, imported when a hash first
    runs. It hashes the DECIMAL text of each signature: with a name the text and the hash are made
    on the GPU (efl_rsa_oneway); with a callable the batch methods below take the text from the GPU
    (efl_rsa_decimal) and call the hash once per string.
  - sign_rows, sign_blinded_rows, blind_rows and deblind_rows are the signers over device tensors:
    a batch is never cut into Python ints, and a signed ID is a row of a uint8 [n, 8] tensor (the
    64-bit hash little-endian; rsa_cipher.oneway_text gives the reference's byte string), what an
    IdStore(8) and efl.psi.rsa_join take.
  - oneway_hash_list and rsa_sign_list are methods, not static: the first needs the hash, the second
    signs by CRT with the loaded private key (d and n, when given, must be that key's).
  - sign_blinded_ids_from_client takes items shorter than the key's row (zero-extended) and values
    >= n (reduced, as powmod does), and refuses items longer than the row with InvalidArgumentError,
    where the reference would sign any length.
  - A value that n.bit_length() // 8 bytes do not hold (possible when n's length is no multiple of 8
    bits) raises the reference's OverflowError wherever it would cross the wire, on the client
    (_blind_ids) as on the server (sign_blinded_ids_from_client); nothing is ever cut short.
  - _deblind_signed_ids raises InvalidArgumentError naming the first blind number without an inverse
    (the reference's divm raises ZeroDivisionError).
  - _blind_ids draws its 256-bit blind numbers from os.urandom (the reference: random.SystemRandom,
    the same source) and redraws a zero; blind_numbers= fixes them for tests.
"""
from __future__ import annotations

import hashlib
import math
import os
import secrets

import numpy as np
import torch

from efl import errors
from efl.psi import pkcs1
from efl.psi import rsa_cipher
from efl.psi.rsa_cipher import RsaKey


def bytes2int(byte, byteorder='little'):
    return int.from_bytes(byte, byteorder)


def int2bytes(digit, byte_len, byteorder='little'):
    return int(digit).to_bytes(byte_len, byteorder)


def wire_bytes(row, byte_len):
    """int2bytes(v, byte_len) of a row's little-endian bytes: the first byte_len of them, or the
    reference's OverflowError when a byte at or past byte_len is not zero. byte_len is
    n.bit_length() // 8, which holds every value below n only when n's length is a multiple of 8 bits."""
    if any(row[byte_len:]):
        raise OverflowError("int too big to convert")
    return bytes(row[:byte_len])


def _cityhash64(text: str) -> int:
    try:
        from cityhash import CityHash64
    except ImportError as e:
        raise ImportError(
            "efl.psi: the default one-way hash is cityhash.CityHash64 and the `cityhash` module is not "
            "installed; install it, or pass oneway_hash= (a callable from str to int) to the signer") from e
    return CityHash64(text)


class RsaSigner(object):
    """RSA signer base."""

    def __init__(self, oneway_hash=None):
        if isinstance(oneway_hash, str) and oneway_hash not in rsa_cipher.ONEWAY_HASHES:
            raise errors.InvalidArgumentError(
                f"oneway_hash {oneway_hash!r}: a callable, None, or one of {sorted(rsa_cipher.ONEWAY_HASHES)}")
        self.oneway_hash_ = oneway_hash
        self._key = None                  # RsaKey: the device context, made on first use
        self._key_numbers = None          # set by the subclasses: (n, e) or (n, e, d, p, q)

    @property
    def key_(self):
        if self._key is None and self._key_numbers is not None:
            v = self._key_numbers
            self._key = RsaKey.private(*v) if len(v) == 5 else RsaKey.public(*v)
        return self._key

    @staticmethod
    def load_key(key_bytes, is_public):
        return pkcs1.load_public(key_bytes) if is_public else pkcs1.load_private(key_bytes)

    @staticmethod
    def generate_rsa_keys(key_length=2048, reps=24):
        """(public PEM, private PEM) of a fresh key whose n has exactly key_length bits, e = 65537.
        The primes come from the native search the Paillier keygen uses (trial division, then
        efl_host_probable_primes' Miller-Rabin on host threads)."""
        from efl.privacy import paillier_cipher as pc
        if key_length < 512 or key_length % 2:
            raise errors.InvalidArgumentError("key_length must be even and at least 512")
        e, bits = 65537, key_length // 2
        rng = secrets.SystemRandom()

        def draw(avoid=None):
            while True:
                # the two top bits set: p q has exactly 2 * bits bits
                cs = [rng.getrandbits(bits) | 1 | (3 << (bits - 2)) for _ in range(64)]
                cs = [c for c in cs if c != avoid and pc._sieved(c) and math.gcd(c - 1, e) == 1]
                for c, ok in zip(cs, pc.probable_primes(cs, reps, rng)):
                    if ok:
                        return c
        p = draw()
        q = draw(p)
        if p < q:
            p, q = q, p                   # PKCS#1's qinv convention, as OpenSSL writes keys
        n = p * q
        d = pow(e, -1, (p - 1) * (q - 1))
        return pkcs1.save_public(n, e), pkcs1.save_private(n, e, d, p, q)

    @staticmethod
    def fdh(value):
        return hashlib.sha256(bytes(str(value), encoding='utf-8')).hexdigest()

    @staticmethod
    def _fdh_rows(ids, words):
        chars, offs = rsa_cipher.pack_strings(ids)
        return rsa_cipher.sha256_rows(chars, offs, words)

    @staticmethod
    def fdh_list(ids, ret_int=False):
        """sha256 of str(id) for every id, on the GPU (efl_sha256_fdh)."""
        ids = list(ids)
        vals = rsa_cipher.ints_from_rows(RsaSigner._fdh_rows(ids, 8))
        return vals if ret_int else [format(v, "064x") for v in vals]

    def oneway_hash_list(self, ids):
        if isinstance(self.oneway_hash_, str):
            return self._oneway_named_list(list(ids), self.oneway_hash_)
        h = self.oneway_hash_ or _cityhash64
        return [hex(h(str(item)))[2:].encode('utf-8') for item in ids]

    @staticmethod
    def _oneway_named_list(ids, name):
        """oneway_hash_list with a device hash: the non-negative ints below 2^4096 in one batch on the
        GPU, any other item through the host twin on str(item), as the reference would hash it."""
        twin = _HOST_TWINS[name]
        out = [None] * len(ids)
        on_device = [i for i, v in enumerate(ids)
                     if isinstance(v, int) and not isinstance(v, bool) and 0 <= v < _DEVICE_BOUND]
        if on_device:
            vals = [ids[i] for i in on_device]
            words = max(1, (max(v.bit_length() for v in vals) + 31) // 32)
            rows = rsa_cipher.oneway_rows(rsa_cipher.rows_from_ints(vals, words).to(_device()), name)
            for i, text in zip(on_device, rsa_cipher.oneway_texts(rows)):
                out[i] = text
        for i, v in enumerate(ids):
            if out[i] is None:
                out[i] = hex(twin(str(v)))[2:].encode('utf-8')
        return out

    def _oneway_rows(self, rows):
        """The one-way hash of every row of signatures as uint8 [n, 8] on the device: the device hash,
        or the decimal strings from the device through the callable (its result's 8 bytes, little-endian)."""
        if isinstance(self.oneway_hash_, str):
            return rsa_cipher.oneway_rows(rows, self.oneway_hash_)
        h = self.oneway_hash_ or _cityhash64
        vals = [int(h(s)) for s in rsa_cipher.decimal_strings(rows)]
        for i, v in enumerate(vals):
            if not 0 <= v < 2 ** 64:
                raise errors.InvalidArgumentError(f"the one-way hash of signature {i} does not fit 64 bits")
        buf = bytearray(b"".join(v.to_bytes(8, "little") for v in vals))
        host = torch.frombuffer(buf, dtype=torch.uint8).view(len(vals), 8) if vals else \
            torch.empty((0, 8), dtype=torch.uint8)
        return host.to(_device())

    def rsa_sign_list(self, ids, d=None, n=None):
        """[x^d mod n] as ints, by CRT on the GPU with the loaded private key."""
        key = self.key_
        if key is None or not key.has_private:
            raise errors.AbortedError("No private key.")
        prv = getattr(self, "rsa_private_key_", None)
        if (n is not None and int(n) != key.n) or (d is not None and prv is not None and int(d) != prv.d):
            raise errors.InvalidArgumentError("rsa_sign_list signs with the loaded key: d and n must be its own")
        ids = [int(x) % key.n for x in ids]
        rows = rsa_cipher.rows_from_ints(ids, key.words)
        return rsa_cipher.ints_from_rows(key.sign(rows.to(_device())))


def _device():
    from efl import lib
    return lib.require_gpu()


_HOST_TWINS = {"sha256": rsa_cipher.oneway_sha256}
_DEVICE_BOUND = 1 << (32 * rsa_cipher.MAX_DECIMAL_WORDS)


class ServerRsaSigner(RsaSigner):
    def __init__(self, rsa_public_key_bytes=None, rsa_private_key_bytes=None, oneway_hash=None):
        """When keys are not specified, the signer generates a pair."""
        super().__init__(oneway_hash)
        if rsa_public_key_bytes is None or rsa_private_key_bytes is None:
            self.pub_key_bytes_, self.prv_key_bytes_ = self.generate_rsa_keys()
        else:
            self.pub_key_bytes_, self.prv_key_bytes_ = rsa_public_key_bytes, rsa_private_key_bytes
        self.rsa_public_key_ = RsaSigner.load_key(self.pub_key_bytes_, True)
        prv = self.rsa_private_key_ = RsaSigner.load_key(self.prv_key_bytes_, False)
        if (prv.n, prv.e) != (self.rsa_public_key_.n, self.rsa_public_key_.e):
            raise errors.InvalidArgumentError("the public and the private key are not one pair")
        self._key_numbers = (prv.n, prv.e, prv.d, prv.p, prv.q)

    def sign_func(self, ids):
        rows = RsaSigner._fdh_rows(list(ids), self.key_.words)
        signed = rsa_cipher.ints_from_rows(self.key_.sign(rows))
        return self.oneway_hash_list(signed)

    def sign_blinded_ids_from_client(self, ids):
        key = self.key_
        W, byte_len = key.words, key.byte_len
        ids = list(ids)
        for i, item in enumerate(ids):
            if len(item) > 4 * W:
                raise errors.InvalidArgumentError(
                    f"blinded id {i} has {len(item)} bytes, more than the key's row of {4 * W}")
        buf = b"".join(bytes(item).ljust(4 * W, b"\0") for item in ids)
        rows = torch.frombuffer(bytearray(buf), dtype=torch.int32).view(len(ids), W) if ids else \
            torch.zeros((0, W), dtype=torch.int32)
        out = key.sign(rows.to(_device())).cpu().contiguous().numpy().tobytes()
        # a signature is below n, but n.bit_length() // 8 bytes hold it only when n's length is a
        # multiple of 8 bits (the reference's int2bytes raises OverflowError otherwise)
        return [wire_bytes(out[i * 4 * W:(i + 1) * 4 * W], byte_len) for i in range(len(ids))]

    def sign_rows(self, ids):
        """sign_func over tensors: uint8 [n, 8] on the device, row i the one-way hash of the signature of
        ids[i] (oneway_text of it is sign_func's item i)."""
        key = self.key_
        return self._oneway_rows(key.sign(RsaSigner._fdh_rows(list(ids), key.words)))

    def sign_blinded_rows(self, rows):
        """PsiSign over tensors: the signatures of `int32` [n, words] rows of blinded hashes, where the
        rows were."""
        t = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(rows)
        if t.dtype != torch.int32:
            raise errors.InvalidArgumentError(f"sign_blinded_rows: rows must be int32 [n, words], got {t.dtype}")
        return self.key_.sign(t)

    def get_public_key_bytes(self):
        return self.pub_key_bytes_


class ClientRsaSigner(RsaSigner):
    def __init__(self, rsa_public_key_bytes, oneway_hash=None):
        super().__init__(oneway_hash)
        self.rsa_public_key_ = RsaSigner.load_key(rsa_public_key_bytes, True)
        self._key_numbers = (self.rsa_public_key_.n, self.rsa_public_key_.e)

    def sign_func(self, ids, data_join_cli, bucket_id):
        hashed_ids = RsaSigner.fdh_list(ids, True)
        blinded_hashed_ids, blind_numbers = self._blind_ids(hashed_ids)
        signed_blinded_hashed_ids = data_join_cli.sign_blinded_ids_from_server(blinded_hashed_ids, bucket_id)
        return self._deblind_signed_ids(signed_blinded_hashed_ids, blind_numbers)

    @staticmethod
    def _draw_blind_number():
        while True:
            r = int.from_bytes(os.urandom(32), "little")
            if r:
                return r

    def _wire(self, rows):
        key = self.key_
        W, byte_len = key.words, key.byte_len
        raw = rows.cpu().contiguous().numpy().tobytes()
        # a blinded value is below n: the server's rule (a value cut short would lose its ID silently)
        return [wire_bytes(raw[i * 4 * W:(i + 1) * 4 * W], byte_len) for i in range(rows.shape[0])]

    def _blind_ids(self, ids, blind_numbers=None):
        key = self.key_
        ids = [int(x) for x in ids]
        if blind_numbers is None:
            blind_numbers = [self._draw_blind_number() for _ in ids]
        blind_numbers = [int(r) for r in blind_numbers]
        if len(blind_numbers) != len(ids):
            raise errors.InvalidArgumentError("as many blind numbers as ids")
        dev = _device()
        h = rsa_cipher.rows_from_ints(ids, key.words).to(dev)
        r = rsa_cipher.rows_from_ints(blind_numbers, key.words).to(dev)
        return self._wire(key.blind(h, r)), blind_numbers

    def blind_rows(self, ids, blind_numbers=None):
        """_blind_ids over tensors: (blinded, r), both `int32` [n, words] on the device; blinded goes to
        the server's sign_blinded_rows, r stays here for deblind_rows. The 256-bit blind numbers are
        one os.urandom(32 n), a zero redrawn; blind_numbers= fixes them for tests."""
        key = self.key_
        ids = list(ids)
        n, W = len(ids), key.words
        if blind_numbers is None:
            a = np.frombuffer(os.urandom(32 * n), dtype="<i4").reshape(n, 8).copy()
            for i in np.flatnonzero(~a.any(axis=1)):
                a[i] = np.frombuffer(int2bytes(self._draw_blind_number(), 32), dtype="<i4")
            r = torch.zeros((n, W), dtype=torch.int32)
            r[:, :8] = torch.from_numpy(a)
        else:
            blind_numbers = [int(x) for x in blind_numbers]
            if len(blind_numbers) != n:
                raise errors.InvalidArgumentError("as many blind numbers as ids")
            r = rsa_cipher.rows_from_ints(blind_numbers, W)
        r = r.to(_device())
        return key.blind(RsaSigner._fdh_rows(ids, W), r), r

    def deblind_rows(self, signed, r):
        """_deblind_signed_ids over tensors: uint8 [n, 8] on the device, the one-way hash of signed
        r^-1 mod n. InvalidArgumentError naming the first blind number without an inverse."""
        return self._oneway_rows(self.key_.unblind(signed, r))

    def _deblind_signed_ids(self, signed_blinded_hashed_ids, blind_numbers):
        key = self.key_
        dev = _device()
        s = rsa_cipher.rows_from_ints([bytes2int(item) for item in signed_blinded_hashed_ids], key.words).to(dev)
        r = rsa_cipher.rows_from_ints(blind_numbers, key.words).to(dev)
        signed_hashed_ids = rsa_cipher.ints_from_rows(key.unblind(s, r))
        return self.oneway_hash_list(signed_hashed_ids)
