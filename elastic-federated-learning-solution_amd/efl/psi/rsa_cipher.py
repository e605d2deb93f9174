"""RsaKey: the RSA key context of libefl_hip.so (include/efl_hip.h, efl_rsa_*) over torch tensors.

This is the level a caller with millions of IDs uses: numbers are rows of a device tensor, `int32`
[n, words] (little-endian 32-bit words) or `uint8` [n, bytes] (the reference's wire form,
int(v).to_bytes(byte_len, 'little'); [n, 4 * words] bytes are the same memory as [n, words] words,
shorter rows are zero-extended, down to (n.bit_length() + 7) // 8 bytes: narrower rows could not hold
every result and are refused). Every method returns rows of the form it was given. The signers of
efl.psi.rsa_signer are thin list-of-int wrappers over it.

Beside the key: the tail of a signature, hex(OneWayHash(str(v)))[2:] in the reference. decimal_rows is
Python's str(int) of every row on the device (efl_rsa_decimal), oneway_rows a 64-bit one-way hash over
that text as uint8 [n, 8] rows (efl_rsa_oneway; ONEWAY_HASHES names the device's hashes, oneway_sha256
is the host twin), oneway_text a row's reference byte string.
"""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np
import torch

from efl import errors
from efl import lib as _efl_lib

_lib = _efl_lib.raw()
_vp = ctypes.c_void_p     # the entry points' ctypes declarations are in efl/lib.py


class RsaCtxInfo(ctypes.Structure):
    """ctypes mirror of efl_rsa_ctx_info (include/efl_hip.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("has_public", "has_private", "n_bits", "words", "byte_len",
                                               "reserved")] + [("e", ctypes.c_uint64)]


def _hx(x: int) -> bytes:
    return format(int(x), "x").encode()


def pack_strings(items):
    """(chars uint8, offsets int64) host tensors of byte strings packed back to back."""
    bs = [s if isinstance(s, (bytes, bytearray)) else str(s).encode("utf-8") for s in items]
    offs = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bs], out=offs[1:])
    chars = np.frombuffer(b"".join(bs) or b"\0", dtype=np.uint8).copy()   # never a null buffer
    return torch.from_numpy(chars), torch.from_numpy(offs)


def sha256_rows(chars: torch.Tensor, offsets: torch.Tensor, words: int = 8) -> torch.Tensor:
    """int(sha256(string i).hexdigest(), 16) as row i of an int32 [n, words] device tensor
    (efl_sha256_fdh); chars uint8 / int8, offsets int64 with n + 1 entries."""
    dev = _efl_lib.require_gpu()
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1:
        raise errors.InvalidArgumentError("fdh: offsets must be int64 [n + 1]")
    if chars.dtype not in (torch.uint8, torch.int8):
        raise errors.InvalidArgumentError("fdh: chars must be bytes")
    n = offsets.numel() - 1
    out = torch.empty((n, words), dtype=torch.int32, device=dev)
    if n == 0:
        return out
    c = chars.contiguous().to(dev)
    if c.numel() == 0:
        c = torch.zeros(1, dtype=torch.uint8, device=dev)
    o = offsets.contiguous().to(dev)
    _efl_lib.check(_lib.efl_sha256_fdh(c.data_ptr(), o.data_ptr(), out.data_ptr(), words, n,
                                       _efl_lib.stream_handle(dev)))
    return out


def rows_from_ints(values, words: int) -> torch.Tensor:
    """Host int32 [n, words] tensor of non-negative Python ints below 2^(32 words)."""
    buf = b"".join(int(v).to_bytes(4 * words, "little") for v in values)
    a = np.frombuffer(buf, dtype="<i4").reshape(len(values), words) if values else np.zeros((0, words), "<i4")
    return torch.from_numpy(a.copy())


def ints_from_rows(rows: torch.Tensor) -> list:
    """Python ints of int32 / uint8 rows (little-endian)."""
    a = rows.detach().cpu().contiguous().numpy()
    raw = a.tobytes()
    k = a.shape[1] * a.itemsize if a.ndim == 2 and a.shape[0] else 0
    return [int.from_bytes(raw[i * k:(i + 1) * k], "little") for i in range(a.shape[0])]


# ---- the tail of a signature: decimal text and one-way hash (efl_rsa_decimal, efl_rsa_oneway) ----

MAX_DECIMAL_WORDS = 128
# the device's one-way hashes by name: the `hash` argument of efl_rsa_oneway
ONEWAY_HASHES = {"sha256": 1}


def oneway_sha256(text: str) -> int:
    """The host twin of ONEWAY_HASHES["sha256"] (EFL_ONEWAY_SHA256_64), a callable for the signers'
    oneway_hash=: the first 8 bytes of sha256(text) as a big-endian number."""
    return int.from_bytes(hashlib.sha256(text.encode("utf-8")).digest()[:8], "big")


def oneway_text(row8) -> bytes:
    """The reference's byte string hex(v)[2:] of one row of oneway_rows (8 bytes, v little-endian)."""
    if isinstance(row8, torch.Tensor):
        row8 = row8.detach().cpu().contiguous().numpy().tobytes()
    row8 = bytes(row8)
    if len(row8) != 8:
        raise errors.InvalidArgumentError(f"oneway_text: a row is 8 bytes, got {len(row8)}")
    return hex(int.from_bytes(row8, "little"))[2:].encode()


def oneway_texts(rows8) -> list:
    """oneway_text of every row of a uint8 [n, 8] tensor: one copy to the host."""
    raw = rows8.detach().cpu().contiguous().numpy().tobytes()
    return [hex(int.from_bytes(raw[o:o + 8], "little"))[2:].encode() for o in range(0, len(raw), 8)]


def _number_rows(rows, what):
    """Device int32 [n, words] rows of `int32` [n, words] or `uint8` [n, bytes] rows (the bytes
    zero-extended to whole words), 1 <= words <= 128: the forms RsaKey._rows takes, without a key."""
    t = _efl_lib.as_tensor(rows)
    if t.dim() != 2:
        raise errors.InvalidArgumentError(f"{what}: rows must be a 2-D tensor, got shape {tuple(t.shape)}")
    if t.dtype not in (torch.int32, torch.uint8):
        raise errors.InvalidArgumentError(f"{what}: rows must be int32 or uint8, got {t.dtype}")
    words = t.shape[1] if t.dtype == torch.int32 else (t.shape[1] + 3) // 4
    if not 1 <= words <= MAX_DECIMAL_WORDS:
        raise errors.InvalidArgumentError(
            f"{what}: rows of {t.shape[1]} {'words' if t.dtype == torch.int32 else 'bytes'}: a number has 1 to "
            f"{MAX_DECIMAL_WORDS} words")
    d, _ = _efl_lib.on_device(t)
    if d.dtype == torch.uint8:
        if d.shape[1] % 4:
            d = torch.nn.functional.pad(d, (0, 4 * words - d.shape[1]))
        if d.data_ptr() % 4:
            d = d.clone()
        d = d.view(torch.int32)
    elif d.data_ptr() % 4:
        d = d.clone()
    return d, words


def decimal_rows(rows, stride=None):
    """Python's str(int) of every row on the device (efl_rsa_decimal): (text uint8 [n, stride], len
    int32 [n]); row i's digits are text[i, stride - len[i]:], the bytes before them are b"0". stride
    defaults to efl_rsa_decimal_digits(words), the most digits a row can have."""
    d, words = _number_rows(rows, "decimal_rows")
    digits = int(_lib.efl_rsa_decimal_digits(words))
    stride = digits if stride is None else int(stride)
    if stride < digits:
        raise errors.InvalidArgumentError(f"decimal_rows: stride {stride} is below the {digits} digits of {words} words")
    n = d.shape[0]
    text = torch.empty((n, stride), dtype=torch.uint8, device=d.device)
    ln = torch.empty(n, dtype=torch.int32, device=d.device)
    if n:
        _efl_lib.check(_lib.efl_rsa_decimal(d.data_ptr(), words, n, text.data_ptr(), stride, ln.data_ptr(),
                                            _efl_lib.stream_handle(d.device)))
    return text, ln


def decimal_strings(rows) -> list:
    """[str(v)] of the rows: decimal_rows, one copy to the host, then slices."""
    text, ln = decimal_rows(rows)
    stride = text.shape[1]
    raw = text.cpu().numpy().tobytes()
    return [raw[(i + 1) * stride - k:(i + 1) * stride].decode("ascii") for i, k in enumerate(ln.tolist())]


def oneway_rows(rows, hash="sha256") -> torch.Tensor:
    """uint8 [n, 8] on the device: ONEWAY_HASHES[hash] of str(v) of every row, the 64-bit value
    little-endian (efl_rsa_oneway); rows for an IdStore(8), oneway_text gives a row's reference form."""
    if hash not in ONEWAY_HASHES:
        raise errors.InvalidArgumentError(f"oneway_rows: hash {hash!r} is not one of {sorted(ONEWAY_HASHES)}")
    d, words = _number_rows(rows, "oneway_rows")
    n = d.shape[0]
    out = torch.empty((n, 8), dtype=torch.uint8, device=d.device)
    if n:
        _efl_lib.check(_lib.efl_rsa_oneway(d.data_ptr(), words, n, ONEWAY_HASHES[hash], out.data_ptr(),
                                           _efl_lib.stream_handle(d.device)))
    return out


class RsaKey:
    """An RSA key on the GPU: rsa.PublicKey / rsa.PrivateKey of the reference's signers."""

    def __init__(self):
        h = _vp()
        _efl_lib.check(_lib.efl_rsa_ctx_create(ctypes.byref(h)))
        self._h = h
        self.n = self.e = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.efl_rsa_ctx_destroy(h)

    @classmethod
    def public(cls, n: int, e: int) -> "RsaKey":
        k = cls()
        k.set_public(n, e)
        return k

    @classmethod
    def private(cls, n: int, e: int, d: int, p: int, q: int) -> "RsaKey":
        k = cls()
        k.set_private(n, e, d, p, q)
        return k

    def set_public(self, n: int, e: int) -> None:
        dev = _efl_lib.require_gpu()
        _efl_lib.check(_lib.efl_rsa_set_public(self._h, _hx(n), _hx(e), _efl_lib.stream_handle(dev)))
        self.n, self.e = int(n), int(e)

    def set_private(self, n: int, e: int, d: int, p: int, q: int) -> None:
        """The context keeps d mod (p - 1), d mod (q - 1) and q^-1 mod p on the device; this object
        keeps no private number."""
        dev = _efl_lib.require_gpu()
        _efl_lib.check(_lib.efl_rsa_set_private(self._h, _hx(n), _hx(e), _hx(d), _hx(p), _hx(q),
                                                _efl_lib.stream_handle(dev)))
        self.n, self.e = int(n), int(e)

    def info(self) -> RsaCtxInfo:
        i = RsaCtxInfo()
        _efl_lib.check(_lib.efl_rsa_ctx_query(self._h, ctypes.byref(i)))
        return i

    @property
    def words(self) -> int:
        return self.info().words

    @property
    def byte_len(self) -> int:
        """n.bit_length() // 8: the length of the reference's wire byte strings."""
        return self.info().byte_len

    @property
    def has_private(self) -> bool:
        return bool(self.info().has_private)

    # ---- rows ------------------------------------------------------------------------------
    def _rows(self, t, what):
        """Device int32 [n, words] view (or zero-extended copy) of `t`, and how to give a result back.

        uint8 rows come back at the width they were given, so they must hold any result, a value
        below n: at least (n.bit_length() + 7) // 8 bytes. Narrower rows are refused (by shape, before
        anything runs): n.bit_length() // 8 bytes, the reference's wire length, hold every value only
        when n's length is a multiple of 8 bits; for other keys pass wider rows, or int32 rows."""
        info = self.info()
        W = info.words
        if W == 0:
            raise errors.AbortedError("No public key.")
        t = _efl_lib.as_tensor(t)
        if t.dim() != 2:
            raise errors.InvalidArgumentError(f"{what}: rows must be a 2-D tensor, got shape {tuple(t.shape)}")
        d, home = _efl_lib.on_device(t)
        if d.dtype == torch.int32:
            if d.shape[1] != W:
                raise errors.InvalidArgumentError(f"{what}: int32 rows have {d.shape[1]} words, the key's have {W}")
            return (d.clone() if d.data_ptr() % 16 else d), (torch.int32, W, home)
        if d.dtype != torch.uint8:
            raise errors.InvalidArgumentError(f"{what}: rows must be int32 or uint8, got {d.dtype}")
        B = d.shape[1]
        if B > 4 * W:
            raise errors.InvalidArgumentError(f"{what}: rows of {B} bytes are longer than the key's {4 * W}")
        if B < (info.n_bits + 7) // 8:
            raise errors.InvalidArgumentError(
                f"{what}: uint8 rows of {B} bytes cannot hold every value below an n of {info.n_bits} bits; "
                f"pass rows of at least {(info.n_bits + 7) // 8} bytes")
        if B < 4 * W:
            d = torch.nn.functional.pad(d, (0, 4 * W - B))
        if d.data_ptr() % 16:
            d = d.clone()
        return d.view(torch.int32), (torch.uint8, B, home)

    @staticmethod
    def _give(out, form):
        dtype, width, home = form
        if dtype == torch.uint8:
            out = out.view(torch.uint8)[:, :width].contiguous()
        return _efl_lib.back(out, home)

    def sign(self, x):
        """x^d mod n for every row (ServerRsaSigner's powmod(x, d, n)); AbortedError without a
        private key."""
        xr, form = self._rows(x, "sign")
        out = torch.empty_like(xr)
        _efl_lib.check(_lib.efl_rsa_sign(self._h, xr.data_ptr(), out.data_ptr(), xr.shape[0],
                                         _efl_lib.stream_handle(xr.device)))
        return self._give(out, form)

    def blind(self, h, r):
        """r^e h mod n for every row (ClientRsaSigner._blind_ids)."""
        hr, form = self._rows(h, "blind")
        rr, _ = self._rows(r, "blind")
        if rr.shape != hr.shape or rr.device != hr.device:
            raise errors.InvalidArgumentError("blind: h and r must have as many rows, on one device")
        out = torch.empty_like(hr)
        _efl_lib.check(_lib.efl_rsa_blind(self._h, hr.data_ptr(), rr.data_ptr(), out.data_ptr(), hr.shape[0],
                                          _efl_lib.stream_handle(hr.device)))
        return self._give(out, form)

    def unblind(self, s, r, check=True):
        """s r^-1 mod n for every row (divm(s, r, n), ClientRsaSigner._deblind_signed_ids).
        InvalidArgumentError naming the first row whose r has no inverse mod n; check=False returns
        (rows, that index or -1) instead, the rows without an inverse zero."""
        sr, form = self._rows(s, "unblind")
        rr, _ = self._rows(r, "unblind")
        if rr.shape != sr.shape or rr.device != sr.device:
            raise errors.InvalidArgumentError("unblind: s and r must have as many rows, on one device")
        out = torch.empty_like(sr)
        if sr.shape[0] == 0:
            return self._give(out, form) if check else (self._give(out, form), -1)
        bad = torch.empty(1, dtype=torch.int64, device=sr.device)
        _efl_lib.check(_lib.efl_rsa_unblind(self._h, sr.data_ptr(), rr.data_ptr(), out.data_ptr(), sr.shape[0],
                                            bad.data_ptr(), _efl_lib.stream_handle(sr.device)))
        b = int(bad.item())
        if not check:
            return self._give(out, form), b
        if b >= 0:
            raise errors.InvalidArgumentError(f"unblind: blind number {b} has no inverse mod n")
        return self._give(out, form)

    def fdh(self, chars, offsets):
        """The full-domain hash int(sha256(id).hexdigest(), 16) of packed byte strings as int32
        [n, words] rows of this key (device)."""
        W = self.words
        if W == 0:
            raise errors.AbortedError("No public key.")
        return sha256_rows(_efl_lib.as_tensor(chars), _efl_lib.as_tensor(offsets), W)
