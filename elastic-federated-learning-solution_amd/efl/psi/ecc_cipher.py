"""X25519 over torch tensors: efl_x25519 / efl_x25519_hash of libefl_hip.so (include/efl_hip.h).

This is the level a caller with millions of IDs uses: points are rows of a `uint8` [n, 32] tensor,
on the host or on the device, and the result comes back in the form it was given. The scalar is 32
bytes on the host; the library clamps it (RFC 7748 §5), so a clamped and an unclamped secret that
clamp alike give the same rows. efl.psi.ecc_signer.EccSigner is a thin list-of-bytes wrapper.
"""
from __future__ import annotations

import torch

from efl import errors
from efl import lib as _efl_lib
from efl.psi.rsa_cipher import pack_strings  # noqa: F401  (the packed form x25519_hash takes)

_lib = _efl_lib.raw()

PREFIX = b"curve25519"      # the reference's _hash_value: sha256(b"curve25519" + value)


def _scalar(scalar) -> bytes:
    if not isinstance(scalar, (bytes, bytearray)) or len(scalar) != 32:
        raise errors.InvalidArgumentError("x25519: the scalar must be 32 bytes")
    return bytes(scalar)


def x25519(scalar: bytes, rows) -> torch.Tensor:
    """X25519(scalar, row) for every row of a uint8 [n, 32] tensor (RFC 7748: bit 255 of a row is
    ignored, values of p and above are accepted, a low-order point gives 32 zero bytes)."""
    k = _scalar(scalar)
    t = _efl_lib.as_tensor(rows)
    if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != 32:
        raise errors.InvalidArgumentError(f"x25519: rows must be uint8 [n, 32], got {t.dtype} {tuple(t.shape)}")
    if t.shape[0] == 0:
        return torch.empty_like(t)
    d, home = _efl_lib.on_device(t)
    if d.data_ptr() % 16:
        d = d.clone()
    out = torch.empty_like(d)
    _efl_lib.check(_lib.efl_x25519(k, d.data_ptr(), out.data_ptr(), d.shape[0], _efl_lib.stream_handle(d.device)))
    return _efl_lib.back(out, home)


def x25519_hash(scalar: bytes, chars, offsets, prefix: bytes = PREFIX) -> torch.Tensor:
    """X25519(scalar, sha256(prefix + string i)) as row i of a uint8 [n, 32] tensor, for n byte strings
    packed back to back (chars uint8 / int8, offsets int64 [n + 1]; pack_strings makes them). The
    result is on the device when either input is, on the host otherwise."""
    k = _scalar(scalar)
    prefix = bytes(prefix)
    chars, offsets = _efl_lib.as_tensor(chars), _efl_lib.as_tensor(offsets)
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1:
        raise errors.InvalidArgumentError("x25519_hash: offsets must be int64 [n + 1]")
    if chars.dtype not in (torch.uint8, torch.int8):
        raise errors.InvalidArgumentError("x25519_hash: chars must be bytes")
    n = offsets.numel() - 1
    home = chars.device if chars.is_cuda else offsets.device
    if n == 0:
        return torch.empty((0, 32), dtype=torch.uint8, device=home)
    dev = home if home.type == "cuda" else _efl_lib.require_gpu()
    c = chars.contiguous().to(dev)
    if c.numel() == 0:
        c = torch.zeros(1, dtype=torch.uint8, device=dev)     # never a null buffer
    o = offsets.contiguous().to(dev)
    out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    _efl_lib.check(_lib.efl_x25519_hash(k, prefix, len(prefix), c.data_ptr(), o.data_ptr(), out.data_ptr(), n,
                                        _efl_lib.stream_handle(dev)))
    return _efl_lib.back(out, home)


def rows_from_bytes(items, what="x25519") -> torch.Tensor:
    """Host uint8 [n, 32] tensor of 32-byte strings; ValueError naming the first item that is not one."""
    for i, v in enumerate(items):
        if not isinstance(v, (bytes, bytearray)) or len(v) != 32:
            raise ValueError(f"{what}: item {i} is not a 32-byte string")
    return torch.frombuffer(bytearray(b"".join(items)), dtype=torch.uint8).reshape(len(items), 32)


def bytes_from_rows(rows: torch.Tensor) -> list:
    raw = rows.detach().cpu().contiguous().numpy().tobytes()
    return [raw[i:i + 32] for i in range(0, len(raw), 32)]
