"""The operand domain of the Stage P ops, for tests (a plain helper, no fixtures).

A ciphertext operand arrives as hex text from a peer and is parsed into 2 ln 32-bit words
(hex_to_limbs(hx, k.lc)), so the kernels can be handed any integer below T = 2^(32 words), not only
the valid ciphertexts (units below M = n^2) the other Paillier tests draw. The reference passes the
same text to mpz_mul / mpz_mod / mpz_powm / mpz_invert, which are defined for every integer.
operands() lists one representative of every class of that domain: units and non-units, below M
and at or above it, up to T - 1, and, for a key that runs zero-padded in a larger limb class,
values hundreds of bits above the modulus.
"""
from __future__ import annotations

import math
from typing import NamedTuple


class Operand(NamedTuple):
    label: str
    x: int
    unit: bool       # gcd(x, n) == 1: x has an inverse mod n^2
    reduced: bool    # x < n^2


def limb_class(n: int) -> int:
    """ln (32-bit words of n) of the kernel class a key runs in: the smallest of 16 .. 256 that
    holds n (efl.privacy.paillier_cipher._LIMB_CLASSES)."""
    for ln in (16, 32, 64, 128, 256):
        if n.bit_length() <= 32 * ln:
            return ln
    raise ValueError("n wider than 8192 bits")


def operands(n: int, p: int, q: int, words: int) -> list[Operand]:
    """Labelled ints below T = 2^(32 words), M = n^2, words = 2 ln of the key's class; the order
    is fixed (unit edges, non-units, then the values at or above M). A value that does not fit
    below T, or that repeats an earlier one, is left out."""
    M, T = n * n, 1 << (32 * words)
    assert M < T
    c = (1 << 64) + 1
    half = ((M - 2) >> 1) | 1                      # a unit of about M / 2 (made one below)
    while math.gcd(half, n) != 1:
        half += 2
    raw = [("1", 1), ("2", 2), ("M-1", M - 1), ("M-2", M - 2), ("2^64+1", c),
           ("0", 0), ("n", n), ("p", p), ("3q", 3 * q), ("p^2", p * p), ("n(n-1)", n * (n - 1)),   # = M - n
           ("M", M), ("M+1", M + 1), ("M+n", M + n), ("M+(2^64+1)", M + c), ("M+c", M + half),
           ("T-1", T - 1), ("2^(32w-1)", T >> 1)]
    if T // M >= 2:                                # a padded class (or an n^2 short of its top word)
        k = (T // M).bit_length() - 1
        while c + (M << k) >= T:
            k -= 1
        raw += [(f"c+M*2^{k}", c + (M << k)), ("floor((T-1)/M)*M+1", (T - 1) // M * M + 1),
                ("floor((T-1)/M)*M", (T - 1) // M * M), ("floor((T-1)/M)*M+n", (T - 1) // M * M + n)]
    out, seen = [], set()
    for label, x in raw:
        if 0 <= x < T and x not in seen:
            seen.add(x)
            out.append(Operand(label, x, math.gcd(x, n) == 1, x < M))
    return out


def tile(items: list, count: int) -> list:
    """The list first, then repeated up to `count` elements (never fewer than the list)."""
    out = list(items)
    i = 0
    while len(out) < count:
        out.append(items[i % len(items)])
        i += 1
    return out


def rotate(items: list, r: int) -> list:
    r %= len(items)
    return items[r:] + items[:r]


def first_mismatch(got: list, want: list, ops: list[Operand]) -> str:
    """'' when got == want, else the first differing element's index and operand label."""
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            o = ops[i % len(ops)]
            return f"element {i} ({o.label}, unit={o.unit}, reduced={o.reduced}): got {g:x}, want {w:x}"
    return "" if len(got) == len(want) else f"{len(got)} results for {len(want)} operands"
