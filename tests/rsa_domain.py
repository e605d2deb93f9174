"""The key and operand domain of the RSA PSI kernels, for tests (a plain helper, no fixtures).

efl_rsa_set_private takes any odd n of 16 to 4096 bits with two distinct odd primes, any e below 2^64
and any d that inverts it mod p - 1 and mod q - 1; a row handed to sign, blind or unblind may hold any
value below T = 2^(32 W). tests/golden/rsa_domain.json (made by tests/golden/make_rsa_domain_golden.py)
holds keys only; this module lists, for a key, one operand of every class of that domain and computes
what the kernels must return with Python integers. Shared by tests/test_rsa_domain_host.py and
tests/test_rsa_domain_gpu.py.
"""
from __future__ import annotations

import json
import math
import os
import random
from typing import NamedTuple, Optional

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "rsa_domain.json")
K_WIN = 5                     # csrc/powm28.h kWin


class Key(NamedTuple):
    name: str
    why: str
    n: int
    e: int
    d: Optional[int]
    p: Optional[int]
    q: Optional[int]

    @property
    def private(self) -> bool:
        return self.d is not None

    @property
    def W(self) -> int:
        """Words of a row: the class of n (csrc/rsaset.hip class_of)."""
        return next(c for c in (32, 64, 128) if 32 * c >= self.n.bit_length())

    @property
    def L(self) -> int:
        """Words of the primes' class: W / 2 for balanced primes, W when one is longer than that."""
        return next(c for c in (16, 32, 64) if 32 * c >= max(self.p.bit_length(), self.q.bit_length()))

    @property
    def wide(self) -> bool:
        return self.W == 2 * self.L

    @property
    def byte_len(self) -> int:
        return self.n.bit_length() // 8

    @property
    def dp(self) -> int:
        return self.d % (self.p - 1)

    @property
    def dq(self) -> int:
        return self.d % (self.q - 1)


def load() -> list[Key]:
    with open(FIXTURE) as f:
        raw = json.load(f)["keys"]
    return [Key(k["name"], k["why"], *(int(k[f], 16) if f in k else None for f in "nedpq")) for k in raw]


def minv(m: int, bits: int) -> int:
    """-m^-1 mod 2^bits: the Montgomery constant of the 32-bit (bits = 32) and radix-2^28 kernels."""
    return -pow(m, -1, 1 << bits) % (1 << bits)


def limbs28(m: int) -> list[int]:
    out = []
    while m:
        out.append(m & 0xFFFFFFF)
        m >>= 28
    return out


def longest_run(x: int, bit: int) -> int:
    """The longest run of `bit` among the bits below x's top bit."""
    s = format(x, "b")[1:]
    return max((len(r) for r in s.split("1" if bit == 0 else "0")), default=0)


def crt(a: int, b: int, p: int, q: int) -> int:
    """The value below p q that is a mod p and b mod q (Garner, as the kernel joins)."""
    b %= q
    return b + (a - b) * pow(q, -1, p) % p * q


def sign_expected(k: Key, x: int) -> int:
    """x^d mod n as k_rsa_sign computes it: x^(d mod (p-1)) mod p and x^(d mod (q-1)) mod q, joined."""
    return crt(pow(x, k.dp, k.p), pow(x, k.dq, k.q), k.p, k.q)


def blind_expected(k: Key, h: int, r: int) -> int:
    return pow(r, k.e, k.n) * h % k.n


def unblind_expected(k: Key, s: int, r: int) -> int:
    return s * pow(r, -1, k.n) % k.n if math.gcd(r, k.n) == 1 else 0


def sign_operands(k: Key) -> list[tuple[str, int]]:
    """Labelled sign inputs of a private key, in a fixed order; drawn values from a generator seeded
    with the key's name."""
    n, p, q, e = k.n, k.p, k.q, k.e
    T, H = 1 << (32 * k.W), 1 << (32 * k.L)
    rng = random.Random("sign " + k.name)
    borrow = pow(crt(1, 2, p, q), e, n)          # its signature is 1 mod p and 2 mod q: sp < sq mod p
    mirror = pow(crt(2, 1, p, q), e, n)
    raw = [("0", 0), ("1", 1), ("2", 2), ("n-1", n - 1), ("n", n), ("n+1", n + 1), ("T-1", T - 1),
           ("p", p), ("q", q), ("2p", 2 * p), ("3q", 3 * q), ("p+1", p + 1), ("p-1", p - 1), ("q+1", q + 1),
           ("q-1", q - 1), ("n-p", n - p), ("n-q", n - q),
           ("2^(32L)-1", H - 1), ("2^(32L)", H), ("2^(32L)+1", H + 1),
           ("1 mod p, 0 mod q", crt(1, 0, p, q)), ("0 mod p, 1 mod q", crt(0, 1, p, q)),
           ("sp < sq mod p", borrow), ("sp > sq mod p", mirror),
           ("drawn below n", rng.randrange(n)), ("drawn over the row", rng.randrange(T)),
           ("drawn multiple of q", q * rng.randrange(1, p))]
    return [(label, x) for label, x in raw if 0 <= x < T]       # equal values stay: a label names a row


def known_factor(n: int) -> Optional[int]:
    """A prime factor of n below 2000, if it has one and is not it."""
    for f in range(3, 2000, 2):
        if n % f == 0 and n != f:
            return f
    return None


def blind_lists(k: Key):
    """(h list, r list) of labelled values; blind and unblind run their cross product (unblind with
    s in the place of h). A private key's r list has a multiple of p, a public-only n's a multiple
    of a known small factor (left out when it has none, as a prime n). A value that does not fit the
    row is left out (n + 1 of an all-ones n)."""
    n, T = k.n, 1 << (32 * k.W)
    rng = random.Random("blind " + k.name)
    hs = [("0", 0), ("1", 1), ("n-1", n - 1), ("n", n), ("n+1", n + 1), ("T-1", T - 1),
          ("drawn below n", rng.randrange(n)), ("drawn over the row", rng.randrange(T))]
    f = k.p if k.private else known_factor(n)
    mult = [("multiple of a factor", f * rng.randrange(1, n // f))] if f else []
    r256 = rng.getrandbits(255) | (1 << 255)
    full = rng.getrandbits(32 * k.W - 1) | (1 << (32 * k.W - 1))
    rs = [("0", 0), ("1", 1), ("2", 2), ("n-1", n - 1), ("n", n), ("n+1", n + 1), ("T-1", T - 1)] + mult + \
        [("256-bit even", r256 & ~1), ("256-bit odd", r256 | 1), ("full-row even", full & ~1), ("full-row odd", full | 1)]
    return [v for v in hs if v[1] < T], [v for v in rs if v[1] < T]


def cross(hs, rs):
    """[(label, h, r)] of the cross product, h-major."""
    return [(f"h = {hl}, r = {rl}", h, r) for hl, h in hs for rl, r in rs]


def tile(items: list, count: int) -> list:
    """`count` items: the list in order, repeated."""
    return [items[i % len(items)] for i in range(count)]


def first_mismatch(got: list, want: list, labels: list) -> str:
    """'' when got == want, else the first differing element's index and operand label."""
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"element {i} ({labels[i % len(labels)]}): got {g:x}, want {w:x}"
    return "" if len(got) == len(want) else f"{len(got)} results for {len(want)} operands"
