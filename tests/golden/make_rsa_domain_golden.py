"""Generate tests/golden/rsa_domain.json: RSA keys over the whole key domain of efl_rsa_set_private /
efl_rsa_set_public, for tests/test_rsa_domain_host.py and tests/test_rsa_domain_gpu.py.

The file holds keys only (name, why, hex n, e, d, p, q; public-only entries n and e): the tests compute
every expected value from them with Python integers (tests/rsa_domain.py). `why` names the code path a
key is there for; tests/test_rsa_domain_host.py asserts the coverage by property, not by name.

Deterministic: random.Random with a fixed seed and this file's own Miller-Rabin, nothing else. The
searches for special primes take under 2 s each except 2^2048 - 1557 and 2^2047 + 1919 (a few
seconds each); the whole run takes about half a minute.

Run:  python tests/golden/make_rsa_domain_golden.py
"""
import json
import math
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261020

SMALL = [p for p in range(2, 2000) if all(p % d for d in range(2, int(p ** 0.5) + 1))]


def is_prime(n, rounds=12):
    """Miller-Rabin with fixed bases (the first `rounds` primes), after trial division."""
    if n < 2:
        return False
    for p in SMALL:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in SMALL[:rounds]:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def lcm(a, b):
    return a // math.gcd(a, b) * b


def hx(v):
    return format(v, "x")


class Maker:
    def __init__(self):
        self.rng = random.Random(SEED)
        self.keys = []
        self.ordinary = {}

    def prime(self, bits, accept=lambda p: True, top2=False):
        """A drawn prime of exactly `bits` bits (top2: the two top bits set)."""
        while True:
            c = self.rng.getrandbits(bits) | 1 | (1 << (bits - 1))
            if top2:
                c |= 1 << (bits - 2)
            if accept(c) and is_prime(c):
                return c

    def ord(self, bits):
        """The one ordinary (drawn) prime of `bits` bits that special primes are paired with; never
        1 mod 3, 5, 17, 257 or 65537, so the small Fermat exponents all serve."""
        if bits not in self.ordinary:
            self.ordinary[bits] = self.prime(bits, lambda p: all(p % f != 1 for f in (3, 5, 17, 257, 65537)))
        return self.ordinary[bits]

    def pair(self, pbits, qbits, nbits, accept=lambda p: True):
        """Drawn primes of pbits and qbits bits whose product has exactly nbits bits: both above 1.5
        times their top bit for pbits + qbits, below 1.5 and 1.25 times for one bit less."""
        if nbits == pbits + qbits:
            p = self.prime(pbits, accept, top2=True)
            q = self.prime(qbits, lambda x: accept(x) and x != p, top2=True)
        else:
            assert nbits == pbits + qbits - 1
            p = self.prime(pbits, lambda x: accept(x) and not x >> (pbits - 2) & 1)
            q = self.prime(qbits, lambda x: accept(x) and not x >> (qbits - 3) & 3 and x != p)
        assert (p * q).bit_length() == nbits
        return p, q

    def add(self, name, why, p, q, e=None, d=None):
        assert p != q and is_prime(p) and is_prime(q), name
        lam = lcm(p - 1, q - 1)
        if e is None:
            e = next(f for f in (65537, 257, 17, 5, 3, 7, 11, 13) if math.gcd(f, lam) == 1)
        assert math.gcd(e, lam) == 1 and 1 <= e < 2 ** 64, name
        if d is None:
            d = pow(e, -1, lam)
        assert e * d % (p - 1) == 1 % (p - 1) and e * d % (q - 1) == 1 % (q - 1), name
        self.keys.append(dict(name=name, why=why, n=hx(p * q), e=hx(e), d=hx(d), p=hx(p), q=hx(q)))
        print(f"{name:28s} n {(p * q).bit_length():5d} bits  p {p.bit_length():5d}  q {q.bit_length():5d}  e {e:#x}")

    def add_public(self, name, why, n, e=65537):
        self.keys.append(dict(name=name, why=why, n=hx(n), e=hx(e)))
        print(f"{name:28s} n {n.bit_length():5d} bits  public only")


def below(x):
    """The largest prime below x."""
    c = x - 1 - (x % 2)
    while not is_prime(c):
        c -= 2
    return c


def above(x):
    """The smallest prime above x."""
    c = x + 1 + (x % 2)
    while not is_prime(c):
        c += 2
    return c


def congruent(m, sign, bits):
    """A drawn prime of `bits` bits that is sign (+1 / -1) mod 2^32."""
    while True:
        c = (m.rng.getrandbits(bits - 32) | (1 << (bits - 33))) * 2 ** 32 + sign
        if is_prime(c):
            return c


def exponent_prime(start, step):
    """p = (3 dp + 1) / 2 for the first dp = start, start + step, ... (odd) that makes p prime: with
    e = 3, d mod (p - 1) is that dp, so the exponent's bits are chosen and the prime follows."""
    dp = start
    while True:
        p = (3 * dp + 1) // 2
        if is_prime(p):
            assert dp % 2 == 1 and 3 * dp % (p - 1) == 1
            return p
        dp += step


def main():
    m = Maker()
    mod3 = lambda p: p % 3 == 2

    # ---- families (W, L): W words of n's class, L words of the primes' class ----------------------
    m.add("family-32-16", "run_sign<8,2>, wide: W=32, L=16, 256 + 256 bits", *m.pair(256, 256, 512))
    m.add("family-32-32-p-longer", "run_sign<32,1>, wide == false, p longer: 576 + 448 bits",
          m.prime(576, top2=True), m.prime(448, top2=True))
    m.add("family-32-32-q-longer", "run_sign<32,1>, wide == false, q longer than p: 448 + 576 bits",
          m.prime(448, top2=True), m.prime(576, top2=True))
    m.add("family-64-32", "run_sign<32,1>, wide: W=64, L=32, 1024 + 1024 bits, n of 2048",
          m.prime(1024, top2=True), m.prime(1024, top2=True))
    m.add("family-64-64-p-longer", "run_sign<32,2>, wide == false, W == L == 64, p longer: 1152 + 896 bits",
          m.prime(1152, top2=True), m.prime(896, top2=True))
    m.add("family-64-64-q-longer", "run_sign<32,2>, wide == false, W == L == 64, q longer than p: 896 + 1152 bits",
          m.prime(896, top2=True), m.prime(1152, top2=True))
    m.add("family-128-64", "run_sign<32,2>, wide: W=128, L=64, n of 4095 bits (byte_len 511)",
          *m.pair(2048, 2048, 4095))

    # ---- lengths of n ----------------------------------------------------------------------------
    m.add("n16", "the smallest n: 16 bits, two 8-bit primes, every high word and limb zero", 251, 241)
    m.add("n17", "n of 17 bits (byte_len 2 holds 16): 9-bit primes", 257, 263)
    m.add("n64", "n of 64 bits: two 32-bit primes, one word each", *m.pair(32, 32, 64))
    m.add("n511", "n of 511 bits: primes of 32k and 32k - 1 bits (k = 8)", *m.pair(256, 255, 511))
    m.add("n513", "n of 513 bits: primes of 32k + 1 and 32k bits (k = 8), one bit into word 8", *m.pair(257, 256, 513))
    m.add("n1000", "n of 1000 bits (byte_len 125): a prime of 28k bits (k = 18) and one of 497", *m.pair(504, 497, 1000))
    m.add("limb28-edges", "primes of 28k + 1 and 28k - 1 bits (k = 18): 505 + 503", m.prime(505), m.prime(503))
    m.add("n1023", "n of 1023 bits (byte_len 127 holds 1016): primes of 512 and 511 bits, W=32 L=16",
          *m.pair(512, 511, 1023))
    m.add("n1025", "the first n of class 64: 1025 bits, primes of 513 and 512 bits (32k + 1, k = 16), L=32 nearly empty",
          *m.pair(513, 512, 1025))
    m.add("n1536", "n of 1536 bits in class 64: primes of 768 bits, 8 top words of each zero",
          m.prime(768, top2=True), m.prime(768, top2=True))
    m.add("n2047", "n of 2047 bits (byte_len 255 holds 2040): primes of 1024 bits", *m.pair(1024, 1024, 2047))
    m.add("n2049", "the first n of class 128: 2049 bits, primes of 1025 bits, L=64 nearly empty", *m.pair(1025, 1025, 2049))

    # ---- unequal primes inside one class -----------------------------------------------------------
    big = m.prime(1000)
    m.add("q-is-3", "q = 3 with p of 1000 bits: wide == false, dq = 1, sq mod p is sq", big, 3)
    m.add("p-is-3", "p = 3 with q of 1000 bits: wide == false, Garner's h is below 3, sq mod p reduces 1000 bits", 3, big)
    m.add("tiny-and-500", "an 8-bit prime with a 500-bit prime, wide, L=16", 239, m.prime(500))

    # ---- modulus shapes ------------------------------------------------------------------------------
    for L in (16, 32, 64):
        bits = 32 * L
        o = m.ord(bits)
        largest, smallest = below(2 ** bits), above(2 ** (bits - 1))
        m.add(f"largest-{L}", f"the largest prime below 2^{bits} (R28 > 4 m tightest, final subtractions) with an ordinary prime",
              largest, o)
        m.add(f"smallest-{L}", f"the smallest prime above 2^{bits - 1} (sparse: zero limbs in the middle) with an ordinary prime",
              o, smallest)
        m.add(f"plus-one-{L}", f"a {bits}-bit prime = 1 mod 2^32 (minv = 2^32 - 1, minv28 = 2^28 - 1) with an ordinary prime",
              congruent(m, 1, bits), o)
        m.add(f"minus-one-{L}", f"a {bits}-bit prime = -1 mod 2^32 (minv = minv28 = 1) with an ordinary prime",
              o, congruent(m, -1, bits))
        m.add(f"largest-smallest-{L}", f"the largest prime below 2^{bits} with the smallest above 2^{bits - 1}",
              largest, smallest)
    m.add("mersenne-521-607", "all-ones primes 2^521 - 1 and 2^607 - 1: W=64, L=32", 2 ** 521 - 1, 2 ** 607 - 1)
    m.add("mersenne-127-521", "all-ones primes 2^127 - 1 and 2^521 - 1: wide == false, q longer than p",
          2 ** 127 - 1, 2 ** 521 - 1)

    # ---- exponent shapes ---------------------------------------------------------------------------------
    p, q = m.pair(256, 256, 512)
    m.add("e-1", "e = 1: d = 1, dbits = 1, signing is x mod n", p, q, e=1)
    m.add("e-3", "e = 3 with ordinary primes = 2 mod 3: dp = (2 p - 1) / 3", *m.pair(512, 512, 1024, mod3), e=3)
    for b in (500, 1000):
        m.add(f"e-3-runs-{b}", f"e = 3, dp = 2^{b} + t (a run of about {b} zeros) and dq = 2^{b} - t (a run of ones)",
              exponent_prime(2 ** b + 1, 2), exponent_prime(2 ** b - 1, -2), e=3)
    m.add("e-3-alternating", "e = 3, dp = 1010...10 + t and dq = 0101...01 + t over 500 bits: every window is 10101 or 1",
          exponent_prime(int("10" * 250, 2) + 1, 2), exponent_prime(int("01" * 250, 2) + 2, 2), e=3)
    for dx in (3, 5, 7, 31, 33):
        while True:
            p, q = m.pair(32, 32, 64)
            if math.gcd(dx, lcm(p - 1, q - 1)) == 1:
                break
        m.add(f"dx-{dx}", f"dp = dq = {dx} ({dx.bit_length()} bits against kWin = 5), e = {dx}^-1 mod lcm below 2^64",
              p, q, e=pow(dx, -1, lcm(p - 1, q - 1)), d=dx)
    m.add("e-64-bit", "a private key with e = 2^64 - 59 (DER needs a leading zero byte)", *m.pair(512, 512, 1024), e=2 ** 64 - 59)
    base = m.keys[0]
    p, q, e, d = (int(base[f], 16) for f in "pqed")
    lam = lcm(p - 1, q - 1)
    m.add("d-plus-3-lcm", "same as family-32-16 with d + 3 lcm(p - 1, q - 1): the host reduces d", p, q, e=e, d=d + 3 * lam)
    long_d = d + lam * (2 ** 1023 // lam + 1)
    assert long_d.bit_length() == 2 * (p * q).bit_length()
    m.add("d-twice-as-long", "same as family-32-16 with a d of 1024 bits, twice as long as n", p, q, e=e, d=long_d)

    # ---- public-only moduli, for blind and unblind ---------------------------------------------------------
    m.add_public("public-prime", "a prime n of 1024 bits: every r but 0 mod n has an inverse", m.ord(1024))
    m.add_public("public-all-ones-1024", "n = 2^1024 - 1: R mod n = 1, every word all ones", 2 ** 1024 - 1)
    m.add_public("public-2047", "n = 2^2047 + 1: one bit at each end of 2048, every word between zero", 2 ** 2047 + 1)
    m.add_public("public-17-bit", "n = 2^16 + 1: 17 bits in a 32-word row", 2 ** 16 + 1, e=3)
    m.add_public("public-all-ones-4096", "n = 2^4096 - 1: the largest n", 2 ** 4096 - 1)

    names = [k["name"] for k in m.keys]
    assert len(set(names)) == len(names)
    out = os.path.join(HERE, "rsa_domain.json")
    with open(out, "w") as f:
        f.write('{"seed": %d, "keys": [\n' % SEED + ",\n".join(json.dumps(k) for k in m.keys) + "\n]}\n")
    print(out, len(m.keys), "keys,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
