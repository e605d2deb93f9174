"""CPU: the key-domain fixture of the RSA PSI kernels (tests/golden/rsa_domain.json) and the host side
of that domain.

The fixture holds keys only. This file proves, with Python integers, that every key is what its `why`
says (real primes, the kernel family, the Montgomery constants, the exponent lengths), that the keys
together cover every line of the list in tests/golden/make_rsa_domain_golden.py by property, and that
the CRT expression the GPU test compares against is pow(x, d, n) on the whole sign list. Then the host
code the domain touches: PKCS#1 on every key, the refusals of efl_rsa_set_private through the raw ABI
(they run before any HIP call) and the wire layer's length rule.
"""
import ctypes
import math
import os
import re

import pytest

import rsa_domain as rd

KEYS = rd.load()
BY_NAME = {k.name: k for k in KEYS}
PRIVATE = [k for k in KEYS if k.private]
PUBLIC_ONLY = [k for k in KEYS if not k.private]

_SMALL = [p for p in range(2, 2000) if all(p % d for d in range(2, int(p ** 0.5) + 1))]


def is_prime(n, rounds=8):
    """Miller-Rabin of this file's own (fixed bases), after trial division."""
    if n < 2:
        return False
    for p in _SMALL:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)[:rounds]:
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


def no_prime_between(lo, hi):
    """Every number strictly between lo and hi is composite (a factor below 2^16, or 2^(c-1) != 1 mod c)."""
    sieve = bytearray([1]) * 65536
    small = [p for p in range(2, 65536) if sieve[p] and not sieve.__setitem__(slice(p * p, None, p), bytes(len(range(p * p, 65536, p))))]
    for c in range(lo + 1, hi):
        if all(c % p for p in small) and pow(2, c - 1, c) == 1:
            return False
    return True


def hx(v):
    return format(v, "x").encode()


def test_fixture_size_and_shape():
    assert os.path.getsize(rd.FIXTURE) < 128 * 1024
    assert len({k.name for k in KEYS}) == len(KEYS)
    for k in KEYS:
        assert k.why and "\n" not in k.why
        assert k.n % 2 == 1 and 16 <= k.n.bit_length() <= 4096 and 1 <= k.e < 2 ** 64
    # the file carries no answers: keys only
    import json
    with open(rd.FIXTURE) as f:
        raw = json.load(f)
    assert set(raw) == {"seed", "keys"}
    assert all(set(k) in ({"name", "why", "n", "e"}, {"name", "why", "n", "e", "d", "p", "q"}) for k in raw["keys"])


@pytest.mark.parametrize("k", PRIVATE, ids=lambda k: k.name)
def test_key_is_what_it_claims(k):
    n, e, d, p, q = k.n, k.e, k.d, k.p, k.q
    assert is_prime(p) and is_prime(q) and p != q
    assert p * q == n
    assert e * d % (p - 1) == 1 % (p - 1) and e * d % (q - 1) == 1 % (q - 1)
    assert k.L in (k.W, k.W // 2)                      # a kernel family exists (csrc/rsaset.hip)
    assert k.dp.bit_length() >= 1 and k.dq.bit_length() >= 1
    # what the `why` states, parsed from its text
    why = k.why
    for pat, got in ((r"W=(\d+)", k.W), (r"\bL=(\d+)", k.L), (r"n of (\d+)", n.bit_length()),
                     (r"byte_len (\d+)", k.byte_len), (r"dbits = (\d+)", k.dp.bit_length()),
                     (r"dbits = (\d+)", k.dq.bit_length())):
        m = re.search(pat, why)
        if m:
            assert got == int(m.group(1)), (pat, got, why)
    m = re.search(r"(\d+) \+ (\d+)(?: bits|$)", why)
    if m:
        assert (p.bit_length(), q.bit_length()) == (int(m.group(1)), int(m.group(2))), why
    if "wide == false" in why:
        assert not k.wide and k.W == k.L
    elif re.search(r"\bwide\b", why):
        assert k.wide
    if "q longer than p" in why:
        assert q.bit_length() > p.bit_length()
    if "p longer" in why:
        assert p.bit_length() > q.bit_length()
    if "minv = 2^32 - 1" in why:
        assert any(rd.minv(x, 32) == 2 ** 32 - 1 and rd.minv(x, 28) == 2 ** 28 - 1 for x in (p, q))
    if "minv = minv28 = 1" in why:
        assert any(rd.minv(x, 32) == 1 and rd.minv(x, 28) == 1 for x in (p, q))
    m = re.match(r"same as (\S+) with", why)
    if m:
        base = BY_NAME[m.group(1)]
        assert (base.n, base.e, base.p, base.q, base.dp, base.dq) == (n, e, p, q, k.dp, k.dq) and base.d != d
        assert base.d < math.lcm(p - 1, q - 1) < d
    # the Montgomery constants the key block will hold
    for x in (p, q, n):
        assert x * rd.minv(x, 32) % 2 ** 32 == 2 ** 32 - 1 and x * rd.minv(x, 28) % 2 ** 28 == 2 ** 28 - 1


@pytest.mark.parametrize("k", PRIVATE, ids=lambda k: k.name)
def test_crt_expectation_is_pow(k):
    """The expression the GPU test compares with (tests/rsa_domain.py sign_expected) is pow(x, d, n),
    also where x shares a factor with n and for an unreduced d; and the labels say what they claim."""
    ops = dict(rd.sign_operands(k))
    for label, x in ops.items():
        assert 0 <= x < 2 ** (32 * k.W)
        s = rd.sign_expected(k, x)
        assert s == pow(x, k.d, k.n), (k.name, label)
        assert 0 <= s < k.n and pow(s, k.e, k.n) == x % k.n, (k.name, label)      # the signature verifies
    p, q = k.p, k.q
    # Garner's subtraction without a borrow and with one, by both routes
    for label, borrow in (("1 mod p, 0 mod q", False), ("0 mod p, 1 mod q", True), ("sp < sq mod p", True),
                          ("sp > sq mod p", False)):
        s = rd.sign_expected(k, ops[label])
        assert (s % p < s % q % p) == borrow, (k.name, label)
    assert ops["drawn multiple of q"] % q == 0 and 0 < ops["drawn multiple of q"] < k.n
    assert ops["drawn below n"] < k.n
    assert {"0", "1", "n-1", "n", "T-1", "p", "q", "n-p", "n-q"} <= set(ops)
    if k.wide:
        assert {"2^(32L)-1", "2^(32L)", "2^(32L)+1"} <= set(ops)    # they sit on the hi / lo split


@pytest.mark.parametrize("k", KEYS, ids=lambda k: k.name)
def test_blind_lists(k):
    hs, rs = rd.blind_lists(k)
    T = 2 ** (32 * k.W)
    fits = k.n + 1 < T                                           # n + 1 of an all-ones n is no row
    assert len(hs) == 7 + fits and all(0 <= v < T for _, v in hs + rs)
    factor = k.private or rd.known_factor(k.n) is not None
    assert len(rs) == 10 + fits + factor and len(rd.cross(hs, rs)) == len(hs) * len(rs)
    if k.private:
        assert len(rd.cross(hs, rs)) == 96
    r = dict(rs)
    assert r["256-bit even"] % 2 == 0 and r["256-bit odd"] % 2 == 1 and r["256-bit odd"].bit_length() == 256
    assert r["full-row even"] % 2 == 0 and r["full-row odd"] % 2 == 1 and r["full-row odd"].bit_length() == 32 * k.W
    if factor:
        assert 1 < math.gcd(r["multiple of a factor"], k.n) < k.n
    # the first row without an inverse, found without an inverse
    units = [math.gcd(v, k.n) == 1 for _, v in rs]
    assert units[:2] == [False, True] and not units[4]          # 0, 1, n
    for (_, h, rr) in rd.cross(hs, rs)[:24]:
        want = rd.unblind_expected(k, h, rr)
        assert want * rr % k.n == (h % k.n if math.gcd(rr, k.n) == 1 else 0)


def test_coverage():
    """Every line of the key list, by property."""
    fam = {(k.W, k.L) for k in PRIVATE}
    assert fam == {(32, 16), (32, 32), (64, 32), (64, 64), (128, 64)}
    for W in (32, 64):
        narrow = [k for k in PRIVATE if k.W == k.L == W]
        assert any(k.p.bit_length() > k.q.bit_length() for k in narrow), W
        assert any(k.q.bit_length() > k.p.bit_length() for k in narrow), W
    # a 2048-bit key with one prime an eighth longer than half, in both orders
    assert {(k.p.bit_length(), k.q.bit_length()) for k in PRIVATE} >= {(1152, 896), (896, 1152), (576, 448), (448, 576)}
    # lengths of n
    nbits = {k.n.bit_length() for k in PRIVATE}
    assert nbits >= {16, 17, 64, 511, 513, 1000, 1023, 1025, 1536, 2047, 2049, 4095, 4096}
    assert any(k.n.bit_length() == 16 and k.p.bit_length() == k.q.bit_length() == 8 for k in PRIVATE)
    assert any(k.n.bit_length() % 8 for k in PRIVATE)
    pbits = {x.bit_length() for k in PRIVATE for x in (k.p, k.q)}
    assert any({28 * j - 1, 28 * j, 28 * j + 1} <= pbits for j in range(1, 74))
    assert any({32 * j - 1, 32 * j, 32 * j + 1} <= pbits for j in range(1, 64))
    # unequal primes inside one class
    assert any(k.q == 3 and k.p.bit_length() >= 990 for k in PRIVATE)
    assert any(k.p == 3 and k.q.bit_length() >= 990 for k in PRIVATE)
    assert any(min(k.p, k.q).bit_length() == 8 and max(k.p, k.q).bit_length() == 500 for k in PRIVATE)
    # modulus shapes per class of the primes
    def ordinary(x, bits):
        return x.bit_length() == bits and rd.minv(x, 32) not in (1, 2 ** 32 - 1) and \
            rd.longest_run(x, 0) < 48 and rd.longest_run(x, 1) < 48
    for L in (16, 32, 64):
        bits = 32 * L
        top, half = 2 ** bits, 2 ** (bits - 1)
        pairs = [(k.p, k.q) for k in PRIVATE] + [(k.q, k.p) for k in PRIVATE]
        largest = {a for a, _ in pairs if top - 4096 < a < top}
        smallest = {a for a, _ in pairs if half < a < half + 4096}
        assert len(largest) == 1 and len(smallest) == 1, L
        (lg,), (sm,) = largest, smallest
        assert no_prime_between(lg, top) and no_prime_between(half, sm), L
        assert any(a == lg and ordinary(b, bits) for a, b in pairs), L
        assert any(a == sm and ordinary(b, bits) for a, b in pairs), L
        assert (lg, sm) in pairs, L
        assert any(a.bit_length() == bits and a % 2 ** 32 == 1 and ordinary(b, bits) for a, b in pairs), L
        assert any(a.bit_length() == bits and a % 2 ** 32 == 2 ** 32 - 1 and ordinary(b, bits) for a, b in pairs), L
        # a sparse prime: zero limbs in the middle
        assert sum(1 for v in rd.limbs28(sm)[1:-1] if v == 0) >= bits // 28 - 3, L
    mers = [{x for x in (k.p, k.q) if x in (2 ** 127 - 1, 2 ** 521 - 1, 2 ** 607 - 1)} for k in PRIVATE]
    assert sum(1 for m in mers if len(m) == 2) == 2 and set().union(*mers) == {2 ** 127 - 1, 2 ** 521 - 1, 2 ** 607 - 1}
    # exponent shapes
    assert any(k.e == 1 and k.d == 1 and k.dp == k.dq == 1 for k in PRIVATE)
    assert any(k.e == 3 and 3 * k.dp == 2 * k.p - 1 and ordinary(k.p, k.p.bit_length()) for k in PRIVATE)
    for b in (500, 1000):
        assert any(k.e == 3 and rd.longest_run(k.dp, 0) >= b - 12 and rd.longest_run(k.dq, 1) >= b - 12
                   and k.dp.bit_length() == b + 1 and k.dq.bit_length() == b for k in PRIVATE), b
    assert any(k.e == 3 and rd.longest_run(k.dp ^ (k.dp >> 1), 1) >= 480 and rd.longest_run(k.dq ^ (k.dq >> 1), 1) >= 480
               for k in PRIVATE)
    short = {k.dp for k in PRIVATE if k.dp == k.dq == k.d and max(k.p, k.q) < 2 ** 64}
    assert short >= {3, 5, 7, 31, 33}                           # 1 is the e = 1 key's, above
    dbits = {x.bit_length() for k in PRIVATE for x in (k.dp, k.dq)}
    assert {1, 2, 3, rd.K_WIN, rd.K_WIN + 1} <= dbits
    assert any(k.e == 2 ** 64 - 59 for k in PRIVATE)
    lam = lambda k: math.lcm(k.p - 1, k.q - 1)
    reduced = {k.n: k for k in PRIVATE if k.d < lam(k)}
    assert any(k.n in reduced and k.d == reduced[k.n].d + 3 * lam(k) for k in PRIVATE)
    assert any(k.n in reduced and k.d != reduced[k.n].d and k.d.bit_length() == 2 * k.n.bit_length() for k in PRIVATE)
    # public-only moduli
    pub = {k.n for k in PUBLIC_ONLY}
    assert pub >= {2 ** 1024 - 1, 2 ** 2047 + 1, 2 ** 16 + 1, 2 ** 4096 - 1}
    assert any(is_prime(n) and n.bit_length() >= 512 for n in pub)
    assert 2 ** 1024 % (2 ** 1024 - 1) == 1                     # R mod n = 1


@pytest.mark.parametrize("k", KEYS, ids=lambda k: k.name)
def test_pkcs1_round_trip(k):
    from efl.psi import pkcs1
    pub = pkcs1.load_public(pkcs1.save_public(k.n, k.e))
    assert (pub.n, pub.e) == (k.n, k.e)
    assert pkcs1.load_public(pkcs1.public_der(k.n, k.e)) == pub
    if k.private:
        prv = pkcs1.load_private(pkcs1.save_private(k.n, k.e, k.d, k.p, k.q))
        assert tuple(prv) == (k.n, k.e, k.d, k.p, k.q)
        assert pkcs1.load_private(pkcs1.private_der(*prv)) == prv
    if k.e >> 63:
        # DER INTEGERs are signed: a 64-bit e with its top bit set takes 9 bytes, the first zero
        der = pkcs1.public_der(k.n, k.e)
        assert der.endswith(b"\x02\x09\x00" + k.e.to_bytes(8, "big"))


def test_pkcs1_covers_the_edges():
    assert any(k.e >> 63 and k.private for k in KEYS) and any(k.e == 1 for k in KEYS)
    assert any(k.n.bit_length() == 16 for k in KEYS)


def test_refusals_without_gpu():
    """efl_rsa_set_private's checks run before any HIP call. Each refused key has an accepted twin one
    step inside the boundary; without a device the twin gets past the argument checks (any status but
    INVALID_ARGUMENT), with one it loads."""
    import efl
    lib = efl.lib.raw()
    h = ctypes.c_void_p()
    assert lib.efl_rsa_ctx_create(ctypes.byref(h)) == 0
    sp = lib.efl_rsa_set_private
    INVALID = -3

    def load(n, e, d, p, q):
        rc = sp(h, hx(n), hx(e), hx(d), hx(p), hx(q), None)
        return rc, lib.efl_last_error().decode() if rc else ""

    def accepted(k):
        rc, msg = load(k.n, k.e, k.d, k.p, k.q)
        assert rc != INVALID, (k.name, msg)

    # n of 15 bits against n of 16
    p, q = 127, 131
    assert (p * q).bit_length() == 15
    rc, msg = load(p * q, 1, 1, p, q)
    assert rc == INVALID and "at least 16 bits" in msg
    accepted(next(k for k in PRIVATE if k.n.bit_length() == 16))
    # p = 1, an even p
    k = BY_NAME["family-32-16"]
    rc, msg = load(k.n, 1, 1, 1, k.n)
    assert rc == INVALID and "distinct odd primes" in msg
    rc, msg = load(k.n, 1, 1, k.n, 1)
    assert rc == INVALID and "distinct odd primes" in msg
    rc, msg = load(2 * k.n, 1, 1, 2 * k.p, k.q)
    assert rc == INVALID and "n must be odd" in msg
    rc, msg = load(k.n, 1, 1, 2 * k.p, k.q)
    assert rc == INVALID and "p q != n" in msg
    # even factors of an odd-looking n cannot exist; an even p with p q = n needs an even n (above)
    # e d = 1 mod p - 1 but not mod q - 1
    d = k.dp
    assert k.e * d % (k.p - 1) == 1 and k.e * d % (k.q - 1) != 1
    rc, msg = load(k.n, k.e, d, k.p, k.q)
    assert rc == INVALID and "e d != 1" in msg
    accepted(k)
    # a 4096-bit n with a 2100-bit prime has no family (e = d = 1 passes the exponent check; the
    # host does not test primality)
    p, q = 2 ** 2099 + 1, 2 ** 1996 + 1
    assert (p * q).bit_length() == 4096
    rc, msg = load(p * q, 1, 1, p, q)
    assert rc == INVALID and "do not fit a kernel family" in msg and "2100 and 1997 bits" in msg
    accepted(next(k for k in PRIVATE if (k.W, k.L) == (128, 64)))
    # the narrow twin: a prime longer than half of n's class runs in n's own class
    accepted(next(k for k in PRIVATE if k.W == k.L == 64))
    # e at its bounds (the public half)
    pub = lib.efl_rsa_set_public
    assert pub(h, hx(k.n), hx(0), None) == INVALID and pub(h, hx(k.n), hx(2 ** 64), None) == INVALID
    assert pub(h, hx(k.n), hx(1), None) != INVALID and pub(h, hx(k.n), hx(2 ** 64 - 1), None) != INVALID
    assert pub(h, hx(2 ** 14 + 1), hx(3), None) == INVALID and pub(h, hx(2 ** 15 + 1), hx(3), None) != INVALID
    assert pub(h, hx(2 ** 4096 - 1), hx(3), None) != INVALID and pub(h, hx(2 ** 4096 + 1), hx(3), None) == INVALID
    assert lib.efl_rsa_ctx_destroy(h) == 0


@pytest.mark.parametrize("bits", [2047, 1023, 17])
def test_wire_length_rule(bits):
    """wire_bytes is the reference's int2bytes(v, n.bit_length() // 8) on a row's bytes: the value's
    bytes when it fits, OverflowError when it does not."""
    from efl.psi.rsa_signer import int2bytes, wire_bytes
    k = next(k for k in PRIVATE if k.n.bit_length() == bits)
    assert bits % 8 and k.byte_len == bits // 8
    B, row = k.byte_len, 4 * k.W
    fits = [0, 1, 2 ** (8 * B) - 1, 2 ** (8 * B - 1)]
    over = [2 ** (8 * B), 2 ** (8 * B) + 1, k.n - 1, 2 ** (bits - 1)]
    assert all(v < k.n for v in fits + over)
    for v in fits:
        got = wire_bytes(v.to_bytes(row, "little"), B)
        assert isinstance(got, bytes) and got == int2bytes(v, B) and len(got) == B
    for v in over:
        with pytest.raises(OverflowError, match="int too big to convert"):
            int2bytes(v, B)
        with pytest.raises(OverflowError, match="int too big to convert"):
            wire_bytes(v.to_bytes(row, "little"), B)
    # any row type that slices to bytes-like serves (the signers pass bytes)
    assert wire_bytes(bytearray((5).to_bytes(row, "little")), B) == int2bytes(5, B)
