"""The u, scalar, output and limb domain of X25519 (csrc/fe25519.h, csrc/x25519.hip), for tests (a
plain helper, no fixtures).

Everything here is Python integers: the ladder of RFC 7748 §5 for any raw scalar, the input families
U (u values), K (scalars), W (crafted outputs: u values whose X25519 is a chosen w) and F (raw limb
vectors for the field functions), and an exact-integer model of fe25519.h's limb arithmetic (the ten
columns of a product and of a square from the radix's definition, the twelve-step carry) that
asserts what the header's comments claim: no column reaches 2^64, no premultiplied operand reaches
2^32, and the limb classes are closed under the functions. tests/golden/x25519_domain.json (made by
tests/golden/make_x25519_domain_golden.py, every non-zero row checked against OpenSSL there) holds
the prime-order w values and one digest per family. Shared by tests/test_x25519_domain_host.py and
tests/test_x25519_domain_gpu.py; the expected rows are computed once per process.
"""
from __future__ import annotations

import functools
import hashlib
import itertools
import json
import os
import random

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "x25519_domain.json")

P = 2 ** 255 - 19
A = 486662
A24 = 121665
M255 = 2 ** 255 - 1
L_CURVE = 2 ** 252 + 27742317777372353535851937790883648493      # the curve has order 8 l
L_TWIST = 2 ** 253 - 55484635554744707071703875581767296995      # the twist has order 4 l'
assert 8 * L_CURVE + 4 * L_TWIST == 2 * P + 2
ORDER8 = (325606250916557431795983626356110631294008115727848805560023387167927233504,
          39382357235489614581723060781553021112529911719440698176882885853963445705823)

SEED = 25519_2
# the fixed scalars of the families (the fixture records them)
U_SCALARS = (hashlib.sha256(b"x25519_domain U 0").digest(), b"\xff" * 32)
W_SCALARS = (hashlib.sha256(b"x25519_domain W 0").digest(), bytes(32))
LANE_SCALAR = hashlib.sha256(b"x25519_domain lanes").digest()


def le(v: int) -> bytes:
    return v.to_bytes(32, "little")


def clamp(k: bytes) -> int:
    return (int.from_bytes(k, "little") & ((1 << 255) - 8)) | 1 << 254


# ---- the reference ------------------------------------------------------------------------------
def ladder(k: int, u: int, bits: int):
    """RFC 7748 §5's ladder on integers for any raw scalar k below 2^bits: (x2, z2), the projective
    u-coordinate of k times the point of u-coordinate u (z2 = 0: the point at infinity)."""
    x1 = u % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(bits - 1, -1, -1):
        kt = (k >> t) & 1
        if swap ^ kt:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b = x2 + z2, x2 - z2
        aa, bb = a * a % P, b * b % P
        e = aa - bb
        da, cb = (x3 - z3) * a % P, (x3 + z3) * b % P
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + A24 * e) % P
    if swap:
        x2, z2 = x3, z3
    return x2, z2


def affine(xz) -> int:
    return xz[0] * pow(xz[1], P - 2, P) % P


def x25519(k_bytes: bytes, u_bytes: bytes) -> bytes:
    """RFC 7748 §5: the scalar clamped, bit 255 of u masked, the result reduced mod p."""
    return le(affine(ladder(clamp(k_bytes), int.from_bytes(u_bytes, "little") & M255, 255)))


def on_curve(u: int) -> bool:
    """u is the u-coordinate of a point of v^2 = u^3 + 486662 u^2 + u over GF(p) (otherwise of its
    twist): the Legendre symbol of the right-hand side."""
    u %= P
    return pow((u * u + A * u + 1) * u % P, (P - 1) // 2, P) in (0, 1)


# ---- the radix ----------------------------------------------------------------------------------
def limb_pos(i: int) -> int:
    return (51 * i + 1) // 2


def limb_bits(i: int) -> int:
    return 25 if i & 1 else 26


def limb_mask(i: int) -> int:
    return (1 << limb_bits(i)) - 1


def limbs_of(v: int) -> list:
    """v in the ten limbs, whatever is above 2^255 left in limb 9."""
    return [(v >> limb_pos(i)) & limb_mask(i) if i < 9 else v >> limb_pos(i) for i in range(10)]


def limbs_value(limbs) -> int:
    return sum(x << limb_pos(i) for i, x in enumerate(limbs))


def limb_patterns() -> list:
    """The twenty single-limb patterns: only limb i all ones, and all limbs but i all ones."""
    full = [limb_mask(i) for i in range(10)]
    out = []
    for i in range(10):
        out.append(limbs_value([full[j] if j == i else 0 for j in range(10)]))
        out.append(limbs_value([0 if j == i else full[j] for j in range(10)]))
    return out


# ---- family U -----------------------------------------------------------------------------------
def _random_us(rng, want_curve: bool, n: int) -> list:
    out = []
    while len(out) < n:
        u = rng.getrandbits(255)
        if on_curve(u) == want_curve and u % P > 1:
            out.append(u)
    return out


@functools.lru_cache(None)
def family_u() -> tuple:
    """((kind, argument, u as a 256-bit integer), ...), about 750 rows."""
    rows = []
    for j in range(19):
        for hi in (0, 1 << 255):
            rows.append(("small", j, j | hi))
            rows.append(("p+small", j, (P + j) | hi))
    for v in (0, 1, P - 1, ORDER8[0], ORDER8[1], P, P + 1):
        for hi in (0, 1 << 255):
            rows.append(("low-order", v, v | hi))
    for t in range(255):
        rows.append(("bit", t, 1 << t))
        rows.append(("all-but-bit", t, M255 - (1 << t)))
    rows += [("limb", i, v) for i, v in enumerate(limb_patterns())]
    full = [limb_mask(i) for i in range(10)]
    rows.append(("even-limbs", 0, limbs_value([full[i] if not i & 1 else 0 for i in range(10)])))
    rows.append(("odd-limbs", 1, limbs_value([full[i] if i & 1 else 0 for i in range(10)])))
    rng = random.Random(SEED)
    rows += [("curve", i, u) for i, u in enumerate(_random_us(rng, True, 64))]
    rows += [("twist", i, u) for i, u in enumerate(_random_us(rng, False, 64))]
    assert all(0 <= v < 1 << 256 for _, _, v in rows)
    return tuple(rows)


@functools.lru_cache(None)
def expected_u() -> tuple:
    """Per scalar of U_SCALARS, the expected row of every u of family U."""
    return tuple(tuple(x25519(k, le(u)) for _, _, u in family_u()) for k in U_SCALARS)


# ---- family K -----------------------------------------------------------------------------------
ALL_ONES = (1 << 256) - 1


@functools.lru_cache(None)
def family_k() -> tuple:
    """((kind, argument, 32 bytes), ...): the all-zero and all-one strings, one bit set, one bit
    cleared, and the alternating patterns; about 520 scalars."""
    rows = [("zeros", 0, bytes(32)), ("ones", 0, b"\xff" * 32)]
    rows += [("bit", t, le(1 << t)) for t in range(256)]
    rows += [("all-but-bit", t, le(ALL_ONES ^ 1 << t)) for t in range(256)]
    rows += [("pattern", 0, b"\x55" * 32), ("pattern", 1, b"\xaa" * 32),
             ("pattern", 2, (bytes(4) + b"\xff" * 4) * 4), ("pattern", 3, (b"\xff" * 4 + bytes(4)) * 4)]
    return tuple(rows)


@functools.lru_cache(None)
def k_points() -> tuple:
    """The two u values family K runs on: the base point 9 and one fixed point of the twist."""
    return (le(9), le(_random_us(random.Random(SEED + 1), False, 1)[0]))


@functools.lru_cache(None)
def expected_k() -> tuple:
    """Per scalar of family K, the expected rows of k_points()."""
    return tuple(tuple(x25519(k, u) for u in k_points()) for _, _, k in family_k())


# ---- family W -----------------------------------------------------------------------------------
def w_candidates() -> list:
    """The crafted outputs tried, each with 1 < w < p - 1, in a fixed order without repeats."""
    c = list(range(2, 200)) + list(range(P - 199, P - 1))
    for t in range(1, 255):
        c += [1 << t, (1 << t) - 1, (1 << t) + 1, P - (1 << t), (M255 - (1 << t)) % P]
    c += [v % P for v in limb_patterns()]
    return [w for w in dict.fromkeys(c) if 1 < w < P - 1]


def prime_order_class(w: int):
    """'curve' or 'twist' when w is the u-coordinate of a point of prime order there, else None."""
    if on_curve(w):
        return "curve" if ladder(L_CURVE, w, 253)[1] == 0 else None
    return "twist" if ladder(L_TWIST, w, 253)[1] == 0 else None


def craft(k_bytes: bytes, w: int, cls: str) -> bytes:
    """The u with X25519(k, u) = w, for w of prime order l (or l'): (kc^-1 mod l) times w's point."""
    order = L_CURVE if cls == "curve" else L_TWIST
    inv = pow(clamp(k_bytes), -1, order)
    return le(affine(ladder(inv, w, 253)))


def load_fixture() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


@functools.lru_cache(None)
def family_w() -> tuple:
    """((class, w), ...) from the fixture."""
    fx = load_fixture()["w"]
    return tuple((cls, int(h, 16)) for cls in ("curve", "twist") for h in fx[cls])


@functools.lru_cache(None)
def crafted_w() -> tuple:
    """Per scalar of W_SCALARS, the crafted u of every w of family W (its expected row is le(w))."""
    return tuple(tuple(craft(k, w, cls) for cls, w in family_w()) for k in W_SCALARS)


def check_w_conditions(per_class: dict) -> None:
    """What the generator and the host test both assert of the kept w values."""
    for cls in ("curve", "twist"):
        ws = per_class[cls]
        assert len(ws) >= 64, (cls, len(ws))
        assert sum(1 for w in ws if P - w <= 200) >= 5, cls
        assert sum(1 for w in ws if w < 19) >= 1, cls
    both = set(per_class["curve"]) | set(per_class["twist"])
    assert {2, 9, 16} <= both
    assert 9 in per_class["curve"] and 16 in per_class["curve"] and 2 in per_class["twist"]


@functools.lru_cache(None)
def lane_us() -> tuple:
    """1,024 distinct seeded u, every second one with bit 255 set, and their rows under LANE_SCALAR."""
    rng = random.Random(SEED + 2)
    us = []
    while len(us) < 1024:
        u = rng.getrandbits(255)
        if u not in us:
            us.append(u)
    rows = tuple(le(u | (i & 1) << 255) for i, u in enumerate(us))
    return rows, tuple(x25519(LANE_SCALAR, r) for r in rows)


def digests() -> dict:
    """One SHA-256 per family over the concatenated expected rows (W: the crafted inputs too)."""
    h = lambda rows: hashlib.sha256(b"".join(rows)).hexdigest()
    return {"u": h(itertools.chain.from_iterable(expected_u())),
            "k": h(itertools.chain.from_iterable(expected_k())),
            "w": h([le(w) for _ in W_SCALARS for _, w in family_w()]),
            "w_inputs": h(itertools.chain.from_iterable(crafted_w())),
            "lanes": h(lane_us()[1])}


# ---- family F and the exact-integer model of the limb arithmetic --------------------------------
TIGHT = tuple((1 << 25) + (1 << 16) - 1 if i & 1 else (1 << 26) - 1 for i in range(10))
LOOSE = tuple(3 * (1 << 25) + (1 << 16) - 1 if i & 1 else 3 * (1 << 26) - 1 for i in range(10))
CLASS_MAX = {"tight": TIGHT, "loose": LOOSE}
CARRY_ORDER = ((0, 1, 1), (4, 5, 1), (1, 2, 1), (5, 6, 1), (2, 3, 1), (6, 7, 1), (3, 4, 1), (7, 8, 1),
               (4, 5, 1), (8, 9, 1), (9, 0, 19), (0, 1, 1))
# the largest limbs carry() leaves for columns mul, sqr and mul_a24 make of loose operands, as
# carry_bounds() proves them: limb 1 and limb 5 receive a last carry after they were masked
CARRY_MAX = tuple({1: (1 << 25) - 1 + 1712, 5: (1 << 25) - 1 + 1063}.get(i, limb_mask(i)) for i in range(10))


def in_class(limbs, cls: str) -> bool:
    return all(0 <= x <= m for x, m in zip(limbs, CLASS_MAX[cls]))


def _u32(x: int) -> int:
    assert 0 <= x < 1 << 32, "a premultiplied operand reaches 2^32"
    return x


def _u64(x: int) -> int:
    assert 0 <= x < 1 << 64, "a column reaches 2^64"
    return x


def mul_columns(f, g) -> list:
    """The ten columns of f g from the radix's definition: limb i of f times limb j of g lands at bit
    limb_pos(i) + limb_pos(j), which is limb_pos(i + j) + (1 if both are odd); past limb 9 the
    position wraps by 2^255 = 19. The operands are premultiplied as mul() does it."""
    g19 = [_u32(19 * x) for x in g]
    f2 = [_u32(2 * x) for x in f]
    t = [0] * 10
    for i in range(10):
        for j in range(10):
            assert limb_pos(i) + limb_pos(j) == limb_pos((i + j) % 10) + 255 * ((i + j) // 10) + (i & j & 1)
            a = f2[i] if i & j & 1 else f[i]
            b = g19[j] if i + j >= 10 else g[j]
            t[(i + j) % 10] = _u64(t[(i + j) % 10] + a * b)
    return t


def sqr_columns(f) -> list:
    """The ten columns of f^2 as sqr() forms them: 55 products, the cross products doubled."""
    f19 = [_u32(19 * x) for x in f]
    t = [0] * 10
    for i in range(10):
        for j in range(i, 10):
            a = _u32(f[i] << ((1 if i != j else 0) + (i & j & 1)))
            b = f19[j] if i + j >= 10 else f[j]
            t[(i + j) % 10] = _u64(t[(i + j) % 10] + a * b)
    return t


def a24_columns(f) -> list:
    return [_u64(x * A24) for x in f]


def carry(t) -> list:
    """carry() of fe25519.h on exact integers: the twelve steps in their order."""
    t = list(t)
    for i, j, m in CARRY_ORDER:
        c = t[i] >> limb_bits(i)
        t[j] = _u64(t[j] + c * m)
        t[i] &= limb_mask(i)
    return t


def carry_bounds(tmax) -> list:
    """Upper bounds of carry()'s limbs for columns at most tmax, column by column. Every carry is
    monotone in the column it leaves and a masked limb is at most its mask, so the bounds of the
    class maxima hold for the whole class."""
    t = list(tmax)
    for i, j, m in CARRY_ORDER:
        c = t[i] >> limb_bits(i)
        t[j] = _u64(t[j] + c * m)
        t[i] = min(t[i], limb_mask(i))
    return t


def mul_model(f, g) -> list:
    return carry(mul_columns(f, g))


def sqr_model(f) -> list:
    return carry(sqr_columns(f))


def a24_model(f) -> list:
    return carry(a24_columns(f))


def sub_model(f, g) -> list:
    bias = [2 * x for x in limbs_of(P)]        # 2 p limb by limb: 0x7ffffda, 0x3fffffe, 0x7fffffe, ...
    out = [a + b - c for a, b, c in zip(f, bias, g)]
    assert all(0 <= x < 1 << 32 for x in out), "sub wraps"
    return out


def family_f(cls: str) -> list:
    """Limb vectors of one class: all at the maximum, each single limb at its maximum with the rest
    zero, each single limb zero with the rest at the maximum, 2,000 uniform inside the class and
    2,000 drawn from {0, 1, max - 1, max}."""
    mx = CLASS_MAX[cls]
    rng = random.Random(SEED + (3 if cls == "tight" else 4))
    out = [list(mx)]
    out += [[mx[j] if j == i else 0 for j in range(10)] for i in range(10)]
    out += [[0 if j == i else mx[j] for j in range(10)] for i in range(10)]
    out += [[rng.randint(0, m) for m in mx] for _ in range(2000)]
    out += [[rng.choice((0, 1, m - 1, m)) for m in mx] for _ in range(2000)]
    return out


def field_pairs() -> list:
    """(f, g) for mul: the loose vectors then the tight ones as f, each with the vector a seeded
    shuffle puts beside it as g; the first two pairs are the class maxima with themselves."""
    v = family_f("loose") + family_f("tight")
    g = v[:]
    random.Random(SEED + 5).shuffle(g)
    pairs = list(zip(v, g))
    pairs[0] = (v[0], v[0])
    k = len(family_f("loose"))
    pairs[k] = (v[k], v[k])
    return pairs


def ladder_step_model(x1, x2, z2, x3, z3):
    """The four results of one ladder step mod p from the integer formulas of RFC 7748 §5."""
    a, b, c, d = x2 + z2, x2 - z2, x3 + z3, x3 - z3
    aa, bb = a * a, b * b
    e = aa - bb
    da, cb = d * a, c * b
    return (aa * bb % P, e * (aa + A24 * e) % P, (da + cb) ** 2 % P, x1 * (da - cb) ** 2 % P)
