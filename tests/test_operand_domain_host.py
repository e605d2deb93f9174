"""The operand generator of the Stage P domain tests (tests/operand_domain.py) delivers every class
it promises, for every known-answer key and for the padded key sizes, and the Python-int oracle
takes each value wherever tests/test_paillier_operand_domain_gpu.py calls it: if either failed, the
GPU tests would shrink without anyone noticing. No GPU."""
import json
import math
import os
import random

import pytest

from conftest import GOLDEN
from operand_domain import limb_class, operands, rotate, tile
from oracle import paillier as P

with open(os.path.join(GOLDEN, "paillier_kat.json")) as f:
    KAT = json.load(f)["keys"]


def _odd(bits, rng):
    return rng.getrandbits(bits) | 1 | (1 << (bits - 1))


def _synthetic(n_bytes):
    """(n, p, q) of a key of n_bytes with p, q odd and coprime (not prime: only gcds matter)."""
    rng = random.Random(n_bytes)
    while True:
        p, q = _odd(4 * n_bytes, rng), _odd(4 * n_bytes, rng)
        if math.gcd(p, q) == 1:
            return p * q, p, q


CASES = [pytest.param(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16), k, id=f"kat-n{8 * k['n_bytes']}")
         for k in KAT] + \
        [pytest.param(*_synthetic(nb), None, id=f"padded-n{8 * nb}") for nb in (96, 125, 192, 384, 1024)]


@pytest.mark.parametrize("n,p,q,k", CASES)
def test_every_class_is_delivered(n, p, q, k):
    words = 2 * limb_class(n)
    if k is not None:
        assert words == k["n_bytes"] // 2          # a known-answer key fills its class
    M, T = n * n, 1 << (32 * words)
    ops = operands(n, p, q, words)
    xs = [o.x for o in ops]
    assert len(set(xs)) == len(xs) and len({o.label for o in ops}) == len(ops)
    for o in ops:
        assert 0 <= o.x < T
        assert o.unit == (math.gcd(o.x, n) == 1) and o.reduced == (o.x < M)
    by = {o.label: o for o in ops}
    # the unit edges and the non-units below M, in the promised order
    assert [o.label for o in ops[:11]] == ["1", "2", "M-1", "M-2", "2^64+1", "0", "n", "p", "3q", "p^2", "n(n-1)"]
    assert all(o.unit and o.reduced for o in ops[:5]) and all(not o.unit and o.reduced for o in ops[5:11])
    assert by["n(n-1)"].x == M - n
    # at or above M: the three residues 0, 1 and a non-unit, a unit c, and the top of the range
    assert by["M"].x == M and by["M+1"].x == M + 1 and by["M+n"].x == M + n and by["T-1"].x == T - 1
    assert not by["M"].unit and by["M+1"].unit and not by["M+n"].unit and by["M+(2^64+1)"].unit
    assert by["2^(32w-1)"].unit and by["2^(32w-1)"].x == T >> 1
    assert sum(o.unit and not o.reduced for o in ops) >= 3
    assert sum(not o.unit and not o.reduced for o in ops) >= 2
    assert {o.x % M for o in ops if not o.reduced} >= {0, 1, n}
    if T // M >= 1 << 32:                          # a padded class: values far above the modulus
        assert by["floor((T-1)/M)*M+1"].unit and by["floor((T-1)/M)*M+1"].x > M << 31
        assert by["T-1"].x // M == (T - 1) // M and any(lbl.startswith("c+M*2^") for lbl in by)
        assert not by["floor((T-1)/M)*M"].unit and not by["floor((T-1)/M)*M+n"].unit
    # the batches of the GPU tests keep the whole list in front
    assert tile(ops, 70)[:len(ops)] == ops and len(tile(ops, 70)) == 70 and len(tile(ops, 3)) == len(ops)
    assert rotate(xs, 5)[0] == xs[5] and sorted(rotate(xs, 11)) == sorted(xs)


@pytest.mark.parametrize("n,p,q,k", CASES)
def test_oracle_accepts_every_operand(n, p, q, k):
    """Every oracle call the GPU tests make on these values returns (Python's % and pow are total;
    inverses and decryption only over the units, as the GPU tests ask)."""
    words = 2 * limb_class(n)
    M = n * n
    okp = P.Keypair(n, 2, 16, 1, p, q)
    ops = operands(n, p, q, words)
    xs = [o.x for o in ops]
    for r in (1, 5, 11):
        for x, y in zip(xs, rotate(xs, r)):
            assert 0 <= P.add(okp, x, y) < M
    for o in ops:
        for y in (0, 1, 2, 3, 2**40 + 1, int("FFFFFFFFFFFFFFFFFFFF", 16)):
            assert P.mul_scalar(okp, o.x, y) == pow(o.x % M, y, M)
        for e in (0, 1, 5, 33):
            assert P.mul_exp2(okp, o.x, e) == pow(o.x % M, 1 << e, M)
        assert P.mul_exp2(okp, o.x, 0) == o.x % M
        assert 0 <= P.fixedpoint_add(okp, o.x, 70, xs[0], 2)[0] < M
        for m in (0, 5, -5, 2**63 - 1, -2**63):
            assert 0 <= P.encrypt(okp, m, o.x) < M
        if o.unit:
            assert P.invert(okp, o.x) * o.x % M == 1
            for y in (-1, -7, -2**63):
                assert P.mul_scalar(okp, o.x, y) == pow(pow(o.x, -1, M), -y, M)
            if k is not None:                      # a real key: decryption is defined on the units
                d = P.decrypt(okp, o.x)
                assert d == P.decrypt(okp, o.x % M) and -n < d < n
        else:
            with pytest.raises(ValueError):
                P.invert(okp, o.x)
            with pytest.raises(ValueError):
                P.mul_scalar(okp, o.x, -1)
    units = [o.x for o in ops if o.unit]
    xm = [units[:3], units[3:6]]
    zm, _ = P.matmul(okp, xm, [[0, 1, 2], [3, 4, 5]], [[2, -3], [0, 5], [-1, 1]], [[0, 0], [1, 1], [2, 2]])
    assert all(0 <= z < M for row in zm for z in row)
