"""Key sizes between and past the round-3 limb classes. The reference takes any n_bytes
(GeneratePaillierKeypair, paillier.cc:799-913: primes of n_bytes * 4 bits); the build runs a key in
the smallest limb class that holds n and p^2 (512 / 1024 / 2048 / 4096 / 8192-bit n: KeyBlock's
_LIMB_CLASSES), the numbers zero-padded to it, so 768-, 1000-, 1536- and 3072-bit keys (3072 bits is
the usual 128-bit security level) run in the 1024-, 1024-, 2048- and 4096-bit kernels. Montgomery
arithmetic only needs the modulus below R, so the results must be the oracle's bit for bit: fresh
randomness encryption by the public path and by CRT, decryption, the homomorphic ops and matmul.
8192-bit keys (round 4) run their n^2 ops over 16 lanes per number and decrypt over 8."""
import random

import numpy as np
import pytest
import torch

from oracle import paillier as P
from oracle import philox

pytestmark = pytest.mark.gpu

# (n_bytes, limb class of n)
SIZES = [(96, 32), (125, 32), (192, 64), (384, 128), (1024, 256)]


@pytest.fixture(scope="module")
def efl():
    import efl as _efl
    _efl.lib.require_gpu()
    return _efl


@pytest.fixture(scope="module", params=SIZES, ids=[f"n{8 * s[0]}" for s in SIZES])
def keys(request, efl):
    n_bytes, ln = request.param
    owner = efl.paillier.Keypair(seed=17)
    owner.generate_keypair(n_bytes=n_bytes, a_bytes=n_bytes // 2, rng=random.Random(n_bytes))
    k = owner.key
    assert k.ln == ln and k.n.bit_length() in (8 * n_bytes - 1, 8 * n_bytes)
    public = efl.paillier.Keypair(seed=17)
    public.set_keys_ints(k.n, k.hs, n_bytes // 2, 1)
    okp = P.Keypair(k.n, k.hs, n_bytes // 2, 1, k.p, k.q)
    return owner, public, okp


def _ms(count, seed):
    rng = np.random.default_rng(seed)
    m = torch.from_numpy(rng.integers(-2**63, 2**63 - 1, count, dtype=np.int64))
    m[:4] = torch.tensor([0, -1, 2**63 - 1, -2**63])
    return m


def test_encrypt_public_and_crt_match_the_oracle(keys):
    owner, public, okp = keys
    m = _ms(200, 1)
    ct_pub = public.encrypt(m, counter_base=300)
    ct_own = owner.encrypt(m, counter_base=300)      # the key owner's CRT path
    got = ct_pub.tensor.to_hex().strings()
    assert ct_own.tensor.to_hex().strings() == got
    a_bits = public.key.a_bits
    for i in (0, 1, 2, 3, 50, 199):
        a = philox.draw_a(17, 300 + i, a_bits)
        assert got[i] == P.hx(P.encrypt(okp, int(m[i]), P.fbpowm(okp.hs, okp.n2, a, 1))), i
    assert torch.equal(owner.decrypt(ct_pub, dtype=torch.int64).cpu(), m)
    assert owner.decrypt(ct_pub).strings()[:4] == [P.hx(v) for v in (0, -1, 2**63 - 1, -2**63)]


def test_decrypt_every_family(keys):
    from test_paillier_gpu import SLICINGS, family
    owner, public, okp = keys
    m = _ms(64, 2)
    ct = public.encrypt(m)
    ln = owner.key.ln
    for c in SLICINGS[ln][1]:
        with family(ln, True, c):
            assert torch.equal(owner.decrypt(ct, dtype=torch.int64).cpu(), m), c


def test_homomorphic_ops_match_the_oracle(keys):
    owner, public, okp = keys
    m = _ms(6, 3)
    ct = public.encrypt(m)
    cs = ct.tensor.to_hex().to_ints()
    ys = [5, -3, 0, 1, 2**40, -(2**33)]
    assert public.add(ct.tensor, ct.tensor).to_hex().to_ints() == [P.add(okp, c, c) for c in cs]
    assert public.mul_scalar(ct.tensor, torch.tensor(ys)).to_hex().to_ints() == \
        [P.mul_scalar(okp, c, y) for c, y in zip(cs, ys)]
    sh = [0, 1, 7, 64, 130, 3]
    assert public.mul_exp2(ct.tensor, torch.tensor(sh)).to_hex().to_ints() == \
        [P.mul_exp2(okp, c, y) for c, y in zip(cs, sh)]
    assert public.invert(ct.tensor).to_hex().to_ints() == [P.invert(okp, c) for c in cs]
    xe, ye = [0, 5, -5, 70, 2, 3], [0, 0, 1, 2, 9, -9]
    z, ze = public.shift_add(ct.tensor, torch.tensor(xe), ct.tensor, torch.tensor(ye))
    want = [P.fixedpoint_add(okp, c, a, c, b) for c, a, b in zip(cs, xe, ye)]
    assert z.to_hex().to_ints() == [w[0] for w in want] and ze.cpu().tolist() == [w[1] for w in want]


def test_matmul_matches_the_oracle(keys):
    owner, public, okp = keys
    rng = np.random.default_rng(4)
    u, v, w = 3, 4, 2
    m = torch.from_numpy(rng.integers(-2**20, 2**20, (u, v)))
    ct = public.encrypt(m)
    xe = rng.integers(-30, -10, (u, v))
    ym = rng.integers(-2**20, 2**20, (v, w))
    ye = rng.integers(-25, -12, (v, w))
    zm, ze = public.matmul(ct.tensor, torch.from_numpy(xe), torch.from_numpy(ym), torch.from_numpy(ye))
    xs = [[int(s, 16) for s in row] for row in np.array(ct.tensor.to_hex().strings()).reshape(u, v)]
    om, oe = P.matmul(okp, xs, xe.tolist(), ym.tolist(), ye.tolist())
    assert ze.cpu().tolist() == oe
    assert zm.to_hex().to_ints() == [c for row in om for c in row]
    dec = owner.decrypt(zm, dtype="string").to_ints()
    assert dec == [sum(int(m[i, j]) * int(ym[j, q]) * 2 ** int(xe[i, j] + ye[j, q] - oe[i][q]) for j in range(v))
                   for i in range(u) for q in range(w)]


def test_operand_domain(keys, efl):
    """The whole operand domain (tests/operand_domain.py) through the default families: in a padded
    class an operand may be hundreds of bits above the modulus (a 768-bit key's n^2 is 2^512 below
    its 2048-bit rows), which the valid ciphertexts of the tests above never are. add, mul_scalar
    (non-negative over the list, negative over the units), mul_exp2, invert, decrypt and a 2 x 3 x 2
    matmul against the oracle, bit for bit."""
    from operand_domain import first_mismatch, operands, rotate, tile
    owner, public, okp = keys
    key = public.key
    HT = efl.HexTensor
    M, T = okp.n2, 1 << (32 * key.lc)
    ops = operands(okp.n, okp.p, okp.q, key.lc)
    padded = T // M >= 1 << 32
    assert padded == (key.ln != 256)                 # every size of this module but the 8192-bit one
    if padded:
        assert sum(o.x > M << 32 for o in ops) >= 4
    count = len(ops) if key.ln == 256 else 70 if key.ln < 128 else 24       # the 8192-bit key: untiled
    xs = [o.x for o in tile(ops, count)]
    units = [o for o in ops if o.unit]
    us = [o.x for o in tile(units, count)]

    def check(got, want, labels, what):
        msg = first_mismatch(got, want, labels)
        assert not msg, f"{what}: {msg}"

    for r in (0, 1, 5, 11):
        ys = tile(rotate([o.x for o in ops], r), count)
        check(public.add(HT.from_ints(xs), HT.from_ints(ys)).to_hex().to_ints(),
              [P.add(okp, x, y) for x, y in zip(xs, ys)], ops, f"add, y rotated by {r}")
    for y in (0, 1, 3, 2**40 + 1):
        check(public.mul_scalar(HT.from_ints(xs), torch.tensor(y)).to_hex().to_ints(),
              [P.mul_scalar(okp, x, y) for x in xs], ops, f"mul_scalar {y}")
    for y in (-1, -7, -2**63):
        check(public.mul_scalar(HT.from_ints(us), torch.tensor(y)).to_hex().to_ints(),
              [P.mul_scalar(okp, x, y) for x in us], units, f"mul_scalar {y} over the units")
    for y in (0, 1, 33):
        check(public.mul_exp2(HT.from_ints(xs), torch.tensor(y)).to_hex().to_ints(),
              [P.mul_exp2(okp, x, y) for x in xs], ops, f"mul_exp2 {y}")
    check(public.invert(HT.from_ints(us)).to_hex().to_ints(), [P.invert(okp, x) for x in us], units, "invert")
    by = {o.label: o.x for o in ops}
    batch = list(us)
    batch[5], batch[9] = by["M+n"], 0
    with pytest.raises(efl.errors.InvalidArgumentError, match="element 5 has no inverse"):
        public.invert(HT.from_ints(batch))
    # decryption: the units, and a fresh ciphertext lifted by multiples of M up to T
    c0 = public.encrypt(torch.tensor([-12345])).tensor.to_hex().to_ints()[0]
    lifted = [c0 + j * M for j in {1, 2, (T - 1 - c0) // M} if j and c0 + j * M < T]
    assert not padded or len(lifted) == 3
    cs = [o.x for o in units] + lifted
    got = owner.decrypt(HT.from_ints(cs)).strings()
    want = [P.hx(P.decrypt(okp, x)) for x in cs]
    assert got == want, next(i for i in range(len(cs)) if got[i] != want[i])
    assert want[len(units):] == ["-3039"] * len(lifted)
    # matmul: every class in some term with y >= 0 (a product of 0 mod n^2 among the outputs),
    # the units with mixed signs
    xe, ye = [[0, 2, 1], [3, 0, 5]], [[0, 1], [2, 0], [1, 3]]
    zeros = 0
    for vals, ym in ([o.x for o in ops], [[2, 1], [0, 3], [0, 1]]), ([o.x for o in units], [[3, -2], [-1, 0], [5, -7]]):
        for i in range(0, len(vals), 6):
            xm = [[vals[(i + j) % len(vals)] for j in range(3)], [vals[(i + 3 + j) % len(vals)] for j in range(3)]]
            zm, ze = public.matmul(HT.from_ints([v for row in xm for v in row], (2, 3)), torch.tensor(xe),
                                   torch.tensor(ym), torch.tensor(ye))
            wm, we = P.matmul(okp, xm, xe, ym, ye)
            assert ze.cpu().tolist() == we
            assert zm.to_hex().strings() == [P.hx(v) for row in wm for v in row], (i, ym)
            zeros += sum(v == 0 for row in wm for v in row)
    assert zeros >= 2
