"""GPU: the RSA PSI kernels over the whole key and operand domain (tests/golden/rsa_domain.json, keys
only; tests/rsa_domain.py lists the operands and computes every expected value with Python integers).

tests/test_rsa_gpu.py runs six well-formed keys on a thin band of operands. Here every kernel family
runs in both orders of the primes, keys shorter than their class, the extreme moduli of each class,
exponents from one bit to runs of a thousand zeros or ones, and every class of row a peer can send:
values at and above n, on the hi / lo split of a wide row, multiples of a prime, the CRT idempotents,
even and full-row blind numbers. All comparisons are exact; a mismatch names the key's `why` and the
operand. tests/test_rsa_domain_host.py proves on the CPU that the fixture covers what it claims and
that the expectations are pow(x, d, n).
"""
import math

import pytest
import torch

import rsa_domain as rd

pytestmark = pytest.mark.gpu

KEYS = rd.load()
BY_NAME = {k.name: k for k in KEYS}
PRIVATE = [k for k in KEYS if k.private]
TILED = 131          # 3 workgroups at one lane per element (64 each), 5 at two lanes (32 each); the last partial
IN_PLACE = ("family-64-32", "family-64-64-q-longer", "family-32-16")


def key_id(k):
    return k.name


@pytest.fixture(scope="module")
def psi():
    import efl
    return efl.psi


def rows(psi, values, W):
    return psi.rsa_cipher.rows_from_ints(values, W).cuda()


def ints(psi, t):
    return psi.rsa_cipher.ints_from_rows(t)


def blake_hash(text):
    import hashlib
    return int.from_bytes(hashlib.blake2b(text.encode()).digest()[:8], "little")


@pytest.mark.parametrize("k", PRIVATE, ids=key_id)
def test_sign(psi, k):
    key = psi.RsaKey.private(k.n, k.e, k.d, k.p, k.q)
    info = key.info()
    assert (info.words, info.n_bits, info.byte_len, info.has_private, info.e) == \
        (k.W, k.n.bit_length(), k.byte_len, 1, k.e), k.why
    ops = rd.sign_operands(k)
    labels, xs = [l for l, _ in ops], [x for _, x in ops]
    want = [rd.sign_expected(k, x) for x in xs]
    if k.why.startswith("same as "):
        # an unreduced d: the reduced key's rows
        base = BY_NAME[k.why.split()[2]]
        assert base.d < k.d and want == [rd.sign_expected(base, x) for x in xs]
    got = ints(psi, key.sign(rows(psi, xs, k.W)))
    miss = rd.first_mismatch(got, want, labels)
    assert not miss, (k.name, k.why, miss)
    got = ints(psi, key.sign(rows(psi, rd.tile(xs, TILED), k.W)))
    miss = rd.first_mismatch(got, rd.tile(want, TILED), labels)
    assert not miss, (k.name, k.why, "tiled", miss)
    if k.name in IN_PLACE:
        # s may be x (the C ABI, in place)
        t = rows(psi, rd.tile(xs, TILED), k.W)
        assert psi.rsa_cipher._lib.efl_rsa_sign(key._h, t.data_ptr(), t.data_ptr(), t.shape[0], None) == 0
        torch.cuda.synchronize()
        miss = rd.first_mismatch(ints(psi, t), rd.tile(want, TILED), labels)
        assert not miss, (k.name, k.why, "in place", miss)


def test_sign_in_place_keys_exist():
    assert {(BY_NAME[n].W, BY_NAME[n].L) for n in IN_PLACE} == {(64, 32), (64, 64), (32, 16)}


@pytest.mark.parametrize("k", KEYS, ids=key_id)
def test_blind(psi, k):
    key = psi.RsaKey.public(k.n, k.e)                    # the client's side: no private key
    assert not key.has_private and key.words == k.W
    hs, rs = rd.blind_lists(k)
    vec = rd.cross(hs, rs)
    want = [rd.blind_expected(k, h, r) for _, h, r in vec]
    got = ints(psi, key.blind(rows(psi, [h for _, h, _ in vec], k.W), rows(psi, [r for _, _, r in vec], k.W)))
    miss = rd.first_mismatch(got, want, [l for l, _, _ in vec])
    assert not miss, (k.name, k.why, miss)


@pytest.mark.parametrize("k", KEYS, ids=key_id)
def test_unblind(psi, k):
    import efl
    key = psi.RsaKey.public(k.n, k.e)
    ss, rs = rd.blind_lists(k)
    vec = rd.cross(ss, rs)
    labels = [l for l, _, _ in vec]

    def run(v, check=False):
        return key.unblind(rows(psi, [s for _, s, _ in v], k.W), rows(psi, [r for _, _, r in v], k.W), check=check)

    def first_bad(v):
        return next((i for i, (_, _, r) in enumerate(v) if math.gcd(r, k.n) != 1), -1)

    # the whole cross product: rows without an inverse read 0; r = 0 comes first
    out, bad = run(vec)
    miss = rd.first_mismatch(ints(psi, out), [rd.unblind_expected(k, s, r) for _, s, r in vec], labels)
    assert not miss, (k.name, k.why, miss)
    assert bad == first_bad(vec) == 0, (k.name, k.why)
    # only rows with an inverse (even, full-row and >= n blind numbers among them)
    units = [v for v in vec if math.gcd(v[2], k.n) == 1]
    assert len(units) >= len(ss) * 3 and any(r % 2 == 0 for _, _, r in units)
    assert any(r > k.n for _, _, r in units) or k.n + 1 == 1 << (32 * k.W)
    out, bad = run(units)
    assert bad == -1, (k.name, k.why)
    miss = rd.first_mismatch(ints(psi, out), [rd.unblind_expected(k, s, r) for _, s, r in units], [l for l, _, _ in units])
    assert not miss, (k.name, k.why, miss)
    assert ints(psi, run(units, check=True)) == ints(psi, out)
    # one row without an inverse past the first workgroup, another after it: the first is named
    nonunit = next(v for v in vec if v[2] and math.gcd(v[2], k.n) != 1)
    at = min(70, len(units) - 2)
    mixed = units[:at] + [nonunit] + units[at:-1] + [vec[0]]
    out, bad = run(mixed)
    assert bad == first_bad(mixed) == at, (k.name, k.why)
    got = ints(psi, out)
    assert got[at] == 0 and got[-1] == 0 and got[:at] == [rd.unblind_expected(k, s, r) for _, s, r in units[:at]]
    with pytest.raises(efl.errors.InvalidArgumentError, match=f"blind number {at} has no inverse"):
        run(mixed, check=True)


class StubClient:
    """data_join_cli of the reference's test: hands the blinded ids to the server's signer."""

    def __init__(self, server):
        self.server, self.seen = server, []

    def sign_blinded_ids_from_server(self, ids, bucket_id):
        self.seen.append(list(ids))
        return self.server.sign_blinded_ids_from_client(ids)


@pytest.mark.parametrize("bits", [2047, 1023])
def test_wire_lengths(psi, bits, monkeypatch):
    """n.bit_length() // 8 bytes do not hold every value below an n whose length is no multiple of 8
    bits: a value that fits crosses the wire as that many bytes, one that does not raises the
    reference's OverflowError (int2bytes) on the server and on the client, never a shortened string."""
    import hashlib
    import random
    k = next(k for k in PRIVATE if k.n.bit_length() == bits)
    n, e, d, B = k.n, k.e, k.d, k.byte_len
    assert B == bits // 8 and 2 ** (8 * B) < n
    pub, prv = psi.pkcs1.save_public(n, e), psi.pkcs1.save_private(n, e, d, k.p, k.q)
    server = psi.ServerRsaSigner(pub, prv, oneway_hash=blake_hash)
    client = psi.ClientRsaSigner(pub, oneway_hash=blake_hash)
    rng = random.Random(f"wire {bits}")
    fit = [1, 2 ** (8 * B) - 1, rng.randrange(2 ** (8 * B))]
    over = [2 ** (8 * B), n - 1, rng.randrange(2 ** (8 * B), n)]
    # the server: the expected signature first, then x = s^e
    got = server.sign_blinded_ids_from_client([pow(s, e, n).to_bytes(4 * k.W, "little") for s in fit])
    assert got == [s.to_bytes(B, "little") for s in fit]
    for s in over:
        with pytest.raises(OverflowError, match="int too big to convert"):
            server.sign_blinded_ids_from_client([pow(f, e, n).to_bytes(4 * k.W, "little") for f in fit[:1]] +
                                                [pow(s, e, n).to_bytes(4 * k.W, "little")])
    # the client: the expected blinded value b first, then h = b r^-e
    for r in (3, rng.randrange(2, n) | 1):
        re_inv = pow(pow(r, e, n), -1, n)
        sent, kept = client._blind_ids([b * re_inv % n for b in fit], blind_numbers=[r] * len(fit))
        assert sent == [b.to_bytes(B, "little") for b in fit] and kept == [r] * len(fit)
        for b in over:
            with pytest.raises(OverflowError, match="int too big to convert"):
                client._blind_ids([fit[0] * re_inv % n, b * re_inv % n], blind_numbers=[r, r])

    # a full PSI round. The blinded hash and its signature must both fit B bytes, which a drawn blind
    # number gives about once in 2^12 times here: the happy path takes blind numbers chosen for it
    # (the signed blinded value sb first, r = sb / sign(h), tried until sb^e fits too)
    ids = [1, 2, 3, 6.5, '7']
    hashes = [int(hashlib.sha256(str(i).encode()).hexdigest(), 16) for i in ids]
    chosen = []
    for h in hashes:
        sh_inv = pow(pow(h, d, n), -1, n)
        while True:
            sb = rng.randrange(1, 2 ** (8 * B))
            if pow(sb, e, n) < 2 ** (8 * B):
                chosen.append(sb * sh_inv % n)
                break
    draws = iter(chosen)
    monkeypatch.setattr(psi.ClientRsaSigner, "_draw_blind_number", staticmethod(lambda: next(draws)))
    stub = StubClient(server)
    a = server.sign_func(ids)
    b = client.sign_func(ids, stub, 0)
    assert a == b and len(set(a)) == len(ids)
    assert a == [hex(blake_hash(str(pow(h, d, n))))[2:].encode() for h in hashes]
    (sent,) = stub.seen
    assert all(len(s) == B for s in sent)
    # with blind numbers that leave a blinded hash too long, the round raises instead of losing the ID
    bad_r = next(r for r in range(3, 1000, 2) if pow(r, e, n) * hashes[0] % n >= 2 ** (8 * B))
    draws = iter([bad_r] * len(ids))
    with pytest.raises(OverflowError, match="int too big to convert"):
        client.sign_func(ids, stub, 0)
    assert len(stub.seen) == 1                               # nothing was sent


@pytest.mark.parametrize("bits", [2047, 1023, 17])
def test_uint8_rows_must_hold_n(psi, bits):
    """uint8 rows come back at the width they were given: rows narrower than the bytes of n (here the
    wire length n.bit_length() // 8, one byte short) cannot hold every result and are refused by
    shape; rows of that many bytes and wider ones serve."""
    import efl
    k = next(k for k in PRIVATE if k.n.bit_length() == bits)
    n, e, B = k.n, k.e, k.byte_len
    key = psi.RsaKey.private(n, e, k.d, k.p, k.q)
    x = n - 2                                                  # needs every byte of n
    assert x >= 2 ** (8 * B)
    row = torch.frombuffer(bytearray(x.to_bytes(4 * k.W, "little") * 2), dtype=torch.uint8).view(2, 4 * k.W).cuda()
    for op in (key.sign, lambda t: key.blind(t, t), lambda t: key.unblind(t, t)):
        with pytest.raises(efl.errors.InvalidArgumentError, match=f"at least {B + 1} bytes"):
            op(row[:, :B].contiguous())
    for width in sorted({B + 1, min(B + 2, 4 * k.W), 4 * k.W}):
        out = key.sign(row[:, :width].contiguous())
        assert out.dtype == torch.uint8 and tuple(out.shape) == (2, width)
        assert ints(psi, out) == [rd.sign_expected(k, x)] * 2
        out = key.blind(row[:, :width].contiguous(), row[:, :width].contiguous())
        assert tuple(out.shape) == (2, width) and ints(psi, out) == [rd.blind_expected(k, x, x)] * 2
