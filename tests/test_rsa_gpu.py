"""GPU: the RSA blind-signature PSI kernels and signers (efl.psi) against Python integers and hashlib
(tests/golden/rsa_kat.json, made by tests/golden/make_rsa_golden.py).

A batch of B elements tiles a key's known answers (the edge values first), so every batch size checks
every row word for word without a big-number power per row on the host: a wave holds 64 / G elements
(G = 1 or 2 lanes each), so 1, 7, 63, 65 and 1000 cross a partial wave, a wave boundary and many
workgroups.
"""
import ctypes
import hashlib
import json
import os

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 63, 65, 1000)

with open(os.path.join(GOLDEN, "rsa_kat.json")) as _f:
    KAT = json.load(_f)
KEYS = {k["name"]: k for k in KAT["keys"]}


def ints(k):
    return {f: int(k[f], 16) for f in "nedpq"}


@pytest.fixture(scope="module")
def psi():
    import efl
    return efl.psi


@pytest.fixture(scope="module")
def private_keys(psi):
    made = {}

    def get(name):
        if name not in made:
            v = ints(KEYS[name])
            made[name] = psi.RsaKey.private(v["n"], v["e"], v["d"], v["p"], v["q"])
        return made[name]
    return get


def sign_vectors(k):
    """[(x, pow(x, d, n))] of a key: the edge values, which follow from the key's own numbers (their
    signatures are in the fixture, in this order), then the fixture's drawn values."""
    v, W = ints(k), k["words"]
    n, p, q = v["n"], v["p"], v["q"]
    edges = [0, 1, 2, n - 1, n, n + 1, 2 ** (32 * W) - 1, p, q, 2 * p, 3 * q]
    assert len(edges) == len(k["sign_edges"])
    return [(x, int(s, 16)) for x, s in zip(edges, k["sign_edges"])] + \
        [(int(x, 16), int(s, 16)) for x, s in k["sign"]]


def tiled(vectors, B):
    """B vectors: the known answers in order, repeated."""
    return [vectors[i % len(vectors)] for i in range(B)]


def rows(psi, values, W):
    return psi.rsa_cipher.rows_from_ints(values, W).cuda()


def blake_hash(text):
    return int.from_bytes(hashlib.blake2b(text.encode()).digest()[:8], "little")


@pytest.mark.parametrize("name", sorted(KEYS))
def test_sign_matches_pow(psi, private_keys, name):
    k, v = KEYS[name], ints(KEYS[name])
    key, W = private_keys(name), KEYS[name]["words"]
    info = key.info()
    assert (info.words, info.n_bits, info.byte_len, info.has_private) == (W, k["bits"], k["bits"] // 8, 1)
    n, e, p, q = v["n"], v["e"], v["p"], v["q"]
    # 0, 1, 2, N-1, N, N+1, 2^(32W)-1, p, q, 2p, 3q, then a multiple of q below N and drawn values
    # (every batch of 14 or more holds them all; the first 7 are in all but the batch of one)
    sv = sign_vectors(k)
    assert sv[11][0] % q == 0 and 0 < sv[11][0] < n and len(sv) == 14
    for B in SIZES:
        vec = tiled(sv, B)
        got = psi.rsa_cipher.ints_from_rows(key.sign(rows(psi, [x for x, _ in vec], W)))
        bad = [i for i in range(B) if got[i] != vec[i][1]]
        assert not bad, (name, B, bad[:8])
    # the fixture's answers are pow(x, d, n): the signatures verify
    for x, s in sv:
        assert pow(s, e, n) == x % n


def test_sign_bytes_rows_and_in_place(psi, private_keys):
    """uint8 rows of byte_len bytes are the reference's wire form; a padded class zero-extends them."""
    for name in ("openssl-2048", "openssl-3072"):
        k, key = KEYS[name], private_keys(name)
        B = k["bits"] // 8
        vec = [(x, s) for x, s in sign_vectors(k) if x < 2 ** (8 * B)]
        x8 = torch.frombuffer(bytearray(b"".join(x.to_bytes(B, "little") for x, _ in vec)), dtype=torch.uint8)
        out = key.sign(x8.view(len(vec), B).cuda())
        assert out.dtype == torch.uint8 and tuple(out.shape) == (len(vec), B)
        assert psi.rsa_cipher.ints_from_rows(out) == [s for _, s in vec]
    # s may be x (the C ABI, in place)
    k, key = KEYS["openssl-1024"], private_keys("openssl-1024")
    t = rows(psi, [x for x, _ in sign_vectors(k)], 32)
    lib = psi.rsa_cipher._lib
    assert lib.efl_rsa_sign(key._h, t.data_ptr(), t.data_ptr(), t.shape[0], None) == 0
    torch.cuda.synchronize()
    assert psi.rsa_cipher.ints_from_rows(t) == [s for _, s in sign_vectors(k)]


def test_padded_class(psi, private_keys):
    k, key = KEYS["openssl-3072"], private_keys("openssl-3072")
    assert key.words == 128 and key.byte_len == 384
    got = psi.rsa_cipher.ints_from_rows(key.sign(rows(psi, [x for x, _ in sign_vectors(k)], 128)))
    assert got == [s for _, s in sign_vectors(k)]


@pytest.mark.parametrize("name", ["openssl-1024", "openssl-2048", "openssl-4096", "openssl-3072"])
def test_blind_and_unblind_match_python(psi, name):
    k, v = KEYS[name], ints(KEYS[name])
    W = k["words"]
    key = psi.RsaKey.public(v["n"], v["e"])      # the client's side: no private key
    assert not key.has_private
    for B in SIZES:
        vec = tiled(k["blind"], B)
        got = key.blind(rows(psi, [int(h, 16) for h, _, _ in vec], W), rows(psi, [int(r, 16) for _, r, _ in vec], W))
        assert psi.rsa_cipher.ints_from_rows(got) == [int(o, 16) for _, _, o in vec], (name, B)
        vec = tiled(k["unblind"], B)
        got = key.unblind(rows(psi, [int(s, 16) for s, _, _ in vec], W), rows(psi, [int(r, 16) for _, r, _ in vec], W))
        assert psi.rsa_cipher.ints_from_rows(got) == [int(o, 16) for _, _, o in vec], (name, B)
    # the fixture's answers are the expressions of _blind_ids / _deblind_signed_ids
    h, r, o = (int(t, 16) for t in k["blind"][-1])
    assert o == pow(r, v["e"], v["n"]) * h % v["n"]
    s, r, o = (int(t, 16) for t in k["unblind"][-1])
    assert o * r % v["n"] == s
    with pytest.raises(Exception, match="No private key"):
        key.sign(rows(psi, [1], W))


@pytest.mark.parametrize("e", [3, 2 ** 64 - 59])
def test_blind_other_public_exponents(psi, e):
    """e = 3 and a 64-bit e, with a public key only: blinding needs no d."""
    k = KEYS["openssl-1024"]
    n = int(k["n"], 16)
    key = psi.RsaKey.public(n, e)
    assert key.info().e == e
    for B in SIZES:
        vec = tiled(k["blind_e"][str(e)], B)
        got = key.blind(rows(psi, [int(h, 16) for h, _, _ in vec], 32), rows(psi, [int(r, 16) for _, r, _ in vec], 32))
        assert psi.rsa_cipher.ints_from_rows(got) == [int(o, 16) for _, _, o in vec], (e, B)
    h, r, o = (int(t, 16) for t in k["blind_e"][str(e)][1])
    assert o == pow(r, e, n) * h % n


def test_unblind_reports_first_blind_number_without_inverse(psi):
    k, v = KEYS["openssl-2048"], ints(KEYS["openssl-2048"])
    key = psi.RsaKey.public(v["n"], v["e"])
    vec = tiled(k["unblind"], 16)
    s = [int(a, 16) for a, _, _ in vec]
    r = [int(b, 16) for _, b, _ in vec]
    want = [int(c, 16) for _, _, c in vec]
    r[5], r[9] = v["p"], 0
    out, bad = key.unblind(rows(psi, s, 64), rows(psi, r, 64), check=False)
    got = psi.rsa_cipher.ints_from_rows(out)
    assert bad == 5
    assert got[5] == 0 and got[9] == 0
    assert [g for i, g in enumerate(got) if i not in (5, 9)] == [w for i, w in enumerate(want) if i not in (5, 9)]
    import efl
    with pytest.raises(efl.errors.InvalidArgumentError, match="5"):
        key.unblind(rows(psi, s, 64), rows(psi, r, 64))


def test_fdh_matches_hashlib(psi):
    texts = [t for t, _ in KAT["fdh"]]
    assert sorted({len(t) for t in texts} & {0, 1, 55, 56, 63, 64, 119, 120, 1000}) == \
        [0, 1, 55, 56, 63, 64, 119, 120, 1000]
    for t, h in KAT["fdh"]:
        assert hashlib.sha256(t.encode()).hexdigest() == h
    want = [int(h, 16) for _, h in KAT["fdh"]]
    chars, offs = psi.rsa_cipher.pack_strings(texts)
    for W in (8, 32, 128):
        got = psi.rsa_cipher.sha256_rows(chars, offs, W)
        assert tuple(got.shape) == (len(texts), W)
        assert psi.rsa_cipher.ints_from_rows(got) == want
    # more strings than one workgroup's lanes, every length 0 .. 299
    many = ["".join(chr(32 + (i * 7 + j) % 95) for j in range(i)) for i in range(300)]
    chars, offs = psi.rsa_cipher.pack_strings(many)
    got = psi.rsa_cipher.ints_from_rows(psi.rsa_cipher.sha256_rows(chars, offs, 8))
    assert got == [int(hashlib.sha256(t.encode()).hexdigest(), 16) for t in many]
    # the reference test's ids, through the signers' own entry points
    ids = [1, 2, 3, 4, 5, 6.5, '7']
    assert psi.RsaSigner.fdh_list(ids) == [psi.RsaSigner.fdh(i) for i in ids]
    assert psi.RsaSigner.fdh_list(ids, True) == [int(hashlib.sha256(str(i).encode()).hexdigest(), 16) for i in ids]


class StubClient:
    """data_join_cli of the reference's test: hands the blinded ids to the server's signer."""

    def __init__(self, server):
        self.server, self.seen = server, []

    def sign_blinded_ids_from_server(self, ids, bucket_id):
        self.seen.append(list(ids))
        return self.server.sign_blinded_ids_from_client(ids)


@pytest.mark.parametrize("source", ["generated", "openssl-2048"])
def test_psi_protocol(psi, source):
    """efls-data/test/psi/test_rsa_psi.py::test_psi: both sides end with the same strings."""
    ids = [1, 2, 3, 4, 5, 6.5, '7']
    if source == "generated":
        server = psi.ServerRsaSigner(oneway_hash=blake_hash)
        assert psi.pkcs1.load_public(server.get_public_key_bytes()).n.bit_length() == 2048
    else:
        k = KEYS[source]
        server = psi.ServerRsaSigner(k["public_pem"].encode(), k["private_pem"].encode(), oneway_hash=blake_hash)
    client = psi.ClientRsaSigner(server.get_public_key_bytes(), oneway_hash=blake_hash)
    stub = StubClient(server)
    a = server.sign_func(ids)
    b = client.sign_func(ids, stub, 0)
    assert a == b and len(set(a)) == len(ids)
    # what the hash hides is the signature pow(fdh(id), d, n)
    prv = server.rsa_private_key_
    fd = [int(hashlib.sha256(str(i).encode()).hexdigest(), 16) for i in ids]
    assert a == [hex(blake_hash(str(pow(h, prv.d, prv.n))))[2:].encode() for h in fd]
    assert server.rsa_sign_list(fd, prv.d, prv.n) == [pow(h, prv.d, prv.n) for h in fd]
    # the bytes that crossed are blinded: none is a hashed id, each has the wire length
    (sent,) = stub.seen
    assert all(len(s) == 256 for s in sent)
    assert not {int.from_bytes(s, "little") for s in sent} & set(fd)


def test_blind_ids_deterministic_and_wire_edges(psi):
    import efl
    k, v = KEYS["openssl-2048"], ints(KEYS["openssl-2048"])
    server = psi.ServerRsaSigner(k["public_pem"].encode(), k["private_pem"].encode(), oneway_hash=blake_hash)
    client = psi.ClientRsaSigner(k["public_pem"].encode(), oneway_hash=blake_hash)
    hs = [int(h, 16) for h, _, _ in k["blind"]]
    rs = [int(r, 16) for _, r, _ in k["blind"]]
    sent, kept = client._blind_ids(hs, blind_numbers=rs)
    assert kept == rs
    assert sent == [int(o, 16).to_bytes(256, "little") for _, _, o in k["blind"]]
    _, drawn = client._blind_ids([1, 2, 3, 4])
    assert all(0 < r < 2 ** 256 for r in drawn) and len(set(drawn)) == 4
    # shorter items are zero-extended, values >= n reduced, longer items refused
    n, d = v["n"], v["d"]
    items = [(5).to_bytes(1, "little"), (n + 7).to_bytes(256, "little"), b"", (2 ** 2048 - 1).to_bytes(256, "little")]
    got = server.sign_blinded_ids_from_client(items)
    assert got == [pow(x, d, n).to_bytes(256, "little") for x in (5, 7, 0, (2 ** 2048 - 1) % n)]
    with pytest.raises(efl.errors.InvalidArgumentError, match="257 bytes"):
        server.sign_blinded_ids_from_client([b"\1" * 257])
    with pytest.raises(efl.errors.InvalidArgumentError, match="blind number 1"):
        client._deblind_signed_ids(got[:2], [3, v["p"]])


def test_context_hygiene(psi):
    """A new key replaces the old one for the next call; destroying a context with work queued waits
    for it (hipFree), as the Paillier context does."""
    a, b = KEYS["openssl-2048"], KEYS["generated-2048-swapped"]
    va, vb = ints(a), ints(b)
    key = psi.RsaKey.private(va["n"], va["e"], va["d"], va["p"], va["q"])
    xa = rows(psi, [int(x, 16) for x, _ in a["sign"]], 64)
    first = key.sign(xa)
    key.set_private(vb["n"], vb["e"], vb["d"], vb["p"], vb["q"])
    xb = rows(psi, [int(x, 16) for x, _ in b["sign"]], 64)
    second = key.sign(xb)
    assert psi.rsa_cipher.ints_from_rows(first) == [int(s, 16) for _, s in a["sign"]]
    assert psi.rsa_cipher.ints_from_rows(second) == [int(s, 16) for _, s in b["sign"]]
    # a refused key leaves the loaded one in place
    import efl
    with pytest.raises(efl.errors.InvalidArgumentError, match="p q != n"):
        key.set_private(vb["n"] + 2, vb["e"], vb["d"], vb["p"], vb["q"])
    assert psi.rsa_cipher.ints_from_rows(key.sign(xb[:3])) == [int(s, 16) for _, s in b["sign"][:3]]
    # set_public drops the private half
    key.set_public(va["n"], va["e"])
    with pytest.raises(efl.errors.AbortedError, match="No private key"):
        key.sign(xa[:1])
    # destroy right after queueing
    key2 = psi.RsaKey.private(va["n"], va["e"], va["d"], va["p"], va["q"])
    big = xa.repeat(8, 1)
    out = key2.sign(big)
    del key2
    torch.cuda.synchronize()
    assert psi.rsa_cipher.ints_from_rows(out) == [int(s, 16) for _, s in a["sign"]] * 8


def test_abi_edges_on_device(psi):
    lib = psi.rsa_cipher._lib
    v = ints(KEYS["openssl-1024"])
    key = psi.RsaKey.public(v["n"], v["e"])
    t = torch.zeros((4, 32), dtype=torch.int32, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    assert lib.efl_rsa_blind(key._h, t.data_ptr(), t.data_ptr(), None, 4, None) == -3
    assert lib.efl_rsa_unblind(key._h, t.data_ptr(), t.data_ptr(), t.data_ptr(), 4, None, None) == -3
    assert lib.efl_rsa_unblind(key._h, None, None, None, 0, bad.data_ptr(), None) == 0
    assert lib.efl_rsa_sign(key._h, t.data_ptr(), t.data_ptr(), 4, None) == -10
    assert lib.efl_rsa_blind(key._h, ctypes.c_void_p(t.data_ptr() + 4), t.data_ptr(), t.data_ptr(), 1, None) == -3
    # 0 has no inverse; 0 * anything = 0
    assert lib.efl_rsa_unblind(key._h, t.data_ptr(), t.data_ptr(), t.data_ptr(), 4, bad.data_ptr(), None) == 0
    assert int(bad.item()) == 0
