"""GPU: the tail of an RSA PSI signature on the device (csrc/decimal.hip; efl_rsa_decimal,
efl_rsa_oneway) against Python's str(int) and hashlib over V(words) (tests/decimal_values.py), and the
signers that use it (efl.psi.rsa_signer: a hash name for oneway_hash=, sign_rows, sign_blinded_rows,
blind_rows, deblind_rows) against the list forms with the host twin of the hash.

A wave converts 64 rows and a hash block 256, so V(128)'s about 3,000 rows are many workgroups and a
ragged last one; the first 1, 63, 64, 65 and 257 rows of V(64) cross a partial wave, a wave boundary and
a hash block. 33 words (and 1, 2) take the word-by-word load, 32, 64 and 128 the 16-byte one."""
import hashlib
import json
import os

import pytest
import torch

from conftest import GOLDEN
from decimal_values import digits, values

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "rsa_kat.json")) as _f:
    KEYS = {k["name"]: k for k in json.load(_f)["keys"]}

IDS = [1, 2, 3, 4, 5, 6.5, '7'] + ["user-%04d" % i for i in range(200)] + list(range(1000, 1093))


@pytest.fixture(scope="module")
def psi():
    import efl
    return efl.psi


def sha64(text):
    return int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "big")


def blake_hash(text):
    return int.from_bytes(hashlib.blake2b(text.encode()).digest()[:8], "little")


def check_rows(psi, vals, words, as_bytes=False):
    """decimal_rows and oneway_rows of `vals` as rows of `words` words, byte for byte."""
    rc = psi.rsa_cipher
    rows = rc.rows_from_ints(vals, words)
    if as_bytes:
        rows = rows.view(torch.uint8)
    rows = rows.cuda()
    text, ln = rc.decimal_rows(rows)
    D = digits(words)
    assert text.is_cuda and text.dtype == torch.uint8 and tuple(text.shape) == (len(vals), D)
    assert ln.is_cuda and ln.dtype == torch.int32 and tuple(ln.shape) == (len(vals),)
    raw, lens = text.cpu().numpy().tobytes(), ln.tolist()
    hashed = rc.oneway_rows(rows)
    assert hashed.is_cuda and hashed.dtype == torch.uint8 and tuple(hashed.shape) == (len(vals), 8)
    hraw = hashed.cpu().numpy().tobytes()
    for i, v in enumerate(vals):
        s = str(v)
        row = raw[i * D:(i + 1) * D]
        assert lens[i] == len(s), (i, lens[i], len(s))
        assert row[D - len(s):] == s.encode(), (i, s[:30])
        assert row[:D - len(s)] == b"0" * (D - len(s)), (i, "padding")
        assert int.from_bytes(hraw[8 * i:8 * i + 8], "little") == sha64(s), (i, s[:30])
    return raw, lens, hraw


@pytest.mark.parametrize("words", (1, 2, 32, 33, 64, 128))
def test_value_set(psi, words):
    vals = values(words)
    check_rows(psi, vals, words)
    assert psi.rsa_cipher.decimal_strings(psi.rsa_cipher.rows_from_ints(vals[:300], words)) == \
        [str(v) for v in vals[:300]]


@pytest.mark.parametrize("count", (1, 63, 64, 65, 257))
def test_batch_sizes(psi, count):
    check_rows(psi, values(64)[-count:], 64)
    check_rows(psi, values(64)[:count], 64)


def test_uint8_rows_and_int32_rows_agree(psi):
    rc = psi.rsa_cipher
    vals = values(64)[::7]
    assert check_rows(psi, vals, 64, as_bytes=True) == check_rows(psi, vals, 64)
    # bytes that are no whole number of words are zero-extended: 5 bytes hold 40 bits
    small = [v for v in values(2) if v < 2 ** 40]
    b5 = torch.frombuffer(bytearray(b"".join(v.to_bytes(5, "little") for v in small)), dtype=torch.uint8).view(-1, 5)
    assert rc.decimal_strings(b5) == [str(v) for v in small]
    assert rc.oneway_texts(rc.oneway_rows(b5)) == [hex(sha64(str(v)))[2:].encode() for v in small]
    # host rows are staged; the result is on the device all the same
    assert rc.oneway_rows(rc.rows_from_ints(vals, 64)).is_cuda


def test_wider_stride_and_unaligned_text(psi):
    """Every byte of text is written at any stride and any alignment of the text: the bytes outside the
    rows keep their fill."""
    import efl
    rc, lib = psi.rsa_cipher, efl.lib.raw()
    vals = values(33)[::5]
    rows = rc.rows_from_ints(vals, 33).cuda()
    D = digits(33)
    text, ln = rc.decimal_rows(rows, stride=D + 23)
    raw = text.cpu().numpy().tobytes()
    for i, v in enumerate(vals):
        assert raw[i * (D + 23):(i + 1) * (D + 23)] == str(v).encode().rjust(D + 23, b"0"), i
    assert ln.tolist() == [len(str(v)) for v in vals]
    for lead in (1, 2, 3):
        for stride in (D, D + 1, D + 2):
            buf = torch.full((lead + len(vals) * stride + 5,), 0x7E, dtype=torch.uint8, device="cuda")
            efl.lib.check(lib.efl_rsa_decimal(rows.data_ptr(), 33, len(vals), buf.data_ptr() + lead, stride,
                                              ln.data_ptr(), efl.lib.stream_handle(rows.device)))
            got = buf.cpu().numpy().tobytes()
            assert got[:lead] == b"~" * lead and got[-5:] == b"~" * 5, (lead, stride)
            assert got[lead:-5] == b"".join(str(v).encode().rjust(stride, b"0") for v in vals), (lead, stride)
    with pytest.raises(efl.errors.InvalidArgumentError, match="stride"):
        rc.decimal_rows(rows, stride=D - 1)


def test_empty_batches_and_shape_errors(psi):
    import efl
    rc = psi.rsa_cipher
    for words in (1, 64, 128):
        e = torch.empty((0, words), dtype=torch.int32, device="cuda")
        text, ln = rc.decimal_rows(e)
        assert tuple(text.shape) == (0, digits(words)) and text.dtype == torch.uint8 and text.is_cuda
        assert tuple(ln.shape) == (0,) and ln.dtype == torch.int32 and ln.is_cuda
        out = rc.oneway_rows(e)
        assert tuple(out.shape) == (0, 8) and out.dtype == torch.uint8 and out.is_cuda
        assert rc.decimal_strings(e) == [] and rc.oneway_texts(out) == []
    for bad in (torch.zeros((2, 129), dtype=torch.int32), torch.zeros((2, 0), dtype=torch.int32),
                torch.zeros((2, 513), dtype=torch.uint8), torch.zeros((2, 4), dtype=torch.int64),
                torch.zeros(8, dtype=torch.int32)):
        with pytest.raises(efl.errors.InvalidArgumentError):
            rc.decimal_rows(bad)
        with pytest.raises(efl.errors.InvalidArgumentError):
            rc.oneway_rows(bad)
    with pytest.raises(efl.errors.InvalidArgumentError, match="sha256"):
        rc.oneway_rows(torch.zeros((1, 4), dtype=torch.int32), hash="city")


class StubClient:
    """data_join_cli of the reference's test: hands the blinded ids to the server's signer."""

    def __init__(self, server):
        self.server = server

    def sign_blinded_ids_from_server(self, ids, bucket_id):
        return self.server.sign_blinded_ids_from_client(ids)


@pytest.mark.parametrize("name", ("openssl-1024", "openssl-2048"))
def test_signers_with_a_hash_name(psi, name):
    rc = psi.rsa_cipher
    k = KEYS[name]
    pub, prv = k["public_pem"].encode(), k["private_pem"].encode()
    ids = IDS if name == "openssl-1024" else IDS[:70]
    named = psi.ServerRsaSigner(pub, prv, oneway_hash="sha256")
    twin = psi.ServerRsaSigner(pub, prv, oneway_hash=rc.oneway_sha256)
    want = twin.sign_func(ids)
    d, n = int(k["d"], 16), int(k["n"], 16)
    assert want[:7] == [hex(sha64(str(pow(int(hashlib.sha256(str(i).encode()).hexdigest(), 16), d, n))))[2:].encode()
                        for i in ids[:7]]
    assert named.sign_func(ids) == want
    client = psi.ClientRsaSigner(pub, oneway_hash="sha256")
    assert client.sign_func(ids, StubClient(named), 0) == want
    # the batch methods: rows whose reference form is the same list, whichever way the hash is given
    for server, cli in ((named, client), (twin, psi.ClientRsaSigner(pub, oneway_hash=rc.oneway_sha256))):
        rows = server.sign_rows(ids)
        assert rows.is_cuda and rows.dtype == torch.uint8 and tuple(rows.shape) == (len(ids), 8)
        assert rc.oneway_texts(rows) == want and rc.oneway_text(rows[5]) == want[5]
        blinded, r = cli.blind_rows(ids)
        assert blinded.is_cuda and r.is_cuda and blinded.dtype == r.dtype == torch.int32
        assert tuple(blinded.shape) == tuple(r.shape) == (len(ids), k["words"])
        assert int((r[:, 8:] != 0).sum()) == 0 and bool((r[:, :8] != 0).any(dim=1).all())   # 256 bits, none zero
        signed = server.sign_blinded_rows(blinded)
        assert signed.is_cuda and signed.dtype == torch.int32 and signed.shape == blinded.shape
        got = cli.deblind_rows(signed, r)
        assert got.is_cuda and got.dtype == torch.uint8 and rc.oneway_texts(got) == want
    # fixed blind numbers: the rows are those of the list form
    rs = [3 + 2 * i for i in range(len(ids))]
    blinded, r = client.blind_rows(ids, blind_numbers=rs)
    sent, _ = client._blind_ids(psi.RsaSigner.fdh_list(ids, True), blind_numbers=rs)
    assert [bytes(b) for b in blinded.cpu().view(torch.uint8)[:, :k["bits"] // 8].numpy()] == sent
    # a blind number without an inverse is named
    import efl
    bad_r = r.clone()
    bad_r[4] = 0
    with pytest.raises(efl.errors.InvalidArgumentError, match="blind number 4 has no inverse"):
        client.deblind_rows(named.sign_blinded_rows(blinded), bad_r)
    with pytest.raises(efl.errors.InvalidArgumentError, match="as many blind numbers"):
        client.blind_rows(ids, blind_numbers=rs[:-1])
    with pytest.raises(efl.errors.InvalidArgumentError, match="int32"):
        named.sign_blinded_rows(blinded.view(torch.uint8))


def test_callable_hash_goes_through_the_device_text(psi):
    """With a callable the batch methods hash the decimal strings the device made: the same rows as the
    list form gives."""
    rc = psi.rsa_cipher
    k = KEYS["openssl-1024"]
    pub, prv = k["public_pem"].encode(), k["private_pem"].encode()
    server = psi.ServerRsaSigner(pub, prv, oneway_hash=blake_hash)
    client = psi.ClientRsaSigner(pub, oneway_hash=blake_hash)
    ids = IDS[:40]
    want = server.sign_func(ids)
    assert rc.oneway_texts(server.sign_rows(ids)) == want
    blinded, r = client.blind_rows(ids)
    assert rc.oneway_texts(client.deblind_rows(server.sign_blinded_rows(blinded), r)) == want
    import efl
    wide = psi.ServerRsaSigner(pub, prv, oneway_hash=lambda s: 2 ** 64)
    with pytest.raises(efl.errors.InvalidArgumentError, match="64 bits"):
        wide.sign_rows(ids[:2])


def test_oneway_hash_list_with_a_name(psi):
    rc = psi.rsa_cipher
    named, twin = psi.RsaSigner(oneway_hash="sha256"), psi.RsaSigner(oneway_hash=rc.oneway_sha256)
    items = [7, "abc", 6.5, -1]
    assert named.oneway_hash_list(items) == twin.oneway_hash_list(items)
    items = [0, 2 ** 4096 - 1, 2 ** 4096, True, 10 ** 300, "12", 12, 2 ** 64]
    assert named.oneway_hash_list(items) == twin.oneway_hash_list(items)
    assert named.oneway_hash_list([]) == []


def test_empty_signer_batches(psi):
    k = KEYS["openssl-1024"]
    pub, prv = k["public_pem"].encode(), k["private_pem"].encode()
    for h in ("sha256", blake_hash):
        server, client = psi.ServerRsaSigner(pub, prv, oneway_hash=h), psi.ClientRsaSigner(pub, oneway_hash=h)
        rows = server.sign_rows([])
        assert tuple(rows.shape) == (0, 8) and rows.dtype == torch.uint8 and rows.is_cuda
        blinded, r = client.blind_rows([])
        assert tuple(blinded.shape) == tuple(r.shape) == (0, 32) and blinded.dtype == r.dtype == torch.int32
        signed = server.sign_blinded_rows(blinded)
        assert tuple(signed.shape) == (0, 32) and signed.dtype == torch.int32
        out = client.deblind_rows(signed, r)
        assert tuple(out.shape) == (0, 8) and out.dtype == torch.uint8 and out.is_cuda
        assert server.sign_func([]) == []
