"""GPU: batched X25519 (csrc/x25519.hip) and efl.psi.EccSigner against tests/golden/x25519_kat.json
(Python integers, checked against OpenSSL by tests/golden/make_x25519_golden.py).

A batch of B rows tiles a scalar's vectors, the edge values first (0, 1, 9, p - 1, p, p + 1,
2^255 - 1, 2^255 + 9, the two order-8 points), so every batch size checks every row byte for byte
without a ladder per row on the host. One element runs per lane in 256-thread blocks: 1, 7 and 63
are a partial wave, 64 and 65 a wave boundary, 255 and 257 a block boundary, 1000 several blocks.
Everything is exact equality.
"""
import hashlib
import json
import os

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 63, 64, 65, 255, 257, 1000)

with open(os.path.join(GOLDEN, "x25519_kat.json")) as _f:
    KAT = json.load(_f)
US = [bytes.fromhex(u) for u in KAT["us"]]
SCALARS = {s["name"]: s for s in KAT["scalars"]}
PREFIX = KAT["hash"]["prefix"].encode()


@pytest.fixture(scope="module")
def psi():
    import efl
    return efl.psi


def tiled(items, n):
    return [items[i % len(items)] for i in range(n)]


def rows(items):
    return torch.frombuffer(bytearray(b"".join(items)), dtype=torch.uint8).reshape(len(items), 32)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", sorted(SCALARS))
def test_every_row_of_every_scalar(psi, name, size):
    s = SCALARS[name]
    want = rows(tiled([bytes.fromhex(o) for o in s["outs"]], size))
    got = psi.ecc_cipher.x25519(bytes.fromhex(s["scalar"]), rows(tiled(US, size)).cuda())
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (size, 32)
    bad = (got.cpu() != want).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"{name}: rows {bad[:8]} differ (u index {[b % len(US) for b in bad[:8]]})"


def test_known_answers(psi):
    for k in KAT["known"]:
        got = psi.ecc_cipher.x25519(bytes.fromhex(k["scalar"]), rows([bytes.fromhex(k["u"])]))
        assert bytes(got.numpy().tobytes()).hex() == k["out"], k["name"]


def test_low_order_points_give_zero_rows(psi):
    for s in SCALARS.values():
        for i in (0, 1, 3, 4, 5, 8, 9):       # 0, 1, p - 1, p, p + 1, the order-8 points
            assert s["outs"][i] == "00" * 32
    got = psi.EccSigner(bytes.fromhex(SCALARS["random"]["scalar"])).sign_list([US[i] for i in (0, 1, 3, 4, 5, 8, 9)])
    assert got == [bytes(32)] * 7


def test_in_place_through_the_c_abi(psi):
    import efl
    lib = efl.lib.raw()
    s = SCALARS["random"]
    t = rows(tiled(US, 300)).cuda()
    assert t.data_ptr() % 16 == 0
    assert lib.efl_x25519(bytes.fromhex(s["scalar"]), t.data_ptr(), t.data_ptr(), 300, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), rows(tiled([bytes.fromhex(o) for o in s["outs"]], 300)))
    # rows at a 32-byte offset inside a buffer: still aligned, the neighbours untouched
    buf = torch.full((4, 32), 0xAB, dtype=torch.uint8).cuda()
    buf[1:3] = rows(US[2:4]).cuda()
    assert lib.efl_x25519(bytes.fromhex(s["scalar"]), buf[1:].data_ptr(), buf[1:].data_ptr(), 2, None) == 0
    torch.cuda.synchronize()
    out = buf.cpu()
    assert torch.equal(out[1:3], rows([bytes.fromhex(o) for o in s["outs"][2:4]]))
    assert bool((out[0] == 0xAB).all()) and bool((out[3] == 0xAB).all())
    # a misaligned row pointer is refused, nothing is written
    assert lib.efl_x25519(bytes.fromhex(s["scalar"]), buf.data_ptr() + 4, buf.data_ptr(), 1, None) == -3
    assert "aligned" in lib.efl_last_error().decode()


def test_rows_come_back_in_the_form_given(psi):
    s = SCALARS["ones"]
    k = bytes.fromhex(s["scalar"])
    want = rows(tiled([bytes.fromhex(o) for o in s["outs"]], 70))
    host = rows(tiled(US, 70))
    before = host.clone()
    got = psi.ecc_cipher.x25519(k, host)
    assert not got.is_cuda and torch.equal(got, want) and torch.equal(host, before)
    dev = host.cuda()
    got = psi.ecc_cipher.x25519(k, dev)
    assert got.is_cuda and torch.equal(got.cpu(), want) and torch.equal(dev.cpu(), before)
    # a view that does not start on 16 bytes is copied, not refused
    flat = torch.zeros(70 * 32 + 8, dtype=torch.uint8).cuda()
    flat[8:] = dev.flatten()
    got = psi.ecc_cipher.x25519(k, flat[8:].view(70, 32))
    assert torch.equal(got.cpu(), want)
    # numpy rows pass as host tensors
    got = psi.ecc_cipher.x25519(k, host.numpy())
    assert not got.is_cuda and torch.equal(got, want)
    import efl
    with pytest.raises(efl.errors.InvalidArgumentError, match=r"uint8 \[n, 32\]"):
        psi.ecc_cipher.x25519(k, torch.zeros((3, 31), dtype=torch.uint8))
    with pytest.raises(efl.errors.InvalidArgumentError, match=r"uint8 \[n, 32\]"):
        psi.ecc_cipher.x25519(k, torch.zeros((3, 8), dtype=torch.int32))


def test_hash_vectors(psi):
    h = KAT["hash"]
    secret = bytes.fromhex(h["secret"])
    ids = [bytes.fromhex(v["id"]) for v in h["vectors"]]
    for ident, v in zip(ids, h["vectors"]):
        assert hashlib.sha256(PREFIX + ident).hexdigest() == v["digest"]
    signed = [bytes.fromhex(v["signed"]) for v in h["vectors"]]
    signer = psi.EccSigner(secret)
    assert signer.sign_hash_list(ids) == signed
    assert [signer.sign_hash(i) for i in ids[:3]] == signed[:3]
    # the digests themselves, signed as points
    assert signer.sign_list([bytes.fromhex(v["digest"]) for v in h["vectors"]]) == signed
    # tensor level, host and device, tiled past a block
    many = tiled(ids, 300)
    chars, offsets = psi.ecc_cipher.pack_strings(many)
    want = rows(tiled(signed, 300))
    got = psi.ecc_cipher.x25519_hash(secret, chars, offsets)
    assert not got.is_cuda and torch.equal(got, want)
    got = psi.ecc_cipher.x25519_hash(secret, chars.cuda(), offsets.cuda())
    assert got.is_cuda and torch.equal(got.cpu(), want)
    # another prefix, the longest one, and none
    for prefix in (b"", b"x25519:", bytes(range(64))):
        got = psi.ecc_cipher.x25519_hash(secret, chars, offsets, prefix=prefix)
        digests = rows([hashlib.sha256(prefix + i).digest() for i in many])
        assert torch.equal(got, psi.ecc_cipher.x25519(secret, digests)), prefix
    # a user hash runs on the host, its results go through efl_x25519
    user = psi.EccSigner(secret, hashfunc=lambda v: hashlib.sha256(PREFIX + v).digest())
    assert user.sign_hash_list(ids) == signed


def test_the_references_own_test(psi):
    v = [b"aaa", b"bbb", b"ccc"]
    s1, s2 = psi.EccSigner(), psi.EccSigner()
    assert s2.sign_list(s1.sign_hash_list(v)) == s1.sign_list(s2.sign_hash_list(v))
    for a, b in zip(s1.sign_hash_list(v), s2.sign_hash_list(v)):
        assert a != b
    for i in v:
        assert s2.sign(s1.sign_hash(i)) == s1.sign(s2.sign_hash(i))
    key = os.urandom(32)
    assert psi.EccSigner(key).sign_hash_list(v) == psi.EccSigner(key).sign_hash_list(v)
    sh1 = psi.EccSigner(secret=b"p" * 32, hashfunc=lambda value: b"a" * 32)
    target = "8bb21ae817643480a77910370fab9d8d0fccf8ec05bb9412531adb3983348104"
    assert [s.hex() for s in sh1.sign_hash_list(v)] == [target] * 3
    assert sh1.sign_hash(b"aaa").hex() == target
    with pytest.raises(TypeError):
        psi.EccSigner(hashfunc=lambda value: None)


def test_rfc7748_thousand_iterations(psi):
    """RFC 7748 §5.2: k, u = X25519(k, u), k from k = u = 9, by 1,000 calls of one element."""
    it = KAT["iterated"]
    k = u = bytes.fromhex(it["start"])
    for i in range(1000):
        k, u = psi.ecc_cipher.x25519(k, rows([u]).cuda()).cpu().numpy().tobytes(), k
        if i == 0:
            assert k.hex() == it["after_1"]
    assert k.hex() == it["after_1000"]


def test_empty_inputs_and_bad_items(psi):
    import efl
    lib = efl.lib.raw()
    s = psi.EccSigner(b"k" * 32)
    assert s.sign_list([]) == [] and s.sign_hash_list([]) == []
    e = psi.ecc_cipher.x25519(b"k" * 32, torch.zeros((0, 32), dtype=torch.uint8).cuda())
    assert e.is_cuda and tuple(e.shape) == (0, 32)
    e = psi.ecc_cipher.x25519(b"k" * 32, torch.zeros((0, 32), dtype=torch.uint8))
    assert not e.is_cuda and tuple(e.shape) == (0, 32)
    e = psi.ecc_cipher.x25519_hash(b"k" * 32, torch.zeros(0, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64))
    assert tuple(e.shape) == (0, 32)
    assert lib.efl_x25519(b"k" * 32, None, None, 0, None) == 0
    # the empty string is an ID like any other
    assert s.sign_hash_list([b""]) == s.sign_list([hashlib.sha256(PREFIX).digest()])
    with pytest.raises(ValueError, match="item 2 is not a 32-byte string"):
        s.sign_list([b"a" * 32, b"b" * 32, b"c" * 31])
    with pytest.raises(ValueError, match="item 0"):
        s.sign(b"c" * 31)
