"""GPU: k_x25519 and k_sha256_rows (csrc/x25519.hip) over the whole u, scalar, output and message
length domain of tests/x25519_domain.py. The expected rows are Python integers whose digests
tests/golden/x25519_domain.json ties to OpenSSL (tests/test_x25519_domain_host.py checks that);
everything is exact equality, row by row.
"""
import hashlib
import random

import pytest
import torch

import x25519_domain as xd

pytestmark = pytest.mark.gpu

P = xd.P


@pytest.fixture(scope="module")
def cipher():
    import efl
    return efl.psi.ecc_cipher


def rows(items):
    return torch.frombuffer(bytearray(b"".join(items)), dtype=torch.uint8).reshape(len(items), 32)


def unrows(t):
    raw = t.cpu().contiguous().numpy().tobytes()
    return [raw[i:i + 32] for i in range(0, len(raw), 32)]


def differing(got, want):
    return [i for i, (a, b) in enumerate(zip(got, want)) if a != b]


def test_u_domain(cipher):
    fam = xd.family_u()
    dev = rows([xd.le(u) for _, _, u in fam]).cuda()
    for k, want in zip(xd.U_SCALARS, xd.expected_u()):
        got = unrows(cipher.x25519(k, dev))
        bad = differing(got, want)
        assert not bad, f"rows {bad[:8]} differ: {[fam[i][:2] for i in bad[:8]]}"
        # from the GPU rows alone: p + j is j, bit 255 is ignored, low order gives zero
        by = {(kind, a, u >> 255): r for (kind, a, u), r in zip(fam, got)}
        for j in range(19):
            assert by["p+small", j, 0] == by["small", j, 0] == by["small", j, 1] == by["p+small", j, 1], j
            assert any(by["small", j, 0]) == (j > 1), j
        low = [r for (kind, _, _), r in zip(fam, got) if kind == "low-order"]
        assert len(low) == 14 and low == [bytes(32)] * 14


def test_scalar_domain(cipher):
    fam = xd.family_k()
    dev = rows(list(xd.k_points())).cuda()
    got = [tuple(unrows(cipher.x25519(k, dev))) for _, _, k in fam]
    by = {(kind, a): r for (kind, a, _), r in zip(fam, got)}
    # from the GPU rows alone: the clamped bits change nothing, every other bit changes the row
    edge = (0, 1, 2, 254, 255)
    for t in edge:
        assert by["bit", t] == by["zeros", 0], t
        assert by["all-but-bit", t] == by["ones", 0], t
    for kind in ("bit", "all-but-bit"):
        rest = [by[kind, t] for t in range(256) if t not in edge]
        assert len(rest) == 251
        for col in (0, 1):
            assert len({r[col] for r in rest}) == 251 and all(any(r[col]) for r in rest), (kind, col)
    want = xd.expected_k()
    bad = differing(got, want)
    assert not bad, f"scalars {[fam[i][:2] for i in bad[:8]]} differ"


def test_crafted_outputs(cipher):
    fam = xd.family_w()
    want = [xd.le(w) for _, w in fam]
    assert sum(1 for _, w in fam if w < 19) >= 3 and sum(1 for _, w in fam if P - w <= 200) >= 10
    for k, us in zip(xd.W_SCALARS, xd.crafted_w()):
        got = unrows(cipher.x25519(k, rows(list(us)).cuda()))
        bad = differing(got, want)
        assert not bad, f"rows {bad[:8]} differ: w = {[hex(fam[i][1]) for i in bad[:8]]}"


def test_every_lane_its_own_u(cipher):
    us, want = xd.lane_us()
    assert len(set(us)) == 1024 and sum(u[31] >> 7 for u in us) == 512
    k = xd.LANE_SCALAR
    dev = rows(list(us)).cuda()
    assert differing(unrows(cipher.x25519(k, dev)), want) == []
    # a strided view: every second row of a batch twice as long
    wide = torch.zeros((2048, 32), dtype=torch.uint8, device=dev.device)
    wide[::2] = dev
    wide[1::2] = dev.flip(0)
    view = wide[::2]
    assert not view.is_contiguous()
    assert differing(unrows(cipher.x25519(k, view)), want) == []
    # a column slice of a [n, 40] tensor
    wider = torch.full((1024, 40), 0xA5, dtype=torch.uint8, device=dev.device)
    wider[:, 8:] = dev
    view = wider[:, 8:]
    assert not view.is_contiguous() and tuple(view.shape) == (1024, 32)
    assert differing(unrows(cipher.x25519(k, view)), want) == []
    assert bool((wider[:, :8] == 0xA5).all()) and torch.equal(wider[:, 8:], dev)


PREFIX_LENGTHS = (0, 1, 3, 4, 5, 10, 31, 32, 33, 63, 64)
ID_LENGTHS = tuple(range(131)) + (191, 192, 193, 1000)


def test_hash_length_sweep(cipher):
    rng = random.Random(xd.SEED + 8)
    ids = [bytes(rng.randrange(256) for _ in range(n)) for n in ID_LENGTHS]
    assert len(set(b"".join(ids))) == 256
    chars, offsets = cipher.pack_strings(ids)
    chars, offsets = chars.cuda(), offsets.cuda()
    k = xd.LANE_SCALAR
    for n in PREFIX_LENGTHS:
        prefix = bytes(rng.randrange(256) for _ in range(n))
        got = cipher.x25519_hash(k, chars, offsets, prefix=prefix)
        want = cipher.x25519(k, rows([hashlib.sha256(prefix + i).digest() for i in ids]).cuda())
        bad = (got != want).any(dim=1).nonzero().flatten().tolist()
        assert not bad, f"prefix of {n} bytes: IDs of {[ID_LENGTHS[i] for i in bad[:8]]} bytes differ"
    # offsets that do not start at 0: the strings from the 40th on, in the same chars
    tail = offsets[40:].contiguous()
    assert int(tail[0]) == sum(ID_LENGTHS[:40]) != 0
    got = cipher.x25519_hash(k, chars, tail)
    want = cipher.x25519(k, rows([hashlib.sha256(cipher.PREFIX + i).digest() for i in ids[40:]]).cuda())
    assert tuple(got.shape) == (len(ids) - 40, 32) and torch.equal(got, want)
    # the digests are not all alike: the comparison above is between distinct rows
    assert len({bytes(r) for r in want.cpu().numpy()}) == len(ids) - 40
