"""GPU: efl_mmh3_hash (efl.psi.mmh3_hash_rows) bit-equal to its host twin (efl_mmh3_hash_rows_host,
which tests/test_mmh3_host.py pins to the golden file) and to tests/golden/mmh3_kat.json itself: packed
batches in which every (start offset mod 4, length mod 4) pair occurs, lengths 0..67, empty strings at
the head, in the middle and at the tail, a 4 KiB string, bytes >= 0x80, batch sizes around the wave and
workgroup sizes, four seeds, n = 0."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "mmh3_kat.json")) as _f:
    KAT = json.load(_f)

SEEDS = (0, 1, 0xFFFFFFFF, 0x9747B28C)


@pytest.fixture(scope="module")
def efl():
    import efl
    return efl


def pack(strings):
    offsets = np.zeros(len(strings) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in strings], out=offsets[1:])
    chars = np.frombuffer(b"".join(strings) or b"\0", dtype=np.uint8).copy()
    return chars, offsets


def host_twin(efl, strings, seed):
    chars, offsets = pack(strings)
    out = np.zeros(len(strings), dtype=np.int32)
    assert efl.lib.raw().efl_mmh3_hash_rows_host(chars.ctypes.data, offsets.ctypes.data, len(strings), seed,
                                                 out.ctypes.data) == 0
    return out


def device(efl, strings, seed):
    chars, offsets = pack(strings)
    out = efl.psi.mmh3_hash_rows(torch.from_numpy(chars), torch.from_numpy(offsets), seed)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (len(strings),)
    return out.cpu().numpy()


def random_strings(rng, lengths):
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lengths]


def test_golden_vectors_on_the_device(efl):
    for seed in SEEDS:
        items = [h for h in KAT["hashes"] if h["seed"] == seed]
        got = device(efl, [bytes.fromhex(h["hex"]) for h in items], seed)
        assert got.tolist() == [h["hash"] for h in items]
    got = device(efl, [str(i).encode() for i in range(4096)], 0)
    assert got.tolist() == KAT["decimal_ids"]["hashes"] and int((got < 0).sum()) == 2129


@pytest.mark.parametrize("seed", SEEDS)
def test_every_offset_and_length(efl, seed):
    rng = np.random.default_rng(seed & 0xFFFF)
    # lengths 0..67 four times over, each round shifted by one more byte of padding string, so that every
    # (start offset mod 4, length mod 4) pair occurs; bytes >= 0x80 are half of all bytes
    strings = []
    for shift in range(4):
        strings += random_strings(rng, range(68)) + [b"\x80" * (shift + 1)]
    _, offsets = pack(strings)
    pairs = {(int(o) % 4, len(s) % 4) for o, s in zip(offsets, strings)}
    assert pairs == {(a, b) for a in range(4) for b in range(4)}
    assert np.array_equal(device(efl, strings, seed), host_twin(efl, strings, seed))
    # empty strings at the head, in the middle and at the tail, and nothing but empty strings
    strings = [b"", b""] + random_strings(rng, [5, 0, 0, 9, 64, 0, 3]) + [b"", b""]
    assert np.array_equal(device(efl, strings, seed), host_twin(efl, strings, seed))
    empty = device(efl, [b""] * 70, seed)
    assert np.array_equal(empty, host_twin(efl, [b""] * 70, seed)) and len(set(empty.tolist())) == 1
    # one 4 KiB string between short ones
    strings = random_strings(rng, [3, 4096, 1, 4095, 0, 4097])
    assert np.array_equal(device(efl, strings, seed), host_twin(efl, strings, seed))
    # 0xFF everywhere: a sign-extended byte would show in every block and every tail
    strings = [b"\xff" * n for n in range(20)]
    assert np.array_equal(device(efl, strings, seed), host_twin(efl, strings, seed))


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, 3 * 256 + 17))
def test_batch_sizes(efl, n):
    rng = np.random.default_rng(n)
    strings = random_strings(rng, rng.integers(0, 40, n))
    for seed in SEEDS:
        assert np.array_equal(device(efl, strings, seed), host_twin(efl, strings, seed)), seed
    # the per-record host call gives the same
    got = device(efl, strings, 0)
    assert got.tolist() == [efl.psi.mmh3_hash(s) for s in strings]


def test_empty_batch_and_devices(efl):
    out = efl.psi.mmh3_hash_rows(torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64))
    assert out.dtype == torch.int32 and tuple(out.shape) == (0,)
    chars, offsets = pack([b"abc", b"hello"])
    dev = efl.lib.require_gpu()
    want = [efl.psi.mmh3_hash(b"abc"), 613153351]
    assert efl.psi.mmh3_hash_rows(torch.from_numpy(chars).to(dev), torch.from_numpy(offsets).to(dev)).tolist() == want
    assert efl.psi.mmh3_hash_rows(torch.from_numpy(chars).view(torch.int8), torch.from_numpy(offsets)).tolist() == want
    with pytest.raises(efl.errors.InvalidArgumentError, match="offsets"):
        efl.psi.mmh3_hash_rows(torch.from_numpy(chars), torch.from_numpy(offsets).to(torch.int32))
    with pytest.raises(efl.errors.InvalidArgumentError, match="chars"):
        efl.psi.mmh3_hash_rows(torch.from_numpy(chars).to(torch.int32), torch.from_numpy(offsets))
