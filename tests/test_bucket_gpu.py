"""GPU: the bucket ids, the partition and the gather of efl.psi.bucket. efl_bucket_ids against the
golden file and against Python's % and // of the golden hashes; efl_bucket_partition against
numpy.argsort(kind="stable"), `order` and `starts` exact, at the sizes around the wave, the tile of
2,048 rows and several tiles, with 1 to 4,096 buckets, skewed, sparse and out-of-range bucket columns,
and byte-identical from run to run; efl_strings_gather against the Python list indexed by `order`."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "mmh3_kat.json")) as _f:
    KAT = json.load(_f)

TILE = 2048                                   # csrc/mmh3.h kTile
SIZES = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)


@pytest.fixture(scope="module")
def psi():
    import efl
    return efl.psi


def model(bucket, buckets):
    """(order, starts) by numpy: a stable sort by slot, rows outside [0, buckets) after the last bucket."""
    b = np.asarray(bucket, dtype=np.int64)
    slot = np.where((b >= 0) & (b < buckets), b, buckets)
    order = np.argsort(slot, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(slot, minlength=buckets + 1))])[:buckets + 1]
    return order, starts


def check(psi, bucket, buckets):
    bucket = np.asarray(bucket, dtype=np.int32)
    order, starts = psi.bucket.partition_rows(torch.from_numpy(bucket), buckets)
    assert order.is_cuda and order.dtype == torch.int64 and tuple(order.shape) == (len(bucket),)
    assert starts.dtype == torch.int64 and tuple(starts.shape) == (buckets + 1,)
    want_order, want_starts = model(bucket, buckets)
    assert np.array_equal(starts.cpu().numpy(), want_starts), (len(bucket), buckets)
    assert np.array_equal(order.cpu().numpy(), want_order), (len(bucket), buckets)
    return order, starts


def test_bucket_ids_against_the_golden_file(psi):
    for case in KAT["buckets"]:
        sel = psi.DefaultKeySelector(case["bucket_num"], case["client2multiserver"])
        ids = [i.encode() for i in case["ids"]]
        assert sel.get_keys(ids).tolist() == case["keys"]
        hashes = psi.mmh3_hash_rows(*psi.bucket.pack_strings(ids))
        assert psi.bucket.bucket_ids(hashes, case["client2multiserver"]).tolist() == case["local"]


@pytest.mark.parametrize("bucket_num", (1, 2, 3, 64, 1000, 4096))
def test_bucket_ids_over_both_signs(psi, bucket_num):
    hashes = np.array(KAT["decimal_ids"]["hashes"] + [-2 ** 31, -1, 0, 2 ** 31 - 1], dtype=np.int32)
    assert (hashes < 0).sum() == 2131
    t = torch.from_numpy(hashes)
    wide = hashes.astype(np.int64)
    for c in (1, 2, 3):
        keys = psi.DefaultKeySelector(bucket_num, c).get_keys(hashes=t)
        local = psi.bucket.bucket_ids(t, c)
        assert keys.is_cuda and keys.dtype == torch.int32
        assert np.array_equal(keys.cpu().numpy(), (wide % (bucket_num * c)) // c)          # numpy's % floors too
        assert np.array_equal(local.cpu().numpy(), wide % c)
        both = keys.cpu().numpy().astype(np.int64) * c + local.cpu().numpy()
        assert np.array_equal(both, wide % (bucket_num * c))
    top = psi.bucket.bucket_ids(t, 2 ** 31 - 1)
    assert np.array_equal(top.cpu().numpy(), wide % (2 ** 31 - 1))
    assert tuple(psi.bucket.bucket_ids(torch.zeros(0, dtype=torch.int32), 64).shape) == (0,)


@pytest.mark.parametrize("buckets", (1, 2, 64, 4096))
def test_partition_sizes(psi, buckets):
    rng = np.random.default_rng(buckets)
    for n in SIZES:
        check(psi, rng.integers(0, buckets, n), buckets)
    order, starts = psi.bucket.partition_rows(torch.zeros(0, dtype=torch.int32), buckets)
    assert tuple(order.shape) == (0,) and starts.tolist() == [0] * (buckets + 1)


def test_partition_skewed_and_sparse_columns(psi):
    n = 3 * TILE + 17
    rng = np.random.default_rng(7)
    for buckets in (2, 64, 4096):
        check(psi, np.zeros(n), buckets)                                   # all rows in the first bucket
        check(psi, np.full(n, buckets - 1), buckets)                       # ... in the last
        check(psi, rng.choice([3 % buckets, buckets - 1], n), buckets)     # two buckets, the others empty
        check(psi, np.sort(rng.integers(0, buckets, n)), buckets)          # already grouped
        check(psi, np.sort(rng.integers(0, buckets, n))[::-1].copy(), buckets)
    # every row in its own bucket, in shuffled order: order is the inverse permutation
    order, starts = check(psi, rng.permutation(4096), 4096)
    assert starts.tolist() == list(range(4097))
    order, _ = check(psi, rng.permutation(64), 64)
    # one wave of equal rows, one wave of distinct rows, and rows that alternate between two buckets
    check(psi, np.concatenate([np.full(64, 5), np.arange(64), np.tile([9, 2], 200)]), 64)
    # 64 buckets over three tiles, each row's bucket its index mod 64 and mod 63
    check(psi, np.arange(n) % 64, 64)
    check(psi, np.arange(n) % 63, 64)


def test_partition_rows_without_a_bucket(psi):
    """A bucket id outside [0, buckets) writes nothing out of bounds: such rows follow the last bucket,
    ascending, and starts[buckets] counts the rows that have a bucket."""
    n = 2 * TILE + 5
    rng = np.random.default_rng(11)
    b = rng.integers(0, 64, n).astype(np.int32)
    b[::7] = -1
    b[3::11] = 64
    b[5::13] = 2 ** 31 - 1
    b[6::17] = -2 ** 31
    order, starts = check(psi, b, 64)
    valid = int(((b >= 0) & (b < 64)).sum())
    assert int(starts[64]) == valid < n
    tail = order[valid:].cpu().numpy()
    assert np.array_equal(tail, np.flatnonzero((b < 0) | (b >= 64)))
    check(psi, np.full(300, -5), 2)
    check(psi, np.full(300, 4096), 4096)


def test_partition_is_deterministic(psi):
    n = 3 * TILE + 17
    rng = np.random.default_rng(13)
    for buckets in (64, 4096):
        b = torch.from_numpy(rng.integers(0, buckets, n).astype(np.int32)).cuda()
        runs = [psi.bucket.partition_rows(b, buckets) for _ in range(3)]
        first = [t.cpu().numpy().tobytes() for t in runs[0]]
        for run in runs[1:]:
            assert [t.cpu().numpy().tobytes() for t in run] == first


def test_gather_against_the_python_list(psi):
    rng = np.random.default_rng(17)
    n = TILE + 300
    ids = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 24, n)]
    ids[0] = ids[1] = ids[n // 2] = ids[-1] = ids[-2] = b""              # empty strings at the head, the middle, the tail
    ids[7] = bytes(range(256)) * 16                                       # one 4 KiB string
    for bucket_num, c in ((1, 1), (64, 1), (64, 2), (4096, 1)):
        p = psi.partition(ids, bucket_num, c)
        order, starts = p.order.cpu().numpy(), p.starts.cpu().numpy()
        hashes = [psi.mmh3_hash(i) for i in ids]
        assert p.hashes.tolist() == hashes
        want_order, want_starts = model([(h % (bucket_num * c)) // c for h in hashes], bucket_num)
        assert np.array_equal(order, want_order) and np.array_equal(starts, want_starts)
        chars, offsets = p.chars.cpu().numpy().tobytes(), p.offsets.tolist()
        assert offsets[0] == 0 and offsets[-1] == sum(len(i) for i in ids)
        got = [chars[offsets[k]:offsets[k + 1]] for k in range(n)]
        assert got == [ids[i] for i in order]
        # a bucket's slice is what the signers' kernels take: offsets into the one chars buffer
        b = int(np.argmax(np.diff(starts)))
        bc, bo = p.bucket(b)
        assert bc is p.chars and bo.tolist() == offsets[starts[b]:starts[b + 1] + 1]
        fdh = psi.rsa_cipher.sha256_rows(bc, bo)
        want = psi.rsa_cipher.sha256_rows(*psi.bucket.pack_strings([ids[i] for i in order[starts[b]:starts[b + 1]]]))
        assert torch.equal(fdh, want)
    # any order, not only a permutation: repeats, and entries outside [0, n) as empty strings
    chars, offsets = psi.bucket.pack_strings(ids)
    for pick in (np.zeros(n, dtype=np.int64) + 7, rng.integers(0, n, n), np.arange(n)[::-1].copy(),
                 np.where(np.arange(n) % 3 == 0, -1, np.arange(n)), np.full(n, n)):
        oc, oo = psi.bucket.gather_strings(chars, offsets, torch.from_numpy(pick.astype(np.int64)))
        raw, oo = oc.cpu().numpy().tobytes(), oo.tolist()
        assert [raw[oo[k]:oo[k + 1]] for k in range(n)] == [ids[i] if 0 <= i < n else b"" for i in pick]
    # nothing but empty strings, and no strings
    oc, oo = psi.bucket.gather_strings(*psi.bucket.pack_strings([b""] * 70), torch.arange(69, -1, -1))
    assert oo.tolist() == [0] * 71
    oc, oo = psi.bucket.gather_strings(*psi.bucket.pack_strings([]), torch.zeros(0, dtype=torch.int64))
    assert oo.tolist() == [0]
