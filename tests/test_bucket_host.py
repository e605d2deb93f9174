"""CPU: the host side of the bucketed join (efl.psi.bucket, efl.psi.check_sum, efl.psi.bucketed_join):
CheckSum and check_sum against tests/golden/mmh3_kat.json and against the definition, the per-record
bucket functions and the identity that ties get_key and get_local_bucket_id to one modulus, the
argument checks of every new entry point (they run before any HIP call) and what the Python layer
refuses without a GPU."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

with open(os.path.join(GOLDEN, "mmh3_kat.json")) as _f:
    KAT = json.load(_f)


@pytest.fixture(scope="module")
def psi():
    import efl
    return efl.psi


def definition(values, cur=0):
    """xfl/data/check_sum.py, over the golden file's hashes only through mmh3_hash."""
    import efl
    for v in values:
        cur = efl.psi.mmh3_hash(str(cur).encode("utf-8") + v)
    return cur


def test_check_sum_against_the_golden_file(psi):
    negative_seen = False
    for case in KAT["check_sums"]:
        values = [bytes.fromhex(v) for v in case["values"]]
        one, many = psi.CheckSum(case["seed"]), psi.CheckSum(case["seed"])
        assert one.get_check_sum() == case["seed"]
        for v, want in zip(values, case["chain"]):
            one.add(v)
            assert one.get_check_sum() == want, case["name"]
        many.add_list(values)
        assert many.get_check_sum() == case["chain"][-1], case["name"]
        negative_seen |= any(c < 0 for c in case["chain"][:-1])
        # any split of the list is the same chain
        for cut in (1, len(values) // 2):
            split = psi.CheckSum(case["seed"])
            split.add_list(values[:cut])
            split.add_list(values[cut:])
            assert split.get_check_sum() == case["chain"][-1]
        if case["seed"] == 0:
            assert psi.check_sum([values]) == case["chain"][-1]
            assert psi.check_sum(values[:3] + [values[3:]]) == case["chain"][-1]
    assert negative_seen                  # str(cur) with its '-' is part of what is pinned


def test_check_sum_against_the_definition(psi):
    lib = __import__("efl").lib.raw()
    rng = np.random.default_rng(5)
    values = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 40, 300)]
    want = definition(values)
    cs = psi.CheckSum()
    cs.add_list(values)
    assert cs.get_check_sum() == want
    assert psi.check_sum([values[:100], values[100], values[101:]]) == want
    assert psi.check_sum([]) == 0 and psi.CheckSum(seed=9).get_check_sum() == 9
    # the C chain from the ends of the int32 range: str(cur) has a '-' and up to ten digits
    for cur in (0, -1, 2 ** 31 - 1, -2 ** 31, 1000000000, -1000000000):
        chars = b"".join(values[:50])
        offsets = np.zeros(51, dtype=np.int64)
        np.cumsum([len(v) for v in values[:50]], out=offsets[1:])
        got = lib.efl_mmh3_checksum_host(cur, chars, offsets.ctypes.data, 50)
        assert got == definition(values[:50], cur), cur
    assert lib.efl_mmh3_checksum_host(77, None, None, 5) == 77 and lib.efl_mmh3_checksum_host(77, b"x", None, 0) == 77
    # the reference's TypeError for a value that is neither bytes nor a list
    for bad in ("text", 5, None, (b"a",), bytearray(b"a")):
        with pytest.raises(TypeError):
            psi.check_sum([b"ok", bad])
    with pytest.raises(TypeError):
        psi.CheckSum().add("text")
    with pytest.raises(TypeError):
        psi.CheckSum().add_list([b"a", b"b", "text"])


def test_bucket_functions_and_their_identity(psi):
    for case in KAT["buckets"]:
        sel = psi.DefaultKeySelector(case["bucket_num"], case["client2multiserver"])
        for i, key, local in zip(case["ids"], case["keys"], case["local"]):
            assert sel.get_key((i, b"payload")) == key
            assert sel.get_key((i.encode(),)) == key
            assert psi.get_local_bucket_id(i, case["client2multiserver"]) == local
    hashes = KAT["decimal_ids"]["hashes"]
    assert sum(h < 0 for h in hashes) == 2129
    for bucket_num in (1, 2, 3, 64, 1000, 4096):
        for c in (1, 2, 3):
            sel = psi.DefaultKeySelector(bucket_num, c)
            for i in range(0, 4096, 7):
                key, local = sel.get_key((str(i),)), psi.get_local_bucket_id(str(i), c)
                assert 0 <= key < bucket_num and 0 <= local < c
                assert key * c + local == hashes[i] % (bucket_num * c)
    sizes = np.bincount([h % 64 for h in hashes], minlength=64)
    assert sizes.min() == 46 and sizes.max() == 79
    assert psi.DefaultKeySelector()._bucket_num == 64
    import efl
    for bad in ((0, 1), (64, 0), (-1, 1), (64.0, 1), (2 ** 31, 1), (2 ** 16, 2 ** 15)):
        with pytest.raises(efl.errors.InvalidArgumentError):
            psi.DefaultKeySelector(*bad)


def test_argument_errors_without_gpu():
    import efl
    lib = efl.lib.raw()
    P = ctypes.c_void_p
    P16, P4, P2 = P(16), P(4), P(2)
    err = lambda: lib.efl_last_error().decode()
    big, top = 1 << 30, 2 ** 31 - 2

    def mmh3(chars=P16, offsets=P16, n=5, out=P16):
        return lib.efl_mmh3_hash(chars, offsets, n, 0, out, None)

    def ids(hash=P16, n=5, modulus=64, divisor=1, out=P16):
        return lib.efl_bucket_ids(hash, n, modulus, divisor, out, None)

    def partition(bucket=P16, n=5, buckets=64, order=P16, starts=P16, scratch=P16, scratch_len=big):
        return lib.efl_bucket_partition(bucket, n, buckets, order, starts, scratch, scratch_len, None)

    def gather(chars=P16, offsets=P16, order=P16, n=5, out_chars=P16, out_offsets=P16, scratch=P16, scratch_len=big):
        return lib.efl_strings_gather(chars, offsets, order, n, out_chars, out_offsets, scratch, scratch_len, None)

    # n == 0 is a no-op, before anything else is looked at
    assert lib.efl_mmh3_hash(None, None, 0, 0, None, None) == 0
    assert lib.efl_bucket_ids(None, 0, -5, 0, None, None) == 0
    assert lib.efl_bucket_partition(None, 0, 0, None, None, None, 0, None) == 0
    assert lib.efl_strings_gather(None, None, None, 0, None, None, None, 0, None) == 0
    # negative counts
    for f in (mmh3, ids, partition, gather):
        assert f(n=-1) == -3 and "negative" in err(), f.__name__
    # null buffers
    for f, names in ((mmh3, ("chars", "offsets", "out")), (ids, ("hash", "out")),
                     (partition, ("bucket", "order", "starts", "scratch")),
                     (gather, ("chars", "offsets", "order", "out_chars", "out_offsets", "scratch"))):
        for name in names:
            assert f(**{name: None}) == -3 and "null buffer" in err(), (f.__name__, name)
    # misaligned buffers
    assert mmh3(offsets=P4) == -3 and "misaligned" in err()
    assert mmh3(out=P2) == -3 and "misaligned" in err()
    assert ids(hash=P2) == -3 and "misaligned" in err()
    for name in ("order", "starts", "scratch"):
        assert partition(**{name: P4}) == -3 and "misaligned" in err(), name
    assert partition(bucket=P2) == -3 and "misaligned" in err()
    for name in ("offsets", "order", "out_offsets", "scratch"):
        assert gather(**{name: P4}) == -3 and "misaligned" in err(), name
    # bucket counts, moduli and divisors out of range
    for b in (0, -1, 4097, 2 ** 20):
        assert partition(buckets=b) == -3 and "1 <= buckets <= 4096" in err(), b
        assert lib.efl_bucket_scratch_bytes(100, b) == 0
    for m, d in ((0, 1), (64, 0), (64, -1), (3, 4), (2 ** 31, 1), (-64, 1), (2 ** 40, 2)):
        assert ids(modulus=m, divisor=d) == -3 and "1 <= divisor <= modulus <= 2^31 - 1" in err(), (m, d)
    # a scratch that is too small
    assert partition(scratch_len=8) == -3 and "efl_bucket_scratch_bytes" in err()
    assert gather(scratch_len=0) == -3 and "efl_strings_gather_scratch_bytes" in err()
    # more than 2^31 - 2 rows
    for f in (mmh3, ids, partition, gather):
        assert f(n=top + 1) == -8 and "2^31 - 2" in err(), f.__name__
    with pytest.raises(efl.errors.ResourceExhaustedError, match="2\\^31 - 2"):
        efl.lib.check(ids(n=top + 1))
    assert lib.efl_bucket_scratch_bytes(top + 1, 64) == 0 and lib.efl_strings_gather_scratch_bytes(top + 1) == 0
    assert lib.efl_bucket_scratch_bytes(0, 64) == 0 and lib.efl_bucket_scratch_bytes(-1, 64) == 0
    assert lib.efl_strings_gather_scratch_bytes(0) == 0 and lib.efl_strings_gather_scratch_bytes(-1) == 0
    # the partition's scratch: a word per slot (the buckets and one more) and tile of 2,048 rows, and 8
    # bytes per 2,048 of those words; the gather's: 8 bytes per 2,048 of its n + 1 offsets
    assert lib.efl_bucket_scratch_bytes(1, 1) == 8 + 4 * 2
    assert lib.efl_bucket_scratch_bytes(2048, 64) == 8 + 4 * 65
    assert lib.efl_bucket_scratch_bytes(2049, 64) == 8 + 4 * 130
    assert lib.efl_bucket_scratch_bytes(3 * 2048, 4096) == 8 * 7 + 4 * 4097 * 3
    assert lib.efl_strings_gather_scratch_bytes(1) == 8 and lib.efl_strings_gather_scratch_bytes(2047) == 8
    assert lib.efl_strings_gather_scratch_bytes(2048) == 16


def test_python_layer_needs_no_gpu_to_refuse(psi):
    import torch
    import efl
    assert psi.BucketedJoinServer is psi.bucketed_join.BucketedJoinServer
    assert psi.BucketedJoinClient is psi.bucketed_join.BucketedJoinClient
    assert psi.CheckSum is __import__("efl.psi.check_sum", fromlist=["CheckSum"]).CheckSum
    assert {"mmh3_hash", "mmh3_hash_rows", "get_local_bucket_id", "DefaultKeySelector", "partition", "CheckSum",
            "check_sum", "BucketedJoinServer", "BucketedJoinClient", "bucket", "bucketed_join"} <= set(psi.__all__)
    made = []
    signer = psi.EccSigner(b"k" * 32)

    def factory(b):
        made.append(b)
        return psi.EcdhJoinServer(signer, batch_size=4)

    server = psi.BucketedJoinServer(factory, bucket_num=4)
    assert made == [0, 1, 2, 3] and server.bucket_num == 4
    assert [server.bucket(b).bucket_id for b in range(4)] == [0, 1, 2, 3]
    server.add_ids([])
    assert server.get_final_ids() == [[], [], [], []]
    rows = torch.empty((0, 32), dtype=torch.uint8)
    with pytest.raises(efl.errors.InvalidArgumentError, match="bucket id not match, expect 1, got 2"):
        server.bucket(1).sync_join(rows, 2)
    with pytest.raises(efl.errors.InvalidArgumentError, match="bucket id not match, expect 0..3, got 4"):
        server.sync_join(rows, 4)
    with pytest.raises(efl.errors.InvalidArgumentError, match="bucket id not match, expect 3, got 0"):
        server.bucket(3).finish_join(0, 0)
    # an empty client against an empty server: every bucket finishes on the empty CheckSum, once
    client = psi.BucketedJoinClient(lambda b: psi.EcdhJoinClient(signer, batch_size=4), bucket_num=2, client2multiserver=2)
    assert client.join([], server) == []
    assert all(server.bucket(b).is_finished() for b in range(4))
    assert server.finish_join(2, 0) is False
    with pytest.raises(ValueError, match="Join finish error"):
        client.join([], server)
    fresh = psi.BucketedJoinServer(factory, bucket_num=4)
    assert fresh.finish_join(1, 1) is False and fresh.finish_join(1, 0) is True and fresh.finish_join(1, 0) is False
    for bad in (0, -1, 4097, 64.0, None):
        with pytest.raises(efl.errors.InvalidArgumentError, match="bucket_num"):
            psi.BucketedJoinServer(factory, bucket_num=bad)
        with pytest.raises(efl.errors.InvalidArgumentError, match="bucket_num"):
            psi.BucketedJoinClient(factory, bucket_num=bad)
    with pytest.raises(efl.errors.InvalidArgumentError):
        psi.BucketedJoinClient(factory, bucket_num=4096, client2multiserver=2)
    with pytest.raises(efl.errors.InvalidArgumentError, match="client2multiserver"):
        psi.BucketedJoinClient(factory, bucket_num=4, client2multiserver=0)
    for bad in ((64, 0), (0, 1), (3, 4), (2 ** 31, 1)):
        with pytest.raises(efl.errors.InvalidArgumentError, match="modulus"):
            psi.bucket.bucket_ids(torch.zeros(3, dtype=torch.int32), *bad)
    for bad in (0, 4097, 1.5):
        with pytest.raises(efl.errors.InvalidArgumentError, match="buckets"):
            psi.bucket.partition_rows(torch.zeros(3, dtype=torch.int32), bad)
    assert psi.bucketed_join.row_bytes(torch.tensor([[1, 2], [3, 4]], dtype=torch.uint8)) == [b"\x01\x02", b"\x03\x04"]
