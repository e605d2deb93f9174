"""GPU: the bucketed join (efl.psi.bucketed_join) end to end, over the ECDH and the RSA halves: the
pairs against the unbucketed join of the same sets and against floor_mod(mmh3(id), buckets) from the
golden generator's pure-Python hash, the order inside a bucket, both sides' CheckSums against the
pure-Python chain over the request rows that hit, FinishJoin once, a CheckSum off by one, a wrong
bucket id, empty buckets and an empty client."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_mmh3_golden", os.path.join(GOLDEN, "make_mmh3_golden.py"))
golden = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(golden)

with open(os.path.join(GOLDEN, "rsa_kat.json")) as _f:
    KEY = {k["name"]: k for k in json.load(_f)["keys"]}["openssl-1024"]
PUB, PRV = KEY["public_pem"].encode(), KEY["private_pem"].encode()

SHARED = [b"user-%05d" % i for i in range(100)]
SERVER_IDS = [b"srv-%d" % i for i in range(100)] + SHARED[:50] + [b"%d" % i for i in range(1, 100)] + SHARED[50:] \
    + [SHARED[7]]                                                       # one duplicated ID on each side
CLIENT_IDS = SHARED[::-1][:40] + [b"cli-%d" % i for i in range(156)] + SHARED[::-1][40:]
CLIENT_IDS.insert(200, SHARED[93])
assert len(SERVER_IDS) == 300 and len(CLIENT_IDS) == 257 and len(set(SERVER_IDS) & set(CLIENT_IDS)) == 100

CASES = [(bucket_num, c) for bucket_num in (1, 4, 64) for c in (1, 2)]


@pytest.fixture(scope="module")
def psi():
    import efl
    return efl.psi


class Ecdh(object):
    """The two factories of an ECDH join and the request rows of a list of IDs (a h(y))."""

    def __init__(self, psi):
        self.psi = psi
        self.server_signer, self.client_signer = psi.EccSigner(b"s" * 32), psi.EccSigner(b"c" * 32)

    def server(self, b):
        return self.psi.EcdhJoinServer(self.server_signer, batch_size=16)

    def client(self, b):
        return self.psi.EcdhJoinClient(self.client_signer, batch_size=16)

    def request_rows(self, ids):
        return self.psi.ecdh_join.sign_hash_rows(self.client_signer, ids)

    def unbucketed(self):
        server = self.server(0)
        server.add_ids(SERVER_IDS)
        return self.client(0).join(CLIENT_IDS, server)


class Rsa(object):
    """The same for RSA: the request rows are H(h(y)^d), which the server's signer gives directly."""

    def __init__(self, psi):
        self.psi = psi
        self.signer = psi.ServerRsaSigner(PUB, PRV, oneway_hash="sha256")

    def server(self, b):
        return self.psi.RsaJoinServer(self.signer, batch_size=16)

    def client(self, b):
        return self.psi.RsaJoinClient(batch_size=16, oneway_hash="sha256")

    def request_rows(self, ids):
        return self.signer.sign_rows(ids)

    def unbucketed(self):
        server = self.server(0)
        server.add_ids(SERVER_IDS)
        return self.client(0).join(CLIENT_IDS, server)


@pytest.fixture(scope="module", params=["ecdh", "rsa"])
def flow(request, psi):
    f = Ecdh(psi) if request.param == "ecdh" else Rsa(psi)
    f.flat = f.unbucketed()                      # computed once, shared by the cases
    assert len(f.flat) == 100
    return f


def expected_pairs(buckets):
    have = set(SERVER_IDS)
    ids = [i for i in dict.fromkeys(CLIENT_IDS) if i in have]
    return [(b, i) for b in range(buckets) for i in ids if golden.mmh3_hash(i) % buckets == b]


@pytest.mark.parametrize("bucket_num,c", CASES)
def test_bucketed_join(psi, flow, bucket_num, c):
    buckets = bucket_num * c
    server = psi.BucketedJoinServer(flow.server, bucket_num=buckets)
    server.add_ids(SERVER_IDS[:130])
    server.add_ids(SERVER_IDS[130:])
    client = psi.BucketedJoinClient(flow.client, bucket_num=bucket_num, client2multiserver=c)
    pairs = client.join(CLIENT_IDS, server)
    # the ID set is the unbucketed join's; each pair's bucket is floor_mod(mmh3(id), bucket_num * c); inside
    # a bucket the order is the order given
    assert sorted(i for _, i in pairs) == sorted(flow.flat) and len(pairs) == 100
    assert pairs == expected_pairs(buckets)
    # both sides' CheckSums, per bucket, against the pure-Python chain over the request rows that hit
    final_ids = server.get_final_ids()
    assert len(final_ids) == buckets
    empty_buckets = 0
    for b in range(buckets):
        hits = [i for k, i in pairs if k == b]
        assert final_ids[b] == hits
        rows = psi.bucketed_join.row_bytes(flow.request_rows(hits)) if hits else []
        want = golden.check_sum_chain(rows)[-1] if rows else 0
        assert client.get_check_sum(b) == server.get_check_sum(b) == want, b
        empty_buckets += not hits
        # FinishJoin answered True once, inside join; now it is False, with the right CheckSum too
        assert server.bucket(b).is_finished() and server.finish_join(b, want) is False
    if buckets >= 64:
        assert empty_buckets > 0                  # 100 hits over 128 buckets: a bucket without one finishes too
    # the server has finished every bucket: a second join cannot finish
    with pytest.raises(ValueError, match="Join finish error"):
        client.join(CLIENT_IDS[:5], server)


def test_check_sum_off_by_one_and_wrong_bucket(psi, flow):
    import efl

    class OffByOne(psi.BucketedJoinServer):
        def finish_join(self, bucket_id, check_sum):
            return super().finish_join(bucket_id, check_sum + (bucket_id == 2))

    server = OffByOne(flow.server, bucket_num=4)
    server.add_ids(SERVER_IDS)
    client = psi.BucketedJoinClient(flow.client, bucket_num=4)
    with pytest.raises(ValueError, match="Join finish error"):
        client.join(CLIENT_IDS, server)
    assert [server.bucket(b).is_finished() for b in range(4)] == [True, True, False, True]
    assert client.get_check_sum(2) == server.get_check_sum(2) != 0
    # a request under another bucket's id is refused before anything is looked up
    server = psi.BucketedJoinServer(flow.server, bucket_num=4)
    server.add_ids(SERVER_IDS)
    rows = flow.request_rows(SHARED[:3])
    before = server.bucket(1)._request_cnt
    with pytest.raises(efl.errors.InvalidArgumentError, match="bucket id not match, expect 1, got 2"):
        server.bucket(1).sync_join(rows, 2)
    with pytest.raises(efl.errors.InvalidArgumentError, match="bucket id not match, expect 0..3, got 4"):
        server.sync_join(rows, 4)
    with pytest.raises(efl.errors.InvalidArgumentError, match="bucket id not match"):
        server.sync_join(rows, -1)
    assert server.bucket(1)._request_cnt == before and server.get_check_sum(1) == 0


def test_empty_buckets_and_empty_client(psi, flow):
    # five IDs over 64 buckets: most buckets are empty on both sides, and all of them finish
    few = SHARED[:5]
    server = psi.BucketedJoinServer(flow.server, bucket_num=64)
    server.add_ids(few + [b"only-here"])
    client = psi.BucketedJoinClient(flow.client, bucket_num=32, client2multiserver=2)
    pairs = client.join([b"not-there"] + few, server)
    assert pairs == sorted(((golden.mmh3_hash(i) % 64, i) for i in few), key=lambda p: p[0])
    assert all(server.bucket(b).is_finished() for b in range(64))
    assert sum(1 for ids in server.get_final_ids() if ids) == len({b for b, _ in pairs})
    # an empty client against a server that has IDs; an empty server against a client that has IDs
    server = psi.BucketedJoinServer(flow.server, bucket_num=4)
    server.add_ids(SERVER_IDS)
    assert psi.BucketedJoinClient(flow.client, bucket_num=4).join([], server) == []
    assert all(server.bucket(b).is_finished() for b in range(4)) and server.get_final_ids() == [[], [], [], []]
    server = psi.BucketedJoinServer(flow.server, bucket_num=4)
    assert psi.BucketedJoinClient(flow.client, bucket_num=2, client2multiserver=2).join(CLIENT_IDS[:20], server) == []
    assert all(server.get_check_sum(b) == 0 for b in range(4))
