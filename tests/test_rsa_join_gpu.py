"""GPU: the transport-free RSA join (efl.psi.rsa_join) end to end on the device: the server's IDs
through sign_rows into an IdStore(8), the client's through blind_rows, psi_sign, deblind_rows and
sync_join, against Python set arithmetic, with the device hash and with a callable on both sides."""
import hashlib
import json
import os

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "rsa_kat.json")) as _f:
    KEY = {k["name"]: k for k in json.load(_f)["keys"]}["openssl-1024"]
PUB, PRV = KEY["public_pem"].encode(), KEY["private_pem"].encode()


@pytest.fixture(scope="module")
def psi():
    import efl
    return efl.psi


def blake_hash(text):
    return int.from_bytes(hashlib.blake2b(text.encode()).digest()[:8], "little")


def the_sets():
    shared = ["user-%05d" % i for i in range(100)]
    server_ids = ["srv-%d" % i for i in range(100)] + shared[:50] + list(range(1, 100)) + shared[50:]
    server_ids.append(shared[7])                                     # one duplicated ID on each side
    client_ids = shared[::-1][:40] + ["cli-%d" % i for i in range(156)] + shared[::-1][40:]
    client_ids.insert(200, shared[93])
    assert len(server_ids) == 300 and len(client_ids) == 257 and len(set(server_ids) & set(client_ids)) == 100
    return server_ids, client_ids


def run_join(psi, oneway_hash):
    server_ids, client_ids = the_sets()
    signer = psi.ServerRsaSigner(PUB, PRV, oneway_hash=oneway_hash)
    server = psi.RsaJoinServer(signer, batch_size=64)
    server.add_ids(server_ids[:130])
    server.add_ids(server_ids[130:])
    assert server.get_rsa_public_key() == PUB
    client = psi.RsaJoinClient(batch_size=64, oneway_hash=oneway_hash)
    got = client.join(client_ids, server)
    want = [i for i in dict.fromkeys(client_ids) if i in set(server_ids)]
    assert got == want and len(got) == 100
    # 299 distinct IDs are 299 keys; 256 distinct requests went in four batches of 64
    assert server._sample_kv_store.size() == 299 and server._sample_kv_store.width == 8
    assert server._request_cnt == 4 and server._all_cnt == 256 and server._hit_cnt == 100
    # the hits are the server's own signed rows of exactly those IDs, in the client's order
    final = server.get_final_result()
    assert final.is_cuda and final.dtype == torch.uint8 and tuple(final.shape) == (100, 8)
    assert torch.equal(final, signer.sign_rows(want))
    assert psi.rsa_cipher.oneway_texts(final) == signer.sign_func(want)
    assert server.get_final_ids() == want
    return got, final.cpu()


def test_end_to_end_join(psi):
    got, final = run_join(psi, "sha256")
    # the host twin of the device hash on both sides: the same rows
    got_twin, final_twin = run_join(psi, psi.rsa_cipher.oneway_sha256)
    assert got_twin == got and torch.equal(final_twin, final)


def test_end_to_end_join_with_a_callable_hash(psi):
    got, final = run_join(psi, blake_hash)
    assert got == run_join(psi, "sha256")[0]
    assert tuple(final.shape) == (100, 8)


def test_error_paths_and_empty_joins(psi):
    import efl
    signer = psi.ServerRsaSigner(PUB, PRV, oneway_hash="sha256")
    server = psi.RsaJoinServer(signer, batch_size=4)
    client = psi.RsaJoinClient(batch_size=4)
    server.add_ids(["id-%d" % i for i in range(6)])
    # shapes and dtypes
    for bad in (torch.zeros((2, 32), dtype=torch.uint8), torch.zeros((2, 8), dtype=torch.int8),
                torch.zeros(8, dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.int32)):
        with pytest.raises(efl.errors.InvalidArgumentError, match="sync_join"):
            server.sync_join(bad)
    for bad in (torch.zeros((2, 31), dtype=torch.int32), torch.zeros((2, 128), dtype=torch.uint8),
                torch.zeros(32, dtype=torch.int32), torch.zeros((2, 32), dtype=torch.int64)):
        with pytest.raises(efl.errors.InvalidArgumentError):
            server.psi_sign(bad)
    assert server._request_cnt == 0 and server._all_cnt == 0
    for bad in (0, -1, 2.0, None):
        with pytest.raises(efl.errors.InvalidArgumentError, match="batch_size"):
            psi.RsaJoinServer(signer, batch_size=bad)
    # disjoint sets: nothing
    assert client.join(["x-%d" % i for i in range(10)], server) == []
    assert tuple(server.get_final_result().shape) == (0, 8) and server.get_final_ids() == []
    assert server._request_cnt == 3 and server._all_cnt == 10 and server._hit_cnt == 0
    # an empty side gives nothing
    assert client.join([], server) == [] and server._request_cnt == 3
    empty = psi.RsaJoinServer(signer)
    empty.add_ids([])
    assert client.join(["id-1", "id-2"], empty) == [] and empty.get_final_ids() == []
    assert tuple(empty.get_final_result().shape) == (0, 8)
    # and the same server joins again: the hits of both joins, in the order asked
    assert client.join(["id-5", "zz", "id-0"], server) == ["id-5", "id-0"]
    assert server.get_final_ids() == ["id-5", "id-0"]
    assert client.join(["id-3", "id-5"], server) == ["id-3", "id-5"]
    assert server.get_final_ids() == ["id-5", "id-0", "id-3", "id-5"]
    assert torch.equal(server.get_final_result(), signer.sign_rows(["id-5", "id-0", "id-3", "id-5"]))
    # an empty batch of rows is a request all the same
    before = server._request_cnt
    res = server.sync_join(torch.empty((0, 8), dtype=torch.uint8))
    assert res.dtype == torch.bool and tuple(res.shape) == (0,) and server._request_cnt == before + 1
    # the client's hash must be the server's: another hash finds nothing
    assert psi.RsaJoinClient(oneway_hash=blake_hash).join(["id-1"], server) == []
