"""GPU: the transport-free ECDH join (efl.psi.ecdh_join) end to end on the device: two EccSigners
with fixed secrets, the server's IDs through sign_hash into an IdStore, the blocks signed by the
client into the signed-id map, the client's IDs through sync_join, against Python set arithmetic and
tests/golden/x25519_kat.json."""
import json
import os

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "x25519_kat.json")) as _f:
    KAT = json.load(_f)

A = bytes(range(1, 33))                 # the client's secret
B = bytes(range(101, 133))              # the server's


@pytest.fixture(scope="module")
def psi():
    import efl
    return efl.psi


def rows(items):
    return torch.frombuffer(bytearray(b"".join(items)), dtype=torch.uint8).reshape(len(items), 32)


def test_end_to_end_join(psi):
    shared = [b"user-%05d" % i for i in range(100)]
    server_ids = [b"srv-%d" % i for i in range(100)] + shared[:50] + [b"s" * i for i in range(1, 100)] + shared[50:]
    server_ids.append(shared[7])                                     # one duplicated ID on each side
    client_ids = shared[::-1][:40] + [b"cli-%d" % i for i in range(156)] + shared[::-1][40:]
    client_ids.insert(200, shared[93])
    assert len(server_ids) == 300 and len(client_ids) == 257 and len(set(server_ids) & set(client_ids)) == 100
    server = psi.EcdhJoinServer(psi.EccSigner(B), batch_size=64)
    server.add_ids(server_ids[:130])
    server.add_ids(server_ids[130:])
    client = psi.EcdhJoinClient(psi.EccSigner(A), batch_size=64)
    got = client.join(client_ids, server)
    want = [i for i in dict.fromkeys(client_ids) if i in set(server_ids)]
    assert got == want and len(got) == 100
    # five blocks flowed (299 distinct IDs in blocks of 64) and none is pending
    assert server._block_id == 5 and not server._data_pending_buffer and server._signed_id_map.size() == 299
    assert server._request_cnt == 4 and server._all_cnt == 256 and server._hit_cnt == 100
    # the hits map back to the server's own signed keys of exactly those IDs, in the client's order
    own = psi.EccSigner(B).sign_hash_list(want)
    final = server.get_final_result()
    assert final.is_cuda and bytes(final.cpu().numpy().tobytes()) == b"".join(own)
    assert server.get_final_ids() == want


def test_against_the_fixture(psi):
    # both orders of signing agree on the fixture's points and digests, and with the fixture's rows
    us = rows([bytes.fromhex(u) for u in KAT["us"]] + [bytes.fromhex(h["digest"]) for h in KAT["hash"]["vectors"]])
    sc = {s["name"]: s for s in KAT["scalars"]}
    a, b = bytes.fromhex(sc["random"]["scalar"]), bytes.fromhex(sc["unclamped"]["scalar"])
    x = psi.ecc_cipher.x25519
    ab, ba = x(b, x(a, us.cuda())), x(a, x(b, us.cuda()))
    assert torch.equal(ab, ba)
    assert torch.equal(x(a, us.cuda()).cpu()[:len(KAT["us"])], rows([bytes.fromhex(o) for o in sc["random"]["outs"]]))
    assert int((ab.cpu() != 0).any(dim=1).sum()) >= len(KAT["hash"]["vectors"])
    # a join over the fixture's hashed IDs: the server's keys are the fixture's signed digests
    secret = bytes.fromhex(KAT["hash"]["secret"])
    ids = [bytes.fromhex(h["id"]) for h in KAT["hash"]["vectors"]]
    server = psi.EcdhJoinServer(psi.EccSigner(secret), batch_size=3)
    server.add_ids(ids)
    assert bytes(server._sample_kv_store.keys().cpu().numpy().tobytes()).hex() == \
        "".join(h["signed"] for h in KAT["hash"]["vectors"])
    asked = [b"not there"] + ids[::-1] + [b"nor this"]
    assert psi.EcdhJoinClient(psi.EccSigner(A)).join(asked, server) == ids[::-1]
    assert server.get_final_ids() == ids[::-1]


def test_error_paths_and_empty_joins(psi):
    import efl
    server = psi.EcdhJoinServer(psi.EccSigner(B), batch_size=4)
    client = psi.EcdhJoinClient(psi.EccSigner(A))
    server.add_ids([b"id-%d" % i for i in range(6)])
    with pytest.raises(efl.errors.FailedPreconditionError, match="not signed by client"):
        server.sync_join(torch.zeros((1, 32), dtype=torch.uint8))
    finished, block_id, block = server.acquire_server_data()
    assert not finished and block_id == 1 and tuple(block.shape) == (4, 32) and block.is_cuda
    signed = client.sign_server_block(block)
    with pytest.raises(efl.errors.InvalidArgumentError, match="unexpected block_id: 2"):
        server.send_server_signed_data(signed, 2)
    with pytest.raises(efl.errors.InvalidArgumentError, match="signed data length error, expected 4, got 3"):
        server.send_server_signed_data(signed[:3], 1)
    server.send_server_signed_data(signed, 1)
    with pytest.raises(efl.errors.InvalidArgumentError, match="unexpected block_id: 1"):
        server.send_server_signed_data(signed, 1)                   # a block is taken once
    with pytest.raises(efl.errors.FailedPreconditionError):
        server.add_ids([b"late"])
    # the rest of the flow, then disjoint sets: nothing
    assert client.join([b"x-%d" % i for i in range(10)], server) == []
    assert tuple(server.get_final_result().shape) == (0, 32) and server.get_final_ids() == []
    assert server._signed_id_map.size() == 6
    # an empty side gives nothing
    assert client.join([], server) == []
    empty = psi.EcdhJoinServer(psi.EccSigner(B))
    assert client.join([b"id-1", b"id-2"], empty) == [] and empty.get_final_ids() == []
    # and the same server still joins
    assert client.join([b"id-5", b"zz", b"id-0"], server) == [b"id-5", b"id-0"]
    assert server.get_final_ids() == [b"id-5", b"id-0"]
