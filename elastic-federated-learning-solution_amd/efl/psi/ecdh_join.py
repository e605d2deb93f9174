"""The reference's ECDH PSI flow without its transport, over tensors, with the reference's names.

In efls-data the flow runs over gRPC between two Flink jobs (xfl/data/ecdh_psi.py,
xfl/service/data_join_server.py: EcdhDataJoinServer). With b the server's secret, a the client's and
h(x) = sha256("curve25519" + x):

  server  process_element        every local ID x goes into the sample store under b h(x)
  step 1  AcquireServerData      the client fetches the store's keys block by block,
          SendServerSignedData   signs each (a b h(x)) and sends the block back; the server fills
                                 the signed-id map  a b h(x) -> b h(x)
  step 2  SyncJoin               the client signs its own IDs (a h(y)); the server signs them once
                                 more (b a h(y)) and answers which are keys of the map
          gather_res             the client keeps the IDs that exist
  server  get_final_result       the hits, mapped back to local keys through the map

Here both stores are efl.psi.IdStore tables on the device, every signature is one batched X25519
launch (efl.psi.ecc_cipher), and a block is a `uint8` [n, 32] tensor that never leaves the device
between the two halves. This is one bucket's join: the bucket hash, the join run bucket by bucket and
the CheckSum that closes each are efl.psi.bucket, efl.psi.bucketed_join and efl.psi.check_sum
(DESIGN.md §5h). Left to the service around it: gRPC, Flink, LevelDB.
"""
from __future__ import annotations

import torch

from efl import errors
from efl import lib as _efl_lib
from efl.psi import ecc_cipher
from efl.psi.id_store import IdStore


def gather_res(ids, existence):
    """xfl/data/utils.py gather_res: the ids whose existence flag is set."""
    assert len(ids) == len(existence), 'ids size {}, existence size {}'.format(len(ids), len(existence))
    return [i for i, e in zip(ids, existence) if e]


def _check_ids(ids, what):
    ids = list(ids)
    for i, v in enumerate(ids):
        if not isinstance(v, (bytes, bytearray)):
            raise ValueError(f"{what}: item {i} is not a byte string")
    return ids


def sign_hash_rows(signer, ids) -> torch.Tensor:
    """signer.sign_hash of every byte string, as rows of a device tensor (uint8 [n, 32])."""
    if signer._hashfunc is not None:
        return sign_rows(signer, ecc_cipher.rows_from_bytes([signer._hashfunc(v) for v in ids], "hashfunc's result"))
    chars, offsets = ecc_cipher.pack_strings(ids)
    return ecc_cipher.x25519_hash(signer._private, chars.to(_efl_lib.require_gpu()), offsets)


def sign_rows(signer, rows) -> torch.Tensor:
    """signer.sign of every row; the result is where the rows were."""
    return ecc_cipher.x25519(signer._private, rows)


class EcdhJoinServer(object):
    def __init__(self, signer, batch_size=2048):
        assert signer is not None, "ecc signer should not be None!"
        if not isinstance(batch_size, int) or batch_size <= 0:
            raise errors.InvalidArgumentError("EcdhJoinServer: batch_size must be a positive int")
        self._ecc_signer = signer
        self._batch_size = batch_size
        self._ids = []                               # local IDs; the sample store's values index it
        self._sample_kv_store = IdStore(32)          # b h(x) -> index of x
        self._signed_id_map = IdStore(32)            # a b h(x) -> position of b h(x) in the sample store
        self._data_pending_buffer = {}               # block_id -> (first position, rows)
        self._data_it = None
        self._next_position = 0
        self._block_id = 0
        self._server_data_exhausted = False
        self._joined_res = []
        self._request_cnt = self._hit_cnt = self._all_cnt = 0

    def add_ids(self, ids):
        """ServerEcdhJoinFunc.process_element for a list of IDs: each goes into the sample store under
        sign_hash(id). Before the first acquire_server_data."""
        if self._data_it is not None:
            raise errors.FailedPreconditionError("add_ids after the server's data has been handed out")
        ids = _check_ids(ids, "add_ids")
        if not ids:
            return
        first = len(self._ids)
        self._ids.extend(ids)
        self._sample_kv_store.put_rows(sign_hash_rows(self._ecc_signer, ids),
                                       torch.arange(first, first + len(ids), dtype=torch.int64))

    def _fetch_a_batch(self):
        if self._data_it is None:
            self._data_it = self._sample_kv_store.iter_batches(self._batch_size)
        batch = next(self._data_it, None)
        if batch is None:
            return None, None
        self._block_id += 1
        return self._block_id, batch

    def acquire_server_data(self):
        """AcquireServerData: (finished, block_id, rows), the next batch_size keys of the sample store
        as a device tensor; (True, 0, an empty tensor) when there are no more."""
        block_id, batch = self._fetch_a_batch()
        if not block_id:
            self._server_data_exhausted = True
            return True, 0, torch.empty((0, 32), dtype=torch.uint8)
        self._data_pending_buffer[block_id] = (self._next_position, batch.shape[0])
        self._next_position += batch.shape[0]
        return False, block_id, batch

    def send_server_signed_data(self, rows, block_id):
        """SendServerSignedData: row i of `rows` is the client's signature of row i of the block."""
        if block_id not in self._data_pending_buffer:
            raise errors.InvalidArgumentError('unexpected block_id: %d' % block_id)
        first, count = self._data_pending_buffer[block_id]
        rows = torch.as_tensor(rows)
        if rows.dim() != 2 or rows.shape[0] != count:
            raise errors.InvalidArgumentError('signed data length error, expected %d, got %d' % (count, rows.shape[0]))
        self._signed_id_map.put_rows(rows, torch.arange(first, first + count, dtype=torch.int64))
        del self._data_pending_buffer[block_id]

    def _all_server_data_ready(self):
        return self._server_data_exhausted and len(self._data_pending_buffer) == 0

    def sync_join(self, rows) -> torch.Tensor:
        """SyncJoin: bool [n], which of the client's signed rows are the server's; the hits are kept
        for get_final_result."""
        if not self._all_server_data_ready():
            raise errors.FailedPreconditionError('there is still server data not signed by client')
        self._request_cnt += 1
        rows = torch.as_tensor(rows)
        if rows.shape[0] == 0:
            return torch.zeros(0, dtype=torch.bool, device=rows.device)
        # in ecdh, ids should be signed before Join
        signed = sign_rows(self._ecc_signer, rows)
        res = self._signed_id_map.exists(signed)
        self._all_cnt += rows.shape[0]
        hits = signed[res]
        self._hit_cnt += hits.shape[0]
        self._joined_res.append(hits)
        return res

    def _final_positions(self):
        if not self._joined_res:
            return torch.empty(0, dtype=torch.int64)
        found, positions = self._signed_id_map.get(torch.cat([h.to(self._signed_id_map.device) for h in self._joined_res]))
        return positions[found]

    def get_final_result(self) -> torch.Tensor:
        """The server's own keys (sign_hash of its IDs, uint8 [hits, 32]) of every hit so far, in the
        order the client asked: each double-signed hit goes through the signed-id map, as the
        reference's `_ecdh_id_map.get(i)` does."""
        positions = self._final_positions()
        if positions.shape[0] == 0:
            return torch.empty((0, 32), dtype=torch.uint8)
        return self._sample_kv_store.keys()[positions]

    def get_final_ids(self) -> list:
        """The server's IDs behind get_final_result (the reference's `_sample_store.get(local_key)`)."""
        positions = self._final_positions()
        if positions.shape[0] == 0:
            return []
        return [self._ids[i] for i in self._sample_kv_store.values()[positions].tolist()]


class EcdhJoinClient(object):
    def __init__(self, signer, batch_size=2048):
        assert signer is not None, "ecc signer should not be None!"
        if not isinstance(batch_size, int) or batch_size <= 0:
            raise errors.InvalidArgumentError("EcdhJoinClient: batch_size must be a positive int")
        self._signer = signer
        self._batch_size = batch_size

    def sign_server_block(self, rows) -> torch.Tensor:
        """Step 1's signature of one block of the server's keys."""
        return sign_rows(self._signer, rows)

    def sign_server_data(self, server) -> int:
        """Step 1: every block of the server signed and sent back; the number of rows."""
        item_cnt = 0
        while True:
            finished, block_id, data = server.acquire_server_data()
            if finished:
                return item_cnt
            item_cnt += data.shape[0]
            server.send_server_signed_data(self.sign_server_block(data), block_id)

    def join(self, ids, server) -> list:
        """ClientEcdhJoinFunc against `server`: step 1, then the IDs in batches (each ID once, as the
        request buffer's keys are) through sign_hash, sync_join and gather_res. The IDs the server
        has too, in the order given."""
        request_ids = list(dict.fromkeys(_check_ids(ids, "join")))
        self.sign_server_data(server)
        res_ids = []
        for o in range(0, len(request_ids), self._batch_size):
            batch = request_ids[o:o + self._batch_size]
            existence = server.sync_join(sign_hash_rows(self._signer, batch))
            res_ids += gather_res(batch, existence.tolist())
        return res_ids
